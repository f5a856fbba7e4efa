"""--multimaf end to end (python -m sibelia_amd over sbl_align_block_groups) on seeded synthetic genomes written here: the file must be
what tests/msa_model.py makes of the coordinates in blocks_coords.txt.

The input: one 20 kbp random record; copy B with about 1 % substitutions, three indels of 1 .. 30 bases and its last 3 kbp
reverse-complemented; copy C with about 1 % substitutions, three indels and the segment [2000, 4000) of the original inserted a second
time at 15000.  The inverted segment lies at the record's end because `-s loose` removes every bulge shorter than 15 kbp: an inversion
in the middle of a 20 kbp record is smoothed away and never becomes a block of its own, one at the end is no bulge.  So the block of
the duplicated segment has two instances in one file, and the inverted segment gives a block with instances on '-' (checked without a
device against the CPU oracle's blocks when the seed was chosen; asserted below).  Blocks are at most 17 kbp long and differ by about
2 % and a few indels: far below every limit of DESIGN.md 0.2, so no block is skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                        # noqa: E402
import msa_model as MM                             # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 505
NAMES = ["genomeA", "genomeB", "genomeC"]


def _edited(rng, s, rate, indel_at):
    out = bytearray(s)
    for at in np.flatnonzero(rng.random(len(s)) < rate):
        out[at] = b"ACGT".replace(bytes(out[at:at + 1]), b"")[int(rng.integers(0, 3))]
    for k, at in enumerate(sorted(indel_at, reverse=True)):
        n = int(rng.integers(1, 31))
        if k % 2:
            del out[at:at + n]
        else:
            out[at:at] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    return bytes(out)


def genomes():
    rng = np.random.default_rng(SEED)
    a = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20000))
    b = bytearray(_edited(rng, a, 0.01, (1500, 6000, 13000)))
    b[-3000:] = MM.reverse_complement(bytes(b[-3000:]))
    c = bytearray(_edited(rng, a, 0.01, (5000, 12500, 18000)))
    c[15000:15000] = _edited(rng, a[2000:4000], 0.01, ())
    return [a, bytes(b), bytes(c)]


def repeat_genome():
    """one record with an internal repeat: 12 kbp, the segment [1000, 3000) once more (1 % substitutions) at 8000"""
    rng = np.random.default_rng(SEED + 1)
    a = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 12000))
    a[8000:8000] = _edited(rng, bytes(a[1000:3000]), 0.01, ())
    return bytes(a)


def run_cli(tmp_path, records, names, extra):
    fa = []
    for name, s in zip(names, records):
        fa.append(str(tmp_path / (name + ".fa")))
        with open(fa[-1], "wb") as f:
            f.write(b">" + name.encode() + b"\n" + s + b"\n")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "sibelia_amd", "-s", "loose", "-m", "500", "--multimaf", "out.maf", "-o", str(out)] + extra + fa,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""                                                       # no block is skipped
    return (out / "out.maf").read_bytes(), (out / "blocks_coords.txt").read_text()


def parse_maf(text):
    lines = text.decode().split("\n")
    assert lines[:2] == ["##maf version=1", ""] and lines[-1] == ""
    paragraphs, at = [], 2
    while at < len(lines) - 1:
        assert lines[at] == "a", lines[at]
        rows = []
        at += 1
        while lines[at] != "":
            tag, name, start, size, strand, total, row = lines[at].split(" ")
            assert tag == "s" and strand in "+-"
            rows.append((name, int(start), int(size), strand, int(total), row.encode()))
            at += 1
        paragraphs.append(rows)
        at += 1
    return paragraphs


def check(maf_text, coords_text, records, names):
    blocks = BM.parse_blocks_coords(coords_text)
    groups = MM.block_groups(blocks, 500)
    paragraphs = parse_maf(maf_text)
    assert len(paragraphs) == len(groups) >= 1
    index = {n: i for i, n in enumerate(names)}
    for (block, insts), rows in zip(groups, paragraphs):                        # ascending id, the instances in the order of the definition
        assert len(rows) == len(insts) >= 2 and len({len(r[5]) for r in rows}) == 1, block
        for (c, s, e, rev), (name, start, size, strand, total, row) in zip(insts, rows):
            assert (index[name], size, strand, total) == (c, e - s, "-" if rev else "+", len(records[c])), block
            lo = total - start - size if rev else start
            assert (lo, lo + size) == (s, e), block
            text = records[c][lo:lo + size]
            assert row.replace(b"-", b"") == (MM.reverse_complement(text) if rev else text), block
    assert maf_text == MM.maf(records, names, groups, MM.pair_banded)       # (band storage: the blocks are thousands of bases long)
    return groups


def test_three_genomes(tmp_path):
    records = genomes()
    maf_text, coords = run_cli(tmp_path, records, NAMES, [])
    groups = check(maf_text, coords, records, NAMES)
    assert any(len(insts) >= 3 for _, insts in groups)                          # a block with three instances or more
    assert any(len({c for c, _, _, _ in insts}) < len(insts) for _, insts in groups)      # ... with two instances in one file
    assert any(rev for _, insts in groups for _, _, _, rev in insts)            # a reversed instance


def test_two_genomes_with_corrected_boundaries(tmp_path):
    records = genomes()[:2]
    maf_text, coords = run_cli(tmp_path, records, NAMES[:2], ["--correctboundaries"])
    check(maf_text, coords, records, NAMES[:2])


def test_one_genome_with_an_internal_repeat(tmp_path):
    records = [repeat_genome()]
    maf_text, coords = run_cli(tmp_path, records, ["repeated"], [])
    groups = check(maf_text, coords, records, ["repeated"])
    assert all(c == 0 for _, insts in groups for c, _, _, _ in insts)
