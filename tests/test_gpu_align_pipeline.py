"""--maf / --variants end to end (sibelia_amd/pipeline.py over csrc/block_align.hip) on a seeded synthetic pair built here, and once on
the Staphylococcus aureus fixture.

The synthetic pair: one 40 kbp random record; a copy with 60 planted substitutions at least 200 apart, one 4 kbp segment
reverse-complemented and four indels of 1..30 bases.  The blocks between the inversion's breakpoints are at most 20 kbp long and carry
at most 60 substitutions (100 each against a match) and 120 gap columns (75 each): 15000 at the very most, while a path that leaves the
first band (w = 64) pays 75 * 130 for gap columns and loses 25 * 65 in matches, 11375 -- so w = 64 or one doubling proves every pair
and nothing comes near the memory caps."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                        # noqa: E402
import galign_model as GM                          # noqa: E402
from correct_fixtures import write_inputs          # noqa: E402

pytestmark = pytest.mark.gpu

ARGS = ["-s", "fine", "-m", "500", "--lastk", "30", "-r", "--correctboundaries", "-q"]
SEGMENT = (21000, 25000)


def synthetic():
    rng = np.random.default_rng(404)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 40000))
    copy = bytearray(ref)
    subs = {}
    for p in range(300, 39700, 650):                            # 61 positions, 650 apart
        if len(subs) == 60:
            break
        at = p + int(rng.integers(0, 400))
        alt = b"ACGT".replace(ref[at:at + 1], b"")[int(rng.integers(0, 3))]
        copy[at] = alt
        subs[at] = alt
    s, e = SEGMENT
    copy[s:e] = BM.reverse_complement(bytes(copy[s:e]))
    edits = []                                                  # (reference position, length): indels, applied from the right
    for at, kind in ((33000, "del"), (29000, "ins"), (12000, "del"), (5000, "ins")):
        n = int(rng.integers(1, 31))
        if kind == "del":
            del copy[at:at + n]
        else:
            copy[at:at] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
        edits.append((at, n))
    return ref, bytes(copy), subs, edits


def run_pipeline(tmp_path, extra):
    from sibelia_amd import pipeline as P
    ref, copy, _, _ = synthetic()
    fa = []
    for name, s in (("refgenome", ref), ("assembly", copy)):
        fa.append(str(tmp_path / (name + ".fa")))
        with open(fa[-1], "wb") as f:
            f.write(b">" + name.encode() + b"\n" + s + b"\n")
    rc, files, out = P.run(ARGS + extra + ["-o", str(tmp_path / "out")] + fa)
    assert rc == 0
    return files, out


def parse_maf(text):
    lines = text.decode().split("\n")
    assert lines[:2] == ["##maf version=1", ""] and lines[-1] == ""
    blocks, at = [], 2
    while at < len(lines) - 1:
        assert lines[at] == "a" and lines[at + 3] == "", lines[at:at + 4]
        rows = []
        for ln in lines[at + 1:at + 3]:
            tag, name, start, size, strand, total, row = ln.split(" ")
            assert tag == "s"
            rows.append((name, int(start), int(size), strand, int(total), row.encode()))
        blocks.append(rows)
        at += 4
    return blocks


def parse_block_sequences(text):
    out, key = {}, None
    for ln in text.decode().split("\n"):
        if ln.startswith(">"):
            m = re.match(r">Seq=\"(.*)\",Strand='(.)',Block_id=(\d+),Start=(\d+),End=(\d+)$", ln)
            key = (m.group(1), m.group(2), int(m.group(4)), int(m.group(5)))
            out[key] = []
        elif ln:
            out[key].append(ln)
    return {k: "".join(v).encode() for k, v in out.items()}


def unique_groups(coords_text, nref, min_size):
    groups = {}
    for b, c, s, e in BM.parse_blocks_coords(coords_text):
        groups.setdefault(abs(b), []).append((c, s, e))
    return {b: v for b, v in groups.items()
            if len(v) == 2 and (v[0][0] < nref) != (v[1][0] < nref) and all(e - s >= min_size for _, s, e in v)}


def test_maf_and_variants_of_the_synthetic_pair(tmp_path, capsys):
    ref, copy, subs, edits = synthetic()
    files, out = run_pipeline(tmp_path, ["--maf", "a.maf", "--variants", "v.vcf"])
    assert capsys.readouterr().err == ""                        # no block is skipped
    assert list(files)[-2:] == ["a.maf", "v.vcf"]
    unique = unique_groups(files["blocks_coords.txt"].decode(), 1, 500)
    maf = parse_maf(files["a.maf"])
    assert len(maf) == len(unique) >= 3
    spelled = parse_block_sequences(files["blocks_sequences.fasta"])
    covered = []
    for (name_a, start_a, size_a, strand_a, total_a, row_a), (name_b, start_b, size_b, strand_b, total_b, row_b) in maf:
        assert (name_a, total_a, name_b, total_b) == ("refgenome", len(ref), "assembly", len(copy))
        assert len(row_a) == len(row_b) and strand_a == "+"     # the correction turns the reference instance to '+'
        for name, start, size, strand, total, row in ((name_a, start_a, size_a, strand_a, total_a, row_a), (name_b, start_b, size_b, strand_b, total_b, row_b)):
            s, e = (start, start + size) if strand == "+" else (total - start - size, total - start)
            key = (name, strand, s + 1, e) if strand == "+" else (name, strand, e, s + 1)
            assert row.replace(b"-", b"") == spelled[key], key  # the degapped row is the instance text of blocks_sequences.fasta
        covered.append((start_a, start_a + size_a))
    # ---- variants
    lines = files["v.vcf"].decode().split("\n")
    assert lines[1] == "##source=sibelia_amd" and lines[2] == "##reference=refgenome" and lines[6].startswith("#CHROM\tPOS\t")
    records = [ln.split("\t") for ln in lines[7:-1]]
    assert records and [(r[0], int(r[1])) for r in records] == sorted((r[0], int(r[1])) for r in records)
    for chrom, pos, _, r, a, *rest in records:
        assert chrom == "refgenome" and rest == [".", ".", "."] and len(rest) == 3
        if r != ".":
            assert ref[int(pos) - 1:int(pos) - 1 + len(r)] == r.encode(), (pos, r)
    single = {int(pos): (r, a) for _, pos, _, r, a, *_ in records if len(r) == 1 and len(a) == 1 and r != "." and a != "."}
    others = sorted(list(subs) + [p for p, _ in edits] + [p + n for p, n in edits] + list(SEGMENT))
    checked = 0
    for at, alt in subs.items():
        inside = any(s + 30 <= at < e - 30 for s, e in covered)
        alone = all(abs(at - o) >= 30 for o in others if o != at)
        if inside and alone:
            assert single.get(at + 1) == (chr(ref[at]), chr(alt)), (at, single.get(at + 1))
            checked += 1
    assert checked >= 40, checked


def test_scores_equal_the_rows_and_the_feature_off_run_is_unchanged(tmp_path, capsys):
    from sibelia_amd import BlockFinder
    from sibelia_amd.pipeline import PARAMETER_SETS, final_k
    ref, copy, _, _ = synthetic()
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    with_options, out_on = run_pipeline(tmp_path / "on", ["--maf", "a.maf", "--variants", "v.vcf"])
    without, out_off = run_pipeline(tmp_path / "off", [])
    assert out_on == out_off
    assert list(without) == ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt", "blocks_sequences.fasta"]
    assert without == {k: v for k, v in with_options.items() if k not in ("a.maf", "v.vcf")}      # the options add two files and change nothing else
    # the same stages through the API: the reported score is the score of the rows, and the rows are the ones in the MAF
    bf = BlockFinder([ref, copy], device=0)
    try:
        stages = PARAMETER_SETS["fine"]
        for k, d in stages:
            bf.PerformGraphSimplifications(k, d, 4)
        _, trim_k = final_k(stages, 500, 30)
        bf.GenerateSyntenyBlocks(30, trim_k, 500, False)
        bf.postprocess(["refgenome", "assembly"])
        bf.correct_boundaries(500, 1, ["refgenome", "assembly"])
        ids, descs, aligned = bf.align_unique_blocks(500, 1)
        st = bf.align_stats()
    finally:
        bf.close()
    maf = parse_maf(with_options["a.maf"])
    assert ids == sorted(ids) and len(ids) == len(maf) == st["pairs"] and st["skipped"] == 0
    for al, rows in zip(aligned, maf):
        assert al.status == 0 and (al.row_a, al.row_b) == (rows[0][5], rows[1][5])
        assert al.score == GM.score_of_rows(al.row_a, al.row_b)
        assert sum(n for _, n in al.runs) == len(al.row_a) and al.band_w <= 256


def test_every_unique_block_of_the_staphylococcus_run_is_aligned_or_named(tmp_path, capsys):
    from sibelia_amd import pipeline as P
    case = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "correct_cases.json")))["cases"] if c["name"] == "saureus_fine_inram_m500_correct"][0]
    names = write_inputs(case["input"], str(tmp_path))
    rc, files, _ = P.run(case["args"] + ["--maf", "a.maf", "--variants", "v.vcf", "-o", str(tmp_path / "out")] + [str(tmp_path / n) for n in names])
    assert rc == 0
    err = capsys.readouterr().err
    skipped = [ln for ln in err.split("\n") if ln]
    assert all(re.match(r"block \d+ not aligned: ", ln) for ln in skipped), err[-2000:]
    final = sorted(n for n in files if n.startswith("blocks_coords"))[-1]
    unique = unique_groups(files[final].decode(), 1, case["min_block_size"])
    maf = parse_maf(files["a.maf"])
    print("unique blocks %d, aligned %d, skipped %d" % (len(unique), len(maf), len(skipped)))
    assert len(maf) + len(skipped) == len(unique) and len(maf) >= 1
    named = {int(ln.split()[1]) for ln in skipped}
    assert named <= set(unique) and len(named) == len(skipped)
    spans = {(s, e) for v in unique.values() for c, s, e in v if c == 0}
    for (name, start, size, strand, total, row), other in maf:
        assert strand == "+" and (start, start + size) in spans and len(row) == len(other[5])
