"""--multivariants end to end (sibelia_amd/pipeline.py over csrc/group_variants.hip): on the seeded synthetic pair of
tests/test_gpu_align_pipeline.py (rebuilt here from the same seed) against --variants, and with a third genome against the
substitutions planted in it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                        # noqa: E402

pytestmark = pytest.mark.gpu

ARGS = ["-s", "fine", "-m", "500", "--lastk", "30", "-r", "--correctboundaries", "-q"]
ARGS3 = ["-s", "fine", "-m", "500", "--lastk", "30", "-r", "-q"]
SEGMENT = (21000, 25000)
FORMAT = '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">'


def synthetic():
    """one 40 kbp random record; a copy with 60 substitutions, one 4 kbp segment reverse-complemented and four indels of 1..30 bases"""
    rng = np.random.default_rng(404)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 40000))
    copy = bytearray(ref)
    subs = {}
    for p in range(300, 39700, 650):
        if len(subs) == 60:
            break
        at = p + int(rng.integers(0, 400))
        alt = b"ACGT".replace(ref[at:at + 1], b"")[int(rng.integers(0, 3))]
        copy[at] = alt
        subs[at] = alt
    s, e = SEGMENT
    copy[s:e] = BM.reverse_complement(bytes(copy[s:e]))
    edits = []
    for at, kind in ((33000, "del"), (29000, "ins"), (12000, "del"), (5000, "ins")):
        n = int(rng.integers(1, 31))
        if kind == "del":
            del copy[at:at + n]
        else:
            copy[at:at] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
        edits.append((at, n))
    return ref, bytes(copy), subs, edits


def third_genome(ref, subs, edits):
    """another copy of the reference with 40 substitutions of its own: 20 on positions of the second genome's (7 of them with the same
    base, 13 with another one), 20 elsewhere, at least 100 bases from every other edit"""
    rng = np.random.default_rng(405)
    third = bytearray(ref)
    mine = {}
    shared = [int(p) for p in rng.choice(sorted(subs), 20, replace=False)]
    for i, at in enumerate(shared):
        mine[at] = subs[at] if i < 7 else [x for x in b"ACGT" if x not in (ref[at], subs[at])][int(rng.integers(0, 2))]
    taken = sorted(list(subs) + [p for p, _ in edits] + [p + n for p, n in edits] + list(SEGMENT))
    while len(mine) < 40:
        at = int(rng.integers(200, len(ref) - 200))
        if all(abs(at - o) >= 100 for o in taken):
            mine[at] = b"ACGT".replace(ref[at:at + 1], b"")[int(rng.integers(0, 3))]
            taken.append(at)
    for at, alt in mine.items():
        third[at] = alt
    return bytes(third), mine


def run_pipeline(tmp_path, args, genomes, extra):
    from sibelia_amd import pipeline as P
    fa = []
    for name, s in genomes:
        fa.append(str(tmp_path / (name + ".fa")))
        with open(fa[-1], "wb") as f:
            f.write(b">" + name.encode() + b"\n" + s + b"\n")
    rc, files, out = P.run(args + extra + ["-o", str(tmp_path / "out")] + fa)
    assert rc == 0
    return files, out


def vcf_records(text, header_lines):
    lines = text.decode().split("\n")
    assert lines[-1] == "" and lines[header_lines - 1].startswith("#CHROM\t") and not lines[header_lines].startswith("#")
    return lines[:header_lines], [ln.split("\t") for ln in lines[header_lines:-1]]


def test_two_files_give_the_records_of_variants(tmp_path, capsys):
    ref, copy, _, _ = synthetic()
    files, _ = run_pipeline(tmp_path, ARGS, (("refgenome", ref), ("assembly", copy)), ["--variants", "v.vcf", "--multivariants", "m.vcf"])
    assert capsys.readouterr().err == "" and list(files)[-2:] == ["v.vcf", "m.vcf"]
    head_v, pair = vcf_records(files["v.vcf"], 7)
    head_m, multi = vcf_records(files["m.vcf"], 8)
    assert head_m[:6] == head_v[:6] and head_m[6] == FORMAT and head_m[7] == head_v[6] + "\tFORMAT\tassembly.fa"
    assert len(pair) > 40 and [r[:5] for r in multi] == [r[:5] for r in pair]
    assert all(r[5:] == [".", ".", ".", "GT", "1"] for r in multi)


def test_three_files_give_the_planted_alleles_and_genotypes(tmp_path, capsys):
    ref, copy, subs, edits = synthetic()
    third, mine = third_genome(ref, subs, edits)
    genomes = (("refgenome", ref), ("assembly", copy), ("third", third))
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    files, out_on = run_pipeline(tmp_path / "on", ARGS3, genomes, ["--multivariants", "m.vcf"])
    without, out_off = run_pipeline(tmp_path / "off", ARGS3, genomes, [])
    assert capsys.readouterr().err == ""
    assert out_on == out_off and list(files)[-1] == "m.vcf" and without == {k: v for k, v in files.items() if k != "m.vcf"}
    head, records = vcf_records(files["m.vcf"], 8)
    assert head[6] == FORMAT and head[7].split("\t")[8:] == ["FORMAT", "assembly.fa", "third.fa"]
    assert [(r[0], int(r[1])) for r in records] == sorted((r[0], int(r[1])) for r in records)
    for chrom, pos, _, r, a, *rest in records:
        assert chrom == "refgenome" and rest[:4] == [".", ".", ".", "GT"] and len(rest) == 6
        assert not all(x == r for x in a.split(","))                              # no record has REF equal to all of its ALT alleles
        assert set(rest[4:]) <= {".", "0"} | {str(i + 1) for i in range(len(a.split(",")))}
        if r != ".":
            assert ref[int(pos) - 1:int(pos) - 1 + len(r)] == r.encode(), (pos, r)
    # the qualifying blocks, from the coordinates the run wrote: all instances at least 500 long, one on the first record, at most one on each other
    by_id = {}
    for b, c, s, e in BM.parse_blocks_coords(files["blocks_coords.txt"].decode()):
        by_id.setdefault(abs(b), []).append((c, s, e))
    qualifying = [v for v in by_id.values() if len(v) >= 2 and all(e - s >= 500 for _, s, e in v)
                  and [c for c, _, _ in v].count(0) == 1 and len({c for c, _, _ in v}) == len(v)]
    assert len(qualifying) >= 3 and any(len(v) == 3 for v in qualifying)
    at_pos = {int(r[1]): r for r in records}
    others = sorted(list(subs) + list(mine) + [p for p, _ in edits] + [p + n for p, n in edits] + list(SEGMENT))
    checked = two_alts = shared_alt = 0
    for at in sorted(set(subs) | set(mine)):
        block = [v for v in qualifying if any(c == 0 and s + 30 <= at < e - 30 for c, s, e in v)]
        if not block or not all(abs(at - o) >= 30 for o in others if o != at):
            continue
        has = {c for c, _, _ in block[0]}
        alleles = [(subs.get(at, ref[at]) if 1 in has else None), (mine.get(at, ref[at]) if 2 in has else None)]
        alts = []
        for x in alleles:
            if x is not None and x != ref[at] and x not in alts:
                alts.append(x)
        if not alts:
            continue
        gt = ["." if x is None else "0" if x == ref[at] else str(alts.index(x) + 1) for x in alleles]
        want = ["refgenome", str(at + 1), ".", chr(ref[at]), ",".join(chr(x) for x in alts), ".", ".", ".", "GT"] + gt
        assert at_pos.get(at + 1) == want, (at, at_pos.get(at + 1), want)
        checked += 1
        two_alts += len(alts) == 2
        shared_alt += gt == ["1", "1"]
    # of the 80 planted positions (13 with two ALT alleles, 7 with one shared by both samples) at least half: the test is not vacuous
    assert checked >= 40 and two_alts >= 5 and shared_alt >= 3, (checked, two_alts, shared_alt)
