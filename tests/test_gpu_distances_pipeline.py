"""--distances / --distancecounts end to end (sibelia_amd/pipeline.py over csrc/group_distances.hip) on the seeded three-genome synthetic of
tests/test_gpu_multivariants_pipeline.py: every count against a recount, on the host, of the MAF text the same run wrote."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                        # noqa: E402
from test_gpu_multivariants_pipeline import ARGS, ARGS3, run_pipeline, synthetic, third_genome      # noqa: E402

pytestmark = pytest.mark.gpu

NAMES3 = ["refgenome.fa", "assembly.fa", "third.fa"]
HEAD = "file_a\tfile_b\tblocks\tmatch\tmismatch\tambiguous\tgap_a\tgap_b"


def genomes3():
    ref, copy, subs, edits = synthetic()
    third, _ = third_genome(ref, subs, edits)
    return (("refgenome", ref), ("assembly", copy), ("third", third))


def paragraphs(maf: bytes):
    """the `s` lines of every paragraph: [(record name, row)]"""
    out = []
    for par in maf.decode().split("\n\n"):
        rows = [ln.split() for ln in par.split("\n") if ln.startswith("s ")]
        if rows:
            out.append([(f[1], f[6]) for f in rows])
    return out


def recount(files, record_names, maf_name, min_size=500):
    """(counts[a][b] = [match, mismatch, ambiguous, gap(a -> b)], blocks[a][b]) from blocks_coords.txt -- which ids are used: at least two
    instances, all of them at least min_size long, at most one per file (every file here has one record) -- and the paragraphs of the
    MAF file, which come in ascending id for the ids with two instances of that length"""
    by_id = {}
    for b, c, s, e in BM.parse_blocks_coords(files["blocks_coords.txt"].decode()):
        by_id.setdefault(abs(b), []).append((c, e - s))
    aligned = sorted(b for b, v in by_id.items() if sum(n >= min_size for _, n in v) >= 2)
    used = {b for b, v in by_id.items() if len(v) >= 2 and all(n >= min_size for _, n in v) and len({c for c, _ in v}) == len(v)}
    pars = paragraphs(files[maf_name])
    assert len(pars) == len(aligned) and used
    n = len(record_names)
    counts = [[[0, 0, 0, 0] for _ in range(n)] for _ in range(n)]
    blocks = [[0] * n for _ in range(n)]
    for block, par in zip(aligned, pars):
        if block not in used:
            continue
        rows = {record_names.index(name): row for name, row in par}
        assert len(rows) == len(par) == len(by_id[block])
        for a, x in rows.items():
            for b, y in rows.items():
                if a == b:
                    continue
                blocks[a][b] += 1
                for p, q in zip(x, y):
                    if p == "-" or q == "-":
                        counts[a][b][3] += p != "-" and q == "-"
                    elif p in "ACGT" and q in "ACGT":
                        counts[a][b][0 if p == q else 1] += 1
                    else:
                        counts[a][b][2] += 1
    return counts, blocks


def counts_lines(names, counts, blocks):
    return ["\t".join([names[a], names[b]] + [str(v) for v in [blocks[a][b]] + counts[a][b] + [counts[b][a][3]]])
            for a in range(len(names)) for b in range(a + 1, len(names))]


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("distances3")
    return run_pipeline(tmp, ARGS3, genomes3(), ["--multimaf", "m.maf", "--distances", "d.phy", "--distancecounts", "d.tsv"])


def test_three_files_give_the_recount_of_their_own_maf(three, capsys):
    from sibelia_amd import formats
    files, _ = three
    assert list(files)[-3:] == ["m.maf", "d.phy", "d.tsv"]
    counts, blocks = recount(files, ["refgenome", "assembly", "third"], "m.maf")
    lines = files["d.tsv"].decode().split("\n")
    assert lines[0] == HEAD and lines[-1] == "" and lines[1:-1] == counts_lines(NAMES3, counts, blocks)
    assert files["d.phy"] == formats.distances_text(NAMES3, counts)
    assert files["d.phy"].decode().split("\n")[0] == "3" and "nan" not in files["d.phy"].decode()
    assert 0 < counts[0][1][1] <= 60 and 0 < counts[0][2][1] <= 40                # the substitutions planted in the copy and in the third genome
    assert blocks[0][1] >= 3 and blocks[0][2] >= 3 and counts[0][1][0] > 20000
    assert counts[0][1][:3] == counts[1][0][:3]


def test_the_counts_alone_and_a_run_without_the_options(three, tmp_path, capsys):
    files, out = three
    (tmp_path / "alone").mkdir(); (tmp_path / "off").mkdir()
    alone, out_alone = run_pipeline(tmp_path / "alone", ARGS3, genomes3(), ["--distancecounts", "d.tsv"])
    assert list(alone)[-1] == "d.tsv" and alone["d.tsv"] == files["d.tsv"] and "d.phy" not in alone and "m.maf" not in alone
    without, out_off = run_pipeline(tmp_path / "off", ARGS3, genomes3(), ["--multimaf", "m.maf"])
    assert capsys.readouterr().err == ""
    assert out == out_off == out_alone
    assert without == {k: v for k, v in files.items() if k not in ("d.phy", "d.tsv")}
    assert {k: v for k, v in alone.items() if k != "d.tsv"} == {k: v for k, v in without.items() if k != "m.maf"}


def test_two_files_with_gapopen_record_it_and_count_that_run(tmp_path, capsys):
    ref, copy, _, _ = synthetic()
    files, _ = run_pipeline(tmp_path, ARGS, (("refgenome", ref), ("assembly", copy)), ["--gapopen", "200", "--multimaf", "m.maf", "--distancecounts", "d.tsv"])
    assert capsys.readouterr().err == ""
    assert files["m.maf"].startswith(b"##maf version=1\n# gapopen=200\n")
    counts, blocks = recount(files, ["refgenome", "assembly"], "m.maf")
    lines = files["d.tsv"].decode().split("\n")
    assert lines[:2] == ["# gapopen=200", HEAD] and lines[-1] == "" and lines[2:-1] == counts_lines(NAMES3[:2], counts, blocks)
    assert 0 < counts[0][1][1] <= 60 and counts[0][1][3] + counts[1][0][3] > 0
