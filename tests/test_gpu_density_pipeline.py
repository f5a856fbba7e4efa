"""--corefiltered / --corefilteredsnps / --corefilteredsites / --coredense end to end (sibelia_amd/pipeline.py over csrc/group_mask.hip
and csrc/group_concat.hip) on the three genomes of tests/test_gpu_core_pipeline.py with a cluster of substitutions planted in the third:
all four files rebuilt, on the host, from blocks_coords.txt and the MAF text the same run wrote with tests/gmask_model.py, and compared
byte by byte."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                        # noqa: E402
import gmask_cases as KC                           # noqa: E402
import gmask_model as KM                           # noqa: E402
from test_gpu_core_pipeline import CORE, NAMES3, SITES_HEAD, wrap      # noqa: E402
from test_gpu_distances_pipeline import genomes3, paragraphs      # noqa: E402
from test_gpu_multivariants_pipeline import ARGS3, SEGMENT, run_pipeline, synthetic, third_genome      # noqa: E402

pytestmark = pytest.mark.gpu

W, T = 60, 2
DENSE = ["--corefiltered", "f.fa", "--corefilteredsnps", "fs.fa", "--corefilteredsites", "fs.tsv", "--coredense", "d.tsv"]
NEW = ("f.fa", "fs.fa", "fs.tsv", "d.tsv")
DENSE_HEAD = "file\tblock\trecord\tfirst\tlast\tstrand\tdifferences\tfirst_column\tlast_column"
OFFSETS = (0, 6, 13, 20, 27)                                                     # 5 substitutions within 30 bases


def planted_at():
    """a place in the reference at least 150 bases from every edit of the other two genomes, the inverted segment and either end"""
    ref, _, subs, edits = synthetic()
    _, mine = third_genome(ref, subs, edits)
    taken = sorted(list(subs) + list(mine) + [p for p, _ in edits] + [p + n for p, n in edits] + list(range(SEGMENT[0], SEGMENT[1], 500)) + [SEGMENT[1], 0, len(ref)])
    return next(at for at in range(3000, len(ref), 100) if all(abs(at - o) >= 150 for o in taken))


def genomes_dense():
    (a, ref), (b, copy), (c, third) = genomes3()
    at = planted_at()
    dense = KC.subst(third, [at + d for d in OFFSETS])
    assert all(dense[at + d] != ref[at + d] for d in OFFSETS) and sum(x != y for x, y in zip(dense, third)) == 5
    return ((a, ref), (b, copy), (c, dense))


def rebuild(files, record_names, file_names, maf_name, gap_open=0, min_size=500):
    """the four files from blocks_coords.txt (the core blocks, as tests/test_gpu_core_pipeline.py picks them) and the paragraphs of the
    MAF file, masked by the model; also the intervals and the number of columns of the unfiltered SNP matrix"""
    by_id = {}
    for b, c, s, e in BM.parse_blocks_coords(files["blocks_coords.txt"].decode()):
        by_id.setdefault(abs(b), []).append((c, s, e, b < 0))
    n = len(record_names)
    aligned = sorted(b for b, v in by_id.items() if sum(e - s >= min_size for _, s, e, _ in v) >= 2)
    core = [b for b in aligned if all(e - s >= min_size for _, s, e, _ in by_id[b]) and sorted(c for c, _, _, _ in by_id[b]) == list(range(n))]
    pars = paragraphs(files[maf_name])
    assert len(pars) == len(aligned) and core
    rows, snps = [""] * n, [""] * n
    sites, dense, found, plain = [], [], [], 0
    for block, par in zip(aligned, pars):
        if block not in core:
            continue
        assert [name for name, _ in par] == record_names
        r = [row.encode() for _, row in par]
        intervals, masked = KM.mask([r], W, T)
        m = [x.decode() for x in masked[0]]
        _, s0, e0, rev0 = sorted(by_id[block])[0]
        place = lambda before: e0 - before if rev0 else s0 + before + 1           # noqa: E731
        for _, row, first, last, bf, bl, ndiff in intervals:
            lo, hi = sorted((place(bf), place(bl)))
            dense.append("%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d" % (file_names[row], block, record_names[0], lo, hi, "-" if rev0 else "+", ndiff,
                                                                   len(rows[0]) + first + 1, len(rows[0]) + last + 1))
            found.append((block, row, first, last, ndiff))
        for x in range(len(m[0])):
            column = [row[x] for row in m]
            plain += all(ch in b"ACGT" for ch in (q[x] for q in r)) and len({q[x] for q in r}) > 1
            if all(ch in "ACGT" for ch in column) and len(set(column)) > 1:
                before = x - m[0][:x].count("-")
                sites.append("%d\t%d\t%s\t%d\t%s" % (len(sites) + 1, block, record_names[0], place(before), "-" if rev0 else "+"))
                for f in range(n):
                    snps[f] += column[f]
        for f in range(n):
            rows[f] += m[f]
    note = ["# gapopen=%d" % gap_open] if gap_open else []
    out = {"f.fa": "".join(">" + a + "\n" + wrap(row) for a, row in zip(file_names, rows)),
           "fs.fa": "".join(">" + a + "\n" + wrap(row) for a, row in zip(file_names, snps)),
           "fs.tsv": "\n".join(note + [SITES_HEAD] + sites) + "\n",
           "d.tsv": "\n".join(["# densitywindow=%d densitymax=%d" % (W, T)] + note + [DENSE_HEAD] + dense) + "\n"}
    return {k: v.encode() for k, v in out.items()}, found, len(snps[0]), plain


@pytest.fixture(scope="module")
def dense3(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dense3")
    return run_pipeline(tmp, ARGS3, genomes_dense(), ["--multimaf", "m.maf"] + CORE + DENSE + ["--densitywindow", str(W), "--densitymax", str(T)])


def test_three_files_give_the_rebuild_of_their_own_maf(dense3, capsys):
    files, _ = dense3
    assert list(files)[-9:] == ["m.maf", "core.fa", "parts.tsv", "snps.fa", "sites.tsv"] + list(NEW)
    want, found, nfiltered, nplain = rebuild(files, ["refgenome", "assembly", "third"], NAMES3, "m.maf")
    for name in NEW:
        assert files[name] == want[name], name
    # not vacuous: the planted cluster is an interval of the third file, and it takes columns out of the SNP matrix
    assert len(found) >= 1 and any(row == 2 and ndiff == 5 and last - first == OFFSETS[-1] for _, row, first, last, ndiff in found)
    snps = len(files["snps.fa"].decode().split(">")[1].partition("\n")[2].replace("\n", ""))
    assert snps == nplain and 0 < nfiltered < snps and nfiltered <= snps - 5
    assert files["f.fa"] != files["core.fa"] and len(files["f.fa"]) == len(files["core.fa"])
    assert files["f.fa"].count(b"N") - files["core.fa"].count(b"N") >= OFFSETS[-1] + 1
    # the table names the planted place on the first genome
    at = planted_at()
    line = next(ln for ln in files["d.tsv"].decode().split("\n")[2:-1] if ln.split("\t")[0] == "third.fa" and ln.split("\t")[6] == "5").split("\t")
    assert line[2] == "refgenome" and (int(line[3]), int(line[4])) == (at + 1, at + OFFSETS[-1] + 1)


def test_a_run_without_the_options_writes_the_same_other_files(dense3, tmp_path, capsys):
    files, out = dense3
    without, out_off = run_pipeline(tmp_path, ARGS3, genomes_dense(), ["--multimaf", "m.maf"] + CORE)
    assert capsys.readouterr().err == ""
    assert out == out_off
    assert without == {k: v for k, v in files.items() if k not in NEW}             # core.fa and snps.fa among them, byte for byte
    assert list(without) == list(files)[:-4] and {"core.fa", "snps.fa"} <= set(without)


def test_the_table_alone_with_gapopen(tmp_path, capsys):
    files, _ = run_pipeline(tmp_path, ARGS3, genomes_dense(), ["--gapopen", "200", "--multimaf", "m.maf", "--coredense", "d.tsv", "--corefilteredsites", "fs.tsv",
                                                                "--densitywindow", str(W), "--densitymax", str(T)])
    assert capsys.readouterr().err == "" and list(files)[-3:] == ["m.maf", "fs.tsv", "d.tsv"]
    want, found, _, _ = rebuild(files, ["refgenome", "assembly", "third"], NAMES3, "m.maf", gap_open=200)
    assert files["d.tsv"] == want["d.tsv"] and files["fs.tsv"] == want["fs.tsv"] and found
    assert files["d.tsv"].startswith(b"# densitywindow=60 densitymax=2\n# gapopen=200\n" + DENSE_HEAD.encode() + b"\n")
