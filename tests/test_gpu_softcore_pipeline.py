"""--coremin / --corepresence end to end (sibelia_amd/pipeline.py over the partial instantiations of csrc/group_concat.hip and
csrc/group_boot.hip) on the seeded three-genome synthetic of tests/test_gpu_core_pipeline.py with one block's worth of
sequence cut out of the third genome: every file rebuilt, on the host, from blocks_coords.txt and the MAF text the same run wrote, and
compared byte by byte; the tree through tests/softcore_model.py and sibelia_amd/tree.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BOOT                          # noqa: E402
import boundary_model as BM                        # noqa: E402
import softcore_model as SM                        # noqa: E402
import gmask_model as KM                           # noqa: E402
from test_gpu_core_pipeline import NAMES3, PARTS_HEAD, SITES_HEAD, rebuild as strict_rebuild, wrap      # noqa: E402
from test_gpu_density_pipeline import DENSE, DENSE_HEAD, NEW, T, W, genomes_dense, rebuild as strict_dense_rebuild      # noqa: E402
from test_gpu_distances_pipeline import paragraphs      # noqa: E402
from test_gpu_multivariants_pipeline import ARGS3, SEGMENT, run_pipeline      # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = ["refgenome", "assembly", "third"]
FILES = ["--corealignment", "core.fa", "--corepartitions", "parts.tsv", "--coresnps", "snps.fa", "--coresites", "sites.tsv", "--corepresence", "presence.tsv"] + DENSE
TREE = ["--coretree", "tree.nwk", "--corefilteredtree", "ftree.nwk", "--bootstrap", "20", "--densitywindow", str(W), "--densitymax", str(T)]
MADE = ("core.fa", "parts.tsv", "snps.fa", "sites.tsv", "f.fa", "fs.fa", "fs.tsv", "d.tsv", "presence.tsv", "tree.nwk", "ftree.nwk")
TABLES = ("parts.tsv", "sites.tsv", "fs.tsv", "d.tsv", "presence.tsv")


def cut_genomes():
    """the three genomes -- the third with the cluster of substitutions of tests/test_gpu_density_pipeline.py -- with the segment the
    second one holds reversed, a block of its own, cut out of the third"""
    ref, copy, third = genomes_dense()
    s, e = SEGMENT
    return ref, copy, ("third", third[1][:s] + third[1][e:])


def concatenated(blocks, n):
    """rows, SNP rows and the lines of the two tables from [(block, the files it holds in row order, its rows, its centre instance)]"""
    rows, snps, parts, sites = [""] * n, [""] * n, [], []
    for block, here, r, (s0, e0, rev0) in blocks:
        parts.append("%d\t%d\t%d" % (block, len(rows[0]) + 1, len(rows[0]) + len(r[0])))
        for x in range(len(r[0])):
            column = [row[x] for row in r]
            if all(ch in "ACGT" for ch in column) and len(set(column)) > 1:
                before = x - r[0][:x].count("-")
                sites.append("%d\t%d\t%s\t%d\t%s" % (len(sites) + 1, block, RECORDS[0], e0 - before if rev0 else s0 + before + 1, "-" if rev0 else "+"))
                for f in range(n):
                    snps[f] += column[here.index(f)] if f in here else "-"
        for f in range(n):
            rows[f] += r[here.index(f)] if f in here else "-" * len(r[0])
    return rows, snps, parts, sites


def tree_of(blocks, n, nsites, replicates, seed):
    from sibelia_amd import tree
    M, C, _, clean = SM.counts_partial([[row.encode() for row in r] for _, _, r, _ in blocks], [f for _, here, _, _ in blocks for f in here], n, replicates, seed)
    assert C == nsites
    return tree.tree_text(M, clean, "p", NAMES3)


def rebuild(files, coremin, maf_name="m.maf", min_size=500, replicates=20, seed=1):
    """the files of a --coremin run from blocks_coords.txt -- which ids are soft-core blocks: every instance at least min_size long,
    exactly one in the first file, at most one in each other (every file here has one record), at least `coremin` files; written with
    the `# coremin=` line where coremin is below the number of files -- and the paragraphs of the MAF file, masked by
    tests/gmask_model.py for the files of the density filter.  Also how many files every used block holds, and the used blocks."""
    by_id = {}
    for b, c, s, e in BM.parse_blocks_coords(files["blocks_coords.txt"].decode()):
        by_id.setdefault(abs(b), []).append((c, s, e, b < 0))
    n = len(RECORDS)
    aligned = sorted(b for b, v in by_id.items() if sum(e - s >= min_size for _, s, e, _ in v) >= 2)
    held = {b: sorted(c for c, _, _, _ in v) for b, v in by_id.items()}
    core = [b for b in aligned if all(e - s >= min_size for _, s, e, _ in by_id[b]) and held[b].count(0) == 1 and len(set(held[b])) == len(held[b]) >= coremin]
    pars = paragraphs(files[maf_name])
    assert len(pars) == len(aligned) and core
    plain, hidden, presence, dense, at = [], [], [], [], 0
    for block, par in zip(aligned, pars):
        if block not in core:
            continue
        here = [RECORDS.index(name) for name, _ in par]
        assert here == held[block] and here[0] == 0                                  # the instances sort by record: the first file's is the centre
        r = [row for _, row in par]
        _, s0, e0, rev0 = sorted(by_id[block])[0]
        plain.append((block, here, r, (s0, e0, rev0)))
        intervals, masked = KM.mask([[row.encode() for row in r]], W, T)
        hidden.append((block, here, [row.decode() for row in masked[0]], (s0, e0, rev0)))
        place = lambda before: e0 - before if rev0 else s0 + before + 1           # noqa: E731
        for _, row, first, last, bf, bl, ndiff in intervals:
            lo, hi = sorted((place(bf), place(bl)))
            dense.append("%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d" % (NAMES3[here[row]], block, RECORDS[0], lo, hi, "-" if rev0 else "+", ndiff, at + first + 1, at + last + 1))
        at += len(r[0])
        presence.append("\t".join(["%d" % block] + ["1" if f in here else "0" for f in range(n)]))
    rows, snps, parts, sites = concatenated(plain, n)
    frows, fsnps, _, fsites = concatenated(hidden, n)
    note = ["# coremin=%d" % coremin] if coremin < n else []
    fasta = lambda rs: "".join(">" + a + "\n" + wrap(row) for a, row in zip(NAMES3, rs))      # noqa: E731
    out = {"core.fa": fasta(rows), "snps.fa": fasta(snps), "f.fa": fasta(frows), "fs.fa": fasta(fsnps),
           "parts.tsv": "\n".join(note + [PARTS_HEAD] + parts) + "\n",
           "sites.tsv": "\n".join(note + [SITES_HEAD] + sites) + "\n",
           "fs.tsv": "\n".join(note + [SITES_HEAD] + fsites) + "\n",
           "d.tsv": "\n".join(["# densitywindow=%d densitymax=%d" % (W, T)] + note + [DENSE_HEAD] + dense) + "\n",
           "presence.tsv": "\n".join(note + ["\t".join(["block"] + NAMES3)] + presence) + "\n",
           "tree.nwk": tree_of(plain, n, len(snps[0]), replicates, seed), "ftree.nwk": tree_of(hidden, n, len(fsnps[0]), replicates, seed)}
    assert dense and len(fsnps[0]) < len(snps[0])                                    # the planted cluster is masked
    return {k: v.encode() for k, v in out.items()}, [len(here) for _, here, _, _ in plain], plain


@pytest.fixture(scope="module")
def cut(tmp_path_factory):
    """the cut genomes: without --coremin, with --coremin 3 and with --coremin 2"""
    runs = {}
    for coremin in (None, 3, 2):
        tmp = tmp_path_factory.mktemp("softcore%s" % coremin)
        runs[coremin] = run_pipeline(tmp, ARGS3, cut_genomes(), ["--multimaf", "m.maf"] + FILES + TREE + (["--coremin", str(coremin)] if coremin else []))
    return runs


def test_coremin_2_gives_the_rebuild_of_its_own_maf(cut, capsys):
    files, _ = cut[2]
    assert list(files)[-12:] == ["m.maf"] + list(MADE)
    want, nheld, _ = rebuild(files, 2)
    for name in MADE:
        assert files[name] == want[name], name
    assert 2 in nheld and 3 in nheld                                                 # a used block lacks the third file and one holds all three
    assert b"\t1\t1\t0\n" in files["presence.tsv"] and b"\t1\t1\t1\n" in files["presence.tsv"]
    for name in TABLES:
        assert files[name].startswith(b"# densitywindow=60 densitymax=2\n# coremin=2\n" if name == "d.tsv" else b"# coremin=2\n"), name
    third = files["core.fa"].split(b">third.fa\n")[1].replace(b"\n", b"")
    assert third.count(b"-") >= SEGMENT[1] - SEGMENT[0] - 200 and files["core.fa"].startswith(b">refgenome.fa\n")
    assert files["tree.nwk"] != files["ftree.nwk"]


def test_the_default_and_coremin_3_are_the_strict_core(cut, capsys):
    from sibelia_amd import tree
    (off, out_off), (three, out_three) = cut[None], cut[3]
    assert off == three and out_off == out_three
    want, _, snps, _ = strict_rebuild(off, RECORDS, NAMES3, "m.maf")
    for name in ("core.fa", "parts.tsv", "snps.fa", "sites.tsv"):
        assert off[name] == want[name], name
    want, _, _, _ = strict_dense_rebuild(off, RECORDS, NAMES3, "m.maf")
    for name in NEW:
        assert off[name] == want[name], name
    soft, nheld, plain = rebuild(off, 3)
    assert set(nheld) == {3} and all(off[name] == soft[name] for name in MADE)
    groups, cls = [[row.encode() for row in r] for _, _, r, _ in plain], [0, 1, 2] * len(plain)
    M, C, K = BOOT.counts(groups, cls, 3, 20, 1)
    assert C == len(snps[0]) and off["tree.nwk"].decode() == tree.tree_text(M, K, "p", NAMES3)
    assert not any(b"coremin" in off[name] for name in TABLES)
    assert len(off["core.fa"]) < len(cut[2][0]["core.fa"])                           # the soft core holds a block more


def test_whole_genomes_with_coremin_2_give_the_strict_files_and_the_comment_lines(tmp_path_factory, capsys):
    strict, _ = run_pipeline(tmp_path_factory.mktemp("whole"), ARGS3, genomes_dense(), ["--multimaf", "m.maf"] + FILES + TREE)
    soft, _ = run_pipeline(tmp_path_factory.mktemp("whole2"), ARGS3, genomes_dense(), ["--multimaf", "m.maf"] + FILES + TREE + ["--coremin", "2"])
    assert capsys.readouterr().err == ""
    assert list(strict) == list(soft)
    for name in strict:
        want = strict[name]
        if name in TABLES:                                                           # the line comes after the parameters of --coredense
            head, _, rest = want.partition(b"\n") if name == "d.tsv" else (b"", b"", want)
            want = (head + b"\n" if head else b"") + b"# coremin=2\n" + rest
        assert soft[name] == want, name
    assert strict["presence.tsv"].count(b"\t1\t1\t1\n") == strict["presence.tsv"].count(b"\n") - 1 >= 3
