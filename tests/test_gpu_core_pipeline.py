"""--corealignment / --corepartitions / --coresnps / --coresites end to end (sibelia_amd/pipeline.py over csrc/group_concat.hip) on the
seeded three-genome synthetic of tests/test_gpu_multivariants_pipeline.py: all four files rebuilt, on the host, from blocks_coords.txt and
the MAF text the same run wrote, and compared byte by byte."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                        # noqa: E402
from test_gpu_distances_pipeline import genomes3, paragraphs      # noqa: E402
from test_gpu_multivariants_pipeline import ARGS, ARGS3, run_pipeline, synthetic      # noqa: E402

pytestmark = pytest.mark.gpu

NAMES3 = ["refgenome.fa", "assembly.fa", "third.fa"]
CORE = ["--corealignment", "core.fa", "--corepartitions", "parts.tsv", "--coresnps", "snps.fa", "--coresites", "sites.tsv"]
PARTS_HEAD, SITES_HEAD = "block\tfirst\tlast", "column\tblock\trecord\tposition\tstrand"


def wrap(row: str, width=80) -> str:
    return "".join(row[i:i + width] + "\n" for i in range(0, len(row), width))


def rebuild(files, record_names, file_names, maf_name, gap_open=0, min_size=500):
    """the four files from blocks_coords.txt -- which ids are core blocks: one instance in every file (every file here has one record),
    all at least min_size long -- and the paragraphs of the MAF file, which come in ascending id for the ids with two instances of that
    length.  Also the instances of the core blocks, for the checks on the sequences."""
    by_id = {}
    for b, c, s, e in BM.parse_blocks_coords(files["blocks_coords.txt"].decode()):
        by_id.setdefault(abs(b), []).append((c, s, e, b < 0))
    n = len(record_names)
    aligned = sorted(b for b, v in by_id.items() if sum(e - s >= min_size for _, s, e, _ in v) >= 2)
    core = [b for b in aligned if all(e - s >= min_size for _, s, e, _ in by_id[b]) and sorted(c for c, _, _, _ in by_id[b]) == list(range(n))]
    pars = paragraphs(files[maf_name])
    assert len(pars) == len(aligned) and core
    rows, snps = [""] * n, [""] * n
    parts, sites = [], []
    for block, par in zip(aligned, pars):
        if block not in core:
            continue
        assert [name for name, _ in par] == record_names                          # the instances sort by record: the first file's is the centre
        r = [row for _, row in par]
        parts.append("%d\t%d\t%d" % (block, len(rows[0]) + 1, len(rows[0]) + len(r[0])))
        _, s0, e0, rev0 = sorted(by_id[block])[0]
        for x in range(len(r[0])):
            column = [row[x] for row in r]
            if all(ch in "ACGT" for ch in column) and len(set(column)) > 1:
                before = x - r[0][:x].count("-")
                sites.append("%d\t%d\t%s\t%d\t%s" % (len(sites) + 1, block, record_names[0], e0 - before if rev0 else s0 + before + 1, "-" if rev0 else "+"))
                for f in range(n):
                    snps[f] += column[f]
        for f in range(n):
            rows[f] += r[f]
    note = ["# gapopen=%d" % gap_open] if gap_open else []
    out = {"core.fa": "".join(">" + a + "\n" + wrap(row) for a, row in zip(file_names, rows)),
           "snps.fa": "".join(">" + a + "\n" + wrap(row) for a, row in zip(file_names, snps)),
           "parts.tsv": "\n".join(note + [PARTS_HEAD] + parts) + "\n",
           "sites.tsv": "\n".join(note + [SITES_HEAD] + sites) + "\n"}
    return {k: v.encode() for k, v in out.items()}, rows, snps, [sorted(by_id[b]) for b in core]


def fasta_rows(text: bytes, names):
    out = {}
    for record in text.decode().split(">")[1:]:
        head, _, body = record.partition("\n")
        out[head] = body.replace("\n", "")
    assert list(out) == names
    return [out[a] for a in names]


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("core3")
    return run_pipeline(tmp, ARGS3, genomes3(), ["--multimaf", "m.maf"] + CORE)


def test_three_files_give_the_rebuild_of_their_own_maf(three, capsys):
    files, _ = three
    assert list(files)[-5:] == ["m.maf", "core.fa", "parts.tsv", "snps.fa", "sites.tsv"]
    want, rows, snps, insts = rebuild(files, ["refgenome", "assembly", "third"], NAMES3, "m.maf")
    for name in ("core.fa", "parts.tsv", "snps.fa", "sites.tsv"):
        assert files[name] == want[name], name
    assert len(insts) >= 3 and len(rows[0]) > 20000 and 40 < len(snps[0]) <= 100     # the substitutions planted in the copy and in the third genome
    assert not files["core.fa"].startswith(b"#") and max(len(ln) for ln in files["core.fa"].split(b"\n")) == 80
    # every row without its gaps is the concatenation of that file's instances
    genomes = [s for _, s in genomes3()]
    got = fasta_rows(files["core.fa"], NAMES3)
    assert got == rows
    for f in range(3):
        spelled = b"".join(BM.reverse_complement(genomes[f][s:e]) if rev else genomes[f][s:e] for inst in insts for c, s, e, rev in inst if c == f)
        assert got[f].replace("-", "").encode() == spelled
    # every position of sites.tsv names, in the first genome, the base snps.fa shows
    first = fasta_rows(files["snps.fa"], NAMES3)[0]
    lines = files["sites.tsv"].decode().split("\n")[1:-1]
    assert len(lines) == len(first)
    for k, ln in enumerate(lines):
        column, _, record, position, strand = ln.split("\t")
        base = genomes[0][int(position) - 1:int(position)]
        assert int(column) == k + 1 and record == "refgenome" and (base if strand == "+" else BM.reverse_complement(base)) == first[k].encode()


def test_a_run_without_the_options_writes_the_same_other_files(three, tmp_path, capsys):
    files, out = three
    without, out_off = run_pipeline(tmp_path, ARGS3, genomes3(), ["--multimaf", "m.maf"])
    assert capsys.readouterr().err == ""
    assert out == out_off
    assert without == {k: v for k, v in files.items() if k not in ("core.fa", "parts.tsv", "snps.fa", "sites.tsv")}
    assert list(without) == list(files)[:-4]


def test_two_files_with_gapopen_and_the_mismatches_of_distancecounts(tmp_path, capsys):
    ref, copy, _, _ = synthetic()
    files, _ = run_pipeline(tmp_path, ARGS, (("refgenome", ref), ("assembly", copy)), ["--gapopen", "200", "--multimaf", "m.maf", "--distancecounts", "d.tsv"] + CORE)
    assert capsys.readouterr().err == ""
    want, rows, snps, _ = rebuild(files, ["refgenome", "assembly"], NAMES3[:2], "m.maf", gap_open=200)
    for name in ("core.fa", "parts.tsv", "snps.fa", "sites.tsv"):
        assert files[name] == want[name], name
    assert files["parts.tsv"].startswith(b"# gapopen=200\n" + PARTS_HEAD.encode()) and files["sites.tsv"].startswith(b"# gapopen=200\n" + SITES_HEAD.encode())
    assert files["core.fa"].startswith(b">refgenome.fa\n") and files["snps.fa"].startswith(b">refgenome.fa\n")      # the FASTA files carry no such line
    counts = files["d.tsv"].decode().split("\n")[2].split("\t")                    # for two files the blocks of --distancecounts are the core blocks
    assert counts[:2] == NAMES3[:2] and int(counts[4]) == len(snps[0]) > 0
    assert "-" in rows[0] + rows[1]
