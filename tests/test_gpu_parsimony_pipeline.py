"""--corebranches / --corebranchsites / --coresnptree and their filtered twins end to end (sibelia_amd/pipeline.py over
csrc/group_boot.hip, csrc/tree_nj.hip and csrc/group_parsimony.hip) on the four genomes of tests/test_gpu_tree_pipeline.py: the three files
rebuilt on the host by tests/parsimony_model.py from the SNP FASTA, the sites table and the Newick text the same run wrote, byte for
byte; once more on the soft core of three genomes of which one lacks a block."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parsimony_model as PM                       # noqa: E402
from test_gpu_core_pipeline import NAMES3          # noqa: E402
from test_gpu_density_pipeline import T, W         # noqa: E402
from test_gpu_multivariants_pipeline import ARGS3, run_pipeline      # noqa: E402
from test_gpu_softcore_pipeline import cut_genomes      # noqa: E402
from test_gpu_tree_pipeline import NAMES4, genomes4      # noqa: E402

pytestmark = pytest.mark.gpu

DENSITY = ["--densitywindow", str(W), "--densitymax", str(T)]
PLAIN = ["--coresnps", "snps.fa", "--coresites", "sites.tsv", "--coretree", "t.nwk", "--bootstrap", "20"]
MAPPED = ["--corebranches", "b.tsv", "--corebranchsites", "s.tsv", "--coresnptree", "n.nwk"]
MASKED = ["--corefilteredsnps", "fs.fa", "--corefilteredsites", "fs.tsv", "--corefilteredtree", "ft.nwk"]
FMAPPED = ["--corefilteredbranches", "fb.tsv", "--corefilteredbranchsites", "fbs.tsv", "--corefilteredsnptree", "fn.nwk"]


def rebuilt(files, snps, sites, newick, names):
    """the three files of one kind of rows from the run's own SNP FASTA, sites table and Newick text"""
    table, comments = PM.branch_sites_text(files[snps], files[newick], files[sites], names)
    return PM.branches_text(files[snps], files[newick], names, comments), table, PM.snp_tree_text(files[snps], files[newick], names)


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    return run_pipeline(tmp_path_factory.mktemp("branches4"), ARGS3, genomes4(), PLAIN + MAPPED + MASKED + FMAPPED + DENSITY)


def test_the_three_files_of_four_genomes(four, capsys):
    files, _ = four
    assert list(files)[-12:] == ["snps.fa", "sites.tsv", "fs.fa", "fs.tsv", "t.nwk", "ft.nwk", "b.tsv", "fb.tsv", "s.tsv", "fbs.tsv", "n.nwk", "fn.nwk"]
    assert (files["b.tsv"], files["s.tsv"], files["n.nwk"]) == rebuilt(files, "snps.fa", "sites.tsv", "t.nwk", NAMES4)
    # not vacuous: five branches, the planted clade of the third and fourth file with its label and changes of its own, no comment line but the summary
    lines = files["b.tsv"].decode().split("\n")
    assert lines[0].startswith("# sites=") and lines[1].startswith("branch\t") and len(lines) == 2 + 5 + 1
    clade = [x.split("\t") for x in lines[2:7] if x.split("\t")[1] == "third.fa,fourth.fa"]
    assert len(clade) == 1 and int(clade[0][3]) > 50 and int(clade[0][4]) > 0
    assert [x.split("\t")[3] for x in lines[2:7]].count(".") == 4
    assert sum(int(x.split("\t")[4]) for x in lines[2:7]) == files["s.tsv"].count(b"\n") - 2 >= 80


def test_the_filtered_trio_of_four_genomes(four, capsys):
    files, _ = four
    assert (files["fb.tsv"], files["fbs.tsv"], files["fn.nwk"]) == rebuilt(files, "fs.fa", "fs.tsv", "ft.nwk", NAMES4)
    assert files["fb.tsv"] != files["b.tsv"] and files["fbs.tsv"].count(b"\n") < files["s.tsv"].count(b"\n")      # the mask took sites away


def test_the_files_alone_and_a_run_without_them(four, tmp_path, capsys):
    files, out = four
    alone, _ = run_pipeline(tmp_path, ARGS3, genomes4(), MAPPED + ["--bootstrap", "20"])
    assert capsys.readouterr().err == "" and list(alone)[-3:] == ["b.tsv", "s.tsv", "n.nwk"] and "t.nwk" not in alone and "snps.fa" not in alone
    assert all(alone[f] == files[f] for f in ("b.tsv", "s.tsv", "n.nwk"))
    (tmp_path / "w").mkdir()
    without, out_off = run_pipeline(tmp_path / "w", ARGS3, genomes4(), PLAIN + MASKED + DENSITY)
    new = ("b.tsv", "fb.tsv", "s.tsv", "fbs.tsv", "n.nwk", "fn.nwk")
    assert out == out_off and without == {k: v for k, v in files.items() if k not in new} and list(without) == list(files)[:-6]


def test_the_soft_core_of_three_genomes_of_which_one_lacks_a_block(tmp_path, capsys):
    files, _ = run_pipeline(tmp_path, ARGS3, cut_genomes(), PLAIN + MAPPED + ["--coremin", "2"])
    assert capsys.readouterr().err == ""
    want = rebuilt(files, "snps.fa", "sites.tsv", "t.nwk", NAMES3)
    assert (files["b.tsv"], files["s.tsv"], files["n.nwk"]) == want
    assert files["b.tsv"].startswith(b"# coremin=2\n# sites=") and files["s.tsv"].startswith(b"# coremin=2\n# sites=")
    third = PM.fasta_rows(files["snps.fa"], NAMES3)[2]
    assert 0 < third.count(b"-") < len(third)                                    # sites of blocks the third file lacks, and sites it holds
    # an absent file carries no change: every change on the third file's branch lies in a column it holds
    branch = [x.split("\t")[0] for x in files["b.tsv"].decode().split("\n")[3:6] if x.split("\t")[1] == "third.fa"]
    columns = [int(x.split("\t")[0]) for x in files["s.tsv"].decode().split("\n")[3:-1] if x.split("\t")[5] == branch[0]]
    assert columns and all(third[c - 1:c] != b"-" for c in columns)
