"""--coreconsensus / --coreboottrees and their filtered twins end to end (sibelia_amd/pipeline.py over csrc/group_boot.hip, csrc/tree_nj.hip
and sibelia_amd/tree.py) on the four genomes of tests/test_gpu_tree_pipeline.py: the two tree files stay what they were, and the four new
files are what tree.py's host path makes, without the device's neighbour joining, from the counts rebuilt from the alignment and SNP
texts the same run wrote -- byte for byte."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_core_pipeline import CORE            # noqa: E402
from test_gpu_density_pipeline import DENSE, T, W  # noqa: E402
from test_gpu_multivariants_pipeline import ARGS3, run_pipeline      # noqa: E402
from test_gpu_tree_pipeline import B, NAMES4, TREES, genomes4, rebuilt_tree      # noqa: E402

pytestmark = pytest.mark.gpu

DENSITY = ["--densitywindow", str(W), "--densitymax", str(T)]
REPLICATES = ["--coreconsensus", "c.nwk", "--corefilteredconsensus", "fc.nwk", "--coreboottrees", "b.nwk", "--corefilteredboottrees", "fb.nwk"]
NEW = ("c.nwk", "fc.nwk", "b.nwk", "fb.nwk")


@pytest.fixture(scope="module")
def six4(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("six4")
    return run_pipeline(tmp, ARGS3, genomes4(), CORE + DENSE + DENSITY + TREES + REPLICATES)


def test_the_six_tree_files_of_four_genomes(six4, capsys):
    from sibelia_amd import tree
    files, _ = six4
    assert list(files)[-14:] == ["core.fa", "parts.tsv", "snps.fa", "sites.tsv", "f.fa", "fs.fa", "fs.tsv", "d.tsv", "t.nwk", "ft.nwk"] + list(NEW)
    for alignment, snps, main, majority, lines in (("core.fa", "snps.fa", "t.nwk", "c.nwk", "b.nwk"), ("f.fa", "fs.fa", "ft.nwk", "fc.nwk", "fb.nwk")):
        want, counts, K, C = rebuilt_tree(files[alignment], files[snps])
        assert files[main] == want                                               # as before: the supports did not move
        host = tree.tree_files(counts, K, "p", NAMES4)                           # nj=None: neighbour_joining on the host
        assert (files[main], files[majority], files[lines]) == tuple(s.encode() for s in host)
        # not vacuous: the planted clade of the third and fourth file is in the consensus, and the replicates are not all one tree
        s = files[majority].decode()
        assert s.count("\n") == 1 and s.startswith("(refgenome.fa:") and s.endswith(");\n")
        label = re.search(r"\(third\.fa:[0-9.]+,fourth\.fa:[0-9.]+\)(\d+):", s)
        assert label and int(label.group(1)) > 50
        reps = files[lines].decode().split("\n")
        assert len(reps) == B + 1 and reps[-1] == "" and len(set(reps[:B])) > 1
        assert all(r.startswith("(refgenome.fa:") and r.endswith(");") and not re.search(r"\)\d", r) for r in reps[:B])
    assert files["c.nwk"] != files["fc.nwk"] and files["b.nwk"] != files["fb.nwk"]


def test_the_consensus_alone_runs(six4, tmp_path, capsys):
    files, _ = six4
    alone, _ = run_pipeline(tmp_path, ARGS3, genomes4(), ["--coreconsensus", "c.nwk", "--bootstrap", str(B)])
    assert capsys.readouterr().err == "" and list(alone)[-1] == "c.nwk" and "t.nwk" not in alone and "core.fa" not in alone
    assert alone["c.nwk"] == files["c.nwk"]
    (tmp_path / "m").mkdir()
    masked, _ = run_pipeline(tmp_path / "m", ARGS3, genomes4(), ["--corefilteredboottrees", "fb.nwk", "--bootstrap", str(B)] + DENSITY)
    assert list(masked)[-1] == "fb.nwk" and masked["fb.nwk"] == files["fb.nwk"]


def test_a_run_without_the_new_options_writes_the_files_it_wrote(six4, tmp_path, capsys):
    files, out = six4
    without, out_off = run_pipeline(tmp_path, ARGS3, genomes4(), CORE + DENSE + DENSITY + TREES)
    assert capsys.readouterr().err == ""
    assert out == out_off
    assert without == {k: v for k, v in files.items() if k not in NEW}
    assert list(without) == list(files)[:-4] and {"t.nwk", "ft.nwk", "core.fa", "fs.fa"} <= set(without)
