"""--coretree / --corefilteredtree end to end (sibelia_amd/pipeline.py over csrc/group_boot.hip and sibelia_amd/tree.py) on the three
genomes of tests/test_gpu_density_pipeline.py and a fourth one, a copy of the third with substitutions of its own -- so the third and the
fourth are a clade and the tree of four files has its one inner branch: both files rebuilt, on the host, from the alignment and SNP
texts the same run wrote with tests/boot_model.py and tree.py, and compared byte by byte."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BM                            # noqa: E402
import gmask_cases as KC                           # noqa: E402
from test_gpu_core_pipeline import CORE, fasta_rows      # noqa: E402
from test_gpu_density_pipeline import DENSE, T, W, genomes_dense, planted_at      # noqa: E402
from test_gpu_multivariants_pipeline import ARGS3, SEGMENT, run_pipeline, synthetic, third_genome      # noqa: E402

pytestmark = pytest.mark.gpu

NAMES4 = ["refgenome.fa", "assembly.fa", "third.fa", "fourth.fa"]
TREES = ["--coretree", "t.nwk", "--corefilteredtree", "ft.nwk", "--bootstrap", "100"]
NEW = ("t.nwk", "ft.nwk")
B = 100


def genomes4():
    """the third genome once more with 25 substitutions of its own, at least 120 bases from every other edit"""
    (a, ref), (b, copy), (c, dense) = genomes_dense()
    _, _, subs, edits = synthetic()
    _, mine = third_genome(ref, subs, edits)
    at = planted_at()
    taken = sorted(list(subs) + list(mine) + [p for p, _ in edits] + [p + n for p, n in edits] + list(range(SEGMENT[0], SEGMENT[1] + 1, 100)) + [at, at + 30, 0, len(ref)])
    rng = np.random.default_rng(406)
    own = []
    while len(own) < 25:
        x = int(rng.integers(200, len(ref) - 200))
        if all(abs(x - o) >= 120 for o in taken):
            own.append(x)
            taken.append(x)
    return ((a, ref), (b, copy), (c, dense), ("fourth", KC.subst(dense, own)))


def rebuilt_tree(alignment: bytes, snps: bytes, seed=1, model="p", replicates=B):
    """the Newick text from the two FASTA texts of the run: K from the alignment, every slab of counts from the SNP matrix"""
    from sibelia_amd import tree
    full = np.array([np.frombuffer(r.encode(), dtype=np.uint8) for r in fasta_rows(alignment, NAMES4)])
    K = int(np.isin(full, np.frombuffer(b"ACGT", dtype=np.uint8)).all(axis=0).sum())
    S = np.array([np.frombuffer(r.encode(), dtype=np.uint8) for r in fasta_rows(snps, NAMES4)]).reshape(4, -1)
    counts = BM.counts_of_sites(S, replicates, seed)
    return tree.tree_text(counts, K, model, NAMES4).encode(), counts, K, S.shape[1]


@pytest.fixture(scope="module")
def trees4(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trees4")
    return run_pipeline(tmp, ARGS3, genomes4(), CORE + DENSE + ["--densitywindow", str(W), "--densitymax", str(T)] + TREES)


def test_four_files_give_the_trees_of_their_own_alignments(trees4, capsys):
    import re
    files, _ = trees4
    assert list(files)[-10:] == ["core.fa", "parts.tsv", "snps.fa", "sites.tsv", "f.fa", "fs.fa", "fs.tsv", "d.tsv"] + list(NEW)
    plain, counts, K, C = rebuilt_tree(files["core.fa"], files["snps.fa"])
    masked, fcounts, fK, fC = rebuilt_tree(files["f.fa"], files["fs.fa"])
    assert files["t.nwk"] == plain and files["ft.nwk"] == masked
    # not vacuous: sites, replicates that differ, a mask that took columns away, and the planted clade with support above half
    assert C > 80 and 0 < fC < C and fK < K and counts[1].tolist() != counts[2].tolist()
    for text in (plain, masked):
        s = text.decode()
        assert s.count("\n") == 1 and s.endswith(");\n") and s.startswith("(refgenome.fa:")
        label = re.search(r"\(third\.fa:[0-9.]+,fourth\.fa:[0-9.]+\)(\d+):", s)
        assert label and int(label.group(1)) > 50


def test_a_run_without_the_options_writes_the_same_other_files(trees4, tmp_path, capsys):
    files, out = trees4
    without, out_off = run_pipeline(tmp_path, ARGS3, genomes4(), CORE + DENSE + ["--densitywindow", str(W), "--densitymax", str(T)])
    assert capsys.readouterr().err == ""
    assert out == out_off
    assert without == {k: v for k, v in files.items() if k not in NEW}
    assert list(without) == list(files)[:-2] and {"core.fa", "snps.fa", "f.fa", "fs.fa"} <= set(without)


def test_the_filtered_tree_alone_with_a_seed_and_the_correction(trees4, tmp_path, capsys):
    files, _ = trees4
    alone, _ = run_pipeline(tmp_path, ARGS3, genomes4(), ["--corefilteredtree", "ft.nwk", "--densitywindow", str(W), "--densitymax", str(T), "--bootstrap", "20",
                                                            "--bootseed", "18446744073709551615", "--treemodel", "jc"])
    assert capsys.readouterr().err == "" and list(alone)[-1] == "ft.nwk" and "f.fa" not in alone
    want, _, _, _ = rebuilt_tree(files["f.fa"], files["fs.fa"], seed=2 ** 64 - 1, model="jc", replicates=20)
    assert alone["ft.nwk"] == want and alone["ft.nwk"] != files["ft.nwk"]
