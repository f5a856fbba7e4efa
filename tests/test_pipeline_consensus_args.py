"""The command line of --coreconsensus / --corefilteredconsensus / --coreboottrees / --corefilteredboottrees (sibelia_amd/pipeline.py), the
settings of the tree with each of them, the file plan and core_files over a stand-in finder: device-free."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import pipeline as P      # noqa: E402
from sibelia_amd import tree as T          # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
OPTIONS = ("--coreconsensus", "--corefilteredconsensus", "--coreboottrees", "--corefilteredboottrees")
FILTERED = ("--corefilteredconsensus", "--corefilteredboottrees")
THREE = ["a/x.fa", "y.fa", "z.fa"]
BOOT = ["--bootstrap", "10"]
PLAN = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]


@pytest.mark.parametrize("option", OPTIONS)
def test_each_file_option_exists_once_with_its_defaults(option):
    actions = [a for a in P.build_parser()._actions if option in a.option_strings]
    assert len(actions) == 1 and actions[0].option_strings == [option] and actions[0].default is None
    assert option + " FILE" in " ".join(P.build_parser().format_help().split())
    o = P.parse_args(BASE + [option, "c.nwk"] + BOOT + THREE)
    assert getattr(o, option[2:]) == "c.nwk" and P.tree_wanted(o) and P.concat_wanted(o) and not P.core_wanted(o)
    assert (o.bootstrap, o.bootseed, o.treemodel, o.gapopen, o.coremin) == (10, 1, "p", 0, 3)
    assert P.density_wanted(o) == (option in FILTERED)                           # the masked rows are made for it
    assert all(getattr(o, x[2:]) is None for x in OPTIONS + ("--coretree", "--corefilteredtree") if x != option)
    off = P.parse_args(BASE + THREE)
    assert all(getattr(off, x[2:]) is None for x in OPTIONS) and not P.tree_wanted(off)


def test_help_says_what_the_files_are():
    text = " ".join(P.build_parser().format_help().split())
    mine = text[text.rindex("--coreconsensus FILE"):text.rindex("--corefilteredconsensus FILE")]
    assert "majority-rule" in mine and "more than half" in mine and "Three or more" in mine and "star" in mine and "64 input files" in mine
    mine = text[text.rindex("--coreboottrees FILE"):text.rindex("--corefilteredboottrees FILE")]
    assert "replicate trees" in mine and "one line each" in mine and "without labels" in mine
    assert "consensus" in text[text.rindex("--bootstrap B"):text.rindex("--bootseed S")]


@pytest.mark.parametrize("option", OPTIONS)
def test_argument_rules_of_each_file_option(option):
    for argv, message in [
            ([option, "c.nwk", "x.fa"] + BOOT, "%s compares files: it needs at least two" % option),
            ([option, "c.nwk", "x.fa", "y.fa"] + BOOT, "%s builds a tree: it needs at least three input files" % option),
            ([option, "c.nwk", "--noblocks"] + BOOT + THREE, "%s needs the synteny blocks: it cannot be combined with --noblocks" % option),
            ([option, "c.nwk", "y.fa", "a/x.fa", "b/x.fa"] + BOOT, "%s names a file by its base name: two files are called x.fa" % option),
            ([option, "coverage_report.txt"] + BOOT + THREE, "%s names a file the program writes itself: coverage_report.txt" % option),
            ([option, "sub/"] + BOOT + THREE, "%s needs a file name, not 'sub/'" % option),
            (["--coretree", "c.out", option, "./c.out"] + BOOT + THREE, "--coretree and %s name the same file: c.out" % option),
            ([option, "c.nwk"] + THREE, "%s is made of the trees of the bootstrap replicates: it needs --bootstrap B with B of 1 or more" % option),
            ([option, "c.nwk", "--bootstrap", "0"] + THREE, "%s is made of the trees of the bootstrap replicates: it needs --bootstrap B with B of 1 or more" % option),
            ([option, "c.nwk", "--coretree", "t.nwk"] + THREE, "%s is made of the trees of the bootstrap replicates: it needs --bootstrap B with B of 1 or more" % option)]:
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + argv)
        assert str(e.value) == message
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + [option, "c.nwk", "x.fa", "dir/a(b.fa", "z.fa"] + BOOT)
    assert str(e.value).startswith("%s names a file by its base name: the name 'a(b.fa' cannot stand in a Newick tree" % option)
    assert P.parse_args(BASE + [option, "c.nwk", "--bootstrap", "1"] + THREE).bootstrap == 1


def test_no_two_of_the_six_share_a_file():
    six = ("--coretree", "--corefilteredtree") + OPTIONS
    for i, a in enumerate(six):
        for b in six[i + 1:]:
            with pytest.raises(P.PipelineError) as e:
                P.parse_args(BASE + [b, "t.nwk", a, "t.nwk"] + BOOT + THREE)
            assert str(e.value) == "%s and %s name the same file: t.nwk" % (a, b)


@pytest.mark.parametrize("option", OPTIONS)
def test_the_settings_are_accepted_with_each_alone(option):
    o = P.parse_args(BASE + [option, "c.nwk", "--bootstrap", "7", "--bootseed", "9", "--treemodel", "jc", "--gapopen", "400", "--wideband", "--coremin", "2"] + THREE)
    assert (o.bootstrap, o.bootseed, o.treemodel, o.gapopen, o.wideband, o.coremin) == (7, 9, "jc", 400, True, 2)
    for setting in ("--densitywindow", "--densitymax"):                         # the density settings go with the filtered ones alone
        if option in FILTERED:
            assert getattr(P.parse_args(BASE + [option, "c.nwk", setting, "60"] + BOOT + THREE), setting[2:]) == 60
        else:
            with pytest.raises(P.PipelineError) as e:
                P.parse_args(BASE + [option, "c.nwk", setting, "60"] + BOOT + THREE)
            assert str(e.value).startswith("%s sets the density filter: it needs at least one of --corefiltered," % setting)


def test_a_setting_alone_keeps_its_refusal():
    for setting, value in (("--bootstrap", "7"), ("--bootseed", "7"), ("--treemodel", "jc")):
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + ["--coresnps", "s.fa", setting, value] + THREE)
        assert str(e.value) == "%s is a setting of the tree: it needs at least one of --coretree and --corefilteredtree" % setting


def test_the_new_files_are_planned_last():
    plan = lambda argv: P.planned_files(P.parse_args(BASE + argv + THREE), 3)      # noqa: E731
    assert P.FILE_OPTIONS[-2:] == P.TREE_OPTIONS and P.ALL_FILE_OPTIONS == P.FILE_OPTIONS + P.REPLICATE_OPTIONS
    assert [o for o, _ in P.REPLICATE_OPTIONS] == list(OPTIONS) and P.GROUP_OPTIONS[-4:] == P.REPLICATE_OPTIONS
    assert plan(["--corefilteredboottrees", "fb.nwk", "--coreboottrees", "b.nwk", "--corefilteredconsensus", "fc.nwk", "--coreconsensus", "c.nwk"] + BOOT) == PLAN + ["c.nwk", "fc.nwk", "b.nwk", "fb.nwk"]
    assert plan(["--coreboottrees", "sub/b.nwk", "--corefilteredtree", "ft.nwk", "--coreconsensus", "c.nwk", "--coretree", "t.nwk", "--coredense", "d.tsv", "--corealignment", "c.fa",
                 "--multimaf", "m.maf", "-q", "-g"] + BOOT) == PLAN + ["blocks_sequences.fasta", "m.maf", "c.fa", "d.tsv", "t.nwk", "ft.nwk", "c.nwk", "sub/b.nwk", "de_bruijn_graph.dot"]
    assert plan(["--coretree", "t.nwk"] + BOOT) == PLAN + ["t.nwk"]


class FakeFinder:
    """what core_files asks of a BlockFinder for the trees, recorded: four files of one record, counts that differ between the replicates;
    nj_batch joins on the host the way the device does"""

    def __init__(self, sites=5, clean=100):
        self.file_records = [1, 1, 1, 1]
        self.calls, self.sites, self.clean = [], sites, clean

    def set_masked(self, on):
        self.calls.append(("set_masked", bool(on)))

    def group_mask(self, window, max_diff, want):
        self.calls.append(("group_mask",))
        return []

    def group_bootstrap(self, cls, n, replicates, seed, draws, want):
        self.calls.append(("group_bootstrap", replicates, seed))
        rng = np.random.default_rng(seed)
        M = np.zeros((replicates + 1, n, n), dtype=np.uint64)
        for r in range(replicates + 1):
            U = np.triu(rng.integers(1, 30, size=(n, n)), 1)
            M[r] = U + U.T
        self.counts = M
        return M, self.sites, self.clean

    def nj_batch(self, D):
        self.calls.append(("nj_batch", D.shape))
        trees = [T.neighbour_joining(d) for d in D]
        return (np.array([t.edges for t in trees], dtype=T.EDGE_RECORD),
                np.array([T.bipartitions(t) for t in trees], dtype=np.uint64).reshape(len(D), D.shape[1] - 3))


FOUR = ["w.fa", "x.fa", "y.fa", "z.fa"]


def run_core_files(argv, bf=None):
    opt = P.parse_args(BASE + argv + FOUR)
    bf = bf or FakeFinder()
    insts = [[(0, 0, 600, False), (1, 0, 600, False), (2, 0, 600, True), (3, 0, 600, False)]]
    said = []
    files = P.core_files(bf, opt, ["w", "x", "y", "z"], [4], insts, [types.SimpleNamespace(status=0, L=600)], {4}, said.append)
    return files, bf, said


def test_core_files_makes_every_file_of_one_kind_of_rows_from_one_pair_of_calls():
    every = ["--coretree", "t.nwk", "--corefilteredtree", "ft.nwk", "--coreconsensus", "c.nwk", "--corefilteredconsensus", "fc.nwk", "--coreboottrees", "b.nwk",
             "--corefilteredboottrees", "fb.nwk", "--bootstrap", "6", "--bootseed", "3"]
    files, bf, said = run_core_files(every)
    assert said == [] and list(files) == ["t.nwk", "ft.nwk", "c.nwk", "fc.nwk", "b.nwk", "fb.nwk"]
    assert bf.calls == [("group_bootstrap", 6, 3), ("nj_batch", (7, 4, 4)), ("group_mask",), ("set_masked", True), ("group_bootstrap", 6, 3), ("nj_batch", (7, 4, 4)),
                        ("set_masked", False)]
    main, majority, lines = T.tree_files(bf.counts, 100, "p", FOUR)               # the host path on the same counts: the same bytes
    assert (files["t.nwk"], files["c.nwk"], files["b.nwk"]) == (main.encode(), majority.encode(), lines.encode())
    assert files["t.nwk"] == T.tree_text(bf.counts, 100, "p", FOUR).encode() and files["b.nwk"].count(b"\n") == 6 and files["c.nwk"].count(b"\n") == 1
    # one option alone makes its file alone, from the same calls
    for option, name in (("--coreconsensus", "c.nwk"), ("--coreboottrees", "b.nwk"), ("--coretree", "t.nwk")):
        alone, bf, said = run_core_files([option, name, "--bootstrap", "6", "--bootseed", "3"])
        assert said == [] and alone == {name: files[name]} and bf.calls == [("group_bootstrap", 6, 3), ("nj_batch", (7, 4, 4))]
    alone, bf, said = run_core_files(["--corefilteredconsensus", "fc.nwk", "--bootstrap", "6", "--bootseed", "3"])
    assert alone == {"fc.nwk": files["fc.nwk"]} and bf.calls[:2] == [("group_mask",), ("set_masked", True)] and bf.calls[-1] == ("set_masked", False)


def test_a_file_that_cannot_be_made_is_named_by_its_option():
    argv = ["--coretree", "t.nwk", "--coreconsensus", "c.nwk", "--coreboottrees", "b.nwk", "--corealignment", "c.fa", "--bootstrap", "4"]
    opt = P.parse_args(BASE + argv + FOUR)
    said = []
    bf = FakeFinder()
    bf.group_concat = lambda *a: (b"", [], [])
    assert list(P.core_files(bf, opt, ["w", "x", "y", "z"], [], [], [], set(), said.append)) == ["c.fa"] and len(said) == 1 and said[0].startswith("no core block")
    bf = FakeFinder(sites=0)
    bf.group_concat = lambda *a: (b"", [], [])
    files, bf, said = run_core_files(argv, bf)
    assert list(files) == ["c.fa"] and said == ["%s not written: no variable column in the core-genome alignment\n" % o for o in ("--coretree", "--coreconsensus", "--coreboottrees")]
    files, bf, said = run_core_files(["--coreconsensus", "c.nwk", "--coreboottrees", "b.nwk", "--bootstrap", "4", "--treemodel", "jc"], FakeFinder(clean=20))
    assert files == {} and [s.split(":")[0] for s in said] == ["--coreconsensus not written", "--coreboottrees not written"]
    assert all("no Jukes-Cantor distance" in s for s in said)                    # counts of up to 29 over 20 columns


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--coreconsensus', 'c.nwk', '--corefilteredboottrees', 'u.nwk', '--bootstrap', '10', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "import sibelia_amd.tree as T, numpy as np; D = np.ones((3, 4, 4)) - np.eye(4); "
            "T.tree_files((D * 5).astype(np.uint64), 100, 'p', list('abcd')); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
