"""The command line of --corebranches / --corebranchsites / --coresnptree and their --corefiltered... twins (sibelia_amd/pipeline.py), the
file plan, the three texts (sibelia_amd/formats.py, tree.py) from fixed inputs and core_files over a stand-in finder: device-free."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BM                            # noqa: E402
import parsimony_model as PM                       # noqa: E402

from sibelia_amd import formats as F       # noqa: E402
from sibelia_amd import pipeline as P      # noqa: E402
from sibelia_amd import tree as T          # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
OPTIONS = ("--corebranches", "--corefilteredbranches", "--corebranchsites", "--corefilteredbranchsites", "--coresnptree", "--corefilteredsnptree")
FILTERED = OPTIONS[1::2]
THREE = ["a/x.fa", "y.fa", "z.fa"]
PLAN = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]


@pytest.mark.parametrize("option", OPTIONS)
def test_each_option_exists_once_and_asks_for_the_tree(option):
    actions = [a for a in P.build_parser()._actions if option in a.option_strings]
    assert len(actions) == 1 and actions[0].option_strings == [option] and actions[0].default is None
    assert option + " FILE" in " ".join(P.build_parser().format_help().split())
    o = P.parse_args(BASE + [option, "b.tsv"] + THREE)
    assert getattr(o, option[2:]) == "b.tsv" and P.tree_wanted(o) and P.concat_wanted(o) and not P.core_wanted(o)
    assert (o.bootstrap, o.bootseed, o.treemodel, o.gapopen, o.coremin) == (0, 1, "p", 0, 3)
    assert P.density_wanted(o) == (option in FILTERED)
    assert all(getattr(o, x[2:]) is None for x in OPTIONS + ("--coretree", "--corefilteredtree") if x != option)
    off = P.parse_args(BASE + THREE)
    assert all(getattr(off, x[2:]) is None for x in OPTIONS) and not P.tree_wanted(off)


def test_help_says_what_the_files_are():
    text = " ".join(P.build_parser().format_help().split())
    mine = text[text.rindex("--corebranches FILE"):text.rindex("--corefilteredbranches FILE")]
    assert all(x in mine for x in ("Three to 64", "parsimony", "transitions", "transversions", "homoplasic", "consistency index", "first file"))
    mine = text[text.rindex("--corebranchsites FILE"):text.rindex("--corefilteredbranchsites FILE")]
    assert "one line per change" in mine and "--coresites" in mine
    assert "SNP-scaled" in text[text.rindex("--coresnptree FILE"):text.rindex("--corefilteredsnptree FILE")]


@pytest.mark.parametrize("option", OPTIONS)
def test_argument_rules_of_each_option(option):
    for argv, message in [
            ([option, "b.tsv", "x.fa"], "%s compares files: it needs at least two" % option),
            ([option, "b.tsv", "x.fa", "y.fa"], "%s builds a tree: it needs at least three input files" % option),
            ([option, "b.tsv", "--noblocks"] + THREE, "%s needs the synteny blocks: it cannot be combined with --noblocks" % option),
            ([option, "b.tsv", "y.fa", "a/x.fa", "b/x.fa"], "%s names a file by its base name: two files are called x.fa" % option),
            ([option, "coverage_report.txt"] + THREE, "%s names a file the program writes itself: coverage_report.txt" % option),
            ([option, "sub/"] + THREE, "%s needs a file name, not 'sub/'" % option),
            (["--coretree", "c.out", option, "./c.out"] + THREE, "--coretree and %s name the same file: c.out" % option),
            ([option, "b.tsv"] + ["f%d.fa" % k for k in range(65)],
             "%s maps the changes onto the tree on the device, which takes at most 64 input files: 65 are given" % option)]:
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + argv)
        assert str(e.value) == message
    assert len(P.parse_args(BASE + [option, "b.tsv"] + ["f%d.fa" % k for k in range(64)]).filenames) == 64
    P.parse_args(BASE + ["--coretree", "t.nwk"] + ["f%d.fa" % k for k in range(65)])      # the tree alone has no such limit
    o = P.parse_args(BASE + [option, "b.tsv", "--bootstrap", "7", "--bootseed", "9", "--treemodel", "jc", "--gapopen", "400", "--wideband", "--coremin", "2"] + THREE)
    assert (o.bootstrap, o.bootseed, o.treemodel, o.gapopen, o.wideband, o.coremin) == (7, 9, "jc", 400, True, 2)
    for setting in ("--densitywindow", "--densitymax"):
        if option in FILTERED:
            assert getattr(P.parse_args(BASE + [option, "b.tsv", setting, "60"] + THREE), setting[2:]) == 60
        else:
            with pytest.raises(P.PipelineError):
                P.parse_args(BASE + [option, "b.tsv", setting, "60"] + THREE)


def test_no_two_options_share_a_file():
    for i, a in enumerate(OPTIONS):
        for b in OPTIONS[i + 1:]:
            with pytest.raises(P.PipelineError) as e:
                P.parse_args(BASE + [b, "t.out", a, "t.out"] + THREE)
            assert str(e.value) == "%s and %s name the same file: t.out" % (a, b)


def test_the_new_files_are_planned_last():
    plan = lambda argv: P.planned_files(P.parse_args(BASE + argv + THREE), 3)      # noqa: E731
    assert [o for o, _ in P.BRANCH_OPTIONS] == list(OPTIONS) and P.EVERY_FILE_OPTIONS == P.ALL_FILE_OPTIONS + P.BRANCH_OPTIONS
    assert P.ALL_TREE_OPTIONS[-6:] == P.BRANCH_OPTIONS and P.ROWS_BRANCH_OPTIONS[True] == P.BRANCH_OPTIONS[1::2]
    every = [x for o in reversed(OPTIONS) for x in (o, o[2:] + ".out")]
    assert plan(every) == PLAN + [o[2:] + ".out" for o in OPTIONS]
    assert plan(["--coresnptree", "s.nwk", "--coreboottrees", "sub/b.nwk", "--corebranches", "b.tsv", "--coretree", "t.nwk", "--coresites", "s.tsv", "--bootstrap", "5", "-g"]) == \
        PLAN + ["s.tsv", "t.nwk", "sub/b.nwk", "b.tsv", "s.nwk", "de_bruijn_graph.dot"]


# ------------------------------------------------------------------------------------------ the texts from fixed inputs

def test_the_summary_line_rounds_by_the_integers():
    assert F.parsimony_summary([2, 1, 1], [1, 1, 1]) == "# sites=3 steps=4 minsteps=3 homoplasic=1 ci=0.750000"
    assert F.parsimony_summary([3], [2]) == "# sites=1 steps=3 minsteps=2 homoplasic=0 ci=0.666667".replace("homoplasic=0", "homoplasic=1")
    assert F.parsimony_summary([2] * 8, [1] * 7 + [2]) == "# sites=8 steps=16 minsteps=9 homoplasic=7 ci=0.562500"
    assert F.parsimony_summary([1] * 2000001 + [2], [1] * 2000002).endswith("steps=2000003 minsteps=2000002 homoplasic=1 ci=1.000000")      # 0.9999995 goes up
    assert F.parsimony_summary([], []) == "# sites=0 steps=0 minsteps=0 homoplasic=0 ci=nan"
    assert F.parsimony_summary([0, 0], [0, 0]) == "# sites=2 steps=0 minsteps=0 homoplasic=0 ci=nan"
    assert F.parsimony_summary([1] * 3, [1] * 3).endswith("ci=1.000000")


TREE4 = T.Tree(4, [(4, 2, 0.25), (4, 3, 0.5), (5, 0, 0.125), (5, 1, 0.0625), (5, 4, 1.0)])      # ((2, 3), 0, 1) read from file 0: top is node 5
NAMES4 = ["w.fa", "x.fa", "y.fa", "z.fa"]


def test_the_branch_order_is_the_order_of_the_newick_text():
    order = T.branches(TREE4)
    assert [(v, e, mask) for v, e, mask, _ in order] == [(0, 2, 1), (1, 3, 2), (4, 4, 12), (2, 0, 4), (3, 1, 8)]
    text = T.newick(TREE4, NAMES4, {12: 7}, 10)
    assert text == "(w.fa:0.125000000,x.fa:0.062500000,(y.fa:0.250000000,z.fa:0.500000000)70:1.000000000);\n"
    names, edges, labels = PM.read_newick(text)                                  # the lengths stand in the text in the order of the branches
    import re
    assert re.findall(r":([0-9.]+)", text) != ["%.9f" % ln for _, _, _, ln in order]      # a closing node's length follows its children's ...
    assert [ln for _, _, _, ln in PM._preorder(names, edges)] == ["%.9f" % ln for _, _, _, ln in order]      # ... so the reader walks the tree
    assert T.newick(TREE4, NAMES4, {12: 7}, 10, {0: 3, 1: 0, 4: 12, 2: 1, 3: 2}) == "(w.fa:3,x.fa:0,(y.fa:1,z.fa:2)70:12);\n"
    assert T.newick(TREE4, NAMES4, None, 0, {0: 3, 1: 0, 4: 12, 2: 1, 3: 2}) == "(w.fa:3,x.fa:0,(y.fa:1,z.fa:2):12);\n"
    assert T.support_label(7, 10) == "70" and T.support_label(1, 8) == "13" and T.support_label(0, 3) == "0"      # 12.5 goes up


def test_the_two_tables_from_fixed_rows():
    zero = [[0] * 4 for _ in range(4)]
    ag = [[0, 0, 0, 2], [0, 0, 1, 0], [0, 0, 0, 0], [1, 0, 0, 0]]               # A -> G twice, C -> T, G -> A: four transitions
    mixed = [[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]            # A -> C, T -> G: two transversions
    rows = [(["w.fa"], 0.125, None, zero), (["y.fa", "z.fa"], 1.0, "70", ag), (["z.fa"], 0.5, None, mixed)]
    text = F.core_branches_text(rows, [2, 1], [1, 1], 400, 3).decode()
    assert text == ("# gapopen=400\n# coremin=3\n# sites=2 steps=3 minsteps=2 homoplasic=1 ci=0.666667\n"
                    "branch\tfiles\tlength\tsupport\tchanges\ttransitions\ttransversions\n"
                    "1\tw.fa\t0.125000000\t.\t0\t0\t0\n2\ty.fa,z.fa\t1.000000000\t70\t4\t4\t0\n3\tz.fa\t0.500000000\t.\t2\t0\t2\n")
    assert F.core_branches_text(rows[:1], [], []).decode().split("\n")[0] == "# sites=0 steps=0 minsteps=0 homoplasic=0 ci=nan"
    sites = [(7, "chr1", 100, 700, False, 10), (9, "chr2", 50, 650, True, 20)]
    table = F.core_sites_text(sites, 400, 3).decode().split("\n")
    text = F.core_branch_sites_text(sites, [(0, 2, 0, 3), (0, 5, 3, 0), (1, 1, 1, 2)], [2, 1], [1, 1], 400, 3).decode().split("\n")
    assert text[:3] == ["# gapopen=400", "# coremin=3", "# sites=2 steps=3 minsteps=2 homoplasic=1 ci=0.666667"]
    assert text[3] == "column\tblock\trecord\tposition\tstrand\tbranch\tfrom\tto\tsteps\tminsteps"
    assert text[4:] == [table[3] + "\t2\tA\tG\t2\t1", table[3] + "\t5\tG\tA\t2\t1", table[4] + "\t1\tC\tT\t1\t1", ""]
    assert table[3] == "1\t7\tchr1\t111\t+" and table[4] == "2\t9\tchr2\t630\t-"


# ------------------------------------------------------------------------------------------ core_files over a stand-in finder

class FakeFinder:
    """what core_files asks of a BlockFinder, recorded, over one fixed SNP matrix of four files: the counts, the SNP text and its sites,
    and the mapping as tests/parsimony_model.py makes it"""
    S = [b"AAACAGTA", b"AACTAGAC", b"GAATCATC", b"GTCTCATG"]                  # the third column: A C A C, two steps for two bases

    def __init__(self, clean=100):
        self.file_records = [1, 1, 1, 1]
        self.calls, self.clean = [], clean

    def set_masked(self, on):
        self.calls.append(("set_masked", bool(on)))

    def set_partial(self, on):
        self.calls.append(("set_partial", bool(on)))

    def group_bootstrap_pairs(self):
        return np.full((4, 4), self.clean, dtype=np.uint64)

    def group_mask(self, window, max_diff, want):
        self.calls.append(("group_mask",))
        return []

    def group_concat(self, cls, n, headers, mode, width, want):
        self.calls.append(("group_concat", mode))
        text = b"".join(h + row + b"\n" for h, row in zip(headers, self.S))
        return text, [(0, 0, 8)], [(0, 10 * k, 10 * k) for k in range(8)]

    def group_bootstrap(self, cls, n, replicates, seed, draws, want):
        self.calls.append(("group_bootstrap", replicates, seed))
        M = BM.counts_of_sites(np.array([np.frombuffer(r, dtype=np.uint8) for r in self.S]), replicates, seed)
        return M, 8, self.clean

    def nj_batch(self, D):
        self.calls.append(("nj_batch", D.shape))
        trees = [T.neighbour_joining(d) for d in D]
        return (np.array([t.edges for t in trees], dtype=T.EDGE_RECORD),
                np.array([T.bipartitions(t) for t in trees], dtype=np.uint64).reshape(len(D), D.shape[1] - 3))

    def group_parsimony(self, edges):
        from sibelia_amd.api import PARSIMONY_CHANGE_DTYPE
        self.calls.append(("group_parsimony", len(edges)))
        counts, steps, least, changes = PM.fitch(self.S, None, edges)
        rec = np.zeros(len(changes), dtype=PARSIMONY_CHANGE_DTYPE)
        for k, (x, e, a, b) in enumerate(changes):
            rec[k]["site"], rec[k]["edge"], rec[k]["from"], rec[k]["to"] = x, e, a, b
        return np.array(counts, dtype=np.uint64), np.array(steps, dtype=np.uint8), np.array(least, dtype=np.uint8), rec


FOUR = ["w.fa", "x.fa", "y.fa", "z.fa"]
MAPPED = ["--corebranches", "b.tsv", "--corebranchsites", "s.tsv", "--coresnptree", "n.nwk"]
FMAPPED = ["--corefilteredbranches", "fb.tsv", "--corefilteredbranchsites", "fs.tsv", "--corefilteredsnptree", "fn.nwk"]


def run_core_files(argv, bf=None):
    opt = P.parse_args(BASE + argv + FOUR)
    bf = bf or FakeFinder()
    insts = [[(0, 0, 600, False), (1, 0, 600, False), (2, 0, 600, True), (3, 0, 600, False)]]
    said = []
    files = P.core_files(bf, opt, ["w", "x", "y", "z"], [4], insts, [types.SimpleNamespace(status=0, L=600)], {4}, said.append)
    return files, bf, said


@pytest.mark.parametrize("boot", (0, 6))
def test_core_files_makes_the_three_files_the_model_makes_of_the_run_s_own_files(boot):
    argv = ["--coresnps", "snps.fa", "--coresites", "sites.tsv", "--coretree", "t.nwk", "--bootstrap", str(boot), "--gapopen", "400"] + MAPPED
    files, bf, said = run_core_files(argv)
    assert said == [] and list(files) == ["snps.fa", "sites.tsv", "t.nwk", "b.tsv", "s.tsv", "n.nwk"]
    assert bf.calls == [("group_concat", 1), ("group_bootstrap", boot, 1), ("nj_batch", (boot + 1, 4, 4)), ("group_parsimony", 5)]
    assert files["t.nwk"] == T.tree_text(BM.counts_of_sites(np.array([np.frombuffer(r, dtype=np.uint8) for r in bf.S]), boot, 1), 100, "p", FOUR).encode()
    sites_text, comments = PM.branch_sites_text(files["snps.fa"], files["t.nwk"], files["sites.tsv"], FOUR)
    assert comments == ["# gapopen=400"]
    assert files["b.tsv"] == PM.branches_text(files["snps.fa"], files["t.nwk"], FOUR, comments)
    assert files["s.tsv"] == sites_text and files["n.nwk"] == PM.snp_tree_text(files["snps.fa"], files["t.nwk"], FOUR)
    # not vacuous: a homoplasic site, changes on inner and leaf branches, '.' and, with replicates, a label
    lines = files["b.tsv"].decode().split("\n")
    assert lines[0] == "# gapopen=400" and lines[1].startswith("# sites=8 steps=") and "homoplasic=0" not in lines[1] and lines[2].startswith("branch\tfiles")
    assert len(lines) == 3 + 5 + 1 and [x.split("\t")[0] for x in lines[3:8]] == list("12345") and lines[3].split("\t")[1] == "w.fa"
    support = [x.split("\t")[3] for x in lines[3:8]]
    assert support.count(".") == (4 if boot else 5) and sum(int(x.split("\t")[4]) for x in lines[3:8]) == int(lines[1].split()[2][len("steps="):])
    assert files["n.nwk"].count(b":") == 5 and b"." not in files["n.nwk"].replace(b".fa", b"")
    assert len(files["s.tsv"].decode().split("\n")) == 3 + sum(int(x.split("\t")[4]) for x in lines[3:8]) + 1
    # each alone: its file alone, from the same three calls (the change table also asks for the sites)
    for option, name in zip(MAPPED[0::2], MAPPED[1::2]):
        alone, bf, said = run_core_files([option, name, "--bootstrap", str(boot), "--gapopen", "400"])
        assert said == [] and alone == {name: files[name]}
        assert bf.calls == ([("group_concat", 1)] if name == "s.tsv" else []) + [("group_bootstrap", boot, 1), ("nj_batch", (boot + 1, 4, 4)), ("group_parsimony", 5)]


def test_the_filtered_trio_reads_the_masked_rows_and_the_soft_core_is_recorded():
    files, bf, said = run_core_files(MAPPED + FMAPPED + ["--coremin", "3", "--bootstrap", "4"])
    assert said == [] and list(files) == ["b.tsv", "fb.tsv", "s.tsv", "fs.tsv", "n.nwk", "fn.nwk"]
    assert bf.calls == [("set_partial", True), ("group_concat", 1), ("group_bootstrap", 4, 1), ("nj_batch", (5, 4, 4)), ("group_parsimony", 5), ("group_mask",), ("set_masked", True),
                        ("group_concat", 1), ("group_bootstrap", 4, 1), ("nj_batch", (5, 4, 4)), ("group_parsimony", 5), ("set_masked", False), ("set_partial", False)]
    assert files["b.tsv"] == files["fb.tsv"] and files["s.tsv"] == files["fs.tsv"] and files["n.nwk"] == files["fn.nwk"]      # the stand-in masks nothing
    assert files["b.tsv"].decode().split("\n")[0] == "# coremin=3" and files["s.tsv"].decode().split("\n")[0] == "# coremin=3"


def test_a_file_that_cannot_be_made_is_named_by_its_option():
    files, bf, said = run_core_files(MAPPED + ["--coretree", "t.nwk", "--treemodel", "jc"], FakeFinder(clean=8))
    assert files == {} and [s.split(":")[0] for s in said] == ["%s not written" % o for o in ("--coretree", "--corebranches", "--corebranchsites", "--coresnptree")]
    assert all("no Jukes-Cantor distance" in s for s in said) and ("group_parsimony", 5) not in bf.calls
    bf = FakeFinder()
    bf.group_bootstrap = lambda *a: (np.zeros((1, 4, 4), dtype=np.uint64), 0, 100)
    files, bf, said = run_core_files(MAPPED, bf)
    assert files == {} and said == ["%s not written: no variable column in the core-genome alignment\n" % o for o in MAPPED[0::2]]
    opt = P.parse_args(BASE + MAPPED + FOUR)
    said = []
    bf = FakeFinder()
    bf.group_concat = lambda *a: (b"", [], [])
    assert P.core_files(bf, opt, ["w", "x", "y", "z"], [], [], [], set(), said.append) == {} and len(said) == 1 and said[0].startswith("no core block")


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--corebranches', 'b.tsv', '--corefilteredsnptree', 'u.nwk', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
