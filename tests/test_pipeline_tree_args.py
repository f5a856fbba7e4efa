"""The command line of --coretree / --corefilteredtree and of --bootstrap / --bootseed / --treemodel (sibelia_amd/pipeline.py) and the file
plan: device-free."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
OPTIONS = ("--coretree", "--corefilteredtree")
SETTINGS = (("--bootstrap", "B", "7"), ("--bootseed", "S", "7"), ("--treemodel", "{p,jc}", "jc"))
NEEDS = "it needs at least one of --coretree and --corefilteredtree"
THREE = ["a/x.fa", "y.fa", "z.fa"]
DENSITY_NEEDS = "it needs at least one of --corefiltered, --corefilteredsnps, --corefilteredsites and --coredense"


@pytest.mark.parametrize("option", OPTIONS)
def test_each_file_option_exists_once_with_its_defaults(option):
    actions = [a for a in P.build_parser()._actions if option in a.option_strings]
    assert len(actions) == 1 and actions[0].option_strings == [option] and actions[0].default is None
    assert option + " FILE" in " ".join(P.build_parser().format_help().split())
    o = P.parse_args(BASE + [option, "t.nwk"] + THREE)
    assert getattr(o, option[2:]) == "t.nwk" and P.tree_wanted(o) and not P.core_wanted(o)
    assert (o.bootstrap, o.bootseed, o.treemodel, o.gapopen) == (0, 1, "p", 0)
    assert P.density_wanted(o) == (option == "--corefilteredtree")               # the masked rows are made for it
    assert getattr(o, [x for x in OPTIONS if x != option][0][2:]) is None
    off = P.parse_args(BASE + THREE)
    assert (off.coretree, off.corefilteredtree, off.bootstrap, off.bootseed, off.treemodel) == (None, None, 0, 1, "p") and not P.tree_wanted(off)


def test_help_says_what_the_tree_is():
    text = " ".join(P.build_parser().format_help().split())
    mine = text[text.rindex("--coretree FILE"):text.rindex("--corefilteredtree FILE")]
    assert "neighbour-joining" in mine and "Newick" in mine and "Three or more" in mine and "--treemodel" in mine
    assert "--corefiltered" in text[text.rindex("--corefilteredtree FILE"):text.rindex("--bootstrap B")]
    assert "default 0" in text[text.rindex("--bootstrap B"):text.rindex("--bootseed S")]
    assert "default 1" in text[text.rindex("--bootseed S"):text.rindex("--treemodel")]
    assert "Jukes and Cantor" in text[text.rindex("--treemodel {p,jc}"):]


@pytest.mark.parametrize("option", OPTIONS)
def test_argument_rules_of_each_file_option(option):
    for argv, message in [
            ([option, "t.nwk", "x.fa"], "%s compares files: it needs at least two" % option),
            ([option, "t.nwk", "x.fa", "y.fa"], "%s builds a tree: it needs at least three input files" % option),
            ([option, "t.nwk", "--noblocks"] + THREE, "%s needs the synteny blocks: it cannot be combined with --noblocks" % option),
            ([option, "t.nwk", "y.fa", "a/x.fa", "b/x.fa"], "%s names a file by its base name: two files are called x.fa" % option),
            ([option, "coverage_report.txt"] + THREE, "%s names a file the program writes itself: coverage_report.txt" % option),
            ([option, "sub/"] + THREE, "%s needs a file name, not 'sub/'" % option),
            ([option, ""] + THREE, "%s needs a file name, not ''" % option),
            (["--multimaf", "c.out", option, "./c.out"] + THREE, "--multimaf and %s name the same file: c.out" % option),
            (["--coredense", "c.out", option, "sub/../c.out"] + THREE, "--coredense and %s name the same file: c.out" % option)]:
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + argv)
        assert str(e.value) == message


def test_the_two_do_not_share_a_file():
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--corefilteredtree", "t.nwk", "--coretree", "t.nwk"] + THREE)
    assert str(e.value) == "--coretree and --corefilteredtree name the same file: t.nwk"


@pytest.mark.parametrize("bad", ["a(b.fa", "a)b.fa", "a[b.fa", "a]b.fa", "a:b.fa", "a;b.fa", "a,b.fa", "a'b.fa", 'a"b.fa', "a b.fa", "a\tb.fa"])
def test_a_name_newick_cannot_hold_is_refused_before_anything_runs(bad):
    for option in OPTIONS:
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + [option, "t.nwk", "x.fa", "dir/" + bad, "z.fa"])
        assert str(e.value).startswith("%s names a file by its base name: the name %r cannot stand in a Newick tree" % (option, bad))
    P.parse_args(BASE + ["--corealignment", "c.fa", "x.fa", "dir/" + bad, "z.fa"])   # the other files take such a name
    P.parse_args(BASE + ["--coretree", "t.nwk", "x.fa", "a(b/y.fa", "z.fa"])         # the directory is not part of the name


def test_the_range_of_bootstrap_and_bootseed():
    for v in (0, 1, 100, 100000):
        assert P.parse_args(BASE + ["--coretree", "t.nwk", "--bootstrap", str(v)] + THREE).bootstrap == v
    for v in ("-1", "100001", "x", "1.5"):
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + ["--coretree", "t.nwk", "--bootstrap", v] + THREE)
        assert "--bootstrap" in str(e.value)
    for v in (0, 1, 2 ** 63, 2 ** 64 - 1):
        assert P.parse_args(BASE + ["--corefilteredtree", "t.nwk", "--bootseed", str(v)] + THREE).bootseed == v
    for v in ("-1", str(2 ** 64), "x"):
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + ["--coretree", "t.nwk", "--bootseed", v] + THREE)
        assert "--bootseed" in str(e.value)
    for v in ("p", "jc"):
        assert P.parse_args(BASE + ["--coretree", "t.nwk", "--treemodel", v] + THREE).treemodel == v
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--coretree", "t.nwk", "--treemodel", "k2p"] + THREE)
    assert "--treemodel" in str(e.value)
    o = P.parse_args(BASE + ["--coretree", "t.nwk", "--corefilteredtree", "u.nwk", "--bootstrap", "100", "--bootseed", "0", "--treemodel", "jc"] + THREE)
    assert (o.bootstrap, o.bootseed, o.treemodel) == (100, 0, "jc")


@pytest.mark.parametrize("setting, metavar, value", SETTINGS)
def test_a_setting_alone_is_refused(setting, metavar, value):
    assert ("%s %s" % (setting, metavar)) in " ".join(P.build_parser().format_help().split())
    for more in ([], ["--corealignment", "c.fa", "--coresnps", "s.fa"], ["--corefiltered", "f.fa", "--distances", "d.phy"]):
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + more + [setting, value] + THREE)
        assert str(e.value) == "%s is a setting of the tree: %s" % (setting, NEEDS)


def test_the_density_settings_go_with_the_filtered_tree_alone():
    o = P.parse_args(BASE + ["--corefilteredtree", "t.nwk", "--densitywindow", "60", "--densitymax", "2"] + THREE)
    assert (o.densitywindow, o.densitymax) == (60, 2) and P.density_wanted(o)
    for setting in ("--densitywindow", "--densitymax"):                         # ... and not with the plain one: the message is the old one
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + ["--coretree", "t.nwk", setting, "5"] + THREE)
        assert str(e.value) == "%s sets the density filter: %s" % (setting, DENSITY_NEEDS)


@pytest.mark.parametrize("option", OPTIONS)
def test_gapopen_and_wideband_are_accepted_with_each_alone(option):
    o = P.parse_args(BASE + [option, "t.nwk", "--gapopen", "400", "--wideband"] + THREE)
    assert o.gapopen == 400 and o.wideband


def test_main_reports_the_error_before_any_file_is_read(tmp_path, capsys):
    missing = [str(tmp_path / ("missing%d.fa" % i)) for i in range(3)]
    assert P.main(BASE + ["--coretree", "t.nwk"] + missing[:2]) == 1
    assert capsys.readouterr().err == "error: --coretree builds a tree: it needs at least three input files\n"
    assert P.main(BASE + ["--bootstrap", "10"] + missing) == 1
    assert capsys.readouterr().err == "error: --bootstrap is a setting of the tree: %s\n" % NEEDS


def test_planned_files_list_the_two_last():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv: P.planned_files(P.parse_args(BASE + argv + THREE), 3)      # noqa: E731
    assert P.FILE_OPTIONS[-2:] == (("--coretree", "coretree"), ("--corefilteredtree", "corefilteredtree"))
    assert plan(["--corefilteredtree", "ft.nwk", "--coretree", "t.nwk"]) == base + ["t.nwk", "ft.nwk"]
    assert plan(["--coretree", "sub/t.nwk", "--bootstrap", "9"]) == base + ["sub/t.nwk"]
    assert plan(["--corefilteredtree", "ft.nwk", "--coretree", "t.nwk", "--coredense", "d.tsv", "--corefiltered", "f.fa", "--coresites", "s.tsv", "--corealignment", "c.fa",
                 "--distancecounts", "n.tsv", "--multimaf", "m.maf", "-q", "-g"]) == base + ["blocks_sequences.fasta", "m.maf", "n.tsv", "c.fa", "s.tsv", "f.fa", "d.tsv", "t.nwk", "ft.nwk",
                                                                                             "de_bruijn_graph.dot"]


@pytest.mark.parametrize("argv, files, plan", [
    ([], ["x.fa"], []),
    (["--multimaf", "m.maf"], ["x.fa"], ["m.maf"]),
    (["--corealignment", "c.fa", "--coredense", "d.tsv", "--gapopen", "9"], ["x.fa", "y.fa"], ["c.fa", "d.tsv"]),
])
def test_existing_option_sets_plan_what_they_planned(argv, files, plan):
    o = P.parse_args(BASE + argv + files)
    assert not P.tree_wanted(o) and (o.bootstrap, o.bootseed, o.treemodel) == (0, 1, "p")
    assert P.planned_files(o, 3) == ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"] + plan


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--coretree', 't.nwk', '--corefilteredtree', 'u.nwk', '--bootstrap', '10', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
