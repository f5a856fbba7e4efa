"""The command line of --coremin / --corepresence (sibelia_amd/pipeline.py), the rule that picks the soft-core blocks, the presence table
and the `# coremin=` lines (sibelia_amd/formats.py), the section of core_files under set_partial, and the tree over a matrix of columns
per pair (sibelia_amd/tree.py): device-free."""
import types

import numpy as np
import pytest

from sibelia_amd import formats            # noqa: E402
from sibelia_amd import pipeline as P      # noqa: E402
from sibelia_amd import tree               # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
THREE = ["x.fa", "y.fa", "z.fa"]
NEEDS = "--coremin sets which blocks the core-genome files are made of: it needs at least one of the --core..., --corefiltered... and tree options and --corepresence"


def test_the_two_options_exist_once_and_are_in_the_help():
    text = " ".join(P.build_parser().format_help().split())
    for option, meta in (("--coremin", "M"), ("--corepresence", "FILE")):
        actions = [a for a in P.build_parser()._actions if option in a.option_strings]
        assert len(actions) == 1 and actions[0].option_strings == [option] and actions[0].default is None
        assert "%s %s" % (option, meta) in text
    mine = text[text.rindex("--coremin M"):text.rindex("--corepresence FILE")]
    assert "at least M input files" in mine and "default the number of files" in mine and "gaps" in mine and "# coremin=M" in mine and "first file" in mine


def test_coremin_its_range_and_its_default():
    for files in (THREE[:2], THREE, THREE + ["w.fa"]):
        assert P.parse_args(BASE + ["--coresnps", "s.fa"] + files).coremin == len(files)
        assert P.parse_args(BASE + files).coremin == len(files)
        for m in range(2, len(files) + 1):
            assert P.parse_args(BASE + ["--coresnps", "s.fa", "--coremin", str(m)] + files).coremin == m
        for m in (0, 1, len(files) + 1):
            with pytest.raises(P.PipelineError) as e:
                P.parse_args(BASE + ["--coresnps", "s.fa", "--coremin", str(m)] + files)
            assert str(e.value) == "--coremin is the number of input files a block must reach: 2 .. %d for these input files" % len(files)
    for bad in ("-1", "two", "2.0", ""):
        with pytest.raises(P.PipelineError):
            P.parse_args(BASE + ["--coresnps", "s.fa", "--coremin", bad] + THREE)


@pytest.mark.parametrize("option", ["--corealignment", "--corepartitions", "--coresnps", "--coresites", "--corefiltered", "--corefilteredsnps", "--corefilteredsites",
                                    "--coredense", "--coretree", "--corefilteredtree", "--corepresence"])
def test_coremin_is_accepted_with_each_of_the_options_it_serves(option):
    o = P.parse_args(BASE + [option, "c.out", "--coremin", "2"] + THREE)
    assert o.coremin == 2 and P.concat_wanted(o)


@pytest.mark.parametrize("more", [[], ["--multimaf", "m.maf"], ["--distances", "d.phy", "--multivariants", "m.vcf"]])
def test_coremin_needs_an_option_it_serves(more):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + more + ["--coremin", "2"] + THREE)
    assert str(e.value) == NEEDS


def test_corepresence_follows_the_rules_of_the_named_files():
    o = P.parse_args(BASE + ["--corepresence", "p.tsv"] + THREE[:2])
    assert o.corepresence == "p.tsv" and P.presence_wanted(o) and P.concat_wanted(o) and not P.core_wanted(o) and not P.tree_wanted(o)
    assert not P.presence_wanted(P.parse_args(BASE + THREE))
    for argv, message in [
            (["--corepresence", "p.tsv", "x.fa"], "--corepresence compares files: it needs at least two"),
            (["--corepresence", "p.tsv", "--noblocks", "x.fa", "y.fa"], "--corepresence needs the synteny blocks: it cannot be combined with --noblocks"),
            (["--corepresence", "p.tsv", "y.fa", "a/x.fa", "b/x.fa"], "--corepresence names a file by its base name: two files are called x.fa"),
            (["--corepresence", "coverage_report.txt", "x.fa", "y.fa"], "--corepresence names a file the program writes itself: coverage_report.txt"),
            (["--corepresence", "sub/", "x.fa", "y.fa"], "--corepresence needs a file name, not 'sub/'"),
            (["--coresites", "p.tsv", "--corepresence", "./p.tsv", "x.fa", "y.fa"], "--coresites and --corepresence name the same file: p.tsv"),
            (["--corepresence", "t.nwk", "--coretree", "t.nwk"] + THREE, "--corepresence and --coretree name the same file: t.nwk")]:
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + argv)
        assert str(e.value) == message


def test_planned_files_list_the_presence_table_before_the_trees():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv: P.planned_files(P.parse_args(BASE + argv + THREE), 3)      # noqa: E731
    assert plan(["--corepresence", "p.tsv", "--coremin", "2"]) == base + ["p.tsv"]
    assert plan(["--corepresence", "sub/p.tsv"]) == base + ["sub/p.tsv"]
    assert plan(["--coretree", "t.nwk", "--corepresence", "p.tsv", "--coredense", "d.tsv", "--coresnps", "s.fa", "--multimaf", "m.maf", "--coremin", "3"]) == base + ["m.maf", "s.fa", "d.tsv", "p.tsv", "t.nwk"]
    assert plan(["--coresnps", "s.fa", "--coremin", "2"]) == plan(["--coresnps", "s.fa"])                  # --coremin adds no file
    assert P.FILE_OPTIONS[-3:] == P.PRESENCE_OPTIONS + P.TREE_OPTIONS


def test_soft_core_blocks():
    """records 0, 1: the first file; 2: the second; 3, 4: the third"""
    rows = [(1, 0, 0, 600), (-1, 2, 0, 600), (1, 3, 0, 600),              # one per file: in at 2 and 3
            (2, 0, 700, 1300), (2, 1, 0, 600), (2, 2, 700, 1300),         # two instances in the first file: out
            (3, 0, 4000, 4600), (3, 2, 4000, 4499), (-3, 4, 0, 700),      # an instance shorter than -m: out
            (4, 2, 2000, 2600), (-4, 3, 2000, 2600),                      # missing from the first file: out
            (5, 1, 6000, 6600),                                           # a single instance: out
            (6, 0, 5000, 5600), (6, 2, 5000, 5600), (6, 3, 5000, 5600), (6, 4, 5000, 5600),      # two instances in the third file: out
            (-7, 1, 100, 900), (7, 2, 3000, 3800), (-7, 4, 900, 1700),    # one per file, on other records: in at 2 and 3
            (8, 1, 2000, 2700), (-8, 4, 3000, 3700),                      # the first and the third file: in at 2
            (9, 0, 8000, 8600), (9, 2, 8000, 8600)]                       # the first and the second file: in at 2
    blocks = np.array(rows, dtype=formats.BLOCK_DTYPE)
    files = [2, 1, 2]
    assert P.soft_core_blocks(blocks, files, 600, 3) == P.core_blocks(blocks, files, 600) == [1, 7]
    assert P.soft_core_blocks(blocks, files, 600, 2) == [1, 7, 8, 9]
    assert P.soft_core_blocks(blocks, files, 499, 2) == [1, 3, 7, 8, 9] and P.soft_core_blocks(blocks, files, 499, 3) == P.core_blocks(blocks, files, 499) == [1, 3, 7]
    assert P.soft_core_blocks(blocks, files, 601, 2) == [7, 8] and P.soft_core_blocks(blocks, files, 701, 2) == [7]
    assert P.soft_core_blocks(blocks[:0], files, 600, 2) == []
    for m in (499, 600, 601):                                                    # qualifying_blocks with a floor on the number of files
        assert P.soft_core_blocks(blocks, files, m, 2) == P.qualifying_blocks(blocks, files, m)
        assert set(P.soft_core_blocks(blocks, files, m, 3)) <= set(P.soft_core_blocks(blocks, files, m, 2))
    four = [2, 1, 1, 1]                                                           # other files: block 6 has one in each of four
    for n in (2, 3, 4):
        assert 6 in P.soft_core_blocks(blocks, four, 600, n)
    assert P.soft_core_blocks(blocks, four, 600, 4) == P.core_blocks(blocks, four, 600) == [6]
    assert P.soft_core_blocks(blocks, four, 600, 3) == [1, 6, 7] and 9 in P.soft_core_blocks(blocks, four, 600, 2)


def test_core_presence_text_and_the_comment_lines():
    names, rows = ["x.fa", "my genome.fa", "z.fa"], [(3, [True, True, True]), (8, [True, False, True]), (21, [True, True, False])]
    head, body = "block\tx.fa\tmy genome.fa\tz.fa\n", "3\t1\t1\t1\n8\t1\t0\t1\n21\t1\t1\t0\n"
    assert formats.core_presence_text(names, rows) == (head + body).encode()
    assert formats.core_presence_text(names, rows, 0, 2) == ("# coremin=2\n" + head + body).encode()
    assert formats.core_presence_text(names, rows, 200) == ("# gapopen=200\n" + head + body).encode()
    assert formats.core_presence_text(names, rows, 200, 2) == ("# gapopen=200\n# coremin=2\n" + head + body).encode()
    assert formats.core_presence_text(names, [], 0, 2) == ("# coremin=2\n" + head).encode()


def test_the_coremin_line_of_the_other_tables_comes_after_gapopen():
    parts, sites = [(3, 0, 5000)], [(3, "chr one", 100, 700, False, 0)]
    dense = [("y.fa", 3, "chr one", 100, 700, False, 10, 20, 4, 10, 20)]
    for text, args in ((formats.core_partitions_text, (parts,)), (formats.core_sites_text, (sites,)), (formats.core_dense_text, (dense, 1000, 3))):
        plain = text(*args).decode().split("\n")
        first = 1 if plain[0].startswith("# densitywindow=") else 0                # --coredense says its parameters first
        assert text(*args, 0, 0).decode().split("\n") == plain
        assert text(*args, 0, 2).decode().split("\n") == plain[:first] + ["# coremin=2"] + plain[first:]
        assert text(*args, 9, 2).decode().split("\n") == plain[:first] + ["# gapopen=9", "# coremin=2"] + plain[first:]
        assert text(*args, 9).decode().split("\n") == plain[:first] + ["# gapopen=9"] + plain[first:]


class FakeFinder:
    """what core_files asks of a BlockFinder, recorded: three files of one record; every answer is empty"""

    def __init__(self):
        self.file_records = [1, 1, 1]
        self.calls, self.on = [], False

    def set_partial(self, on):
        self.calls.append(("set_partial", bool(on)))
        self.on = bool(on)

    def set_masked(self, on):
        self.calls.append(("set_masked", bool(on)))

    def group_concat(self, cls, n, headers, mode, width, want):
        self.calls.append(("group_concat", self.on))
        return b"".join(headers), [(g, 0, 0) for g, w in enumerate(want) if w], []

    def group_bootstrap(self, cls, n, replicates, seed, draws, want):
        self.calls.append(("group_bootstrap", self.on))
        M = np.zeros((replicates + 1, n, n), dtype=np.uint64)
        M[:, 0, 1] = M[:, 1, 0] = 2
        M[:, 0, 2] = M[:, 2, 0] = 3
        M[:, 1, 2] = M[:, 2, 1] = 4
        return M, 5, 100

    def group_bootstrap_pairs(self):
        self.calls.append(("group_bootstrap_pairs", self.on))
        return np.array(self.pairs, dtype=np.uint64)

    def group_mask(self, window, max_diff, want):
        self.calls.append(("group_mask", self.on))
        return []


def run_core_files(argv, pairs=None, fail=False):
    from sibelia_amd.api import SibeliaError
    opt = P.parse_args(BASE + argv + THREE)
    bf = FakeFinder()
    bf.pairs = pairs or [[100] * 3] * 3
    if fail:
        def boom(*a):
            raise SibeliaError("sbl_group_concat: bad argument (made up)")
        bf.group_concat = boom
    ids, insts = [4, 9], [[(0, 0, 600, False), (1, 0, 600, False), (2, 0, 600, True)], [(0, 700, 1300, False), (2, 700, 1300, False)]]
    aligned = [types.SimpleNamespace(status=0, L=600), types.SimpleNamespace(status=0, L=600)]
    said = []
    core = {4, 9} if opt.coremin < 3 else {4}
    try:
        files = P.core_files(bf, opt, ["x", "y", "z"], ids, insts, aligned, core, said.append)
    except P.PipelineError:
        files = None
    return files, bf.calls, said


EVERY = ["--corealignment", "c.fa", "--corepartitions", "p.tsv", "--coresnps", "s.fa", "--coresites", "s.tsv", "--corefiltered", "f.fa", "--corefilteredsites", "fs.tsv",
         "--coredense", "d.tsv", "--corepresence", "h.tsv", "--coretree", "t.nwk", "--corefilteredtree", "ft.nwk"]


def test_core_files_runs_the_soft_core_inside_set_partial_and_the_strict_core_without():
    for argv in (EVERY, EVERY + ["--coremin", "3"]):
        files, calls, said = run_core_files(argv)
        assert not any(name in ("set_partial", "group_bootstrap_pairs") for name, _ in calls) and said == []
        assert not any(v.startswith(b"#") and b"coremin" in v for v in files.values())
        assert files["h.tsv"] == b"block\tx.fa\ty.fa\tz.fa\n4\t1\t1\t1\n"
    strict_tree = files["t.nwk"]
    files, calls, said = run_core_files(EVERY + ["--coremin", "2", "--gapopen", "9", "--multimaf", "m.maf"])
    assert calls[0] == ("set_partial", True) and calls[-1] == ("set_partial", False) and [c for c in calls if c[0] == "set_partial"] == [calls[0], calls[-1]]
    assert all(on for name, on in calls[1:-1] if name != "set_masked") and [name for name, _ in calls].count("group_bootstrap_pairs") == 2 and said == []
    assert files["h.tsv"] == b"# gapopen=9\n# coremin=2\nblock\tx.fa\ty.fa\tz.fa\n4\t1\t1\t1\n9\t1\t0\t1\n"
    for name in ("p.tsv", "s.tsv", "fs.tsv"):
        assert files[name].startswith(b"# gapopen=9\n# coremin=2\n"), name
    assert files["d.tsv"].startswith(b"# densitywindow=1000 densitymax=3\n# gapopen=9\n# coremin=2\n")
    assert not files["c.fa"].startswith(b"#") and files["t.nwk"] == strict_tree       # a uniform matrix is the scalar
    assert list(files) == ["c.fa", "p.tsv", "s.fa", "s.tsv", "f.fa", "fs.tsv", "d.tsv", "h.tsv", "t.nwk", "ft.nwk"]


def test_core_files_switches_the_setting_off_after_an_error():
    files, calls, _ = run_core_files(["--coresnps", "s.fa", "--coremin", "2"], fail=True)
    assert files is None and calls == [("set_partial", True), ("set_partial", False)]


def test_a_tree_is_not_written_where_two_files_share_no_column():
    files, calls, said = run_core_files(["--coretree", "t.nwk", "--corepresence", "h.tsv", "--coremin", "2"], pairs=[[100, 0, 100], [0, 50, 50], [100, 50, 100]])
    assert list(files) == ["h.tsv"] and calls[-1] == ("set_partial", False)
    assert said == ["--coretree not written: files x.fa and y.fa share no column in which both hold one of A C G T: they have no distance\n"]


def test_no_core_block_states_the_coremin_in_force():
    def none(argv):
        opt = P.parse_args(BASE + argv + THREE)
        said = []
        P.core_files(FakeFinder(), opt, ["x", "y", "z"], [], [], [], set(), said.append)
        return said
    assert none(["--corepartitions", "p.tsv"]) == ["no core block: no block has exactly one instance of at least 5000 bases in every input file and was aligned\n"]
    (line,) = none(["--corepartitions", "p.tsv", "--coremin", "2", "-m", "700"])
    assert line.startswith("no core block: ") and "at least 700 bases" in line and "--coremin 2" in line and "at least 2 input files" in line and line.endswith("\n")


def test_tree_with_a_matrix_of_columns_per_pair():
    M = np.array([[[0, 3, 5, 6], [3, 0, 4, 7], [5, 4, 0, 2], [6, 7, 2, 0]]] * 3, dtype=np.uint64)
    M[1, 0, 1] = M[1, 1, 0] = 9
    names = ["a.fa", "b.fa", "c.fa", "d.fa"]
    for model in tree.MODELS:
        scalar = tree.tree_text(M, 40, model, names)
        assert tree.tree_text(M, np.full((4, 4), 40, dtype=np.uint64), model, names) == scalar
        assert tree.tree_text(M, [[40] * 4] * 4, model, names) == scalar
        assert (tree.distances(M[0], np.full((4, 4), 40), model) == tree.distances(M[0], 40, model)).all()
    K = np.full((4, 4), 40, dtype=np.uint64)
    K[1, 3] = K[3, 1] = 20                                                          # a pair over fewer columns is further apart
    assert tree.distances(M[0], K)[1, 3] == 7 / 20 and tree.distances(M[0], K)[0, 1] == 3 / 40
    assert tree.tree_text(M, K, "p", names) != tree.tree_text(M, 40, "p", names)
    K[2, 2] = 0                                                                     # a diagonal cell is no pair
    assert tree.distances(M[0], K)[2, 2] == 0
    K[1, 3] = K[3, 1] = 0
    with pytest.raises(tree.NoSharedColumn) as e:
        tree.distances(M[0], K)
    assert e.value.pair == (1, 3) and "files 1 and 3 " in str(e.value)
    with pytest.raises(tree.NoSharedColumn) as e:
        tree.tree_text(M, K, "p", names)
    assert e.value.pair == (1, 3) and "files b.fa and d.fa share no column" in str(e.value)
    with pytest.raises(ValueError):
        tree.distances(M[0], np.full((3, 3), 40))
