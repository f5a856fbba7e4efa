"""The command line of --corealignment / --corepartitions / --coresnps / --coresites (sibelia_amd/pipeline.py), the rule that picks
the core blocks and the two tables (sibelia_amd/formats.py): device-free."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import formats            # noqa: E402
from sibelia_amd import pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
OPTIONS = ("--corealignment", "--corepartitions", "--coresnps", "--coresites")


@pytest.mark.parametrize("option", OPTIONS)
def test_each_option_exists_once_and_is_in_the_help(option):
    actions = [a for a in P.build_parser()._actions if option in a.option_strings]
    assert len(actions) == 1 and actions[0].option_strings == [option] and actions[0].default is None
    assert option + " FILE" in " ".join(P.build_parser().format_help().split())
    o = P.parse_args(BASE + [option, "c.out", "a/x.fa", "y.fa", "z.fa"])
    assert getattr(o, option[2:]) == "c.out" and o.gapopen == 0 and P.core_wanted(o)
    assert [getattr(o, other[2:]) for other in OPTIONS if other != option] == [None] * 3
    off = P.parse_args(BASE + ["x.fa", "y.fa"])
    assert [getattr(off, other[2:]) for other in OPTIONS] == [None] * 4 and not P.core_wanted(off)


def test_help_says_what_a_core_block_is():
    text = " ".join(P.build_parser().format_help().split())
    mine = text[text.rindex("--corealignment FILE"):text.rindex("--corepartitions FILE")]
    assert "exactly one instance in every input file" in mine and "FASTA" in mine and "base name" in mine and "80" in mine
    assert "A C G T" in text[text.rindex("--coresnps FILE"):text.rindex("--coresites FILE")]


@pytest.mark.parametrize("option", OPTIONS)
def test_argument_rules_of_each_option(option):
    for argv, message in [
            ([option, "c.out", "x.fa"], "%s compares files: it needs at least two" % option),
            ([option, "c.out", "--noblocks", "x.fa", "y.fa"], "%s needs the synteny blocks: it cannot be combined with --noblocks" % option),
            ([option, "c.out", "y.fa", "a/x.fa", "b/x.fa"], "%s names a file by its base name: two files are called x.fa" % option),
            ([option, "coverage_report.txt", "x.fa", "y.fa"], "%s names a file the program writes itself: coverage_report.txt" % option),
            ([option, "blocks_coords3.txt", "x.fa", "y.fa"], "%s names a file the program writes itself: blocks_coords3.txt" % option),
            ([option, "sub/", "x.fa", "y.fa"], "%s needs a file name, not 'sub/'" % option),
            ([option, "", "x.fa", "y.fa"], "%s needs a file name, not ''" % option),
            (["--multimaf", "c.out", option, "./c.out", "x.fa", "y.fa"], "--multimaf and %s name the same file: c.out" % option),
            (["--distancecounts", "c.out", option, "c.out", "x.fa", "y.fa"], "--distancecounts and %s name the same file: c.out" % option)]:
        with pytest.raises(P.PipelineError) as e:
            P.parse_args(BASE + argv)
        assert str(e.value) == message


def test_two_core_options_do_not_share_a_file():
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--coresnps", "c.fa", "--corealignment", "c.fa", "x.fa", "y.fa"])
    assert str(e.value) == "--corealignment and --coresnps name the same file: c.fa"
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--corepartitions", "t.tsv", "--coresites", "sub/../t.tsv", "x.fa", "y.fa"])
    assert str(e.value) == "--corepartitions and --coresites name the same file: t.tsv"


def test_white_space_in_a_file_name_is_fine():
    assert P.parse_args(BASE + ["--corealignment", "c.fa", "x.fa", "my genome.fa"]).corealignment == "c.fa"


@pytest.mark.parametrize("option", OPTIONS)
def test_gapopen_and_wideband_are_accepted_with_each_alone(option):
    o = P.parse_args(BASE + [option, "c.out", "--gapopen", "400", "--wideband", "x.fa", "y.fa"])
    assert o.gapopen == 400 and o.wideband


def test_main_reports_the_error_before_any_file_is_read(tmp_path, capsys):
    assert P.main(BASE + ["--coresnps", "s.fa", str(tmp_path / "missing.fa")]) == 1
    assert capsys.readouterr().err == "error: --coresnps compares files: it needs at least two\n"


def test_planned_files_list_the_four_after_distancecounts():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv, files: P.planned_files(P.parse_args(BASE + argv + files), 3)      # noqa: E731
    assert plan(["--coresites", "s.tsv", "--coresnps", "s.fa", "--corepartitions", "p.tsv", "--corealignment", "c.fa"], ["x.fa", "y.fa"]) == base + ["c.fa", "p.tsv", "s.fa", "s.tsv"]
    assert plan(["--coresnps", "sub/s.fa"], ["x.fa", "y.fa", "z.fa"]) == base + ["sub/s.fa"]
    assert plan(["--coresites", "s.tsv", "--corealignment", "c.fa", "--distances", "d.phy", "--distancecounts", "d.tsv", "--multivariants", "m.vcf", "--multimaf", "m.maf", "-q", "-g"],
                ["x.fa", "y.fa", "z.fa"]) == base + ["blocks_sequences.fasta", "m.maf", "m.vcf", "d.phy", "d.tsv", "c.fa", "s.tsv", "de_bruijn_graph.dot"]


def test_core_blocks():
    """records 0, 1: the first file; 2: the second; 3, 4: the third"""
    rows = [(1, 0, 0, 600), (-1, 2, 0, 600), (1, 3, 0, 600),              # one per file: in
            (2, 0, 700, 1300), (2, 1, 0, 600), (2, 2, 700, 1300),         # two instances in the first file, none in the third: out
            (3, 0, 4000, 4600), (3, 2, 4000, 4499), (-3, 4, 0, 700),      # an instance shorter than -m: out
            (4, 2, 2000, 2600), (-4, 3, 2000, 2600),                      # missing from the first file: out (--distances takes it)
            (5, 1, 6000, 6600),                                           # a single instance: out
            (6, 0, 5000, 5600), (6, 2, 5000, 5600), (6, 3, 5000, 5600), (6, 4, 5000, 5600),      # two instances in the third file: out
            (-7, 1, 100, 900), (7, 2, 3000, 3800), (-7, 4, 900, 1700)]    # one per file, on other records: in
    blocks = np.array(rows, dtype=formats.BLOCK_DTYPE)
    assert P.core_blocks(blocks, [2, 1, 2], 600) == [1, 7]
    assert P.core_blocks(blocks, [2, 1, 2], 499) == [1, 3, 7]
    assert P.core_blocks(blocks, [2, 1, 2], 601) == [7]
    assert P.core_blocks(blocks, [2, 1, 1, 1], 600) == [6]                        # other files: block 6 has one in each of four
    assert P.core_blocks(blocks[:0], [2, 1, 2], 600) == []
    for m in (499, 600, 601):                                                    # the subset of distance_blocks that reaches every file
        assert set(P.core_blocks(blocks, [2, 1, 2], m)) <= set(P.distance_blocks(blocks, [2, 1, 2], m))
    two = np.array([(1, 0, 0, 600), (1, 1, 0, 600), (2, 0, 700, 1300), (2, 0, 1400, 2000), (3, 1, 700, 1300), (4, 0, 5000, 5600), (4, 1, 5000, 5100)], dtype=formats.BLOCK_DTYPE)
    for m in (50, 600):                                                          # for two files the two sets are the same
        assert P.core_blocks(two, [1, 1], m) == P.distance_blocks(two, [1, 1], m) == ([1, 4] if m == 50 else [1])


def test_core_headers():
    assert formats.core_headers(["x.fa", "my genome.fa"]) == (b">x.fa\n>my genome.fa\n", [0, 6, 20])
    assert formats.CORE_WIDTH == 80


def test_core_partitions_text_and_the_gapopen_line():
    head = "block\tfirst\tlast\n"
    body = "3\t1\t5000\n8\t5001\t5001\n21\t5002\t11000\n"
    rows = [(3, 0, 5000), (8, 5000, 1), (21, 5001, 5999)]
    assert formats.core_partitions_text(rows) == (head + body).encode()
    assert formats.core_partitions_text(rows, 0) == (head + body).encode()
    assert formats.core_partitions_text(rows, 200) == ("# gapopen=200\n" + head + body).encode()
    assert formats.core_partitions_text([]) == head.encode()
    assert formats.core_partitions_text([], 7) == ("# gapopen=7\n" + head).encode()


def test_core_sites_text_positions_by_strand_and_the_gapopen_line():
    head = "column\tblock\trecord\tposition\tstrand\n"
    # block 3 forwards on [100, 700): the base of index 0 is position 101, of index 599 position 700; block 8 reversed on [1000, 1600):
    # index 0 is the record's position 1600, index 599 position 1001
    rows = [(3, "chr one", 100, 700, False, 0), (3, "chr one", 100, 700, False, 599), (8, "gi|1|ref|NC_000915.1|", 1000, 1600, True, 0), (8, "gi|1|ref|NC_000915.1|", 1000, 1600, True, 599)]
    body = "1\t3\tchr one\t101\t+\n2\t3\tchr one\t700\t+\n3\t8\tgi|1|ref|NC_000915.1|\t1600\t-\n4\t8\tgi|1|ref|NC_000915.1|\t1001\t-\n"
    assert formats.core_sites_text(rows) == (head + body).encode()
    assert formats.core_sites_text(rows, 300) == ("# gapopen=300\n" + head + body).encode()
    assert formats.core_sites_text([]) == head.encode()


@pytest.mark.parametrize("argv, files, plan", [
    ([], ["x.fa"], []),
    (["--multimaf", "m.maf"], ["x.fa"], ["m.maf"]),
    (["--maf", "a.maf", "--variants", "v.vcf"], ["x.fa", "y.fa"], ["a.maf", "v.vcf"]),
    (["--multivariants", "m.vcf", "--distances", "d.phy", "--distancecounts", "d.tsv", "--gapopen", "9"], ["x.fa", "y.fa", "z.fa"], ["m.vcf", "d.phy", "d.tsv"]),
])
def test_existing_option_sets_plan_what_they_planned(argv, files, plan):
    o = P.parse_args(BASE + argv + files)
    assert not P.core_wanted(o)
    assert P.planned_files(o, 3) == ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"] + plan


@pytest.mark.parametrize("argv, message", [
    (["--gapopen", "5", "x.fa", "y.fa"], "--gapopen sets a cost of the alignments: it needs at least one of --maf, --variants and --multimaf"),
    (["--wideband", "x.fa", "y.fa"], "--wideband widens the bands of the alignments: it needs at least one of --maf, --variants, --multimaf and --multivariants"),
    (["--distances", "d.phy", "x.fa"], "--distances compares files: it needs at least two"),
    (["--multivariants", "m.vcf", "a/x.fa", "b/x.fa", "c/x.fa"], "--multivariants names a sample by its file's base name: two files are called x.fa"),
    (["--distances", "d.out", "--distancecounts", "./d.out", "x.fa", "y.fa"], "--distances and --distancecounts name the same file: d.out"),
    (["--maf", "a.maf", "x.fa"], "In alignment mode only two FASTA files are acceptable"),
])
def test_existing_errors_keep_their_words(argv, message):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv)
    assert str(e.value) == message


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--corealignment', 'c.fa', '--coresites', 's.tsv', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
