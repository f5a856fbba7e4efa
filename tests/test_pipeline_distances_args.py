"""The command line of --distances / --distancecounts (sibelia_amd/pipeline.py), the rule that picks their blocks and the two texts
(sibelia_amd/formats.py): device-free."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import formats            # noqa: E402
from sibelia_amd import pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
OPTIONS = ("--distances", "--distancecounts")


@pytest.mark.parametrize("option", OPTIONS)
def test_each_option_exists_once_and_is_in_the_help(option):
    actions = [a for a in P.build_parser()._actions if option in a.option_strings]
    assert len(actions) == 1 and actions[0].option_strings == [option] and actions[0].default is None
    assert option + " FILE" in " ".join(P.build_parser().format_help().split())
    o = P.parse_args(BASE + [option, "d.out", "a/x.fa", "y.fa", "z.fa"])
    assert getattr(o, option[2:]) == "d.out" and o.gapopen == 0
    assert P.file_names(o.filenames) == ["x.fa", "y.fa", "z.fa"]
    off = P.parse_args(BASE + ["x.fa", "y.fa"])
    assert off.distances is None and off.distancecounts is None


def test_help_says_which_blocks_are_used():
    text = " ".join(P.build_parser().format_help().split())
    mine = text[text.rindex("--distances FILE"):text.rindex("--distancecounts FILE")]
    assert "at most one in each file" in mine and "PHYLIP" in mine and "base names" in mine and "No correction" in mine


@pytest.mark.parametrize("argv, message", [
    (["--distances", "d.phy", "x.fa"], "--distances compares files: it needs at least two"),
    (["--distancecounts", "d.tsv", "x.fa"], "--distancecounts compares files: it needs at least two"),
    (["--distances", "d.phy", "--noblocks", "x.fa", "y.fa"], "--distances needs the synteny blocks: it cannot be combined with --noblocks"),
    (["--distancecounts", "d.tsv", "--noblocks", "x.fa", "y.fa"], "--distancecounts needs the synteny blocks: it cannot be combined with --noblocks"),
    (["--distances", "d.phy", "a/x.fa", "b/x.fa"], "--distances names a file by its base name: two files are called x.fa"),
    (["--distancecounts", "d.tsv", "y.fa", "a/x.fa", "b/x.fa"], "--distancecounts names a file by its base name: two files are called x.fa"),
    (["--distances", "d.phy", "x.fa", "my genome.fa"], "--distances writes PHYLIP, which separates by blanks: the file name 'my genome.fa' holds white space"),
    (["--distances", "d.out", "--distancecounts", "./d.out", "x.fa", "y.fa"], "--distances and --distancecounts name the same file: d.out"),
    (["--multimaf", "d.out", "--distancecounts", "d.out", "x.fa", "y.fa"], "--multimaf and --distancecounts name the same file: d.out"),
    (["--distances", "coverage_report.txt", "x.fa", "y.fa"], "--distances names a file the program writes itself: coverage_report.txt"),
    (["--distancecounts", "sub/", "x.fa", "y.fa"], "--distancecounts needs a file name, not 'sub/'"),
    (["--gapopen", "5", "x.fa", "y.fa"], "--gapopen sets a cost of the alignments: it needs at least one of --maf, --variants and --multimaf"),
    (["--wideband", "x.fa", "y.fa"], "--wideband widens the bands of the alignments: it needs at least one of --maf, --variants, --multimaf and --multivariants"),
])
def test_argument_rules(argv, message):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv)
    assert str(e.value) == message


def test_white_space_in_a_name_is_fine_for_the_counts_alone():
    assert P.parse_args(BASE + ["--distancecounts", "d.tsv", "x.fa", "my genome.fa"]).distancecounts == "d.tsv"


@pytest.mark.parametrize("option", OPTIONS)
def test_gapopen_and_wideband_are_accepted_with_either_alone(option):
    o = P.parse_args(BASE + [option, "d.out", "--gapopen", "400", "--wideband", "x.fa", "y.fa"])
    assert o.gapopen == 400 and o.wideband


def test_main_reports_the_error_before_any_file_is_read(tmp_path, capsys):
    assert P.main(BASE + ["--distances", "d.phy", str(tmp_path / "missing.fa")]) == 1
    assert capsys.readouterr().err == "error: --distances compares files: it needs at least two\n"


def test_planned_files_list_the_output_after_multivariants():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv, files: P.planned_files(P.parse_args(BASE + argv + files), 3)      # noqa: E731
    assert plan(["--distancecounts", "d.tsv", "--distances", "d.phy"], ["x.fa", "y.fa"]) == base + ["d.phy", "d.tsv"]
    assert plan(["--distancecounts", "sub/d.tsv"], ["x.fa", "y.fa", "z.fa"]) == base + ["sub/d.tsv"]
    assert plan(["--distances", "d.phy", "--distancecounts", "d.tsv", "--multivariants", "m.vcf", "--multimaf", "m.maf", "-q", "-g"], ["x.fa", "y.fa", "z.fa"]) == \
        base + ["blocks_sequences.fasta", "m.maf", "m.vcf", "d.phy", "d.tsv", "de_bruijn_graph.dot"]


def test_distance_blocks():
    """records 0, 1: the first file; 2: the second; 3, 4: the third"""
    rows = [(1, 0, 0, 600), (-1, 2, 0, 600), (1, 3, 0, 600),              # one per file
            (2, 0, 700, 1300), (2, 1, 0, 600), (2, 2, 700, 1300),         # two instances in one file: out
            (3, 0, 4000, 4600), (3, 2, 4000, 4499),                       # an instance shorter than -m: out
            (4, 2, 2000, 2600), (-4, 3, 2000, 2600),                      # none in the first file: in
            (5, 1, 6000, 6600),                                           # a single instance: out
            (6, 0, 5000, 5600), (6, 2, 5000, 5600), (6, 3, 5000, 5010)]   # a short one next to two long ones: out
    blocks = np.array(rows, dtype=formats.BLOCK_DTYPE)
    assert P.distance_blocks(blocks, [2, 1, 2], 600) == [1, 4]
    assert P.distance_blocks(blocks, [2, 1, 2], 499) == [1, 3, 4]
    assert P.distance_blocks(blocks, [2, 1, 2], 10) == [1, 3, 4, 6]
    assert P.distance_blocks(blocks, [1, 1, 1, 2], 600) == [1, 2, 4]             # other files: block 2 has one in each of three
    assert P.distance_blocks(blocks[:0], [2, 1, 2], 600) == []
    assert P.qualifying_blocks(blocks, [2, 1, 2], 600) == [1]                    # --multivariants asks for the first file as well


def test_p_distance_rounds_at_the_sixth_digit_from_the_integers():
    assert formats.p_distance_text(10, 0) == "0.000000"
    assert formats.p_distance_text(0, 7) == "1.000000"
    assert formats.p_distance_text(0, 0) == "nan"
    assert formats.p_distance_text(2, 1) == "0.333333" and formats.p_distance_text(1, 2) == "0.666667"
    assert formats.p_distance_text(1999999, 1) == "0.000001"                     # 0.0000005: a tie goes up
    assert formats.p_distance_text(2000000, 1) == "0.000000"                     # just below it
    assert formats.p_distance_text(7, 1) == "0.125000"
    assert formats.p_distance_text(3 * 10 ** 18, 10 ** 18) == "0.250000"         # beyond 53 bits: no float is involved
    assert formats.p_distance_text(np.uint64(3), np.uint64(1)) == "0.250000"


def matrix(n, cells):
    M = np.zeros((n, n, 4), dtype=np.uint64)
    for (a, b), v in cells.items():
        M[a, b] = v
    return M


def test_distances_text_and_the_pair_without_a_column():
    M = matrix(3, {(0, 1): (90, 10, 3, 4), (1, 0): (90, 10, 3, 5), (0, 2): (0, 0, 2, 7), (2, 0): (0, 0, 2, 1), (1, 2): (2, 1, 0, 0), (2, 1): (2, 1, 0, 0), (1, 1): (8, 8, 8, 8)})
    said = []
    text = formats.distances_text(["x.fa", "y.fa", "z.fa"], M, said.append)
    assert text == b"3\nx.fa 0.000000 0.100000 nan\ny.fa 0.100000 0.000000 0.333333\nz.fa nan 0.333333 0.000000\n"
    assert said == ["no distance between x.fa and z.fa: the blocks used hold no column with one of A C G T in both\n"]
    assert formats.distances_text(["x.fa", "y.fa", "z.fa"], M) == text


def test_distance_counts_text_columns_and_the_gapopen_line():
    M = matrix(3, {(0, 1): (90, 10, 3, 4), (1, 0): (90, 10, 3, 5), (0, 2): (0, 0, 2, 7), (2, 0): (0, 0, 2, 1), (1, 2): (2, 1, 0, 0), (2, 1): (2, 1, 0, 6)})
    blocks = [[0, 4, 1], [4, 0, 2], [1, 2, 0]]
    head = "file_a\tfile_b\tblocks\tmatch\tmismatch\tambiguous\tgap_a\tgap_b\n"
    body = "x.fa\ty.fa\t4\t90\t10\t3\t4\t5\nx.fa\tz.fa\t1\t0\t0\t2\t7\t1\ny.fa\tz.fa\t2\t2\t1\t0\t0\t6\n"
    assert formats.distance_counts_text(["x.fa", "y.fa", "z.fa"], M, blocks) == (head + body).encode()
    assert formats.distance_counts_text(["x.fa", "y.fa", "z.fa"], M, blocks, 0) == (head + body).encode()
    assert formats.distance_counts_text(["x.fa", "y.fa", "z.fa"], M, blocks, 200) == ("# gapopen=200\n" + head + body).encode()


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--distances', 'd.phy', '--distancecounts', 'd.tsv', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
