"""The command line of --multivariants (sibelia_amd/pipeline.py) and the rule that picks its blocks: device-free."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import formats            # noqa: E402
from sibelia_amd import pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]


@pytest.mark.parametrize("files", [["x.fa", "y.fa"], ["x.fa", "y.fa", "z.fa"], ["a/x.fa", "b/y.fa", "z.fa", "w.fa"]])
def test_multivariants_parses_with_two_or_more_files(files):
    o = P.parse_args(BASE + ["--multivariants", "m.vcf"] + files)
    assert (o.multivariants, o.filenames, o.multimaf, o.maf, o.variants, o.gapopen) == ("m.vcf", files, None, None, None, 0)
    assert P.sample_names(files) == [os.path.basename(f) for f in files[1:]]


def test_multivariants_is_off_by_default_and_has_no_short_form():
    assert P.parse_args(BASE + ["x.fa", "y.fa"]).multivariants is None
    assert not [a for a in P.build_parser()._actions if "--multivariants" in a.option_strings and len(a.option_strings) != 1]


@pytest.mark.parametrize("argv, message", [
    (["--multivariants", "m.vcf", "x.fa"], "--multivariants compares files: it needs at least two"),
    (["--multivariants", "m.vcf", "--noblocks", "x.fa", "y.fa"], "--multivariants needs the synteny blocks: it cannot be combined with --noblocks"),
    (["--multivariants", "m.vcf", "x.fa", "a/y.fa", "b/y.fa"], "--multivariants names a sample by its file's base name: two files are called y.fa"),
    (["--multimaf", "x.out", "--multivariants", "x.out", "x.fa", "y.fa"], "--multimaf and --multivariants name the same file: x.out"),
    (["--variants", "sub/../v.vcf", "--multivariants", "./v.vcf", "x.fa", "y.fa"], "--variants and --multivariants name the same file: sub/../v.vcf"),
    (["--multivariants", "coverage_report.txt", "x.fa", "y.fa"], "--multivariants names a file the program writes itself: coverage_report.txt"),
    (["--allstages", "--multivariants", "blocks_coords1.txt", "x.fa", "y.fa"], "--multivariants names a file the program writes itself: blocks_coords1.txt"),
    (["--multivariants", "sub/", "x.fa", "y.fa"], "--multivariants needs a file name, not 'sub/'"),
    (["--gapopen", "5", "x.fa", "y.fa"], "--gapopen sets a cost of the alignments: it needs at least one of --maf, --variants and --multimaf"),
    (["--maf", "a.maf", "--multivariants", "m.vcf", "x.fa", "y.fa", "z.fa"], "In alignment mode only two FASTA files are acceptable"),
])
def test_argument_rules(argv, message):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv)
    assert str(e.value) == message


def test_the_first_file_may_share_its_base_name_with_a_sample():
    assert P.parse_args(BASE + ["--multivariants", "m.vcf", "a/x.fa", "b/x.fa"]).multivariants == "m.vcf"


def test_gapopen_is_accepted_with_multivariants_alone():
    assert P.parse_args(BASE + ["--multivariants", "m.vcf", "--gapopen", "400", "x.fa", "y.fa"]).gapopen == 400


def test_main_reports_the_error_before_any_file_is_read(tmp_path, capsys):
    assert P.main(BASE + ["--multivariants", "m.vcf", str(tmp_path / "missing.fa")]) == 1
    assert capsys.readouterr().err == "error: --multivariants compares files: it needs at least two\n"


def test_planned_files_list_the_output():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv, files: P.planned_files(P.parse_args(BASE + argv + files), 3)      # noqa: E731
    assert plan(["--multivariants", "m.vcf"], ["x.fa", "y.fa"]) == base + ["m.vcf"]
    assert plan(["--multivariants", "sub/m.vcf", "--multimaf", "m.maf", "-q", "-g"], ["x.fa", "y.fa", "z.fa"]) == base + ["blocks_sequences.fasta", "m.maf", "sub/m.vcf", "de_bruijn_graph.dot"]
    assert plan(["--maf", "a.maf", "--variants", "v.vcf", "--multimaf", "m.maf", "--multivariants", "m.vcf"], ["x.fa", "y.fa"]) == base + ["a.maf", "v.vcf", "m.maf", "m.vcf"]


def test_qualifying_blocks():
    """records 0, 1: the first file; 2: the second; 3, 4: the third"""
    rows = [(1, 0, 0, 600), (-1, 2, 0, 600), (1, 3, 0, 600),              # one per file
            (2, 1, 0, 600), (2, 4, 0, 700),                               # the second file has no instance
            (3, 0, 700, 1300), (3, 1, 0, 600), (3, 2, 700, 1300),         # two in the first file
            (4, 2, 2000, 2600), (4, 3, 2000, 2600),                       # none in the first file
            (5, 0, 2000, 2600), (5, 3, 3000, 3600), (-5, 4, 3000, 3600),  # two in the third file
            (6, 0, 4000, 4600), (6, 2, 4000, 4499),                       # an instance shorter than -m
            (7, 0, 5000, 5600), (7, 2, 5000, 5600), (7, 3, 5000, 5010),   # ... even if two long ones remain
            (8, 1, 6000, 6600)]                                           # a single instance
    blocks = np.array(rows, dtype=formats.BLOCK_DTYPE)
    assert P.qualifying_blocks(blocks, [2, 1, 2], 600) == [1, 2]
    assert P.qualifying_blocks(blocks, [2, 1, 2], 500) == [1, 2]
    assert P.qualifying_blocks(blocks, [2, 1, 2], 10) == [1, 2, 6, 7]
    assert P.qualifying_blocks(blocks, [2, 3], 600) == [2]                # two files: determine_unique_block (block 1 has two in the second)
    assert P.qualifying_blocks(blocks[:0], [2, 1, 2], 600) == []


def test_help_says_which_blocks_are_used():
    text = " ".join(P.build_parser().format_help().split())
    at = text.rindex("--multivariants FILE")
    mine = text[at:text.index("--gapopen", at)]
    assert "exactly one of them lies in the first file" in mine and "at most one in each other file" in mine and "base name" in mine


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--multivariants', 'm.vcf', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
