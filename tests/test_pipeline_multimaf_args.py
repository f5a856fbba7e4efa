"""The command line of --multimaf (sibelia_amd/pipeline.py): device-free."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]


@pytest.mark.parametrize("files", [["x.fa"], ["x.fa", "y.fa"], ["x.fa", "y.fa", "z.fa"]])
def test_multimaf_parses_with_any_number_of_files(files):
    o = P.parse_args(BASE + ["--multimaf", "m.maf"] + files)
    assert (o.multimaf, o.filenames, o.maf, o.variants) == ("m.maf", files, None, None)


def test_multimaf_has_no_short_form_and_is_off_by_default():
    assert P.parse_args(BASE + ["-m", "500", "x.fa"]).multimaf is None           # -m stays --minblocksize
    assert not [a for a in P.build_parser()._actions if "--multimaf" in a.option_strings and len(a.option_strings) != 1]


def test_multimaf_contradicts_noblocks():
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--multimaf", "m.maf", "--noblocks", "x.fa", "y.fa", "z.fa"])
    assert str(e.value) == "--multimaf needs the synteny blocks: it cannot be combined with --noblocks"


@pytest.mark.parametrize("argv, message", [
    (["--maf", "x.out", "--multimaf", "x.out"], "--maf and --multimaf name the same file: x.out"),
    (["--variants", "sub/../x.out", "--multimaf", "./x.out"], "--variants and --multimaf name the same file: sub/../x.out"),
    (["--multimaf", "blocks_coords.txt"], "--multimaf names a file the program writes itself: blocks_coords.txt"),
    (["--multimaf", "./coverage_report.txt"], "--multimaf names a file the program writes itself: ./coverage_report.txt"),
    (["--allstages", "--multimaf", "blocks_coords2.txt"], "--multimaf names a file the program writes itself: blocks_coords2.txt"),
    (["--multimaf", "sub/"], "--multimaf needs a file name, not 'sub/'"),
])
def test_output_names_that_collide_are_refused_before_any_file_is_read(argv, message, tmp_path):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv + [str(tmp_path / "missing_x.fa"), str(tmp_path / "missing_y.fa")])
    assert str(e.value) == message


def test_a_collision_is_reported_by_main_before_any_file_is_read(tmp_path, capsys):
    assert P.main(BASE + ["--multimaf", "blocks_coords.txt", str(tmp_path / "missing.fa")]) == 1
    assert capsys.readouterr().err == "error: --multimaf names a file the program writes itself: blocks_coords.txt\n"


def test_planned_files_list_the_output():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv, files: P.planned_files(P.parse_args(BASE + argv + files), 3)      # noqa: E731
    assert plan(["--multimaf", "m.maf"], ["x.fa"]) == base + ["m.maf"]
    assert plan(["--multimaf", "sub/m.maf", "-q", "-g"], ["x.fa", "y.fa", "z.fa"]) == base + ["blocks_sequences.fasta", "sub/m.maf", "de_bruijn_graph.dot"]
    assert plan(["--maf", "a.maf", "--variants", "v.vcf", "--multimaf", "m.maf"], ["x.fa", "y.fa"]) == base + ["a.maf", "v.vcf", "m.maf"]


def test_maf_with_three_files_still_fails_with_its_message():
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--maf", "a.maf", "--multimaf", "m.maf", "x.fa", "y.fa", "z.fa"])
    assert str(e.value) == "In alignment mode only two FASTA files are acceptable"


def test_help_says_what_is_aligned_and_that_it_is_not_mlagan():
    text = " ".join(P.build_parser().format_help().split())
    at = text.rindex("--multimaf FILE")                                         # the option's own entry, not the usage line
    mine = text[at:text.index("--device", at)]
    assert "at least two instances" in mine and "centre-star" in mine and "first instance" in mine and "not mlagan" in mine


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--multimaf', 'm.maf', 'x.fa', 'y.fa', 'z.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
