"""The command line of --maf / --variants (sibelia_amd/pipeline.py): device-free."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]


@pytest.mark.parametrize("option", [["--maf", "a.maf"], ["--variants", "v.vcf"], ["--maf", "a.maf", "--variants", "v.vcf"]])
@pytest.mark.parametrize("files", [["x.fa"], ["x.fa", "y.fa", "z.fa"]])
def test_alignment_options_need_exactly_two_files(option, files):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + option + files)
    assert str(e.value) == "In alignment mode only two FASTA files are acceptable"


def test_the_file_count_is_checked_before_any_file_is_read(tmp_path, capsys):
    assert P.main(BASE + ["--maf", "a.maf", str(tmp_path / "missing.fa")]) == 1
    assert capsys.readouterr().err == "error: In alignment mode only two FASTA files are acceptable\n"


@pytest.mark.parametrize("option", [["--maf", "a.maf"], ["--variants", "v.vcf"]])
def test_alignment_options_contradict_noblocks(option):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + option + ["--noblocks", "x.fa", "y.fa"])
    assert str(e.value) == "--maf and --variants need the synteny blocks: they cannot be combined with --noblocks"


@pytest.mark.parametrize("argv, message", [
    (["--maf", "x.out", "--variants", "x.out"], "--maf and --variants name the same file: x.out"),
    (["--maf", "sub/../x.out", "--variants", "./x.out"], "--maf and --variants name the same file: sub/../x.out"),
    (["--maf", "blocks_coords.txt"], "--maf names a file the program writes itself: blocks_coords.txt"),
    (["--variants", "./coverage_report.txt"], "--variants names a file the program writes itself: ./coverage_report.txt"),
    (["--allstages", "--maf", "blocks_coords2.txt"], "--maf names a file the program writes itself: blocks_coords2.txt"),
    (["-g", "--variants", "de_bruijn_graph.dot"], "--variants names a file the program writes itself: de_bruijn_graph.dot"),
    (["--maf", "sub/"], "--maf needs a file name, not 'sub/'"),
    (["--variants", ""], "--variants needs a file name, not ''"),
])
def test_output_names_that_collide_are_refused_before_any_file_is_read(argv, message):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv + ["x.fa", "y.fa"])
    assert str(e.value) == message


def test_a_reserved_name_in_another_directory_is_a_name_like_any_other():
    o = P.parse_args(BASE + ["--maf", "sub/blocks_coords.txt", "--variants", "sub/v.vcf", "x.fa", "y.fa"])
    assert (o.maf, o.variants) == ("sub/blocks_coords.txt", "sub/v.vcf")


def test_both_options_parse_with_two_files_and_have_no_short_form():
    o = P.parse_args(BASE + ["--maf", "a.maf", "--variants", "v.vcf", "--correctboundaries", "x.fa", "y.fa"])
    assert (o.maf, o.variants, o.filenames) == ("a.maf", "v.vcf", ["x.fa", "y.fa"])
    o = P.parse_args(BASE + ["-v", "x.fa", "y.fa"])                 # -v stays --visualize
    assert o.visualize and o.maf is None and o.variants is None


def test_planned_files_list_both_outputs():
    base = ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv: P.planned_files(P.parse_args(BASE + argv + ["x.fa", "y.fa"]), 3)      # noqa: E731
    assert plan([]) == base
    assert plan(["--maf", "a.maf"]) == base + ["a.maf"]
    assert plan(["--variants", "v.vcf"]) == base + ["v.vcf"]
    assert plan(["-q", "-g", "--maf", "a.maf", "--variants", "sub/v.vcf"]) == base + ["blocks_sequences.fasta", "a.maf", "sub/v.vcf", "de_bruijn_graph.dot"]


def test_a_planned_name_with_a_directory_part_gets_its_directory(tmp_path):
    out = tmp_path / "out"
    P.write_files(str(out), {"blocks_coords.txt": b"x\n", "sub/deeper/v.vcf": b"y\n"})
    assert (out / "blocks_coords.txt").read_bytes() == b"x\n" and (out / "sub" / "deeper" / "v.vcf").read_bytes() == b"y\n"


def test_help_says_which_blocks_are_not_aligned():
    text = " ".join(P.build_parser().format_help().split())
    assert "--maf" in text and "--variants" in text and "mlagan" in text and "not aligned" in text


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--maf', 'a.maf', '--variants', 'v.vcf', 'x.fa', 'y.fa']); P.planned_files(o, 3); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
