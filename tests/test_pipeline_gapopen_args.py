"""The command line of --gapopen (sibelia_amd/pipeline.py) and the header lines that record it (sibelia_amd/formats.py): device-free."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import formats, pipeline as P      # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
TWO = ["x.fa", "y.fa"]


def test_gapopen_is_off_by_default_and_has_no_short_form():
    assert P.parse_args(BASE + ["--maf", "a.maf"] + TWO).gapopen == 0
    assert P.parse_args(BASE + TWO).gapopen == 0
    assert not [a for a in P.build_parser()._actions if "--gapopen" in a.option_strings and len(a.option_strings) != 1]


@pytest.mark.parametrize("with_option", [["--maf", "a.maf"], ["--variants", "v.vcf"], ["--multimaf", "m.maf"],
                                         ["--maf", "a.maf", "--variants", "v.vcf", "--multimaf", "m.maf"]])
@pytest.mark.parametrize("value", [0, 1, 300, 100000])
def test_gapopen_parses_next_to_an_alignment_option(with_option, value):
    assert P.parse_args(BASE + with_option + ["--gapopen", str(value)] + TWO).gapopen == value


def test_gapopen_goes_with_multimaf_on_any_number_of_files():
    assert P.parse_args(BASE + ["--multimaf", "m.maf", "--gapopen", "300", "x.fa"]).gapopen == 300
    assert P.parse_args(BASE + ["--multimaf", "m.maf", "--gapopen", "300", "x.fa", "y.fa", "z.fa"]).gapopen == 300


@pytest.mark.parametrize("value", ["100001", "-1", "4294967296", "x", "3.5", ""])
def test_values_outside_the_range_are_refused(value):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + ["--maf", "a.maf", "--gapopen=" + value] + TWO)
    assert "--gapopen" in str(e.value)


@pytest.mark.parametrize("argv", [[], ["--correctboundaries"], ["-q"], ["--allstages"]])
def test_gapopen_needs_an_alignment_option(argv):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv + ["--gapopen", "300"] + TWO)
    assert str(e.value) == "--gapopen sets a cost of the alignments: it needs at least one of --maf, --variants and --multimaf"
    with pytest.raises(P.PipelineError):
        P.parse_args(BASE + argv + ["--gapopen", "0"] + TWO)                         # 0 is the option too
    assert P.parse_args(BASE + argv + TWO).gapopen == 0


def test_the_refusal_is_reported_by_main_before_any_file_is_read(tmp_path, capsys):
    assert P.main(BASE + ["--gapopen", "300", str(tmp_path / "missing.fa")]) == 1
    assert capsys.readouterr().err == "error: --gapopen sets a cost of the alignments: it needs at least one of --maf, --variants and --multimaf\n"


def test_planned_files_do_not_change():
    for argv, files in ((["--maf", "a.maf", "--variants", "v.vcf"], TWO), (["--multimaf", "m.maf", "-q", "-g"], ["x.fa"]),
                        (["--maf", "a.maf", "--variants", "v.vcf", "--allstages", "--uncovered", "--unmapped", "u.fa"], TWO)):
        without = P.planned_files(P.parse_args(BASE + argv + files), 3)
        for value in ("0", "300"):
            assert P.planned_files(P.parse_args(BASE + argv + ["--gapopen", value] + files), 3) == without


def test_help_says_what_the_option_costs_and_what_it_leaves_alone():
    text = " ".join(P.build_parser().format_help().split())
    at = text.rindex("--gapopen N")
    mine = text[at:text.index("--device", at)]
    assert "100000" in mine and "default 0" in mine and "N + 75 L" in mine
    assert "Not applied to --correctboundaries" in mine and "reference program's own" in mine


def test_the_header_lines():
    groups = [[b"s a 0 2 + 9 AC", b"s b 0 2 + 9 AC"]]
    plain = formats.maf_text(groups)
    assert formats.maf_text(groups, 0) == plain and plain.startswith(b"##maf version=1\n\na\n")
    assert formats.maf_text(groups, 300) == plain.replace(b"##maf version=1\n", b"##maf version=1\n# gapopen=300\n", 1)
    records = [("ref", 5, b"A", b"C")]
    vcf = formats.vcf_text("ref", records)
    assert formats.vcf_text("ref", records, 0) == vcf
    assert formats.vcf_text("ref", records, 300) == vcf.replace(b"##source=sibelia_amd\n", b"##source=sibelia_amd\n##sibelia_amd_gapopen=300\n", 1)
    import numpy as np
    calls = np.zeros(0, dtype=[("kind", "<u4"), ("chr", "<u4"), ("start", "<u8"), ("end", "<u8"), ("ref_chr", "<u4"), ("pad_", "<u4"), ("pos", "<u8")])
    base = formats.vcf_pieces(["ref", "asm"], 9, b"A", records, calls, True)
    with_cost = formats.vcf_pieces(["ref", "asm"], 9, b"A", records, calls, True, 300)
    assert bytes(formats.vcf_pieces(["ref", "asm"], 9, b"A", records, calls, True, 0).literals) == bytes(base.literals)
    assert bytes(with_cost.literals) == bytes(base.literals).replace(b"##source=sibelia_amd\n", b"##source=sibelia_amd\n##sibelia_amd_gapopen=300\n", 1)


def test_the_pipeline_module_still_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; "
            "o = P.parse_args(['-s', 'fine', '--maf', 'a.maf', '--gapopen', '300', 'x.fa', 'y.fa']); P.planned_files(o, 3); "
            "assert o.gapopen == 300 and A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
