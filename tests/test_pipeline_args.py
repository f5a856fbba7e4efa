"""The device-free parts of sibelia_amd/pipeline.py: the reference's command line (reference src/sibelia.cpp:43-185), stage files
(src/util.cpp:11-50), the trimK / lastK rule (src/sibelia.cpp:242-272) and which files an option set yields (:256-345)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from sibelia_amd import pipeline as P      # noqa: E402


def test_the_pipeline_module_does_not_load_the_library():
    code = ("import sys, sibelia_amd.pipeline as P, sibelia_amd.api as A; P.parse_args(['-s', 'loose', 'x.fa']); "
            "assert A._lib is None; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_options_follow_the_reference_letters_and_names():
    o = P.parse_args(["-s", "fine", "-i", "7", "-m", "1234", "-a", "-r", "-t", "tmp", "-o", "out", "-g", "-q", "-v", "--allstages", "--gff",
                      "--lastk", "77", "--nopostprocess", "--noblocks", "--device", "3", "a.fa", "b.fa"])
    assert (o.parameters, o.maxiterations, o.minblocksize, o.sharedonly, o.inram, o.tempdir, o.outdir) == ("fine", 7, 1234, True, True, "tmp", "out")
    assert (o.graphfile, o.sequencesfile, o.visualize, o.allstages, o.gff, o.lastk, o.nopostprocess, o.noblocks, o.device) == (True, True, True, True, True, 77, True, True, 3)
    assert o.filenames == ["a.fa", "b.fa"]
    o = P.parse_args(["--parameters", "far", "--maxiterations", "2", "--minblocksize", "9", "--sharedonly", "--inram", "--tempdir", "t", "--outdir", "o",
                      "--graphfile", "--sequencesfile", "--visualize", "x.fa"])
    assert (o.parameters, o.maxiterations, o.minblocksize, o.sharedonly, o.inram, o.tempdir, o.outdir, o.graphfile, o.sequencesfile, o.visualize) == \
        ("far", 2, 9, True, True, "t", "o", True, True, True)
    d = P.parse_args(["-s", "loose", "x.fa"])          # the reference's defaults
    assert (d.maxiterations, d.minblocksize, d.outdir, d.tempdir, d.lastk, d.device) == (4, 5000, ".", None, None, -1)
    assert P.tempdir_of(d) == "." and P.tempdir_of(o) == "t"
    assert P.tempdir_of(P.parse_args(["-s", "loose", "-o", "out", "x.fa"])) == "out"      # default temp directory: the output directory


def test_parameter_sets_are_the_reference_number_pairs():
    assert P.PARAMETER_SETS == {"loose": [(30, 150), (100, 1000), (1000, 5000), (5000, 15000)],
                                "fine": [(30, 150), (100, 500), (500, 1500)],
                                "far": [(15, 120), (100, 500), (500, 1500)]}
    assert P.stages_of(P.parse_args(["-s", "far", "x.fa"])) == [(15, 120), (100, 500), (500, 1500)]


@pytest.mark.parametrize("argv", [["x.fa"], ["-s", "loose", "-k", "stages.txt", "x.fa"], ["-s", "loose"], ["-s", "coarse", "x.fa"],
                                  ["-s", "loose", "-i", "0", "x.fa"], ["-s", "loose", "--lastk", "1", "x.fa"], ["-s", "loose", "-m", "-5", "x.fa"],
                                  ["-s", "loose", "--correctboundaries", "x.fa"]])
def test_bad_command_lines_are_errors(argv):
    with pytest.raises(P.PipelineError):
        P.parse_args(argv)


def test_a_bad_command_line_prints_error_and_returns_1(capsys):
    assert P.main(["-s", "loose", "-k", "stages.txt", "x.fa"]) == 1
    assert capsys.readouterr().err.startswith("error: ")


def test_a_missing_input_file_is_the_reference_error(tmp_path, capsys):
    assert P.main(["-s", "loose", "-o", str(tmp_path / "out"), str(tmp_path / "nothing.fa")]) == 1
    assert capsys.readouterr().err == "error: Cannot open file %s\n" % (tmp_path / "nothing.fa")
    assert not (tmp_path / "out").exists()


def test_help_says_what_is_not_written():
    text = P.build_parser().format_help()
    assert "circos" in " ".join(text.split()) and "d3_blocks_diagram.html" in " ".join(text.split())


def test_stage_file_grammar():
    assert P.parse_stage_text("3\n30 150\n100 1000\n1000 5000\n") == [(30, 150), (100, 1000), (1000, 5000)]
    assert P.parse_stage_text("  2 30\t150 100\n\n1000 trailing words") == [(30, 150), (100, 1000)]
    assert P.parse_stage_text("0") == []
    assert P.parse_stage_text("1 2 0") == [(2, 0)]
    assert P.parse_stage_text("1 +30 150") == [(30, 150)]


@pytest.mark.parametrize("text, message", [
    ("", "cannot read stage file"),
    ("three", "cannot read stage file"),
    ("-1", "number of stages must be nonnegative"),
    ("2 30 150", "too few records in the stage file"),
    ("2 30 150 100", "too few records in the stage file"),
    ("1 30 x", "too few records in the stage file"),
    ("1 1 150", "vertex size in stage record must be at least 2"),
    ("2 30 150 0 5", "vertex size in stage record must be at least 2"),
    ("1 30 -1", "minimum branch size in stage record must be nonnegative"),
])
def test_stage_file_errors_carry_the_reference_messages(text, message):
    with pytest.raises(P.PipelineError) as e:
        P.parse_stage_text(text)
    assert str(e.value) == message


def test_stage_file_from_disk(tmp_path):
    f = tmp_path / "stages.txt"
    f.write_text("2\n20 100\n200 800\n")
    assert P.stages_of(P.parse_args(["-k", str(f), "x.fa"])) == [(20, 100), (200, 800)]
    with pytest.raises(P.PipelineError) as e:
        P.read_stage_file(str(tmp_path / "missing.txt"))
    assert str(e.value) == "cannot open stage file"


def test_trim_k_and_last_k_rule():
    loose, fine = P.PARAMETER_SETS["loose"], P.PARAMETER_SETS["fine"]
    # per-stage blocks: GenerateSyntenyBlocks(k_i, min(k_0..k_i), k_i)
    assert [P.stage_trim_k(loose, i) for i in range(4)] == [30, 30, 30, 30]
    assert [P.stage_trim_k([(100, 1), (30, 1), (500, 1)], i) for i in range(3)] == [100, 30, 30]
    # final: trimK = min(all k, minBlockSize); lastK = --lastk, else min(last stage's k, minBlockSize)
    assert P.final_k(loose, 5000) == (5000, 30)
    assert P.final_k(fine, 5000) == (500, 30)
    assert P.final_k(fine, 200) == (200, 30)
    assert P.final_k(fine, 20) == (20, 20)
    assert P.final_k(fine, 5000, lastk=200) == (200, 30)
    assert P.final_k(fine, 20, lastk=200) == (200, 20)
    assert P.final_k([], 5000) == (5000, 5000)         # no stages: INT_MAX against the block size
    assert P.final_k([], 700, lastk=90) == (90, 700)


def _files(argv, nstages, exists=False):
    return P.planned_files(P.parse_args(argv + ["-o", "out", "x.fa"]), nstages, exists)


def test_which_files_an_option_set_yields():
    base = ["genomes_permutations.txt", "coverage_report.txt"]
    assert _files(["-s", "loose"], 4) == ["blocks_coords.txt"] + base
    assert _files(["-s", "loose", "--gff"], 4) == ["blocks_coords.gff"] + base
    assert _files(["-s", "loose", "-q"], 4) == ["blocks_coords.txt"] + base + ["blocks_sequences.fasta"]
    assert _files(["-s", "loose", "-g"], 4) == ["blocks_coords.txt"] + base + ["de_bruijn_graph.dot"]
    assert _files(["-s", "far", "-v", "-r"], 3) == ["blocks_coords.txt"] + base                      # the hierarchy diagram itself is not written
    assert _files(["-s", "loose", "--noblocks"], 4) == []
    assert _files(["-s", "loose", "--noblocks", "-g", "-q"], 4) == ["de_bruijn_graph.dot"]
    assert _files(["-s", "fine", "--allstages", "--gff", "-q"], 3) == ["blocks_coords%d.gff" % i for i in range(4)] + base + ["blocks_sequences.fasta"]


def test_per_stage_graph_files_need_the_output_directory_to_exist():
    coords = ["blocks_coords%d.txt" % i for i in range(4)] + ["genomes_permutations.txt", "coverage_report.txt"]
    stage_graphs = ["de_bruijn_graph%d.dot" % i for i in range(3)]
    # without -r the first index creates the temp directory, by default the output directory: all per-stage graphs appear
    assert _files(["-s", "fine", "--allstages", "-g"], 3) == stage_graphs + coords + ["de_bruijn_graph3.dot"]
    # with -r nothing creates it before the end: only the last graph is written ...
    assert _files(["-s", "fine", "--allstages", "-g", "-r"], 3) == coords + ["de_bruijn_graph3.dot"]
    # ... unless it was there all along
    assert _files(["-s", "fine", "--allstages", "-g", "-r"], 3, exists=True) == stage_graphs + coords + ["de_bruijn_graph3.dot"]
    # a temp directory elsewhere does not help
    assert _files(["-s", "fine", "--allstages", "-g", "-t", "elsewhere"], 3) == coords + ["de_bruijn_graph3.dot"]
    # --noblocks: stage 0's graph is opened before any index has run
    assert _files(["-s", "fine", "--allstages", "-g", "--noblocks"], 3) == stage_graphs[1:] + ["de_bruijn_graph3.dot"]
    # -v alone numbers the per-stage graphs but not the last one
    assert _files(["-s", "fine", "-v", "-g"], 3) == stage_graphs + ["blocks_coords.txt", "genomes_permutations.txt", "coverage_report.txt", "de_bruijn_graph.dot"]


def test_progress_bar_keeps_its_static_between_bars():
    out = []
    bar = P.ProgressBar(out.append)
    bar(0, bar.START)
    for p in (1, 2, 2, 5):
        bar(p, bar.RUN)
    bar(50, bar.END)
    assert "".join(out) == "[" + "." * 50 + "]\n"
    # `prev` is reset when a bar starts -- after the dots for the progress it is called with, which are counted from the old value
    out.clear()
    bar(0, bar.START)
    bar(50, bar.END)
    assert "".join(out) == "[" + "." * 50 + "]\n"
    out.clear()
    bar.prev = 3
    bar(5, bar.START)
    assert "".join(out) == "..[" and bar.prev == 0


def test_fasta_error_messages_follow_the_reference_reader(tmp_path):
    def message(text):
        f = tmp_path / "x.fa"
        f.write_bytes(text)
        m = P._fasta_error(str(f))
        return None if m is None else m.split(": ", 1)[0].rsplit(" ", 1)[1] + ": " + m.split(": ", 1)[1]
    assert message(b">a\nACGT\n>b\nNNRY\n") is None
    assert message(b">a\nACGT\n\n>b\n>c\nAC\n") == "4: empty sequence"          # empty lines are not counted
    assert message(b">a\nACGT\n>b\n") == "4: empty sequence"
    assert message(b">a\nACZT\n") == "2: illegal character: Z"
    assert message(b">a\nacgt\n> b\nAC\n") == "3: empty header"
