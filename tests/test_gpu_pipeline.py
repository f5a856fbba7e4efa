"""`python -m sibelia_amd` end to end against what the unmodified reference program wrote.

Every command line of tests/golden/dropin_cases.json and tests/golden/pipeline_cases.json (recorded from oracle/_ref/sibelia_ref on
the CPU by tests/golden/gen/make_dropin_golden.py / make_pipeline_golden.py) is run through the package's own command line in a
fresh child process, one at a time.  The return code, the standard output (progress bars included) and every file the reference
wrote must be the same, byte for byte -- except the two outputs the package does not write, circos/ and d3_blocks_diagram.html,
which are instantiated from templates embedded in the reference's sources -- and the package may write no file the reference did
not.  Needs neither the reference nor anything built from it."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "gen"))
from make_dropin_golden import run_case      # noqa: E402

CASES = [c for name in ("dropin_cases.json", "pipeline_cases.json") for c in json.load(open(os.path.join(ROOT, "tests", "golden", name)))["cases"]]

pytestmark = pytest.mark.gpu


def expected_files(case):
    return {name: v for name, v in case["files"].items() if not name.startswith("circos" + os.sep) and name != "d3_blocks_diagram.html"}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_line_equals_the_reference_program(case, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    # a fresh child process per case: `python -m sibelia_amd <args> -o out <input>` (run_case prepares the input and has its own timeout)
    rc, stdout_sha, files, stdout, stderr = run_case(sys.executable, case["input"], ["-m", "sibelia_amd"] + case["args"], str(tmp_path), env=env)
    assert rc == case["returncode"], stderr.decode(errors="replace")[-2000:]
    assert stdout_sha == case["stdout_sha256"], stdout.decode(errors="replace")[-2000:]
    want = expected_files(case)
    assert sorted(files) == sorted(want)
    wrong = [name for name in sorted(files) if files[name] != want[name]]
    assert not wrong, "files differ from the reference program's: %s" % wrong


def test_the_fixtures_exercise_both_new_reports():
    cases = {c["name"]: c for c in CASES}
    for name in ("hpylori_loose_inram_sequences_gff", "ambig_fine_inram_sequences_gff", "ambig_fine_tempfiles_allstages_sequences_gff",
                 "saureus_loose_inram_sequences_gff"):
        f = cases[name]["files"]
        assert f["blocks_sequences.fasta"][0] > 1000
        assert max(v[0] for n, v in f.items() if n.endswith(".gff")) > 58          # more than the three header lines
