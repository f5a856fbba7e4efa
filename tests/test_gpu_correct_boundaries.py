"""--correctboundaries end to end against what the unmodified reference program wrote (tests/golden/correct_cases.json, recorded on
the CPU by tests/golden/gen/make_correct_golden.py): `python -m sibelia_amd` in a fresh child process per case -- return code,
standard output and every file byte for byte (circos/ and d3_blocks_diagram.html excepted, which the package does not write) --
and the schedule of the correction through the API: the batched levels must give what the serial schedule gives."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from correct_fixtures import records_of, run_case          # noqa: E402

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "correct_cases.json")))["cases"]

pytestmark = pytest.mark.gpu


def expected_files(case):
    return {name: v for name, v in case["files"].items() if not name.startswith("circos" + os.sep) and name != "d3_blocks_diagram.html"}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_line_equals_the_reference_program(case, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    rc, stdout_sha, files, stdout, stderr = run_case(sys.executable, case["input"], ["-m", "sibelia_amd"] + case["args"], str(tmp_path), env=env)
    assert rc == case["returncode"], stderr.decode(errors="replace")[-2000:]
    assert stdout_sha == case["stdout_sha256"], stdout.decode(errors="replace")[-2000:]
    if "stderr" in case:
        assert stderr.decode() == case["stderr"]
    want = expected_files(case)
    assert sorted(files) == sorted(want)
    wrong = [name for name in sorted(files) if files[name] != want[name]]
    if wrong and "coords_with_flag" in case and "blocks_coords.txt" in wrong:
        got = open(os.path.join(str(tmp_path), "out", "blocks_coords.txt")).read().splitlines()
        diff = [(a, b) for a, b in zip(got, case["coords_with_flag"].splitlines()) if a != b]
        assert not diff, diff[:10]
    assert not wrong, "files differ from the reference program's: %s" % wrong


def _finder(case):
    from sibelia_amd import BlockFinder
    from sibelia_amd.pipeline import PARAMETER_SETS, final_k
    files = records_of(case["input"])[0]
    names = [n for f in files for n, _ in f]
    bf = BlockFinder([s for f in files for _, s in f], device=0)
    args = case["args"]
    stages = PARAMETER_SETS[args[args.index("-s") + 1]]
    for k, d in stages:
        bf.PerformGraphSimplifications(k, d, 4)
    last_k, trim_k = final_k(stages, case["min_block_size"])
    bf.GenerateSyntenyBlocks(last_k, trim_k, case["min_block_size"], False)
    bf.postprocess(names)
    return bf, names, len(files[0])


@pytest.fixture(scope="module")
def staged():
    """the `fine` and `loose` Staphylococcus aureus runs up to the correction, once for the tests below"""
    by_name = {c["name"]: c for c in CASES}
    out = {n: _finder(by_name[n]) + (by_name[n],) for n in ("saureus_fine_inram_m500_correct", "saureus_loose_inram_correct_gff_sequences")}
    yield out
    for v in out.values():
        v[0].close()


def test_batched_levels_equal_the_serial_schedule(staged, monkeypatch):
    bf, names, nref, case = staged["saureus_fine_inram_m500_correct"]
    before, _ = bf.postprocess(names, glue=False)                # the list as it stands (already glued): a copy
    batched, texts = bf.correct_boundaries(case["min_block_size"], nref, names)
    st = bf.correct_stats()
    assert texts[0].decode() == case["coords_with_flag"]
    assert st["groups"] > 50 and st["alignments"] == 2 * st["groups"] and st["levels"] < st["groups"]
    # the same list again, one group per level
    bf2, names2, _ = _finder(case)
    try:
        again, _ = bf2.postprocess(names2, glue=False)
        assert np.array_equal(again, before)
        monkeypatch.setenv("SBL_TEST_CORRECT_SERIAL", "1")
        serial, texts2 = bf2.correct_boundaries(case["min_block_size"], nref, names2)
        st2 = bf2.correct_stats()
    finally:
        bf2.close()
    assert st2["levels"] == st2["groups"] == st["groups"] and st2["launches"] >= st2["groups"]
    assert np.array_equal(serial, batched) and texts2 == texts


def test_batching_happens_on_the_loose_run(staged, monkeypatch):
    bf, names, nref, case = staged["saureus_loose_inram_correct_gff_sequences"]
    bf.correct_boundaries(case["min_block_size"], nref, names)
    st = bf.correct_stats()
    print("correction of the loose run:", st)
    assert st["groups"] > 1 and st["levels"] < st["groups"] and st["kernel_ms"] > 0
    monkeypatch.setenv("SBL_TEST_CORRECT_SERIAL", "0")          # the switch is a number: 0 leaves the batched schedule on
    bf.correct_boundaries(case["min_block_size"], nref, names)
    st = bf.correct_stats()
    assert st["groups"] > 1 and st["levels"] < st["groups"]


def test_an_empty_list_is_corrected_to_an_empty_list():
    """two inputs that share no block: the list after the post-processing is empty, which is a list (the reference's loop runs over
    nothing and its writers write their usual files)"""
    case = {c["name"]: c for c in CASES}["craft_no_shared_block"]
    bf, names, nref = _craft_finder(case)
    try:
        before, texts = bf.postprocess(names)
        assert len(before) == 0
        got, again = bf.correct_boundaries(case["min_block_size"], nref, names)
        st = bf.correct_stats()
        assert len(got) == 0 and again == texts
        assert st["groups"] == 0 and st["alignments"] == 0 and st["launches"] == 0 and st["levels"] == 0
    finally:
        bf.close()


def test_bad_arguments():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    bf = BlockFinder([b"ACGT" * 50, b"ACGT" * 50], device=0)
    try:
        with pytest.raises(SibeliaError, match="bad argument"):      # no block list
            bf.correct_boundaries(300, 1)
    finally:
        bf.close()
    by_name = {c["name"]: c for c in CASES}
    bf, names, nref = _craft_finder(by_name["craft_two_contigs"])
    try:
        for m, ref in ((257, 0), (257, len(names)), (257, len(names) + 3), (0, nref)):      # n_reference_chr of 0 or >= nchr; R == 0
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.correct_boundaries(m, ref, names)
        got, texts = bf.correct_boundaries(257, nref, names)          # ... and the list is still there
        assert texts[0].decode() == by_name["craft_two_contigs"]["coords_with_flag"]
    finally:
        bf.close()


def _craft_finder(case):
    from sibelia_amd import BlockFinder
    from sibelia_amd.pipeline import final_k, parse_stage_text
    files, stage, m = records_of(case["input"])
    names = [n for f in files for n, _ in f]
    bf = BlockFinder([s for f in files for _, s in f], device=0)
    stages = parse_stage_text(stage)
    for k, d in stages:
        bf.PerformGraphSimplifications(k, d, 4)
    last_k, trim_k = final_k(stages, m)
    bf.GenerateSyntenyBlocks(last_k, trim_k, m, False)
    bf.postprocess(names)
    return bf, names, len(files[0])
