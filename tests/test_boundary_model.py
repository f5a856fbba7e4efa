"""tests/boundary_model.py -- the numpy restatement of Postprocessor::ImproveBlockBoundaries and of SeqAn's local alignment as the
reference calls it -- against what the unmodified reference program wrote (tests/golden/correct_cases.json, recorded by
tests/golden/gen/make_correct_golden.py): applied to the blocks_coords.txt of a run WITHOUT --correctboundaries it must give the
coordinates of the run WITH it.  This pins the reading of the reference that the device code is tested against, without a GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                       # noqa: E402
from correct_fixtures import records_of            # noqa: E402

CASES = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "correct_cases.json")))["cases"] if "coords_with_flag" in c]


def sequences(case):
    return [s for f in records_of(case["input"])[0] for _, s in f]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_reference_program(case):
    before, want = BM.parse_blocks_coords(case["coords_without_flag"]), BM.parse_blocks_coords(case["coords_with_flag"])
    assert before and case["moved"]
    assert not BM.hits_undefined_case([list(b) for b in before], case["n_reference_records"], case["min_block_size"])
    got = BM.correct(before, sequences(case), case["n_reference_records"], case["min_block_size"])
    assert sorted(map(tuple, got)) == sorted(want)


def test_the_fixtures_cover_the_edge_cases():
    cases = {c["name"]: c for c in CASES}

    def pairs(name):
        """[(reference instance, assembly instance)] of the corrected groups before the correction, R, record sizes, all instances"""
        c = cases[name]
        b = BM.parse_blocks_coords(c["coords_without_flag"])
        nref = c["n_reference_records"]
        out = []
        for i in sorted({abs(x[0]) for x in b}):
            g = [x for x in b if abs(x[0]) == i]
            if len(g) == 2 and sum(x[1] < nref for x in g) == 1:
                out.append(tuple(sorted(g, key=lambda x: x[1] >= nref)))
        return out, min(c["min_block_size"], 1024), [len(s) for s in sequences(c)], b

    p, R, size, b = pairs("craft_near_start")
    assert any(x[2] < R and not any(y[1] == x[1] and y[3] <= x[2] for y in b) for g in p for x in g)        # no predecessor, start < R
    p, R, size, b = pairs("craft_near_end")
    assert any(x[3] + R > size[x[1]] and not any(y[1] == x[1] and y[2] >= x[3] for y in b) for g in p for x in g)      # cut by the record's end
    p, R, size, b = pairs("craft_reverse_reference")
    assert any(g[0][0] < 0 for g in p)                                                                      # a negative reference instance
    p, R, size, b = pairs("craft_adjacent_blocks")
    assert any(0 <= y[2] - x[3] < R for g in p for x in g for y in b if y[1] == x[1] and y is not x)        # a neighbour closer than R
    p, R, size, b = pairs("craft_two_contigs")
    assert R % 2 == 1
    p, R, size, b = pairs("craft_ambiguity_codes")
    seq = sequences(cases["craft_ambiguity_codes"])
    assert any(set(seq[x[1]][max(0, x[2] - R):x[2] + R]) - set(b"ACGT") for g in p for x in g)              # ambiguity codes inside a window
    p, R, size, b = pairs("saureus_fine_inram_m500_correct")
    assert len(p) > 50 and sum(g[0][0] < 0 for g in p) > 5


def test_alignment_tie_breaks():
    # equal maxima: the largest j wins, then the largest i
    assert BM.align(b"ACGTTTTTTTTACGT", b"ACGT") == ((11, 15), (0, 4))
    assert BM.align(b"ACGT", b"ACGTCCCCCCCACGT") == ((0, 4), (11, 15))
    assert BM.align(b"AAAA", b"AAAA") == ((0, 4), (0, 4))
    assert BM.align(b"AAAA", b"CCCC") == ((0, 4), (0, 4))          # score 0: no trace, the rows stay as assigned
    assert BM.align(b"", b"ACGT") == ((0, 0), (0, 4))
    assert BM.align(b"NNNN", b"TNNNNT") == ((0, 4), (1, 5))        # bytes are compared as they are
