"""Preconditions of the band-edge and walk cases (tests/bandedge_cases.py), without a GPU, on the numpy models alone: every edge pair has
exactly the offsets of its class limit, both models certify it at the first band with the result of the unbanded matrix, and its optimal
path runs along the band's first or last offset; every walk pair has the one run it was built for and certifies in one pass.  So the
device must end at one pass for each of them (tests/test_gpu_band_edges.py), and a wrong read across the band's border, or a wrong
count in a walk window, changes a result."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bandedge_cases as BC                        # noqa: E402
import galign_model as GM                          # noqa: E402

W0, offsets = BC.W0, BC.offsets

EDGE_W = [(model, T + d) for model in BC.MODELS for T in BC.LIMITS[model] for d in (-1, 0, 1)]


def certified(model, a, b, w, unbanded=None):
    """the certificate holds at w, and the banded model equals the unbanded matrix (computed here unless given) -> its (score, steps)"""
    score, steps, ok = BC.align_banded(model, a, b, w)
    assert ok and (score, steps) == (unbanded or BC.align(model, a, b))
    return score, steps


def at_edge(a, b, steps, kind):
    """the path reaches the band's first offset (low) or its last (high) at w = 64, and never goes beyond either"""
    n, m = len(a), len(b)
    lo, hi = min(0, m - n), max(0, m - n)
    least, most = BC.reach(steps)
    assert lo - W0 <= least and most <= hi + W0
    return least == lo - W0 if kind.startswith("low") else most == hi + W0


def test_the_opening_cost_leaves_the_edge_pairs_their_certificate():
    assert BC.OPEN["linear"] == 0 and 0 < 2 * BC.OPEN["affine"] < 175
    assert len(EDGE_W) == 18 and len(set(EDGE_W)) == 18


@pytest.mark.parametrize("model,W", EDGE_W)
def test_edge_pairs_have_their_offsets_and_hug_their_edge(model, W):
    pairs, revs = BC.edge_pairs(model, W)
    assert len(pairs) == 4 and sorted(revs) == [(False, False)] * 3 + [(True, True)]
    for kind, (a, b), kept in zip(BC.KINDS, pairs, BC.edge_model(model, W)):
        n, m = len(a), len(b)
        assert offsets(n, m) == W and abs(m - n) == W - 129 and (n > m) == kind.endswith("swapped"), kind
        score, steps = certified(model, a, b, W0, kept)
        assert score == GM.bound(n, m, W0) + 175 - 2 * BC.OPEN[model], kind      # two gap runs; the bound is cleared by 175 without them
        assert at_edge(a, b, steps, kind), kind
        # the gap columns are the 64 unmatched bases and the filler (the linear model may cut the 64 where a base of U equals one of core)
        assert sorted((steps.count("I"), steps.count("D"))) == sorted((BC.EDGE, len(BC.filler(W)))) and steps.count("M") == BC.CORE, kind
        assert model == "linear" or sum(1 for op, _ in GM.runs(a, b, steps) if op in "ID") == 2, kind


def test_every_kind_is_staged_downwards_at_every_class_limit():
    for model in BC.MODELS:
        for T in BC.LIMITS[model]:
            down = {BC.edge_pairs(model, W)[1].index((True, True)) for W in (T - 1, T, T + 1)}
            assert len(down) == 3, (model, T)


@pytest.mark.parametrize("model", BC.MODELS)
def test_walk_pairs_have_one_run_and_certify_in_one_pass(model):
    cases, kept = BC.walk_cases(model), BC.walk_model(model)
    assert len(cases) == 3 * 3 * len(BC.WALK_L) == len(kept)
    assert {(op, L, where) for op, L, where, _, _ in cases} == {(op, L, where) for op in "XID" for L in BC.WALK_L for where in ("mid", "start", "end")}
    for (op, L, where, a, b), (score, steps) in zip(cases, kept):
        what = (op, L, where)
        runs = GM.runs(a, b, steps)
        assert [r for r in runs if r[0] == op] == [(op, L)], what
        assert runs == BC.walk_runs(op, L, where), what
        w = BC.walk_first_w(op, L)
        certified(model, a, b, w, (score, steps))
        if w != W0:                                             # the arithmetic of walk_first_w: no band of 64 certifies these
            assert op == "X" and len(a) == len(b) and not BC.align_banded(model, a, b, W0)[2], what
    assert sorted((op, L) for op, L, where, _, _ in cases if BC.walk_first_w(op, L) != W0 and where == "mid") == [("X", 127), ("X", 128), ("X", 129)]


@pytest.mark.parametrize("model", BC.MODELS)
def test_the_group_has_a_member_either_side_of_the_register_limit(model):
    c, high, low, copy = BC.group_case(model)
    reg_w = BC.LIMITS[model][0]
    assert (offsets(len(c), len(high)), offsets(len(c), len(low))) == (reg_w + 1, reg_w) and offsets(len(c), len(copy)) < reg_w
    assert at_edge(c, high, certified(model, c, high, W0)[1], "high")
    assert at_edge(c, low, certified(model, c, low, W0)[1], "low")
    certified(model, c, copy, W0)
