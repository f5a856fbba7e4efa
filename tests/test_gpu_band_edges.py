"""k_block_align (csrc/block_align.hip) at the limits of its band classes and of its trace walk, against the
UNBANDED numpy models (tests/galign_model.py, tests/gapopen_model.py), exactly: status, score, runs and both device-spelled rows.

Band classes  pairs with REG_W / MID_W / MAX_W - 1, + 0 and + 1 offsets at the first band, whose optimal path runs along the band's
              first or last offset (tests/bandedge_cases.py): the lane that holds a band's last offsets, the minus-infinity borders
              either side of the score arrays and the LDS footprint at MAX_W decide their result.  The same pairs through the global class.
Walk          one X / I / D run of 63 .. 129 steps, from (0, 0), in the middle and up to n / m: the 64 steps a ballot consumes.
Group         sbl_align_groups with one member either side of the register limit.

Every pair ends after ONE pass: tests/test_bandedge_cases.py holds that precondition, and no result here stands on a doubled band."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bandedge_cases as BC                        # noqa: E402
import gapopen_model as AM                         # noqa: E402
import msa_model as MM                             # noqa: E402
import wideband_cases as WC                        # noqa: E402

pytestmark = pytest.mark.gpu

ZERO = {"pairs": 0, "passes": 0, "launches": 0, "cells": 0, "kernel_ms": 0.0}
LIMITS = [(model, T) for model in BC.MODELS for T in BC.LIMITS[model]]
INNER = [(model, T) for model in BC.MODELS for T in BC.LIMITS[model][:2]]      # REG_W, MID_W: a class on either side
LAST = [(model, BC.LIMITS[model][2]) for model in BC.MODELS]                  # MAX_W: beyond it the global class or nothing


def one_pass_each(got, w=BC.W0):
    assert [(g.status, g.passes, g.band_w) for g in got] == [(0, 1, w)] * len(got)


@pytest.mark.parametrize("model,T", LIMITS)
def test_below_and_at_a_class_limit_in_one_launch(model, T):
    bt, want = BC.edge_batch(model, (T - 1, T))
    got, st, wide = WC.run(bt, BC.OPEN[model], False)
    bt.check(got, want)
    one_pass_each(got)
    assert st["launches"] == 1 and st["passes"] == 8 and st["skipped"] == 0 and wide == ZERO
    assert st["cells"] == BC.cells(bt.pairs)


@pytest.mark.parametrize("model,T", INNER)
def test_at_and_beyond_a_class_limit_in_two_launches(model, T):
    bt, want = BC.edge_batch(model, (T, T + 1))
    got, st, wide = WC.run(bt, BC.OPEN[model], False)
    bt.check(got, want)
    one_pass_each(got)
    assert st["launches"] == 2 and st["passes"] == 8 and st["skipped"] == 0 and wide == ZERO      # the two sides took different kernels
    assert st["cells"] == BC.cells(bt.pairs)


@pytest.mark.parametrize("model,T", LAST)
def test_beyond_the_last_limit_is_skipped_without_the_setting(model, T):
    bt, want = BC.edge_batch(model, (T, T + 1))
    got, st, wide = WC.run(bt, BC.OPEN[model], False)
    bt.check(got, want, skipped={4, 5, 6, 7})
    one_pass_each(got[:4])
    assert st["skipped"] == 4 and st["launches"] == 1 and st["passes"] == 4 and wide == ZERO
    assert st["cells"] == BC.cells(bt.pairs[:4])


@pytest.mark.parametrize("model,T", LAST)
def test_beyond_the_last_limit_takes_the_global_class_with_the_setting(model, T):
    bt, want = BC.edge_batch(model, (T, T + 1))
    got, st, wide = WC.run(bt, BC.OPEN[model], True)
    bt.check(got, want)
    one_pass_each(got)
    assert st["skipped"] == 0 and st["launches"] == 2 and st["passes"] == 8 and st["cells"] == BC.cells(bt.pairs)
    assert wide["pairs"] == wide["passes"] == 4 and wide["launches"] == 1 and wide["cells"] == BC.cells(bt.pairs[4:])      # the T + 1 pairs alone


@pytest.mark.parametrize("model,T", INNER)
def test_the_edge_pairs_through_the_global_class(monkeypatch, model, T):
    bt, want = BC.edge_batch(model, (T - 1, T, T + 1))
    off, st_off, wide_off = WC.run(bt, BC.OPEN[model], False)
    monkeypatch.setenv("SBL_TEST_GALIGN_WIDE_FROM", "0")
    on, st_on, wide_on = WC.run(bt, BC.OPEN[model], True)
    bt.check(on, want)
    one_pass_each(on)
    assert WC.key(on) == WC.key(off)
    assert wide_off == ZERO and st_off["launches"] == 2
    assert wide_on["pairs"] == wide_on["passes"] == st_on["passes"] == 12 and wide_on["launches"] == st_on["launches"] == 1
    assert wide_on["cells"] == st_on["cells"] == st_off["cells"] == BC.cells(bt.pairs)


@pytest.mark.parametrize("model", BC.MODELS)
def test_walk_windows(model):
    bt, want = BC.walk_batch(model, BC.W0)
    assert len(bt.pairs) == 54 - 9                              # all but the X runs of 127 .. 129
    got, st, _ = WC.run(bt, BC.OPEN[model], False)
    bt.check(got, want)
    one_pass_each(got)
    assert st["launches"] == 1 and st["passes"] == len(bt.pairs)


@pytest.mark.parametrize("model", BC.MODELS)
def test_walk_windows_of_mismatch_runs_no_band_of_64_certifies(monkeypatch, model):
    """X runs of 127, 128 and 129: 100 L > 175 * 65 (bandedge_cases.walk_first_w), so their one pass is at a first band of 128"""
    bt, want = BC.walk_batch(model, 2 * BC.W0)
    assert len(bt.pairs) == 9
    monkeypatch.setenv("SBL_TEST_GALIGN_W0", str(2 * BC.W0))
    got, st, _ = WC.run(bt, BC.OPEN[model], False)
    bt.check(got, want)
    one_pass_each(got, 2 * BC.W0)
    assert st["launches"] == 1 and st["passes"] == 9


@pytest.mark.parametrize("model", BC.MODELS)
def test_a_group_across_the_register_limit(model):
    from sibelia_amd import BlockFinder
    strings, o = BC.group_case(model), BC.OPEN[model]
    record, insts = bytearray(b"N"), []
    for s in strings:
        insts.append((0, len(record), len(record) + len(s), False))
        record += s + b"N"
    rows, scores = MM.msa(strings) if model == "linear" else AM.msa(strings, o)
    bf = BlockFinder([bytes(record)], device=0)
    try:
        bf.set_gap_open(o)
        got = bf.align_groups([insts])
        st = bf.align_stats()
    finally:
        bf.close()
    assert len(got) == 1 and got[0].status == 0 and got[0].L == len(rows[0]) and got[0].rows == rows
    assert got[0].members == [(score, BC.W0, 1) for score in scores]
    assert st["launches"] == 2 and st["passes"] == 3 and st["skipped"] == 0      # the register class and the LDS class of 256 lanes
