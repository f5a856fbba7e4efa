"""The global band class of k_block_align (sbl_align_set_wide; csrc/block_align.hip) against the numpy models
tests/galign_model.py and tests/gapopen_model.py and against the same pairs through the LDS classes: the class a pair runs in decides
whether it gets a result, never what the result is.  tests/test_wideband_cases.py holds the preconditions of the cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_model as MM                             # noqa: E402
import mvariants_model as MV                       # noqa: E402
import wideband_cases as WC                        # noqa: E402
from galign_cases import Batch, mutated, rand      # noqa: E402

pytestmark = pytest.mark.gpu

ZERO = {"pairs": 0, "passes": 0, "launches": 0, "cells": 0, "kernel_ms": 0.0}


def test_the_setting_round_trips_and_a_bad_value_leaves_it():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    bt = Batch([(b"ACGTACGTAC", b"ACGTTCGTAC")])
    bf = BlockFinder(bt.records, device=0)
    try:
        assert bf.wide == 0 and bf.align_wide_stats() == ZERO
        for on in (True, False, 1):
            bf.set_wide(on)
            assert bf.wide == int(on)
            for bad in (2, 2 ** 32 - 1):
                with pytest.raises(SibeliaError, match="bad argument"):
                    bf.set_wide(bad)
                assert bf.wide == int(on)
        bf.set_wide(False)
        got = bf.align_pairs(bt.desc)
        assert got[0].status == 0 and got[0].runs == [("=", 4), ("X", 1), ("=", 5)]
        assert bf.align_wide_stats() == ZERO and bf.align_stats()["passes"] == 1
    finally:
        bf.close()


@pytest.fixture(scope="module", params=[0, 1])
def limit_case(request):
    o = request.param
    bt, far = WC.limit_batch(o)
    return o, bt, far, bt.want(o, linear=o == 0)


def test_the_band_limit_skips_without_the_setting(limit_case):
    o, bt, far, want = limit_case
    got, st, wide = WC.run(bt, o, False)
    bt.check(got, want, skipped=far)
    assert st["skipped"] == len(far) and wide == ZERO


def test_pairs_beyond_the_band_limit_are_aligned_with_the_setting(limit_case):
    o, bt, far, want = limit_case
    got, st, wide = WC.run(bt, o, True)
    assert [g.status for g in got] == [0] * len(bt.pairs)
    bt.check(got, want)
    assert st["skipped"] == 0 and st["passes"] == len(bt.pairs)
    assert all(g.band_w == min(64, len(a), len(b)) and g.passes == 1 for g, (a, b) in zip(got, bt.pairs))      # 60 bases: the band covers the matrix
    assert wide["pairs"] == wide["passes"] == len(far) and wide["launches"] == 1 and 0 < wide["kernel_ms"] <= st["kernel_ms"]
    assert wide["cells"] == sum((len(a) + len(b) + 1) * ((WC.offsets(len(a), len(b)) + 1) // 2) for a, b in bt.pairs[:len(far)]) < st["cells"]


@pytest.fixture(scope="module")
def shapes():
    return Batch(*WC.shape_pairs())


@pytest.mark.parametrize("o", [0, 300])
def test_every_shape_through_the_global_class(shapes, monkeypatch, o):
    bt = shapes
    off, st_off, wide_off = WC.run(bt, o, False)
    monkeypatch.setenv("SBL_TEST_GALIGN_WIDE_FROM", "0")
    unset, st_unset, wide_unset = WC.run(bt, o, False)          # the switch alone does nothing
    on, st_on, wide_on = WC.run(bt, o, True)
    bt.check(on, bt.want(o, linear=o == 0))
    assert WC.key(on) == WC.key(off) == WC.key(unset)
    assert st_on["skipped"] == st_off["skipped"] == st_unset["skipped"] == 0
    assert wide_off == wide_unset == ZERO
    assert wide_on["passes"] == st_on["passes"] == st_off["passes"] and wide_on["cells"] == st_on["cells"] == st_off["cells"]
    assert wide_on["launches"] == st_on["launches"]
    assert wide_on["pairs"] == sum(1 for a, b in bt.pairs if a and b)      # a pair with an empty side is all gaps: nothing is launched
    assert max(g.passes for g in on) >= 3 and any(g.band_w == min(len(a), len(b)) > 64 for g, (a, b) in zip(on, bt.pairs))


@pytest.mark.parametrize("o", [300, 0])
def test_doubling_goes_on_into_the_global_class(monkeypatch, o):
    """nothing matches: the certificate needs w + 1 > 100 * 1200 / 175, first met at w = 1024.  The passes at 64 .. 512 run in the
    register and LDS classes (at most 1025 offsets: the switch is set to that, 1000 would send the pass at w = 512 along as well), the
    last one with 2049 offsets in the global class"""
    bt = Batch([(b"A" * 1200, b"C" * 1200)])
    monkeypatch.setenv("SBL_TEST_GALIGN_WIDE_FROM", "1025")
    got, st, wide = WC.run(bt, o, True)
    bt.check(got, bt.want(o, linear=o == 0))
    assert got[0].band_w == 1024 and got[0].passes == 5 and got[0].runs == [("X", 1200)]
    assert st["passes"] == 5 and wide["pairs"] == wide["passes"] == wide["launches"] == 1
    assert wide["cells"] == 2401 * 1025


def test_the_caps_skip_in_either_mode(monkeypatch):
    """the construction of test_the_per_alignment_cap_skips_long_pairs_only (tests/test_gpu_block_align.py)"""
    rng = np.random.default_rng(26)
    pairs, long_ones = [], set()
    for k in range(24):
        n = 900 if k % 4 == 1 else int(rng.integers(1, 60))      # 1800 diagonals * 17 bytes at w = 64: beyond 4 KiB
        a = rand(rng, n)
        pairs.append((a, mutated(rng, a) or b"C"))
        if n == 900:
            long_ones.add(k)
    bt = Batch(pairs)
    want = bt.want(0, linear=True)
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    off, st_off, _ = WC.run(bt, 0, False)
    on, st_on, _ = WC.run(bt, 0, True)
    monkeypatch.setenv("SBL_TEST_GALIGN_WIDE_FROM", "0")
    forced, st_forced, wide = WC.run(bt, 0, True)
    for got, st in ((off, st_off), (on, st_on), (forced, st_forced)):
        bt.check(got, want, skipped=long_ones)
        assert st["skipped"] == len(long_ones) == 6
    assert WC.key(off) == WC.key(on) == WC.key(forced) and wide["pairs"] == 18
    monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
    single, st1, wide1 = WC.run(bt, 0, True)
    monkeypatch.setenv("SBL_TEST_GALIGN_TOTAL_KB", "64")         # a small total cap: several launches of the global class, the same results
    split, st2, wide2 = WC.run(bt, 0, True)
    bt.check(single, want)
    assert WC.key(split) == WC.key(single) and st1["skipped"] == st2["skipped"] == 0
    assert wide2["launches"] > wide1["launches"] and wide2["passes"] == wide1["passes"] == st1["passes"]


def test_a_group_with_a_far_member():
    from sibelia_amd import BlockFinder
    bt, far = WC.limit_batch(0)
    a, long_one = bt.pairs[0]
    rng = np.random.default_rng(63)
    c = rand(rng, 200)
    texts = [[a, mutated(rng, a), long_one], [c, mutated(rng, c), mutated(rng, c)]]
    record, groups = bytearray(b"N"), []
    for strings in texts:
        insts = []
        for s in strings:
            insts.append((0, len(record), len(record) + len(s), False))
            record += s + b"N"
        groups.append(insts)
    want = [MM.msa(strings) for strings in texts]
    bf = BlockFinder([bytes(record)], device=0)
    try:
        got = bf.align_groups(groups)
        assert (got[0].status, got[0].L, got[0].rows) == (1, 0, []) and bf.align_stats()["skipped"] == 1
        assert got[1].status == 0 and got[1].rows == want[1][0]
        bf.set_wide(True)
        got = bf.align_groups(groups)
        segs = bf.group_variants(None)
        st, wide = bf.align_stats(), bf.align_wide_stats()
    finally:
        bf.close()
    for g, (rows, scores) in zip(got, want):
        assert g.status == 0 and g.rows == rows and [m[0] for m in g.members] == scores
    assert st["skipped"] == 0 and wide["pairs"] == wide["passes"] == 1
    model = [(k, s, e, before, lead, slices) for k, g in enumerate(got) for s, e, before, lead, _, slices in MV.segments(g.rows)]
    assert segs == model
    longest = max((s for s in segs if s[0] == 0), key=lambda s: s[2] - s[1])
    assert longest[2] - longest[1] >= 12300 and longest[5][0].count(b"-") >= 12300      # the insertion: one gapped segment
