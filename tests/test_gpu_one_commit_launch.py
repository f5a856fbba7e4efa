"""One commit launch per ordered round: the parked transactions of a window resume in workgroups [0, nres) of k_commit's grid
(nres = min(transactions parked when the round started, window entries)), the window's entries run in workgroups [nres, nres + nwin).
Nothing of the round protocol changed with it, so every case must leave the state the oracle leaves -- with a park after every
collapse (SBL_PARK=1: nearly every round has resume workgroups) and with the default cap; with windows of 1, 2 and 37 entries, where
more transactions are parked than the window has entries and rounds without a parked entry in the window (nres workgroups that find
their list empty) alternate with rounds that have them; over more than 1024 rounds of one iteration, where the sweep of park_of's
finished markers comes due; and on three virtual ranks, which must all take the same rounds.

The input of cases 1, 2 and 4 is the one tools/stress.py draws for seed 93194 (12 strains x 24.5 kbp, k = 15, D = 91, 8 % SNPs, 8609
bulges): the case that found round 6's last parity bug of the parked transactions."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle(seqs, stages):
    from oracle.oracle import Oracle
    orc = Oracle(seqs)
    out = []
    for k, D in stages:
        n = orc.simplify_stage(k, D, 4)
        so, po = orc.state()
        out.append((n, so, po))
    return out


@pytest.fixture(scope="module")
def parky():
    """(strains, stages, the oracle's result): computed once, read by every test that uses it"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import stress
    seqs, stages = stress.draw_case(93194, many=False)[:2]
    ref = _oracle(seqs, stages)
    assert ref[0][0] == 8609
    return seqs, stages, ref


def _run(seqs, stages, window=0, ranks=0):
    """per stage: (bulges, sequences, positions, rounds, transactions); ranks > 0: the same job on that many virtual ranks of device 0"""
    from sibelia_amd import BlockFinder
    if ranks:
        from sibelia_amd.dist import LocalShardedFinder
        bf = LocalShardedFinder(seqs, [0] * ranks)
    else:
        bf = BlockFinder(seqs, device=0)
    try:
        if window:
            bf.set_window(window)
        out = []
        for k, D in stages:
            n = bf.simplify_stage(k, D, 4)
            st = bf.stats()
            if ranks:
                assert len({int(x["rounds"]) for x in st}) == 1, "the ranks took different numbers of rounds: %s" % [int(x["rounds"]) for x in st]
                st = st[0]
            seq, pos = bf.state()
            out.append((n, seq, pos, int(st["rounds"]), int(st["transactions"])))
        return out
    finally:
        bf.close()


def _same_state(got, ref, what):
    assert len(got) == len(ref)
    for x, y in zip(got, ref):
        assert x[0] == y[0], "bulges differ (%d, oracle %d): %s" % (x[0], y[0], what)
        assert x[1] == y[1] and all(np.array_equal(p, q) for p, q in zip(x[2], y[2])), "state differs: " + what


def _set_park(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("SBL_PARK", raising=False)
    else:
        monkeypatch.setenv("SBL_PARK", cap)


def test_parity_with_frequent_parking(monkeypatch, parky):
    """SBL_PARK=1 and the default cap against the oracle; rounds and transactions against a run without parking, within the bound of
    test_gpu_parking.py (parking trades rounds for shorter launches: at most 4 x); and something must have parked"""
    seqs, stages, ref = parky
    _set_park(monkeypatch, "0")
    plain = _run(seqs, stages)
    _same_state(plain, ref, "SBL_PARK=0")
    for cap in ("1", None):
        _set_park(monkeypatch, cap)
        a = _run(seqs, stages)
        print("SBL_PARK=%s: rounds %s transactions %s (without parking: %s, %s)" % (cap, [x[3] for x in a], [x[4] for x in a], [x[3] for x in plain], [x[4] for x in plain]))
        _same_state(a, ref, "SBL_PARK=%s" % cap)
        for x, y in zip(a, plain):
            assert x[3] <= 4 * max(y[3], 8), "SBL_PARK=%s: %d rounds with parking against %d without" % (cap, x[3], y[3])
            assert x[4] <= 4 * max(y[4], 8) and 4 * max(x[4], 8) >= y[4], "SBL_PARK=%s: %d transactions with parking against %d without" % (cap, x[4], y[4])
        if cap == "1":
            assert sum(x[3] for x in a) > sum(y[3] for y in plain), "SBL_PARK=1 parked nothing: the test does not exercise what it is for"


@pytest.mark.parametrize("window", [1, 2, 37])
def test_block_mapping_at_its_edges(monkeypatch, parky, window):
    """a pinned window of 1, 2 and 37 entries with a park after every collapse: more parked transactions than window entries (nres is
    capped by the window), rounds whose window holds none of them (every resume workgroup finds the list short and leaves)"""
    seqs, stages, ref = parky
    _set_park(monkeypatch, "1")
    _same_state(_run(seqs, stages, window=window), ref, "window %d, SBL_PARK=1" % window)


def test_marker_sweep_beyond_1024_rounds(monkeypatch):
    """8 strains x 3 kbp (8 % SNPs, k = 12, D = 80) with the window pinned to 2: tests/hostsim counts 1259 rounds in the first
    iteration, so a round with (round & 1023) == 0 comes and the finished markers of park_of are swept there, whatever kind of round it
    is (the sweep used to belong to the ordered commit alone).  The input is small enough for the one-launch path: switched off."""
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=3000, n=8, seed=7, snp=0.08, inv_min=100, inv_max=400)
    stages = [(12, 80)]
    ref = _oracle(seqs, stages)
    monkeypatch.setenv("SBL_NO_DENSE_PATH", "1")
    _set_park(monkeypatch, "1")
    a = _run(seqs, stages, window=2)
    _same_state(a, ref, "8 x 3 kbp, window 2, SBL_PARK=1")
    assert a[0][3] > 1024, "%d rounds: the sweep never came due" % a[0][3]


def test_three_virtual_ranks_take_the_same_rounds(monkeypatch, parky):
    """replicated commits: every rank parks and resumes the same transactions in the same rounds (_run asserts equal rounds)"""
    seqs, stages, ref = parky
    _set_park(monkeypatch, "1")
    _same_state(_run(seqs, stages, ranks=3), ref, "three ranks, SBL_PARK=1")
