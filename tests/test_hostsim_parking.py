"""Parked transactions (GraphView::park_of) in tests/hostsim: the product's transaction code stops after park_cap collapses, its Txn,
BulgeWork and fast scratch are copied into the end of its arena slice and copied back in a later round, fresh and resumed entries of a
round run interleaved in the round's order (k_commit and k_resume on two streams) -- and the result must still be the oracle's.

The model keeps the device protocol (reservation of the erase chain, the snapshot of slice_busy, shadow slices, park_hold, the
finished-marker sweep on DeviceBackend::commit's schedule, the claim-list overflow fallback) and checks its invariants as it goes:
nothing parked at a snapshot or at the end of an iteration, list sizes = live nodes at every round end except for the ids a parked
transaction has erased instances of, no resume in the round of the park, no park from a shadow slice, no finished marker left in a
later round with the same tag.  A violation ends the stage with an error, which fails the test like a mismatch.

Every case asserts that something parked, and that parking at most quadruples the rounds (test_gpu_parking.py's bound)."""
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from sibelia_amd import workloads as W
from tests.hostsim import hostsim as H
from tests.test_hostsim import SEEDS, HUGE


def _ref(seqs, k, D, it=4):
    bc, p, n = Oracle(seqs).enumerate(k)
    o = Oracle(seqs)
    b = o.simplify_stage(k, D, it)
    es, ep = o.state()
    return (bc, p, n), (b, es, ep)


def _stage(seqs, k, D, enum, it=4, **kw):
    bc, p, n = enum
    op = [np.arange(len(s), dtype=np.uint32) for s in seqs]
    return H.stage(seqs, op, k, D, it, bc, p, n, **kw)


def _same(got, want):
    hb, hs, hp, st = got
    b, es, ep = want
    return hb == b and hs == es and all(np.array_equal(a, c) for a, c in zip(hp, ep))


def _check(seqs, k, D, caps, configs, it=4, must_park=True, **kw):
    """every (window, order) of configs at every park cap of caps: the oracle's state, rounds within 4 x those without parking;
    returns the stats of the parking runs"""
    enum, want = _ref(seqs, k, D, it)
    out = []
    for window, order in configs:
        plain = _stage(seqs, k, D, enum, it, window=window, order_mode=order, **kw)
        assert _same(plain, want), ("park_cap 0", window, order, plain[3])
        for cap in caps:
            got = _stage(seqs, k, D, enum, it, window=window, order_mode=order, park_cap=cap, **kw)
            st = got[3]
            assert _same(got, want), ("park_cap", cap, window, order, st)
            assert st["rounds"] <= 4 * max(plain[3]["rounds"], 8), ("rounds", cap, window, order, st["rounds"], plain[3]["rounds"])
            out.append(st)
    if must_park:
        assert sum(s["parks"] for s in out) > 0, "nothing parked: the case does not exercise what it is for"
    return out


CONFIGS = [(w, o) for w in (1, 37, 1024) for o in (0, 1, 2)]


# (small seeds 11 and 26 have no transaction with two collapses: nothing parks there)
PARK_SEEDS = [s for s in SEEDS if s not in (11, 26)]


@pytest.mark.slow
@pytest.mark.parametrize("seed", PARK_SEEDS)
def test_parking_small_seeds(seed):
    """the golden small seeds of test_hostsim.py, park caps 1, 2, 4 x ascending, descending, shuffled order x windows 1, 37, 1024
    (some seeds have so few multi-collapse transactions that only cap 1 parks: the assertion is on the seed's runs together)"""
    seqs, k, D = W.small_case(seed)
    _check(seqs, k, D, (1, 2, 4), CONFIGS)


@pytest.mark.parametrize("k,D", [(15, 90), (25, 150)])
def test_parking_multi_snp_and_indels_many_chromosomes(k, D):
    seqs = W.gen_strains(L0=12_000, n=10, seed=21, snp=0.03, indel_every=200, inv_min=120, inv_max=600)
    st = _check(seqs, k, D, (1, 2), [(64, 2), (1024, 1)])
    assert all(s["parks"] > 0 for s in st), [s["parks"] for s in st]


def test_parking_in_a_dense_low_complexity_graph():
    """test_gpu_parking.py's dense case, made smaller: a 2 % mutated repeat of a 40-base motif, k = 12"""
    rng = np.random.default_rng(8)
    motif = rng.integers(0, 4, 40)
    seqs = []
    for _ in range(3):
        g = np.tile(motif, 60)
        m = rng.random(len(g)) < 0.02
        g[m] = (g[m] + rng.integers(1, 4, int(m.sum()))) % 4
        seqs.append(bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[g]))
    _check(seqs, 12, 80, (1, 2), [(37, 2), (1024, 0)])


def test_parking_through_grow_and_replay():
    """a node / element pool far too small (slack): capacity errors, grow, the iteration replays -- with transactions parked"""
    seqs = W.gen_strains(L0=12_000, n=6, seed=12, snp=0.03, indel_every=200, inv_min=120, inv_max=600)
    st = _check(seqs, 15, 90, (1,), [(64, 2)], slack=64)
    assert st[0]["grow_replays"] > 0, st[0]


def _stress(seed):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    from tools import stress as S
    seqs, stages, *_ = S.draw_case(seed)
    return seqs, stages[0]


@pytest.mark.slow
@pytest.mark.parametrize("cap", [1, 2, 4])
def test_parking_stress_seed_93194(cap):
    """round 6's last parity bug: tools/stress.py seed 93194 (12 strains x 24.6 kbp, k = 15), 8609 bulges"""
    seqs, (k, D) = _stress(93194)
    st = _check(seqs, k, D, (cap,), [(64, 2), (1024, 0)])
    assert all(s["parks"] > 0 for s in st)


@pytest.mark.slow
@pytest.mark.parametrize("v", HUGE, ids=[v["name"] for v in HUGE])
def test_parking_on_the_densest_vectors(v):
    """test_hostsim.py's densest golden vectors, every stage command at park cap 1, against the reference's fixtures"""
    from tests import vectors as V
    from sibelia_amd import formats as F
    ACGT = set(b"ACGT")
    seqs = V.vector_input(v)
    o, rng = Oracle(seqs), Oracle([])
    cur = [bytes(s) for s in seqs]
    op = [np.arange(len(s), dtype=np.uint32) for s in seqs]
    parks = 0
    for out in v["outputs"]:
        p = out["cmd"].split(":")
        namb = sum(1 for s in cur for c in s if c not in ACGT)
        if p[0] != "stage":
            for _ in range(namb):
                rng.rand()
            (o.enumerate if p[0] == "enum" else o.list_edges)(int(p[1]))
            continue
        k, D, it = int(p[1]), int(p[2]), int(p[3])
        if namb:
            cur = [bytes((c if c in ACGT else b"ACGT"[rng.rand() % 4]) for c in s) for s in cur]
        bc, pp, nn = Oracle(cur).enumerate(k)
        hb, hs, hp, st = H.stage(cur, op, k, D, it, bc, pp, nn, window=64, order_mode=2, arena_bytes=1 << 16, slack=1 << 21, park_cap=1)
        ob = o.simplify_stage(k, D, it)
        es, ep = o.state()
        assert hb == ob == out["bulges"] and hs == es and all(np.array_equal(a, c) for a, c in zip(hp, ep)), (out["cmd"], st)
        got = F.state_bytes(hb, hs, hp)
        assert len(got) == out["size"] and F.sha256(got) == out["sha256"], "differs from the reference fixture"
        parks += st["parks"]
        cur, op = hs, hp
    assert parks > 0


def test_parking_across_the_round_tag_wrap():
    """window 1, cap 1: one iteration takes more than SS_ROUND_MAX = 4095 rounds, the round counter wraps and every 11-bit tag of
    park_of comes round again (test_gpu_parking.py runs the same case on the device)"""
    seqs = W.gen_strains(L0=20_000, n=6, seed=3, snp=0.03, indel_every=1000, inv_min=200, inv_max=1000)
    for order in (0, 2):
        st = _check(seqs, 25, 150, (1,), [(1, order)])
        assert st[0]["max_iter_rounds"] > 4095 and st[0]["parks"] > 0, st[0]


@pytest.mark.parametrize("claim_cap", [4, 32])
def test_parking_with_claim_list_overflow(claim_cap):
    """claim lists longer than claim_cap (CLAIM_CAP on the device) fall back to ss_owns_footprint, which cannot see the erase-chain
    ids of a parked entry (ADVICE on rounds.hip:873): still exact"""
    seqs = W.gen_strains(L0=12_000, n=10, seed=21, snp=0.03, indel_every=200, inv_min=120, inv_max=600)
    st = _check(seqs, 15, 90, (1, 2), [(64, 2), (1024, 0)], claim_cap=claim_cap)
    assert all(s["fallbacks"] > 0 for s in st) and sum(s["parked_fallbacks"] for s in st) > 0, st
    seqs, k, D = W.small_case(SEEDS[2])
    st = _check(seqs, k, D, (1,), [(37, 2)], claim_cap=claim_cap)
    assert st[0]["fallbacks"] > 0


def test_negative_control_cleanup_when_parking(monkeypatch):
    """the model must be able to fail: with Cleanup run when a transaction parks instead of at its end, the list sizes a parked
    transaction reads stop being its own view -- tools/stress.py PARKY=1 seed 93194 then counts 5410 bulges for 5408"""
    monkeypatch.setenv("PARKY", "1")
    seqs, (k, D) = _stress(93194)
    monkeypatch.delenv("PARKY")
    enum, want = _ref(seqs, k, D)
    assert _same(_stage(seqs, k, D, enum, window=1024, order_mode=2, park_cap=1), want)
    monkeypatch.setenv("HOSTSIM_CLEANUP_AT_PARK", "1")
    try:
        got = _stage(seqs, k, D, enum, window=1024, order_mode=2, park_cap=1)
    except RuntimeError:
        return                                           # (a model invariant fired)
    assert not _same(got, want), "Cleanup at the park went unnoticed"
