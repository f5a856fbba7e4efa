"""Parked transactions (GraphView::park_of, round 5): a transaction that has made SBL_PARK collapses in one launch of k_commit and has
decided another one parks -- its LDS state goes to the end of its arena slice, the id stays pending -- and k_resume takes it up in a
later round.  Parking must change NOTHING but the number of rounds: every setting (0 = off, 1 = park after every collapse, 2 = the
default, 3) leaves the state the oracle leaves.  The workloads have multi-collapse transactions (several strains with their own SNPs at
the same place), indels (non-pristine blocks, deferred Cleanup visible to the probes of neighbouring ids), many chromosomes, wide
windows (the walking probe for every entry: the arena slice of a parked transaction must survive it), replays with checkpoints, and
the many-instances regime (mark lists and AnyBulges tables in the arena)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(seqs, stages, ranks=0):
    """ranks > 0: the same job on that many virtual ranks of device 0 (sharded enumeration, split probes, REPLICATED commits: every rank
    parks and resumes the same transactions)"""
    from sibelia_amd import BlockFinder
    if ranks:
        from sibelia_amd.dist import LocalShardedFinder
        bf = LocalShardedFinder(seqs, [0] * ranks)
    else:
        bf = BlockFinder(seqs, device=0)
    try:
        out = []
        for k, D in stages:
            n = bf.simplify_stage(k, D, 4)
            st = bf.stats()
            if ranks:
                assert len({int(x["rounds"]) for x in st}) == 1, "the ranks took different numbers of rounds"
                st = st[0]
            seq, pos = bf.state()
            out.append((n, int(st["rounds"]), seq, pos))
        return out
    finally:
        bf.close()


def _bounded_rounds(parked, plain, what):
    """parking trades rounds for shorter launches; a setting that multiplies the rounds is the livelock of round 5 (17 734 rounds where the
    serial chain would not start while anything was parked), not a trade"""
    for a, b in zip(parked, plain):
        assert a[1] <= 4 * max(b[1], 8), "%s: %d rounds with parking against %d without" % (what, a[1], b[1])


def _same_state(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0], "bulges differ: " + what
        assert x[2] == y[2] and all(np.array_equal(p, q) for p, q in zip(x[3], y[3])), "state differs: " + what


def _oracle(seqs, stages):
    from oracle.oracle import Oracle
    orc = Oracle(seqs)
    out = []
    for k, D in stages:
        n = orc.simplify_stage(k, D, 4)
        so, po = orc.state()
        out.append((n, 0, so, po))
    return out


@pytest.mark.parametrize("k,D", [(25, 150), (15, 60), (31, 300), (20, 500)])
def test_parking_changes_nothing(monkeypatch, k, D):
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=120_000, n=8, seed=41, snp=0.03, inv_min=1000, inv_max=6000)
    ref = _oracle(seqs, [(k, D)])
    rounds = {}
    for cap in ("0", "1", "2", "3"):
        monkeypatch.setenv("SBL_PARK", cap)
        monkeypatch.setenv("SBL_CHECK_INDEX", "1")
        a = _run(seqs, [(k, D)])
        _same_state(a, ref, "SBL_PARK=" + cap)
        rounds[cap] = a[0][1]
    assert rounds["1"] > rounds["0"], "SBL_PARK=1 parked nothing (%s): the test does not exercise what it is for" % rounds
    assert max(rounds.values()) <= 4 * rounds["0"], "parking multiplied the rounds: %s" % rounds


@pytest.mark.parametrize("k,D", [(25, 150), (15, 60)])
def test_parking_changes_nothing_on_three_virtual_ranks(monkeypatch, k, D):
    """round 5 switched parking off whenever a communicator was attached (the virtual-rank cases crashed); it is on everywhere now"""
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=120_000, n=8, seed=41, snp=0.03, inv_min=1000, inv_max=6000)
    ref = _oracle(seqs, [(k, D)])
    rounds = {}
    for cap in ("0", "1", "2"):
        monkeypatch.setenv("SBL_PARK", cap)
        a = _run(seqs, [(k, D)], ranks=3)
        _same_state(a, ref, "three ranks, SBL_PARK=" + cap)
        rounds[cap] = a[0][1]
    assert rounds["1"] > rounds["0"], "SBL_PARK=1 parked nothing on three ranks (%s)" % rounds
    assert max(rounds.values()) <= 4 * rounds["0"], "parking multiplied the rounds: %s" % rounds


def test_parking_over_a_cascade_with_many_chromosomes(monkeypatch):
    from sibelia_amd import workloads as W
    base = W.gen_strains(L0=60_000, n=6, seed=9, snp=0.03, inv_min=500, inv_max=3000)
    rng = np.random.default_rng(6)
    seqs = []
    for s in base:
        p = 0
        while p < len(s):
            q = min(len(s), p + int(rng.integers(40, 6000)))
            seqs.append(s[p:q]); p = q
    stages = [(22, 100), (25, 150), (30, 150)]
    ref = _oracle(seqs, stages)
    monkeypatch.setenv("SBL_PARK", "0")
    plain = _run(seqs, stages)
    for cap in ("1", "2"):
        monkeypatch.setenv("SBL_PARK", cap)
        a = _run(seqs, stages)
        _same_state(a, ref, "cascade, SBL_PARK=" + cap)
        _bounded_rounds(a, plain, "cascade, SBL_PARK=" + cap)


def test_parking_with_walking_probes_and_reservations(monkeypatch):
    """block index off: every probe walks in the arena slice of its window position -- the spare slice where a parked transaction lives"""
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=100_000, n=6, seed=13, snp=0.03, inv_min=1000, inv_max=4000)
    ref = _oracle(seqs, [(25, 150)])
    monkeypatch.setenv("SBL_NO_BLOCK_INDEX", "1")
    monkeypatch.setenv("SBL_PARK", "0")
    plain = _run(seqs, [(25, 150)])
    for cap in ("1", "2"):
        monkeypatch.setenv("SBL_PARK", cap)
        a = _run(seqs, [(25, 150)])
        _same_state(a, ref, "walking probes, SBL_PARK=" + cap)
        _bounded_rounds(a, plain, "walking probes, SBL_PARK=" + cap)


def test_parking_survives_checkpointed_replays(monkeypatch):
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=80_000, n=6, seed=12, snp=0.03, inv_min=1000, inv_max=4000)
    ref = _oracle(seqs, [(25, 150)])
    monkeypatch.setenv("SBL_PARK", "1")
    monkeypatch.setenv("SBL_TEST_ELEM_SLACK", "64")
    _same_state(_run(seqs, [(25, 150)]), ref, "grow + replay, SBL_PARK=1")


def test_parking_with_dozens_of_instances(monkeypatch):
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=8_000, n=48, seed=5, inv_min=100, inv_max=400)
    ref = _oracle(seqs, [(25, 150)])
    monkeypatch.setenv("SBL_PARK", "0")
    plain = _run(seqs, [(25, 150)])
    for cap in ("1", "2", "4"):
        monkeypatch.setenv("SBL_PARK", cap)
        a = _run(seqs, [(25, 150)])
        _same_state(a, ref, "48 strains, SBL_PARK=" + cap)
        _bounded_rounds(a, plain, "48 strains, SBL_PARK=" + cap)


def _stress_case(seed, many):
    """the case tools/stress.py draws for `seed` (MANY=1: 30 - 70 strains of a few kbp)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import stress
    return stress.draw_case(seed, many=many)[:2]


def test_list_sizes_of_a_parked_transaction_stay_private(monkeypatch):
    """tools/stress.py seed 93194 (12 strains x 24.5 kbp, k = 15, D = 91, 8 % SNPs): id 8111 parked after two collapses; the instances it
    had erased no longer carried a mark, so its reservation of the next round did not claim their ids, and their list sizes -- decremented
    by Cleanup at the transaction's END only (bifurcationstorage.cpp:33-41, :71-75) -- were read one too high by id 8125 running beside the
    resumed transaction: it collapsed in the other direction and the stage counted 8608 bulges instead of 8609 (the final sequences
    happened to agree).  k_reserve now claims the ids of a parked transaction's erase chain until it is through (bulge_txn.h: PARK_IMG)."""
    seqs, stages = _stress_case(93194, False)
    ref = _oracle(seqs, stages)
    assert ref[0][0] == 8609
    for cap in ("1", "2", None):
        if cap is None:
            monkeypatch.delenv("SBL_PARK", raising=False)
        else:
            monkeypatch.setenv("SBL_PARK", cap)
        _same_state(_run(seqs, stages), ref, "seed 93194, SBL_PARK=%s" % cap)


def test_the_serial_chain_starts_although_transactions_are_parked(monkeypatch):
    """The regime of tools/stress.py MANY=1, seed 67000 (57 strains x 8 kbp, k = 31, D = 369: a transaction's neighbourhood is a tenth of
    a genome, the rounds are serial and the driver asks for the chain from id 7 on), cut to 24 strains x 3 kbp so that it runs in seconds.
    Round 5 blamed parking for that case's 17 734 rounds; measured in round 6 it takes as many WITHOUT parking (docs/history/r06.md: the
    serial chain stops at the first id it made pending itself, ~10 ids per round, whatever the park cap).  What parking must not do is
    add to it: chain() used to refuse while anything was parked and nothing stopped new parking -- now the request for the chain stops
    it (GraphView::park_hold), what is parked drains, and the chain runs."""
    seqs, stages = _stress_case(67000, True)
    seqs = [s[:3000] for s in seqs[:24]]
    ref = _oracle(seqs, stages)
    monkeypatch.setenv("SBL_PARK", "0")
    plain = _run(seqs, stages)
    _same_state(plain, ref, "chain regime, SBL_PARK=0")
    for cap in ("1", "2", "4", None):                  # None: the default of this regime
        if cap is None:
            monkeypatch.delenv("SBL_PARK", raising=False)
        else:
            monkeypatch.setenv("SBL_PARK", cap)
        a = _run(seqs, stages)
        _same_state(a, ref, "chain regime, SBL_PARK=%s" % cap)
        for x, y in zip(a, plain):
            assert x[1] <= 1.5 * y[1] + 16, "chain regime, SBL_PARK=%s: %d rounds against %d without parking" % (cap, x[1], y[1])


def test_parking_in_a_dense_low_complexity_graph_with_few_instances_per_id(monkeypatch):
    """at most a dozen instances per id (round 5's fence `instances > 12 ids` did not cover it) but dense conflict neighbourhoods: a few
    strains of low-complexity sequence at a small k -- chain mode with parking on"""
    rng = np.random.default_rng(77)
    unit = rng.integers(0, 4, 400)
    base = np.concatenate([unit if rng.random() < 0.7 else rng.integers(0, 4, 400) for _ in range(60)])
    seqs = []
    for s in range(5):
        g = base.copy()
        m = rng.random(len(g)) < 0.02
        g[m] = (g[m] + rng.integers(1, 4, int(m.sum()))) % 4
        seqs.append(bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[g]))
    stages = [(12, 80)]
    ref = _oracle(seqs, stages)
    monkeypatch.setenv("SBL_NO_DENSE_PATH", "1")       # (the ordered rounds, not the one-launch path)
    monkeypatch.setenv("SBL_PARK", "0")
    plain = _run(seqs, stages)
    _same_state(plain, ref, "dense, SBL_PARK=0")
    for cap in ("1", "2"):
        monkeypatch.setenv("SBL_PARK", cap)
        a = _run(seqs, stages)
        _same_state(a, ref, "dense, SBL_PARK=" + cap)
        _bounded_rounds(a, plain, "dense, SBL_PARK=" + cap)


def test_rounds_that_turn_into_a_slow_serial_chain_give_way_to_the_one_launch_path(monkeypatch):
    """tools/stress.py MANY=1, seed 67012 (57 strains x 2 kbp, k = 16, D = 148: a transaction's neighbourhood is the genome): the ordered
    rounds commit one or two transactions each and took 19.8 s (1 220 rounds) where the oracle takes 0.6 s.  After a second in chain
    mode with less than 40 % of the stage done the attempt is given up and the stage runs through k_dense_stage (2.5 s on its own):
    exact either way, `rounds` = 0 and one replay in the stats, and SBL_NO_DENSE_SWITCH=1 keeps the rounds."""
    import time
    seqs, stages = _stress_case(67012, True)
    ref = _oracle(seqs, stages[:1])
    t0 = time.time()
    a = _run(seqs, stages[:1])
    dt = time.time() - t0
    _same_state(a, ref, "seed 67012, switch to the one-launch path")
    assert a[0][1] == 0, "the stage finished in the ordered rounds (%d rounds): the switch did not happen" % a[0][1]
    assert dt < 10.0, "seed 67012 took %.1f s" % dt


def test_parking_across_the_round_tag_wrap(monkeypatch):
    """A window of one entry and a park after every collapse: one iteration takes more than SS_ROUND_MAX = 4095 rounds (tests/hostsim
    counts 6 231 for this case), so the round counter wraps (4095 -> 1) and every 11-bit round tag of park_of comes round again --
    a finished marker that survived its sweep would make k_commit skip an id as "finished in this round".  Same state as the oracle."""
    from sibelia_amd import BlockFinder, workloads as W
    seqs = W.gen_strains(L0=20_000, n=6, seed=3, snp=0.03, indel_every=1000, inv_min=200, inv_max=1000)
    ref = _oracle(seqs, [(25, 150)])
    monkeypatch.setenv("SBL_PARK", "1")
    bf = BlockFinder(seqs, device=0)
    try:
        bf.set_window(1)
        n = bf.simplify_stage(25, 150, 4)
        rounds = int(bf.stats()["rounds"])
        seq, pos = bf.state()
    finally:
        bf.close()
    _same_state([(n, rounds, seq, pos)], ref, "window 1, SBL_PARK=1")
    assert rounds > 4095, "%d rounds: the round counter never wrapped" % rounds
