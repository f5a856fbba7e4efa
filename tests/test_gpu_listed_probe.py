"""The walking probe over a list.  k_probe_idx appends the window entries it cannot serve to a list, and k_probe_listed runs over that
list with a small fixed grid -- in the ordered rounds and behind the ONE index-probe launch of an incremental snapshot -- instead of one workgroup
per window entry.  Where there is no index probe (no block index, SBL_NO_IDX_PROBE, windows of more than 16 blocks) and in the shares of
a split probe the walker keeps its grid of one workgroup per entry.  Only launch shapes changed, so every case must leave the state the
oracle leaves, without a replay.

Also here: k_touched_list (the list an incremental snapshot starts from; one atomic per 4096 ids instead of one per wave) on three
patterns of flags, through its test entry point."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, D = 25, 150
WALKER_LINE = re.compile(r"\[sbl\] listed walker: entries (\d+), beyond a workgroup's first (\d+), in a shadow slice (\d+)")
STATS_LINE = re.compile(r"\[sbl\] block index: probes known-live (\d+), < 2 instances (\d+), clean (\d+), live (\d+), table full (\d+), not served (\d+)")


def _oracle(seqs, stages):
    from oracle.oracle import Oracle
    orc = Oracle(seqs)
    out = []
    for k, d in stages:
        n = orc.simplify_stage(k, d, 4)
        so, po = orc.state()
        out.append((n, so, po))
    return out


def _plant(seqs, copies, motifs=3, mlen=60, seed=99):
    """`motifs` random 60-mers written over every strain at copies x motifs evenly spaced places: repeat families.  The k-mers at a
    repeat's ends are ids with copies x strains instances in unrelated contexts -- more marks between them than k_probe_idx's verdict
    table holds, which is what sends an entry to the walking probe (strain sets without repeats never do: measured, 0 of 115 000)"""
    rng = np.random.default_rng(seed)
    ms = [bytes(rng.choice(list(b"ACGT"), mlen).tolist()) for _ in range(motifs)]
    out = []
    for s in seqs:
        b = bytearray(s)
        step = (len(b) - 2 * mlen) // (copies * motifs)
        for j in range(copies * motifs):
            o = mlen + j * step
            b[o:o + mlen] = ms[j % motifs]
        out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def strains():
    """8 x 30 kbp with SNPs, indels and inversions: (strains, the oracle's result at default k and D)"""
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=30_000, n=8, seed=5, snp=0.02, indel_every=300, inv_min=1000, inv_max=4000)
    return seqs, _oracle(seqs, [(K, D)])


@pytest.fixture(scope="module")
def diverged():
    """8 x 30 kbp, 8 % SNPs and an indel every 100 bp, for D = 1000: 180 ordered rounds (the less diverged set above turns into one
    serial chain there and is handed to the one-launch path, which counts as a replay)"""
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=30_000, n=8, seed=5, snp=0.08, indel_every=100, inv_min=1000, inv_max=4000)
    return seqs, _oracle(seqs, [(K, 1000)])


@pytest.fixture(scope="module")
def repeats():
    """the same strain set with three repeat families of 12 copies planted (default k and D): 1805 of 527 000 probes fall through"""
    from sibelia_amd import workloads as W
    seqs = _plant(W.gen_strains(L0=30_000, n=8, seed=5, snp=0.02, indel_every=300, inv_min=1000, inv_max=4000), 12)
    return seqs, _oracle(seqs, [(K, D)])


@pytest.fixture(scope="module")
def small_repeats():
    """8 x 6 kbp, k = 15, D = 91, three repeat families of 8 copies: small enough for a window of one entry"""
    from sibelia_amd import workloads as W
    seqs = _plant(W.gen_strains(L0=6000, n=8, seed=7, snp=0.03, indel_every=300, inv_min=200, inv_max=600), 8)
    stages = [(15, 91)]
    return seqs, stages, _oracle(seqs, stages)


@pytest.fixture(scope="module")
def parky():
    """tools/stress.py's case for seed 93194 (12 strains x 24.5 kbp, k = 15, D = 91: the one the parked transactions' tests use) with
    three repeat families of 8 copies planted"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import stress
    seqs, stages = stress.draw_case(93194, many=False)[:2]
    seqs = _plant(seqs, 8)
    return seqs, stages, _oracle(seqs, stages)


def _run(seqs, stages, window=0, ranks=0):
    """per stage: (bulges, sequences, positions, stats); ranks > 0: the same job on that many virtual ranks of device 0"""
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
        for k, d in stages:
            n = bf.simplify_stage(k, d, 4)
            st = bf.stats()
            if ranks:
                assert len({int(x["rounds"]) for x in st}) == 1, "the ranks took different numbers of rounds: %s" % [int(x["rounds"]) for x in st]
                assert all(int(x["replays"]) == 0 for x in st)
                st = st[0]
            seq, pos = bf.state()
            out.append((n, seq, pos, dict(st)))
        return out
    finally:
        bf.close()


def _exact(got, ref, what):
    assert len(got) == len(ref)
    for x, y in zip(got, ref):
        assert x[0] == y[0], "bulges differ (%d, oracle %d): %s" % (x[0], y[0], what)
        assert x[1] == y[1] and all(np.array_equal(p, q) for p, q in zip(x[2], y[2])), "state differs: " + what
        assert int(x[3]["replays"]) == 0, "%d replays: %s" % (x[3]["replays"], what)


def _index_stats(capfd):
    """what k_probe_idx did in the stages since the last call, by outcome (SBL_TEST_FLAGS=32: reported on stderr at the end of a stage)"""
    z, w = np.zeros(6, dtype=np.int64), np.zeros(3, dtype=np.int64)
    err = capfd.readouterr().err
    for m in STATS_LINE.finditer(err):
        z += np.array([int(v) for v in m.groups()], dtype=np.int64)
    for m in WALKER_LINE.finditer(err):
        w += np.array([int(v) for v in m.groups()], dtype=np.int64)
    return {"known_live": int(z[0]), "served": int(z[1] + z[2] + z[3]), "unserved": int(z[4] + z[5]),
            "walked": int(w[0]), "beyond_first": int(w[1]), "shadow": int(w[2])}


def test_walker_takes_the_few_entries_the_index_cannot_serve(monkeypatch, capfd, repeats):
    """all four iterations: the rounds and the incremental snapshots of iterations 2 - 4 probe from the block index, and a small share
    of the entries (the repeat families' ids) falls through to the listed walker, which walks exactly those"""
    seqs, ref = repeats
    monkeypatch.setenv("SBL_TEST_FLAGS", "32")
    capfd.readouterr()
    a = _run(seqs, [(K, D)])
    z = _index_stats(capfd)
    print("iterations %d rounds %d, k_probe_idx: %s" % (a[0][3]["iterations"], a[0][3]["rounds"], z))
    _exact(a, ref, "8 x 30 kbp with repeats, defaults")
    assert int(a[0][3]["iterations"]) == 4 and int(a[0][3]["rounds"]) > 0, "the incremental snapshots of iterations 2 - 4 did not run"
    assert z["served"] > 0 and z["unserved"] > 0, "k_probe_idx outcomes %s: the test needs entries of both kinds" % z
    assert z["unserved"] * 4 < z["served"], "k_probe_idx outcomes %s: the walker was meant to see a small share" % z
    assert z["walked"] == z["unserved"], "%d entries listed, %d walked" % (z["unserved"], z["walked"])


@pytest.mark.parametrize("case", ["no_block_index", "no_idx_probe", "wide_windows"])
def test_walker_keeps_its_full_grid_without_an_index_probe(monkeypatch, capfd, strains, diverged, case):
    """the walker serves every entry: one workgroup per window entry, as before"""
    monkeypatch.setenv("SBL_TEST_FLAGS", "32")
    if case == "no_block_index":
        monkeypatch.setenv("SBL_NO_BLOCK_INDEX", "1")
    if case == "no_idx_probe":
        monkeypatch.setenv("SBL_NO_IDX_PROBE", "1")
    (seqs, ref), d = (diverged, 1000) if case == "wide_windows" else (strains, D)      # D + k + 2 = 1027 steps: 17 blocks of 64 slots, probe_idx serves nobody
    capfd.readouterr()
    a = _run(seqs, [(K, d)])
    z = _index_stats(capfd)
    _exact(a, ref, case)
    assert int(a[0][3]["rounds"]) > 0
    assert z["served"] == 0 and z["unserved"] == 0 and z["known_live"] == 0 and z["walked"] == 0, "k_probe_idx or the listed walker ran (%s) where the walker serves everything" % z


@pytest.mark.parametrize("window", [1, 2, 37])
def test_list_with_tiny_windows(monkeypatch, small_repeats, window):
    """a window of 1, 2 and 37 entries: a list of at most that many, and as few arena slices for the snapshots' walker"""
    seqs, stages, ref = small_repeats
    monkeypatch.setenv("SBL_NO_DENSE_PATH", "1")
    _exact(_run(seqs, stages, window=window), ref, "window %d" % window)


@pytest.mark.parametrize("grid", [1, 3])
def test_stride_loop_over_the_list(monkeypatch, capfd, parky, grid):
    """the walker's grid pinned to 1 and 3 workgroups (SBL_TEST_WALK_GRID): launches with more entries than that send a workgroup round
    its loop -- in a snapshot, where all entries of a workgroup share its arena slice, and in the rounds"""
    seqs, stages, ref = parky
    monkeypatch.setenv("SBL_TEST_FLAGS", "32")
    monkeypatch.setenv("SBL_TEST_WALK_GRID", str(grid))
    capfd.readouterr()
    a = _run(seqs, stages)
    z = _index_stats(capfd)
    print("grid %d: %s" % (grid, z))
    _exact(a, ref, "walker grid %d" % grid)
    assert z["walked"] == z["unserved"] and z["beyond_first"] > 0, "walker grid %d, %s: no workgroup took a second entry" % (grid, z)


def test_walked_probe_beside_parked_transactions(monkeypatch, capfd, parky):
    """SBL_PARK=1: a park after every collapse.  With the default window and with one of 37 entries some entry the walker takes finds
    its own arena slice holding a parked transaction and works in the shadow slice.  Exact, and the rounds within the bound of the
    other parking tests (at most 4 x those without parking)"""
    seqs, stages, ref = parky
    monkeypatch.setenv("SBL_TEST_FLAGS", "32")
    monkeypatch.setenv("SBL_PARK", "0")
    plain = _run(seqs, stages)
    _exact(plain, ref, "SBL_PARK=0")
    monkeypatch.setenv("SBL_PARK", "1")
    capfd.readouterr()
    a = _run(seqs, stages)
    b = _run(seqs, stages, window=37)
    z = _index_stats(capfd)
    print("SBL_PARK=1: %s" % z)
    _exact(a, ref, "SBL_PARK=1")
    _exact(b, ref, "SBL_PARK=1, window 37")
    for x, y in zip(a, plain):
        rx, ry = int(x[3]["rounds"]), int(y[3]["rounds"])
        print("rounds: %d with SBL_PARK=1, %d without" % (rx, ry))
        assert rx <= 4 * max(ry, 8), "%d rounds with parking against %d without" % (rx, ry)
    assert sum(int(x[3]["rounds"]) for x in a) > sum(int(y[3]["rounds"]) for y in plain), "SBL_PARK=1 parked nothing: the test does not exercise what it is for"
    assert z["shadow"] > 0, "%s: no walked entry met a parked transaction in its slice" % z


def test_three_virtual_ranks(parky):
    """a split probe keeps the full grid over each rank's share; the three ranks leave what one rank leaves"""
    seqs, stages, ref = parky
    one = _run(seqs, stages)
    three = _run(seqs, stages, ranks=3)
    _exact(one, ref, "one rank")
    _exact(three, ref, "three ranks")
    assert one[0][1] == three[0][1] and all(np.array_equal(p, q) for p, q in zip(one[0][2], three[0][2]))


@pytest.mark.parametrize("pattern", ["none", "all", "one_per_cent"])
@pytest.mark.parametrize("nid", [4096 * 3 + 1234, 300, 2 * 4096 * 1024 + 77])
def test_touched_list(pattern, nid):
    """k_touched_list on flags for ids 0 .. nid with nid no multiple of a workgroup's span (4096 ids) -- a few spans, less than one span,
    and more spans than the grid has workgroups (1024), so that they go round the grid-stride loop: exactly the touched ids below nid
    are listed, once each; touch and need are left 0 for every id; the walking probe's list is left empty"""
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(20250)
    touch = np.zeros(nid + 1, dtype=np.uint8)
    if pattern == "all":
        touch[:] = 1
    elif pattern == "one_per_cent":
        touch[rng.random(nid + 1) < 0.01] = 1
        touch[nid - 1] = 1                       # the last id that can be listed
    touch[nid] = 1                               # never listed, but cleared
    bf = BlockFinder([b"ACGTACGTAC"], device=0)
    try:
        lst, wcount, touch_after, need_after = bf.test_touched_list(touch)
    finally:
        bf.close()
    want = np.flatnonzero(touch[:nid]).astype(np.uint32)
    assert len(lst) == len(want), "%d ids listed, %d touched" % (len(lst), len(want))
    assert np.array_equal(np.sort(lst), want)
    assert wcount == 0 and not touch_after.any() and not need_after.any()
