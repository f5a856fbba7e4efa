"""The copy-back of a simplification stage (csrc/graphbuild.hip: k_seg_flags .. k_scatter_linear, DeviceBackend::rank_segments): the
final list is a chain of segments -- maximal runs of consecutive slots linked consecutively --, whose heads are kept as one 64-bit
mask per 64 slots; a collapse with dS == dT rewrites slots in place (no new segment), one with dS > dT links fresh slots from the end
of the pool into the list (the list leaves slot order: two more segments), one with dS < dT leaves dead slots behind (one more).

Every case compares the final state (sequences, original positions) and the bulge count with the oracle, as `bench.py --check` does,
as a plain run, with SBL_CHECK_INDEX=1 (the maintained block index against a rebuild) and with SBL_CHECK_DICTIONARY=1 (the only reader
of the full old-slot -> new-slot map, which the copy-back otherwise no longer writes).

Inputs: two copies of one random sequence (k = 15, D = 60), the second with planted sites -- L changed bases (substitution), L more
(insertion) or L less (deletion).  Which branch is rewritten is the reference's choice (multiplicities, then instance order), so
whether an indel shortens or lengthens the rewritten record is read off the oracle's result, not assumed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, D = 15, 60
SWITCHES = ({}, {"SBL_CHECK_INDEX": "1"}, {"SBL_CHECK_DICTIONARY": "1"})
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _plant(seed, n, sites):
    """(first, second): n random bases and their copy with the sites = (kind, start, L) planted, starts ascending and apart"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, n, dtype=np.uint8)
    out, p = [], 0
    for kind, q, L in sites:
        assert q >= p
        out.append(a[p:q])
        if kind == "sub":
            out.append((a[q:q + L] + rng.integers(1, 4, L, dtype=np.uint8)) % 4)
            p = q + L
        elif kind == "ins":
            new = rng.integers(0, 4, L, dtype=np.uint8)
            new[0] = (a[q] + 1 + new[0] % 3) % 4                   # (an inserted stretch must not extend a flank)
            new[-1] = (a[q - 1] + 1 + new[-1] % 3) % 4
            out.append(new)
            p = q
        else:
            if a[q] == a[q + L]:
                a[q] = (a[q] + 1) % 4
            if a[q + L - 1] == a[q - 1]:
                a[q + L - 1] = (a[q + L - 1] + 1) % 4
            p = q + L
    out.append(a[p:])
    return _ACGT[a].tobytes(), _ACGT[np.concatenate(out)].tobytes()


def _oracle(seqs):
    from oracle.oracle import Oracle
    orc = Oracle(seqs)
    try:
        nid = orc.enumerate(K)[0]
        n = orc.simplify_stage(K, D, 4)
        so, po = orc.state()
        return n, so, [np.array(p) for p in po], nid
    finally:
        orc.close()


def _gpu(seqs):
    from sibelia_amd import BlockFinder
    bf = BlockFinder(seqs, device=0)
    try:
        n = bf.simplify_stage(K, D, 4)
        seq, pos = bf.state()
        st = bf.stats()
        return n, seq, [np.array(p) for p in pos], st
    finally:
        bf.close()


def _check(monkeypatch, seqs, ref, what, switches=SWITCHES, dense=False):
    # (inputs of this size would take the one-launch path, which keeps no block index: the ordered rounds, as on real inputs)
    if not dense:
        monkeypatch.setenv("SBL_NO_DENSE_PATH", "1")
    for sw in switches:
        for name in ("SBL_CHECK_INDEX", "SBL_CHECK_DICTIONARY", "SBL_TEST_ELEM_SLACK"):
            monkeypatch.delenv(name, raising=False)
        for name, v in sw.items():
            monkeypatch.setenv(name, v)
        n, seq, pos, st = _gpu(seqs)
        tag = "%s, %s" % (what, ", ".join("%s=%s" % x for x in sw.items()) or "plain")
        assert n == ref[0], "bulges differ (%d, oracle %d): %s" % (n, ref[0], tag)
        assert seq == ref[1], "sequences differ: " + tag
        assert all(np.array_equal(p, q) for p, q in zip(pos, ref[2])), "original positions differ: " + tag
        if "SBL_CHECK_DICTIONARY" in sw:
            assert st["dict_checked"] > 0 and st["dict_mismatches"] == 0, "dictionary check %s: %s" % (st, tag)
        yield st


def _run(monkeypatch, seqs, ref, what, **kw):
    return list(_check(monkeypatch, seqs, ref, what, **kw))


def test_no_collapse_one_segment(monkeypatch):
    """bifurcations but no bulge: the second record follows the first for 700 bases and then goes its own way.  The list stays one
    segment, and SBL_CHECK_INDEX sees the index of the stage start (written by the marks pass) untouched"""
    rng = np.random.default_rng(1)
    a = _ACGT[rng.integers(0, 4, 1500)].tobytes()
    seqs = [a, a[:700] + _ACGT[rng.integers(0, 4, 800)].tobytes()]
    ref = _oracle(seqs)
    assert ref[3] > 0 and ref[0] == 0, "the case wants bifurcations (%d) and no bulge (%d)" % (ref[3], ref[0])
    assert ref[1] == seqs
    _run(monkeypatch, seqs, ref, "no collapse")


@pytest.mark.parametrize("kind", ["sub", "ins", "del"])
def test_one_collapse(monkeypatch, kind):
    """one site: a substitution (dS == dT: one segment), an indel (the rewritten record grows: dS > dT, three segments; or shrinks:
    dS < dT, two segments -- whichever the reference chooses, the other indel kind gives the other one)"""
    seqs = list(_plant(2, 1200, [(kind, 600, 20)]))
    ref = _oracle(seqs)
    assert ref[0] == 1, "one planted site, %d bulges" % ref[0]
    la, lb = len(ref[1][0]), len(ref[1][1])
    assert la == lb and (la == 1200 if kind == "sub" else la in (1200, 1200 + (20 if kind == "ins" else -20)))
    _run(monkeypatch, seqs, ref, "one %s" % kind)


def test_collapses_at_the_separators_and_across_a_block(monkeypatch):
    """substitutions whose branches start at the first k-mer of the first record (abutting the first separator) and end at the last
    k-mer of both records (the second abuts the last separator); a site whose branch lies across slot 640 = 10 x 64; insertions
    and deletions in between (dS > dT, dS < dT)"""
    n = 1500
    sites = [("sub", K, 12), ("ins", 200, 9), ("del", 400, 11), ("sub", 630, 20), ("ins", 800, 30), ("del", 1000, 30), ("sub", n - K - 12, 12)]
    seqs = list(_plant(3, n, sites))
    ref = _oracle(seqs)
    assert ref[0] == len(sites), "%d planted sites, %d bulges: a site at a record end did not collapse" % (len(sites), ref[0])
    assert ref[1][0] == ref[1][1], "after every site collapsed the two records spell the same"
    assert ref[1][0][:K + 12 + K] in (seqs[0][:K + 12 + K], seqs[1][:K + 12 + K])
    _run(monkeypatch, seqs, ref, "sites at the separators")


def test_more_than_1024_segments(monkeypatch):
    """700 indels of 3 bases, 60 bases apart: every collapse has dS != dT (the branches of an indel differ in length whichever is
    rewritten), so the final list has more than 1024 segments (one or two more per collapse) -- more than one workgroup of the
    ranking kernels and ten rounds of pointer jumping"""
    nsites = 700
    sites = [("ins" if i % 2 else "del", 60 * (i + 1), 3) for i in range(nsites)]
    seqs = list(_plant(4, 60 * (nsites + 2), sites))
    ref = _oracle(seqs)
    assert ref[0] == nsites, "%d planted sites, %d bulges" % (nsites, ref[0])
    assert ref[1][0] == ref[1][1] and len(seqs[0]) == len(seqs[1]), "350 insertions and 350 deletions of 3 bases, all collapsed"
    _run(monkeypatch, seqs, ref, "700 indels")


def test_rebuild_of_the_index_after_a_restart(monkeypatch):
    """SBL_TEST_ELEM_SLACK=64: the insertions run out of element slots, the optimistic attempt is abandoned and the stage runs again
    with checkpoints, where a roll-back rebuilds the block index from the arrays (k_build_blkidx); SBL_CHECK_INDEX compares the
    maintained index with a rebuild at the end"""
    sites = [("ins" if i % 2 else "del", 100 * (i + 1), 12) for i in range(24)]
    seqs = list(_plant(5, 2600, sites))
    ref = _oracle(seqs)
    assert ref[0] == len(sites)
    st = _run(monkeypatch, seqs, ref, "element slack 64", switches=({"SBL_TEST_ELEM_SLACK": "64", "SBL_CHECK_INDEX": "1"},))[0]
    assert st["replays"] >= 1, "the stage never restarted: %s" % st
