"""Gather-first collapses of more than one register chunk (commit.hip: wave_collapse_g<NC>, chosen by wave_collapse_any from
span = max(dS, dT) + k + 1): k_commit takes spans up to 64 through <1>, up to 128 through <2>, up to 192 through <3> and longer ones
through the older wave_collapse.  Every case must leave the state the oracle leaves -- bulge count, sequences, positions --, once as a plain run and
once with SBL_PHASES=1, where every transaction is timed and the library counts its collapses by form, by dS == dT / dS > dT / dS < dT
and by span (sbl_collapse_hist); the counts show that the case went through the instantiation it aims at.

The planted inputs are two copies of one random sequence (k = 25, D = 150).  The second copy differs at sites 600 bases apart: a
stretch of L bases of which every one is changed (a substitution: both branches are L + k steps), L bases more (an insertion) or L
bases less (a deletion: one branch is k steps, the other L + k).  span = L + 2 k + 1, and L is chosen to put it at 62 .. 66,
126 .. 130 and 173 .. 177: the edges of the chunks with a step more on either side, and the largest span D allows -- 175: FillVisit
stops below D steps (bulgeremoval.cpp:122-146), so the longest branch is 149 steps; the sites planted at 176 and 177 stay as they
are, in the oracle as on the device.  Which branch is the source is decided by bifurcation multiplicities and, at a tie, by instance
order -- not by length --, so of an insertion and a deletion of the same length one has dS > dT and the other dS < dT.
D = 150 reaches no span beyond 192; test_planted_beyond_three_chunks plants 190 .. 194 and the largest span at D = 200.

Inputs of this size would take the one-launch path (k_dense_stage), which never reaches k_commit: SBL_NO_DENSE_PATH=1."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, D = 25, 150
EDGES = (63, 64, 65, 127, 128, 129, D + K)            # spans every planted case must collapse at, each as dS == dT, dS > dT and dS < dT
PLANTED = tuple(range(62, 67)) + tuple(range(126, 131)) + tuple(range(D + K - 2, D + K + 3))
SPACING = 600
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
REL = ("dS == dT", "dS > dT", "dS < dT")
FORM = ("wave_collapse_g<1>", "wave_collapse_g<2>", "wave_collapse_g<3>", "wave_collapse")


def _form_of(span):
    """the form k_commit gives a collapse of this span"""
    return 0 if span <= 64 else 1 if span <= 128 else 2 if span <= 192 else 3


def _rc(s):
    return s.translate(_COMP)[::-1]


def _differs(rng, ref, n):
    """n bases, the first different from ref[0] and the last from ref[1] (an inserted stretch must not extend a flank)"""
    v = rng.integers(0, 4, n, dtype=np.uint8)
    v[0] = (ref[0] + 1 + v[0] % 3) % 4
    v[-1] = (ref[1] + 1 + v[-1] % 3) % 4
    return v


def _planted(seed, spans=PLANTED, marks=False, reverse=False, D=D):
    """(strains, sites): sites = (kind, L, start in the first strain); marks: a third record of decoys, see _decoys"""
    rng = np.random.default_rng(seed)
    sites = [(kind, s - 2 * K - 1) for s in spans for kind in ("sub", "ins", "del")]
    n = SPACING * (len(sites) + 1)
    a = rng.integers(0, 4, n, dtype=np.uint8)
    pieces, p, where, decoys = [], 0, [], []
    for i, (kind, L) in enumerate(sites):
        q = SPACING * (i + 1)
        pieces.append(a[p:q])
        if kind == "sub":
            new = (a[q:q + L] + rng.integers(1, 4, L, dtype=np.uint8)) % 4
            pieces.append(new)
            p = q + L
            longs = [a[q - K:q + L + K], np.concatenate([a[q - K:q], new, a[q + L:q + L + K]])]
            short = None
        elif kind == "ins":
            new = _differs(rng, (a[q], a[q - 1]), L)
            pieces.append(new)
            p = q
            longs = [np.concatenate([a[q - K:q], new, a[q:q + K]])]
            short = a[q - K:q + K]
        else:
            # the deleted stretch must not extend a flank either: a[q] != a[q + L] and a[q + L - 1] != a[q - 1]
            if a[q] == a[q + L]:
                a[q] = (a[q] + 1) % 4
            if a[q + L - 1] == a[q - 1]:
                a[q + L - 1] = (a[q + L - 1] + 1) % 4
            p = q + L
            longs = [a[q - K:q + L + K]]
            short = np.concatenate([a[q - K:q], a[q + L:q + L + K]])
        where.append((kind, L, q))
        if marks:
            decoys.append((kind, longs, short))
    pieces.append(a[p:])
    b = np.concatenate(pieces)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s0, s1 = acgt[a].tobytes(), acgt[b].tobytes()
    seqs = [s0, _rc(s1) if reverse else s1]
    if marks:
        seqs.append(acgt[_decoys(rng, decoys, D)].tobytes())
    return seqs, where


def _decoys(rng, regions, D):
    """One record of decoys: windows of K + 1 bases cut out of the branches and of their K-flanks, every third base, each between
    random bases.  The two K-mers of a window occur once more in the graph with another neighbour on either side, so both become
    bifurcations: marks to erase and to restore in the flanks, marks to copy along the source branch -- in every chunk, and more than
    64 of them per collapse on the long branches (test_planted_with_marks counts them).  Windows are dealt out site after site, and
    two windows of one site are kept more than D + 2 K bases apart: a decoy never leads from one window into the next within D steps,
    so the decoys add marks and no bulges of their own.  The source of a collapse is the branch with the larger multiplicity: at an
    insertion only the long branch gets decoys, at a deletion the short one gets each of its windows twice, so the long branch is
    the source of the one and the target of the other."""
    per_site = []
    for kind, longs, short in regions:
        ws = [r[o:o + K + 1] for r in longs for o in range(0, len(r) - K, 3)]
        if short is not None and kind == "del":
            ws += [short[o:o + K + 1] for o in range(0, len(short) - K, 3)] * 2
        per_site.append(ws)
    out, n, last = [], 0, [None] * len(per_site)
    for i in range(max(len(ws) for ws in per_site)):
        for s, ws in enumerate(per_site):
            if i >= len(ws):
                continue
            gap = 40 if last[s] is None else max(40, last[s] + D + 2 * K + 40 - n)
            out += [rng.integers(0, 4, gap, dtype=np.uint8), ws[i]]
            n += gap + K + 1
            last[s] = n
    out.append(rng.integers(0, 4, 40, dtype=np.uint8))
    return np.concatenate(out)


def _oracle(seqs, D=D):
    from oracle.oracle import Oracle
    orc = Oracle(seqs)
    try:
        _, pos, _ = orc.enumerate(K)
        marks = np.stack([pos["chr"], pos["pos"]], 1).astype(np.int64)
        n = orc.simplify_stage(K, D, 4)
        so, po = orc.state()
        return n, so, [np.array(p) for p in po], marks
    finally:
        orc.close()


def _hist():
    from sibelia_amd import load_library
    lib = load_library()
    lib.sbl_collapse_hist.argtypes = [C.c_void_p]
    lib.sbl_collapse_hist.restype = None
    h = np.zeros((4, 3, 256), dtype=np.uint32)
    lib.sbl_collapse_hist(C.c_void_p(h.ctypes.data))
    return h


def _gpu(seqs, window, D):
    from sibelia_amd import BlockFinder
    bf = BlockFinder(seqs, device=0)
    try:
        if window:
            bf.set_window(window)
        n = bf.simplify_stage(K, D, 4)
        seq, pos = bf.state()
        st = bf.stats()
        return n, seq, pos, int(st["rounds"]), int(st["chain_transactions"])
    finally:
        bf.close()


def _check(monkeypatch, seqs, ref, what, window=0, D=D):
    """plain run and timed run against the oracle; the timed run's collapses [form][relation][span].  No transaction may have gone
    through the serial chain (k_chain keeps one chunk): what the counts say is then what k_commit did."""
    monkeypatch.setenv("SBL_NO_DENSE_PATH", "1")
    hist = None
    for phases in (None, "1"):
        if phases is None:
            monkeypatch.delenv("SBL_PHASES", raising=False)
        else:
            monkeypatch.setenv("SBL_PHASES", phases)
        n, seq, pos, rounds, chained = _gpu(seqs, window, D)
        tag = "%s, %s" % (what, "SBL_PHASES=" + phases if phases else "plain")
        assert rounds > 0, "no ordered rounds: the case never reached k_commit (%s)" % tag
        assert chained == 0, "%d transactions went through the serial chain: %s" % (chained, tag)
        assert n == ref[0], "bulges differ (%d, oracle %d): %s" % (n, ref[0], tag)
        assert seq == ref[1] and all(np.array_equal(p, q) for p, q in zip(pos, ref[2])), "state differs: " + tag
        if phases:
            hist = _hist()
    counted = int(hist.sum())
    print("%s: %d bulges, collapses by form %s" % (what, ref[0], {FORM[f]: int(hist[f].sum()) for f in range(4)}))
    for f in range(4):
        for r in range(3):
            sp = np.nonzero(hist[f][r])[0]
            if len(sp):
                print("  %-18s %-8s spans %s" % (FORM[f], REL[r], ", ".join("%d x%d" % (s, hist[f][r][s]) for s in sp)))
    assert counted >= ref[0], "%d collapses counted (a replayed round counts its collapses again), %d bulges: %s" % (counted, ref[0], what)
    for f in range(4):
        lo, hi = ((0, 64), (65, 128), (129, 192), (193, 255))[f]
        assert hist[f][:, :lo].sum() == 0 and hist[f][:, hi + 1:].sum() == 0, "%s took spans outside %d .. %d: %s" % (FORM[f], lo, hi, what)
    return hist


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse-complemented"])
def test_planted_edges(monkeypatch, reverse):
    """every edge span, as a substitution, an insertion and a deletion; the second strain as it is (source and target on one strand)
    and reverse-complemented (on opposite strands)"""
    seqs, _ = _planted(11, reverse=reverse)
    ref = _oracle(seqs)
    hist = _check(monkeypatch, seqs, ref, "planted, second strain %s" % ("reverse-complemented" if reverse else "forward"))
    for span in EDGES:
        f = _form_of(span)
        got = [int(hist[f][r][span]) for r in range(3)]
        if not reverse:
            # instance order decides the source at a tie: the first strain's branch, longer at the deletion, shorter at the insertion
            assert min(got) >= 1, "span %d through %s: %s collapses with %s" % (span, FORM[f], got, REL)
        else:
            # ... which on opposite strands goes either way from site to site: both indels at this span, in whichever direction
            assert got[0] >= 1 and got[1] + got[2] >= 2, "span %d through %s: %s collapses with %s" % (span, FORM[f], got, REL)
    for f in (0, 1, 2):
        got = [int(hist[f][r].sum()) for r in range(3)]
        assert min(got) >= 1, "%s: %s collapses with %s" % (FORM[f], got, REL)
    assert hist[:, :, D + K + 1:].sum() == 0, "a collapse beyond the largest span D allows"


def test_planted_beyond_three_chunks(monkeypatch):
    """D = 200: spans 190 .. 194 around the last chunk's edge and 223 .. 227 around the largest span (D + K = 225); from 193 on k_commit
    takes the older form"""
    d = 200
    edges = (191, 192, 193, d + K)
    seqs, _ = _planted(14, spans=tuple(range(190, 195)) + tuple(range(d + K - 2, d + K + 3)), D=d)
    ref = _oracle(seqs, d)
    hist = _check(monkeypatch, seqs, ref, "planted, D = 200", D=d)
    for span in edges:
        f = _form_of(span)
        got = [int(hist[f][r][span]) for r in range(3)]
        assert min(got) >= 1, "span %d through %s: %s collapses with %s" % (span, FORM[f], got, REL)
    assert hist[:, :, d + K + 1:].sum() == 0, "a collapse beyond the largest span D allows"


def test_planted_with_marks(monkeypatch):
    """the same sites with bifurcations inside both branches and in the K-flanks (_decoys).  The decoys' own instances add collapses
    of their own, so the check is per form and relation, not per span.  One long-branch site must carry more than 64 bifurcations
    over the branch and its flanks as the graph stands before the stage (counted here from the oracle's enumeration, forward strand
    of the first strain only): its collapse restores and copies more marks than one chunk of AddPoints holds (nlb + nlf + nact > 64)."""
    seqs, where = _planted(12, spans=EDGES, marks=True)
    ref = _oracle(seqs)
    marks = ref[3]
    most = 0
    for kind, L, q in where:
        if L + 2 * K + 1 > D + K:
            continue
        m = marks[(marks[:, 0] == 0) & (marks[:, 1] >= q - K) & (marks[:, 1] <= q + (L if kind != "ins" else 0) + K)]
        most = max(most, len(m))
    assert most > 64, "at most %d bifurcations over a branch and its flanks: no collapse restores and copies more than 64 marks" % most
    # (the decoy record ties the sites' neighbourhoods together, and a driver that sees eight blocked entries beside two commits turns
    # to the serial chain: a window of six entries never shows it eight)
    hist = _check(monkeypatch, seqs, ref, "planted with decoys", window=6)
    for f in (0, 1, 2):
        for r in range(3):
            got = int(hist[f][r].sum())
            assert got >= 1, "%d collapses with %s through %s" % (got, REL[r], FORM[f])


def test_mixed_strains(monkeypatch):
    """three strains x 30 kbp of workloads.gen_strains at 6 % SNPs: neighbouring SNPs chain into branches of every length"""
    from sibelia_amd import workloads as W
    seqs = W.gen_strains(L0=30_000, n=3, seed=5, snp=0.06, inv_min=1000, inv_max=3000)
    ref = _oracle(seqs)
    hist = _check(monkeypatch, seqs, ref, "gen_strains 3 x 30 kbp, 6 % SNPs")
    for f in (0, 1, 2):
        got = int(hist[f].sum())
        assert got >= 1, "%d collapses through %s" % (got, FORM[f])
