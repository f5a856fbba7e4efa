"""tests/gmask_model.py, the plain restatement of the SNP-density mask, against intervals and masked rows written out by
hand, against the brute force over all pairs of differences of a row, and the invariants of the definition; and the preconditions of the
crafted groups of tests/gmask_cases.py: the rows msa_model.msa makes of them have the shape each case intends."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmask_cases as KC                           # noqa: E402
import gmask_model as KM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
import msa_model as MM                             # noqa: E402


def brute(diffs, W, T):
    """every pair a < b of differences with at least T + 1 differences in [a, b] and p[b] - p[a] < W links a .. b; the intervals are the
    maximal chains of linked differences"""
    n = len(diffs)
    link = [False] * max(0, n - 1)                             # link[i]: differences i and i + 1 lie in one hull
    for a in range(n):
        for b in range(a + T, n):
            if diffs[b][1] - diffs[a][1] < W:
                for i in range(a, b):
                    link[i] = True
    out, i = [], 0
    while i < n - 1:
        if not link[i]:
            i += 1
            continue
        j = i
        while j < n - 1 and link[j]:
            j += 1
        out.append((diffs[i][0], diffs[j][0], diffs[i][1], diffs[j][1], j - i + 1))
        i = j
    return out


def check_invariants(groups, W, T, want=None):
    intervals, masked = KM.mask(groups, W, T, want)
    assert intervals == sorted(intervals)
    for (g, i, first, last, bf, bl, nd), nxt in zip(intervals, intervals[1:] + [None]):
        cols = [x for x, _ in KM.differences(groups[g], i)]
        assert nd >= T + 1 and first in cols and last in cols and nd == sum(first <= x <= last for x in cols)
        assert bf == first - groups[g][0][:first].count(b"-") and bl == last - groups[g][0][:last].count(b"-")
        if nxt is not None and nxt[:2] == (g, i):
            assert last < nxt[2]
    for rows, out in zip(groups, masked):
        if isinstance(rows, int):
            assert out == rows
            continue
        assert out[0] == rows[0]
        for a, b in zip(rows, out):
            assert len(a) == len(b) and [x == 45 for x in a] == [x == 45 for x in b]
            assert all(x == y or y == KM.N for x, y in zip(a, b))
    for g, rows in enumerate(groups):
        if not isinstance(rows, int) and g in KM.used(groups, want):
            for i in range(1, len(rows)):
                assert [iv[2:] for iv in intervals if iv[:2] == (g, i)] == brute(KM.differences(rows, i), W, T)
    return intervals, masked


def test_by_hand():
    rows = [b"AC--GTACGTAC", b"AG--CTAtGNTC", b"ACTTGTACGTAC"]
    #          0123456789ab       columns 1, 4 and 10 of row 1 are differences (before 1, 2, 8); t, N are none
    assert KM.differences(rows, 1) == [(1, 1), (4, 2), (10, 8)] and KM.differences(rows, 2) == []
    assert KM.mask([rows], 2, 1) == ([(0, 1, 1, 4, 1, 2, 2)], [[rows[0], b"AN--NTAtGNTC", rows[2]]])
    assert KM.mask([rows], 8, 2) == ([(0, 1, 1, 10, 1, 8, 3)], [[rows[0], b"AN--NNNNNNNC", rows[2]]])
    assert KM.mask([rows], 7, 2) == ([], [rows])
    assert KM.mask([rows, 3, [b"ACGT"], [b"", b""]], 2, 1, [False, True, True, True]) == ([], [rows, 3, [b"ACGT"], [b"", b""]])
    gapped = [b"ACGTACGT", b"T-G-TCGT"]                        # a deletion inside an interval stays '-'
    assert KM.mask([gapped], 5, 1) == ([(0, 1, 0, 4, 0, 4, 2)], [[gapped[0], b"N-N-NCGT"]])
    for W, T in ((0, 1), (1, 0), (2 ** 32, 1), (1, 2 ** 32)):
        with pytest.raises(KM.Refused):
            KM.mask([rows], W, T)


@pytest.mark.parametrize("name", sorted(KC.CASES))
def test_crafted_cases(name):
    c = KC.CASES[name]
    rows = KC.rows_of(c)
    intervals, masked = check_invariants(rows, c["W"], c["T"])
    assert intervals == KC.BY_HAND.get(name, intervals)
    if name == "neighbouring_runs":
        assert masked[0][1][13:18] == rows[0][1][13:18] and masked[0][1][10:13] == b"NNN"
    if name == "column_edges":
        assert [len(r[0]) for r in rows] == list(KC.L_EDGES) and len(intervals) == 1 + 2 * (len(KC.L_EDGES) - 2)
    if name == "codes_inside":
        assert masked[0][1][20:30] == b"N" * 10 and masked[0][2] == rows[0][2]


def test_preconditions_of_the_crafted_cases():
    """what the alignment makes of the strings: substitution-only members align as the identity, a planted insertion stays one gap slot, a planted deletion one gap run"""
    for name, c in sorted(KC.CASES.items()):
        if c["identity"]:
            for g in c["groups"]:
                assert len({len(s) for s in g}) == 1
                assert MM.msa(g, MM.pair_banded)[0] == g, name
    rows = KC.rows_of(KC.CASES["insertion_inside"])[0]
    assert len(rows[0]) == 300 and rows[0].count(b"-") == 100 and b"-" * 100 in rows[0] and rows[2].count(b"-") == 100 and b"-" not in rows[1]
    assert [x for x, _ in KM.differences(rows, 1)] == [50, 52, 160] == [x for x, _ in KM.differences(rows, 2)]
    assert 52 < rows[0].index(b"-") <= 60
    rows = KC.rows_of(KC.CASES["deletion_inside"])[0]
    assert len(rows[0]) == 200 and b"-" not in rows[0] and rows[1].count(b"-") == 3 and b"---" in rows[1][50:61]
    assert [x for x, _ in KM.differences(rows, 1)] == [50, 52, 60]
    assert KM.mask([rows], 12, 2)[1][0][1][50:61].count(b"-") == 3


def test_random_groups_against_the_brute_force():
    seen = 0
    groups = [MM.msa(g)[0] for g in MC.random_groups(77, 200, 1, 5, 120, 6)]
    for W, T in ((20, 2), (50, 4), (8, 1)):
        intervals, masked = check_invariants(groups, W, T)
        seen += len(intervals)
    assert seen > 50
    rng = np.random.default_rng(78)
    want = [bool(x) for x in rng.integers(0, 2, len(groups))]
    intervals, masked = check_invariants(groups, 20, 2, want)
    assert {g for g, *_ in intervals} <= {g for g, w in enumerate(want) if w}
    assert all(m == r for m, r, w in zip(masked, groups, want) if not w)
