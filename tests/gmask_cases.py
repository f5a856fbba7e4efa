"""Crafted groups for the SNP-density mask, shared by tests/test_gmask_model.py and tests/test_gpu_group_mask.py.

CASES: name -> {"groups": groups of strings (centre first), "W", "T", "identity": the members differ from the centre by substitutions
only and the alignment is the identity, so the rows are the strings themselves}.  BY_HAND: name -> the intervals written out by hand.
`rows_of(case)`: the rows of a case's groups: the strings, or the model's alignment of them.
"""
import numpy as np

import msa_cases as MC
import msa_model as MM


def other(base: int, step: int = 1) -> int:
    return b"ACGT"[(b"ACGT".index(base) + step) % 4]


def subst(c: bytes, at, put=None) -> bytes:
    """c with another base at every index of `at`; put: {index: byte} written as given"""
    b = bytearray(c)
    for x in at:                                               # a base that the centre does not hold there or next to it: a shift by one gains nothing
        b[x] = next(y for y in b"ACGT" if y not in c[max(0, x - 1):x + 2])
    for x, ch in (put or {}).items():
        b[x] = ch
    return bytes(b)


def _centre(seed, n):
    return MC.rand(np.random.default_rng(seed), n)


def _edges(L):
    """a group of three rows of L columns for W = 4, T = 1: row 1 has a dense pair at either end, row 2 two lone differences"""
    c = _centre(300 + L, L)
    if L < 5:
        return [c, subst(c, [0]), c]
    return [c, subst(c, sorted({0, 2, L - 3, L - 1})), subst(c, [0, L - 1])]


def _case(groups, W, T, identity=True, revs=None):
    return {"groups": groups, "W": W, "T": T, "identity": identity, "revs": revs}


C64, C200, C40 = _centre(1, 64), _centre(2, 200), _centre(3, 40)
INSERT = bytes([next(x for x in b"ACGT" if x not in (C200[55], C200[56]))]) * 100      # no base of it can stand under a centre base next to it
L_EDGES = (1, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)

CASES = {
    # 3 differences over exactly 10 centre bases (row 1: masked) and over 11 (row 2: not)
    "exact_span": _case([[C64, subst(C64, [20, 25, 29]), subst(C64, [20, 25, 30])]], 10, 2),
    "window_of_one": _case([[C64, subst(C64, [20, 21, 40, 41])]], 1, 1),
    # every k = 0 .. 3 is a start: one interval
    "chain_of_starts": _case([[C64, subst(C64, [10, 12, 14, 16, 18, 20])]], 6, 2),
    # T = 3: starts 0 and 2 (18 - 10 = 8, 26 - 17 = 9), 1 is none (21 - 11 = 10): they share differences 2 and 3
    "starts_two_apart": _case([[C64, subst(C64, [10, 11, 17, 18, 21, 26])]], 10, 3),
    # starts 0 and 3 = 0 + T + 1: two intervals, columns 13 .. 17 stay
    "neighbouring_runs": _case([[C64, subst(C64, [10, 11, 12, 18, 19, 20])]], 6, 2),
    # 100 bases inserted behind centre base 55, between the differences at 52 and 60: the distance is 10 centre bases; row 2 has the
    # same differences and no insertion
    "insertion_inside": _case([[C200, subst(C200, [50, 52, 60])[:56] + INSERT + subst(C200, [50, 52, 60])[56:], subst(C200, [50, 52, 60])]], 12, 2, identity=False),
    "deletion_inside": _case([[C200, subst(C200, [50, 52, 60])[:54] + subst(C200, [50, 52, 60])[57:]]], 12, 2, identity=False),
    # N, R and a lower-case base inside an interval; in row 2 the third difference is an N: no interval
    "codes_inside": _case([[C64, subst(C64, [20, 22, 29], {23: ord("N"), 25: ord("R"), 27: C64[27] | 32}), subst(C64, [20, 22], {29: ord("N")})]], 12, 2),
    # T differences at the end of row 1, one at the start of row 2 with a larger centre index
    "rows_not_linked": _case([[C40, subst(C40, [36, 38]), subst(C40, [39])]], 50, 2),
    "groups_not_linked": _case([[C40, subst(C40, [36, 38])], [C40, subst(C40, [39])]], 50, 2),
    "column_edges": _case([_edges(L) for L in L_EDGES], 4, 1),
    # rows of 5 columns, an interval in each of three consecutive rows: several intervals in one 16-byte word
    "short_rows": _case([[C40[:5], subst(C40[:5], [0, 1]), subst(C40[:5], [2, 4]), subst(C40[:5], [1, 3])]], 5, 1),
    "row_end_and_row_start": _case([[C40[:20], subst(C40[:20], [17, 19]), subst(C40[:20], [0, 2])]], 4, 1),
    "whole_row": _case([[C40[:20], subst(C40[:20], [0, 19])]], 20, 1),
    # the first group of a call: row 1 starts at byte 48.  Bounds at byte 0, 15 and 16 of a word and on the last column
    "word_bounds": _case([[C64[:48], subst(C64[:48], [0, 1, 15, 16, 30, 31, 45, 47])]], 3, 1),
    # 700 differences, every fifth column; every k <= 399 is a start (1500 < 1510): more look-ahead than a workgroup has lanes
    "long_look_ahead": _case([[_centre(5, 3510), subst(_centre(5, 3510), range(0, 3500, 5))]], 1510, 300),
    "identical": _case([[C64, C64, C64]], 1000, 3),
    "no_run": _case([[C64, subst(C64, [5, 30, 60]), subst(C64, [10])]], 10, 1),
}

BY_HAND = {
    "exact_span": [(0, 1, 20, 29, 20, 29, 3)],
    "window_of_one": [],
    "chain_of_starts": [(0, 1, 10, 20, 10, 20, 6)],
    "starts_two_apart": [(0, 1, 10, 26, 10, 26, 6)],
    "neighbouring_runs": [(0, 1, 10, 12, 10, 12, 3), (0, 1, 18, 20, 18, 20, 3)],
    "insertion_inside": [(0, 1, 50, 160, 50, 60, 3), (0, 2, 50, 160, 50, 60, 3)],
    "deletion_inside": [(0, 1, 50, 60, 50, 60, 3)],
    "codes_inside": [(0, 1, 20, 29, 20, 29, 3)],
    "rows_not_linked": [],
    "groups_not_linked": [],
    "short_rows": [(0, 1, 0, 1, 0, 1, 2), (0, 2, 2, 4, 2, 4, 2), (0, 3, 1, 3, 1, 3, 2)],
    "row_end_and_row_start": [(0, 1, 17, 19, 17, 19, 2), (0, 2, 0, 2, 0, 2, 2)],
    "whole_row": [(0, 1, 0, 19, 0, 19, 2)],
    "word_bounds": [(0, 1, 0, 1, 0, 1, 2), (0, 1, 15, 16, 15, 16, 2), (0, 1, 30, 31, 30, 31, 2), (0, 1, 45, 47, 45, 47, 2)],
    "long_look_ahead": [(0, 1, 0, 3495, 0, 3495, 700)],
    "identical": [],
    "no_run": [],
}


def rows_of(case, pair_fn=MM.pair):
    return [list(g) if case["identity"] else MM.msa(g, pair_fn)[0] for g in case["groups"]]
