"""A plain numpy restatement of the block alignment with a gap opening cost (include/sibelia_amd.h), for the tests (never
used by the product).  It stands next to tests/galign_model.py, whose scores, `runs`, `rows`, `bound` and `variants` it shares.

`align(a, b, o)`              the full, unbanded matrices H / E / F and their trace -> (score, steps); steps is a string over 'M', 'I'
                              and 'D' as in galign_model.
`align_banded(a, b, o, w)`    the same inside the band lo - w <= j - i <= hi + w -> (score, steps, ok); ok: the certificate holds.
`align_doubling(a, b, o, w0)` w0, 2 w0, ... until the certificate holds -> (score, steps, w, passes).
`score_of_rows(row_a, row_b, o)`  the two gapped rows scored again: +25 / -75 per aligned column, o + 75 L per maximal gap run of
                              one row (a gap run of row a directly followed by one of row b is two runs).
`gap_runs(a, b, steps)`       the number of 'I' / 'D' runs of a trace.
`pair(c, s, o)`, `msa(group, o)`  the centre-star merge of tests/msa_model.py over these pairs.
`pair_banded(c, s, o)`        (score, steps) from band storage only, w = 64, 128, ... until the certificate holds: for instances of
                              thousands of bases.

A gap run of L columns costs o + 75 L.  The matrices are filled from the ends, by anti-diagonals:
  H[n][m] = 0
  E[i][j] = max(E[i+1][j] - 75, H[i+1][j] - o - 75)      i < n   (a[i] over '-')
  F[i][j] = max(F[i][j+1] - 75, H[i][j+1] - o - 75)      j < m   ('-' over b[j])
  H[i][j] = max(H[i+1][j+1] + (a[i] == b[j] ? 25 : -75), E[i][j], F[i][j])
absent terms minus infinity.  The trace runs from (0, 0) in state H: the diagonal step if it attains H, else state E if E attains it,
else state F; state E at (i, j) emits 'I' and closes (back to H at (i + 1, j)) if H[i+1][j] - o - 75 == E[i][j], else stays; F likewise.
"""
import numpy as np

import galign_model as GM
import msa_model as MM

MATCH, PENALTY, NEG = GM.MATCH, GM.PENALTY, GM.NEG
MAX_OPEN = 100000


def _fill(a: bytes, b: bytes, o: int, lo_off=None, hi_off=None):
    """H, E, F as (n + 1) x (m + 1) int64 arrays; cells with j - i outside [lo_off, hi_off] are NEG in all three."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, dtype=np.uint8)
    B = np.frombuffer(b, dtype=np.uint8)
    H = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    E = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    F = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    H[n, :m] = F[n, :m] = -o - PENALTY * (m - np.arange(m))
    H[:n, m] = E[:n, m] = -o - PENALTY * (n - np.arange(n))
    H[n, m] = 0
    inside = None
    if lo_off is not None:
        off = np.arange(m + 1)[None, :] - np.arange(n + 1)[:, None]
        inside = (off >= lo_off) & (off <= hi_off)
        for X in (H, E, F):
            X[~inside] = NEG
    for d in range(n + m - 2, -1, -1):                     # anti-diagonals: every cell of one depends on the two behind it only
        i = np.arange(max(0, d - (m - 1)), min(n - 1, d) + 1)
        j = d - i
        e = np.maximum(E[i + 1, j] - PENALTY, H[i + 1, j] - o - PENALTY)
        f = np.maximum(F[i, j + 1] - PENALTY, H[i, j + 1] - o - PENALTY)
        h = np.maximum(H[i + 1, j + 1] + np.where(A[i] == B[j], MATCH, -PENALTY), np.maximum(e, f))
        keep = True if inside is None else inside[i, j]
        H[i, j] = np.where(keep, np.maximum(h, NEG), NEG)
        E[i, j] = np.where(keep, np.maximum(e, NEG), NEG)
        F[i, j] = np.where(keep, np.maximum(f, NEG), NEG)
    return H, E, F


def _trace(a: bytes, b: bytes, o: int, H, E, F) -> str:
    """H, E, F: functions (i, j) -> value"""
    n, m = len(a), len(b)
    i = j = 0
    state = "H"
    out = []
    while i < n or j < m:
        if state == "H":
            if i < n and j < m and H(i + 1, j + 1) + (MATCH if a[i] == b[j] else -PENALTY) == H(i, j):
                out.append("M"); i += 1; j += 1
            elif i < n and E(i, j) == H(i, j):
                state = "E"
            else:
                assert j < m and F(i, j) == H(i, j)
                state = "F"
        elif state == "E":
            out.append("I")
            if H(i + 1, j) - o - PENALTY == E(i, j):
                state = "H"
            else:
                assert E(i + 1, j) - PENALTY == E(i, j)
            i += 1
        else:
            out.append("D")
            if H(i, j + 1) - o - PENALTY == F(i, j):
                state = "H"
            else:
                assert F(i, j + 1) - PENALTY == F(i, j)
            j += 1
    assert state == "H"
    return "".join(out)


def _of(X):
    return lambda i, j: int(X[i, j])


def align(a: bytes, b: bytes, o: int):
    assert 0 <= o <= MAX_OPEN
    H, E, F = _fill(a, b, o)
    return int(H[0, 0]), _trace(a, b, o, _of(H), _of(E), _of(F))


bound = GM.bound                                           # U(w) is the one of the linear cost: o >= 0 only lowers a path that leaves the band


def align_banded(a: bytes, b: bytes, o: int, w: int):
    n, m = len(a), len(b)
    lo, hi = min(0, m - n), max(0, m - n)
    H, E, F = _fill(a, b, o, lo - w, hi + w)
    score = int(H[0, 0])
    ok = w >= min(n, m) or score > bound(n, m, w)
    return score, (_trace(a, b, o, _of(H), _of(E), _of(F)) if ok else None), ok      # the trace of a band that cut the optimum is not defined


def align_doubling(a: bytes, b: bytes, o: int, w0: int):
    w, passes = w0, 0
    while True:
        w = min(w, min(len(a), len(b)))
        score, steps, ok = align_banded(a, b, o, w)
        passes += 1
        if ok:
            return score, steps, w, passes
        w *= 2


def _band_only(a: bytes, b: bytes, o: int, w: int):
    """align_banded with the band as the only storage, like msa_model._banded: X[i, j - i - omin + 1], one column of minus infinity
    either side -> (score, steps or None, ok).  For instances of thousands of bases, where the full matrices do not fit."""
    n, m = len(a), len(b)
    omin, omax = min(0, m - n) - w, max(0, m - n) + w
    W = omax - omin + 1
    A, B = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    TH, TE, TF = (np.full((n + 2, W + 2), NEG, dtype=np.int64) for _ in range(3))
    for d in range(n + m, -1, -1):
        i_lo, i_hi = max(0, d - m, -((omax - d) // 2)), min(n, d, (d - omin) // 2)
        if i_lo > i_hi:
            continue
        i = np.arange(i_lo, i_hi + 1)
        j = d - i
        k = j - i - omin + 1
        e = np.maximum(TE[i + 1, k - 1] - PENALTY, TH[i + 1, k - 1] - o - PENALTY)
        f = np.maximum(TF[i, k + 1] - PENALTY, TH[i, k + 1] - o - PENALTY)
        sub = np.where(A[np.minimum(i, n - 1)] == B[np.minimum(j, m - 1)], MATCH, -PENALTY)
        h = np.maximum(TH[i + 1, k] + sub, np.maximum(e, f))
        rest = (n - i) + (m - j)
        border, gap = (i == n) | (j == m), np.where(rest > 0, -o - PENALTY * rest, 0)
        TH[i, k] = np.where(border, gap, np.maximum(h, NEG))
        TE[i, k] = np.where(border, np.where(i < n, gap, NEG), np.maximum(e, NEG))
        TF[i, k] = np.where(border, np.where(j < m, gap, NEG), np.maximum(f, NEG))

    def of(T):
        def get(i, j):
            k = j - i - omin
            return int(T[i, k + 1]) if 0 <= k < W else NEG
        return get
    score = of(TH)(0, 0)
    ok = w >= min(n, m) or score > bound(n, m, w)
    return score, (_trace(a, b, o, of(TH), of(TE), of(TF)) if ok else None), ok


def pair_banded(c: bytes, s: bytes, o: int, w0: int = 64):
    """(score, steps) from band storage only, w = w0, 2 w0, ... until the certificate holds"""
    if not c or not s:
        return align(c, s, o)
    w = w0
    while True:
        w = min(w, len(c), len(s))
        score, steps, ok = _band_only(c, s, o, w)
        if ok:
            return score, steps
        w *= 2


def gap_runs(a: bytes, b: bytes, steps: str) -> int:
    return sum(1 for op, _ in GM.runs(a, b, steps) if op in "ID")


def score_of_rows(row_a: bytes, row_b: bytes, o: int) -> int:
    total, last = 0, None                                  # last: which row held the gap in the column before
    for x, y in zip(row_a, row_b):
        assert x != 45 or y != 45
        now = "a" if x == 45 else "b" if y == 45 else None
        if now is None:
            total += MATCH if x == y else -PENALTY
        else:
            total -= PENALTY + (o if now != last else 0)
        last = now
    return total


def pair(c: bytes, s: bytes, o: int):
    score, steps = align(c, s, o)
    return score, GM.runs(c, s, steps)


def msa(group, o: int):
    """msa_model.msa with every member aligned to the centre under the opening cost o: the merge itself does not change."""
    return MM.msa(group, pair_fn=lambda c, s: pair(c, s, o))
