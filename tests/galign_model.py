"""A plain numpy restatement of the block alignment (include/sibelia_amd.h), for the tests (never used by the product).

`align(a, b)`            the full, unbanded matrix and its trace -> (score, steps); steps is a string over 'M' (diagonal), 'I' (a[i]
                         over '-') and 'D' ('-' over b[j]).
`align_banded(a, b, w)`  the same inside the band lo - w <= j - i <= hi + w, everything outside it minus infinity -> (score, steps, ok);
                         ok: the certificate holds (score > U(w), or the band covers the matrix).
`align_doubling(a, b, w0)`  w0, 2 w0, ... until the certificate holds -> (score, steps, w, passes).
`runs(a, b, steps)`, `rows(a, b, steps)`  the run list [(op, length)], op in '=XID', and the two gapped rows.
`variants(row_a, row_b, start, end, reverse)`  the variant rules of C-Sibelia.py's parse_alignment (reference
                         src/csibelia/C-Sibelia.py:206-252), column by column as the reference does it -> [(POS, REF, ALT)].
`maf_fields(start, end, reverse, record_size)`  start / size / strand / record size of an `s` line (write_alignments_maf, :473-484).

Scores: match +25, mismatch -75, gap column -75.  The matrix is filled from the ends, S[i][j] = best score of aligning a[i:] with b[j:];
the trace runs forward from (0, 0) and prefers the diagonal step, then the i step, then the j step.
"""
import numpy as np

MATCH, PENALTY = 25, 75
NEG = -(1 << 40)
MINIMUM_CONTEXT_SIZE = 30


def _fill(a: bytes, b: bytes, lo_off=None, hi_off=None):
    """S as an (n + 1) x (m + 1) int64 array; cells with j - i outside [lo_off, hi_off] are NEG."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, dtype=np.uint8)
    B = np.frombuffer(b, dtype=np.uint8)
    S = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    inside = np.ones((n + 1, m + 1), dtype=bool)
    if lo_off is not None:
        off = np.arange(m + 1)[None, :] - np.arange(n + 1)[:, None]
        inside = (off >= lo_off) & (off <= hi_off)
    S[n, :] = -PENALTY * (m - np.arange(m + 1))
    S[:, m] = -PENALTY * (n - np.arange(n + 1))
    S[~inside] = NEG
    for d in range(n + m - 2, -1, -1):                     # anti-diagonals: every cell of one depends on the two behind it only
        i = np.arange(max(0, d - (m - 1)), min(n - 1, d) + 1)
        j = d - i
        sub = np.where(A[i] == B[j], MATCH, -PENALTY)
        v = np.maximum(S[i + 1, j + 1] + sub, np.maximum(S[i + 1, j], S[i, j + 1]) - PENALTY)
        S[i, j] = np.where(inside[i, j], np.maximum(v, NEG), NEG)
    return S


def _trace(a: bytes, b: bytes, S) -> str:
    n, m = len(a), len(b)
    i = j = 0
    out = []
    while i < n or j < m:
        if i == n:
            out.append("D"); j += 1
        elif j == m:
            out.append("I"); i += 1
        else:
            best = S[i, j]
            if S[i + 1, j + 1] + (MATCH if a[i] == b[j] else -PENALTY) == best:
                out.append("M"); i += 1; j += 1
            elif S[i + 1, j] - PENALTY == best:
                out.append("I"); i += 1
            else:
                assert S[i, j + 1] - PENALTY == best
                out.append("D"); j += 1
    return "".join(out)


def align(a: bytes, b: bytes):
    S = _fill(a, b)
    return int(S[0, 0]), _trace(a, b, S)


def bound(n: int, m: int, w: int) -> int:
    """U(w): no path that leaves the band scores more."""
    return MATCH * (min(n, m) - (w + 1)) - PENALTY * (abs(m - n) + 2 * (w + 1))


def align_banded(a: bytes, b: bytes, w: int):
    n, m = len(a), len(b)
    lo, hi = min(0, m - n), max(0, m - n)
    S = _fill(a, b, lo - w, hi + w)
    score = int(S[0, 0])
    return score, _trace(a, b, S), (w >= min(n, m) or score > bound(n, m, w))


def align_doubling(a: bytes, b: bytes, w0: int):
    w, passes = w0, 0
    while True:
        w = min(w, min(len(a), len(b)))
        score, steps, ok = align_banded(a, b, w)
        passes += 1
        if ok:
            return score, steps, w, passes
        w *= 2


def required_w(a: bytes, b: bytes, w0: int = 64) -> int:
    return align_doubling(a, b, w0)[2]


def runs(a: bytes, b: bytes, steps: str):
    out, i, j = [], 0, 0
    for s in steps:
        op = ("=" if a[i] == b[j] else "X") if s == "M" else s
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
        i += s != "D"
        j += s != "I"
    return [(op, n) for op, n in out]


def rows(a: bytes, b: bytes, steps: str):
    ra, rb, i, j = bytearray(), bytearray(), 0, 0
    for s in steps:
        ra.append(a[i] if s != "D" else 45)
        rb.append(b[j] if s != "I" else 45)
        i += s != "D"
        j += s != "I"
    return bytes(ra), bytes(rb)


def score_of_rows(row_a: bytes, row_b: bytes) -> int:
    return sum(MATCH if x == y else -PENALTY for x, y in zip(row_a, row_b))


_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def variants(row_a: bytes, row_b: bytes, start: int, end: int, reverse: bool):
    """parse_alignment on the two rows; [start, end): the reference-side instance, 0-based half-open -- the reference program reports it
    as start + 1 .. end, from the far end (`end`) for a '-' instance."""
    segment, last, at = [], None, None
    for now, (x, y) in enumerate(zip(row_a, row_b)):
        match = x == y
        if last is None:
            last, at = match, 0
        elif last != match:
            if last is False or now - at >= MINIMUM_CONTEXT_SIZE or at == 0:
                segment.append([at, now, last])
                at = now
            elif segment:
                at = segment[-1][0]
                del segment[-1]
            last = match
    if last is None:
        return []
    segment.append([at, len(row_a), last])
    position, step, pos_map = (end, -1, []) if reverse else (start + 1, 1, [])
    for x in row_a:
        pos_map.append(position)
        position += step if x != 45 else 0
    out = []
    for s, e, match in segment:
        if match:
            continue
        snp = e - s == 1 and row_a[s] != 45 and row_b[s] != 45
        shift = 0 if s == 0 or snp else 1
        ref = bytes(x for x in row_a[s - shift:e] if x != 45)
        alt = bytes(x for x in row_b[s - shift:e] if x != 45)
        if reverse:
            ref, alt = ref.translate(_COMPLEMENT)[::-1], alt.translate(_COMPLEMENT)[::-1]
        out.append((pos_map[s] - shift, ref, alt))
    return out


def maf_fields(start: int, end: int, reverse: bool, record_size: int):
    """(start, size, strand, record size) of the `s` line of the instance [start, end): the reference computes min(start, end) - 1 from
    its 1-based inclusive coordinates, and record size - max(start, end) for '-'."""
    return (record_size - end if reverse else start), end - start, "-" if reverse else "+", record_size
