"""Cases that pin k_boundary_align (csrc/boundary_align.hip) at the edges of its 16-bit scores, of the 11-bit fields of its maximum key,
of its one-wave trace walk and of its code packing, shared by tests/test_boundary_cases.py (their preconditions, on the numpy model
alone) and tests/test_gpu_boundary_edges.py (the device).  The reference is tests/boundary_model.py: align, exactly.

Run cases     a run of 63 .. 129 matches -- what one ballot of the walk consumes, one less, one more, and the same around two -- that ends
              in a substitution, a gap in either string, a zero cell or the end of either string, or starts deep inside `a` (the ilo > 0
              half of the matrix); each with 0 .. 3 leading characters on `a`, so the start cell sits at every position of a code byte.
Score cases   identical strings whose score is just below 2^15, just above it and at the most a window can reach.
Key fields    start cells at i = 2046 and at j = 2046.
Far ties      equal maxima far apart: on different diagonals, on one diagonal, and in different waves of the workgroup either way round.
Turns         a mismatch on the trace whose two gap neighbours hold equal scores: only the order of the comparisons decides the step.
Sweeps        every shape up to 16 x 16 and 1000 random pairs over `AC`: dense in matches, so dense in equal scores.
Wide shapes   the four residues of min(n, m) mod 4 at the largest sizes, n < m, n = m and n > m.
Packing       shapes whose trace codes fill a multiple of 256 bytes exactly, or one byte more.

A case is (name, a, b, geometry): geometry is the (a_begin, a_end, b_begin, b_end) the construction fixes, or None.  The model results
are computed once per process and kept."""
import functools

import numpy as np

import boundary_model as BM

MAXLEN = 2047                  # SBL_ALIGN_MAX_LEN
CELLS, THREADS, ALIGN = 4, 512, 256      # BA_CELLS, BA_THREADS, BA_ALIGN of the kernel


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def other(ch, k=1):
    """a base that differs from the byte ch (k = 1, 2, 3: the three of them)"""
    return b"ACGT"[(b"ACGT".index(ch) + k) % 4:][:1]


def related(rng, n, m):
    """two strings that share a mutated stretch, so that the alignment has matches, mismatches and gaps (the recipe of
    tests/test_gpu_boundary_align.py)"""
    core = rand(rng, max(n, m))
    b = bytearray()
    for ch in core:
        u = rng.random()
        if u < 0.02:
            continue
        if u < 0.04:
            b += rand(rng, 1)
        b += rand(rng, 1) if rng.random() < 0.06 else bytes([ch])
    cut = int(rng.integers(0, 1 + len(core) // 8))
    return core[cut:cut + n].ljust(n, b"A")[:n], (rand(rng, int(rng.integers(0, 1 + m // 8))) + bytes(b)).ljust(m, b"C")[:m]


# ---- what the kernel's layout is checked against

def cells(d, n, m):
    return min(d, n - 1) - max(0, d - (m - 1)) + 1


def code_bytes(n, m):
    """bytes of trace codes of an n x m matrix, counted diagonal by diagonal: four cells to a byte, every diagonal a new byte"""
    total = 0
    for d in range(n + m - 1):
        total += (cells(d, n, m) + CELLS - 1) // CELLS
    return total


def rounded(n, m):
    """what one alignment takes of a launch's code buffer"""
    return (code_bytes(n, m) + ALIGN - 1) // ALIGN * ALIGN


def wave_of(i, j, n, m):
    """the wave of the workgroup that fills cell (i, j): lane q of a diagonal takes its cells 4 q .. 4 q + 3, counted from the lowest i"""
    q = (i - max(0, i + j - (m - 1))) // CELLS
    return q % THREADS // 64


def matrix(a, b):
    """the model's matrix by the model's own recurrence (boundary_model.align), skewed as there: K[i + j][i] = M[i][j]"""
    n, m = len(a), len(b)
    A = np.frombuffer(a, dtype=np.uint8)
    Brev = np.frombuffer(b, dtype=np.uint8)[::-1]
    K = np.zeros((n + m + 1, n + 1), dtype=np.int32)
    for d in range(n + m - 2, -1, -1):
        lo, hi = max(0, d - (m - 1)), min(n - 1, d)
        eq = A[lo:hi + 1] == Brev[m - 1 - d + lo:m - d + hi]
        v, h, g = K[d + 1, lo + 1:hi + 2], K[d + 1, lo:hi + 1], K[d + 2, lo + 1:hi + 2]
        K[d, lo:hi + 1] = np.where(eq, g + BM.MATCH, np.maximum(0, np.maximum(g, np.maximum(v, h)) - BM.PENALTY))
    return K


def max_score(a, b):
    return int(matrix(a, b).max()) if a and b else 0


def maxima(a, b):
    """the cells that hold the matrix maximum -> (maximum, [(i, j)])"""
    K = matrix(a, b)
    dd, ii = np.nonzero(K == K.max())
    return int(K.max()), sorted((int(i), int(d - i)) for d, i in zip(dd, ii))


def flat(x):
    (ab, ae), (bb, be) = x
    return ab, ae, bb, be


@functools.lru_cache(maxsize=None)
def model(family):
    """BM.align of every case of a family, as rows (a_begin, a_end, b_begin, b_end)"""
    return tuple(flat(BM.align(a, b)) for _, a, b, _ in FAMILIES[family]())


# ---- one run of matches for the trace walk

RUN_L = (63, 64, 65, 127, 128, 129)
ENDINGS = ("sub", "igap", "jgap", "stop", "enda", "endb", "deep")
SHIFTS = (0, 1, 2, 3)
TAIL, DEEP = 40, 301


@functools.lru_cache(maxsize=None)
def run_cases():
    """[(name, a, b, geometry)] for every L, ending and shift; the name is 'run-<ending>-<L>-<shift>'"""
    out = []
    for L in RUN_L:
        rng = np.random.default_rng(8100 + L)
        # (Y begins with neither of the two bases put in front of it, or the run would be one longer)
        X, Y, junk = rand(rng, L), rand(rng, 1, b"GT") + rand(rng, TAIL - 1), rand(rng, DEEP + max(SHIFTS))
        for ending in ENDINGS:
            a, b = {"sub": (X + b"A" + Y, X + b"C" + Y), "igap": (X + b"A" + Y, X + Y), "jgap": (X + Y, X + b"A" + Y),
                    "stop": (X + b"A" * 6, X + b"C" * 6), "enda": (X, X + Y), "endb": (X + Y, X), "deep": (X + b"A" + Y, X + Y)}[ending]
            for s in SHIFTS:
                lead = junk[:s + DEEP] if ending == "deep" else junk[:s]      # bases in front of `a` alone: nothing of `b` is left to pair them with
                n, m = len(lead) + len(a), len(b)
                whole = ending in ("sub", "igap", "jgap", "deep")
                out.append(("run-%s-%d-%d" % (ending, L, s), lead + a, b, (len(lead), n, 0, m) if whole else (len(lead), len(lead) + L, 0, L)))
    return out


# ---- scores beyond 15 bits

SCORES = {"score-1310": 32750, "score-1311": 32775, "score-2047": 51175, "score-2047-sub": 51075,
          "score-2047-sub-100": 51075, "score-2047-sub-735": 51075, "score-2047-igap-100": 51075, "score-2047-jgap-100": 51075}
EARLY = (100, 735)             # a mismatch at p has M[p + 1][p + 1] = 25 (2046 - p) beside it: 2^15 or more up to p = 735


@functools.lru_cache(maxsize=None)
def score_cases():
    rng = np.random.default_rng(8200)
    S = rand(rng, MAXLEN)
    mid = MAXLEN // 2
    out = [("score-%d" % n, S[:n], S[:n], (0, n, 0, n)) for n in (1310, 1311, MAXLEN)]
    out.append(("score-2047-sub", S, S[:mid] + other(S[mid]) + S[mid + 1:], (0, MAXLEN, 0, MAXLEN)))
    # The matrix is filled from the ends: in the middle the scores are still below 2^15.  A mismatch or a gap near the START is
    # where a score of 2^15 and more is compared and has the penalty taken off it.
    for p in EARLY:
        out.append(("score-2047-sub-%d" % p, S, S[:p] + other(S[p]) + S[p + 1:], (0, MAXLEN, 0, MAXLEN)))
    p = EARLY[0]
    out.append(("score-2047-igap-%d" % p, S, S[:p] + S[p + 1:], (0, MAXLEN, 0, MAXLEN - 1)))
    out.append(("score-2047-jgap-%d" % p, S[:p] + S[p + 1:], S, (0, MAXLEN - 1, 0, MAXLEN)))
    return out


# ---- the 11-bit fields of the maximum key

@functools.lru_cache(maxsize=None)
def key_cases():
    c, g = b"C" * (MAXLEN - 1), b"G" * (MAXLEN - 1)
    return [("key-i-j", c + b"A", g + b"A", (MAXLEN - 1, MAXLEN, MAXLEN - 1, MAXLEN)),
            ("key-j", b"A" + c, g + b"A", (0, 1, MAXLEN - 1, MAXLEN)),
            ("key-i", g + b"A", b"A" + c, (MAXLEN - 1, MAXLEN, 0, 1))]


# ---- equal maxima far apart

WORD, FAR, NEAR = 20, 1900, 1500


@functools.lru_cache(maxsize=None)
def tie_cases():
    """Two or four cells hold the maximum, 25 * WORD; the start is the one with the largest j, then the largest i.
    On ONE diagonal the cell with the larger j has the smaller i, so the lower lane: there the winner is never in the higher wave.
    'tie-wave-up' has it there, on another diagonal (tests/test_boundary_cases.py checks the waves)."""
    rng = np.random.default_rng(8300)
    X, Z = rand(rng, WORD), rand(rng, WORD)
    R = rand(rng, FAR)
    R1, R2 = rand(rng, FAR), rand(rng, NEAR)                    # a word next to them must not be extended: the ends differ
    R2 = other(R1[0]) + R2[1:-1] + other(R1[-1])
    S1, S2 = rand(rng, FAR), rand(rng, FAR)
    S2 = other(S1[0]) + S2[1:-1] + other(S1[-1])
    T = other(R[0]) + rand(rng, FAR - 1)
    w, f, e = WORD, WORD + FAR, WORD + NEAR
    out = [("tie-i", X + R + X, X, (f, f + w, 0, w)),
           ("tie-j", X, X + R + X, (0, w, f, f + w)),
           ("tie-ij", X + R1 + X, X + R2 + X, (f, f + w, e, e + w)),
           # ... two of them on one diagonal
           ("tie-diag", X + S1 + Z, Z + S2 + X, (0, w, f, f + w)),
           ("tie-diag-t", Z + S2 + X, X + S1 + Z, (0, w, f, f + w)),
           ("tie-diag-ij", X + S1 + X, X + S2 + X, (f, f + w, f, f + w)),
           # ... the winner in the last wave and the other cell in the first, and the transpose
           ("tie-wave-up", X + R + X, X + T, (f, f + w, 0, w)),
           ("tie-wave-t", X + T, X + R + X, (0, w, f, f + w))]
    return out


# ---- a turn of the trace that only the order of the comparisons decides

TURN_K = (3, 4, 33)
TURN_LEAD = (20, 21, 22, 23)


@functools.lru_cache(maxsize=None)
def turn_cases():
    """`P + AC..AC` against `P + CA..CA`: behind P the trace stands on a mismatch whose two gap neighbours hold the SAME score,
    25 (2 k - 1), above the diagonal one's.  The reference steps i there (v >= h), so the alignment ends at (n, m - 1); stepping j
    would end it at (n - 1, m)."""
    rng = np.random.default_rng(8350)
    out = []
    for k in TURN_K:
        for lead in TURN_LEAD:
            P = rand(rng, lead, b"GT")
            a, b = P + b"AC" * k, P + b"CA" * k
            out.append(("turn-%d-%d" % (k, lead), a, b, (0, len(a), 0, len(b) - 1)))
            out.append(("turn-%d-%d-t" % (k, lead), b, a, (0, len(b), 0, len(a) - 1)))
    return out


# ---- sweeps over small shapes

SWEEP = 16


@functools.lru_cache(maxsize=None)
def sweep_cases():
    rng = np.random.default_rng(8400)
    return [("sweep-%dx%d" % (n, m), rand(rng, n, b"AC"), rand(rng, m, b"AC"), None) for n in range(1, SWEEP + 1) for m in range(1, SWEEP + 1)]


@functools.lru_cache(maxsize=None)
def random_cases():
    rng = np.random.default_rng(8500)
    return [("random-%d" % k, rand(rng, int(rng.integers(1, 41)), b"AC"), rand(rng, int(rng.integers(1, 41)), b"AC"), None) for k in range(1000)]


# ---- the widest shapes

WIDE = ((2044, 2044), (2045, 2045), (2046, 2046), (2047, 2047), (2047, 2044), (2044, 2047), (2047, 1), (1, 2047))


@functools.lru_cache(maxsize=None)
def wide_cases():
    rng = np.random.default_rng(8600)
    out = []
    for n, m in WIDE:
        a, b = related(rng, n, m)
        out.append(("wide-related-%dx%d" % (n, m), a, b, None))
        S = rand(rng, max(n, m))
        p = min(n, m)
        last = S.rindex(S[:1])                                           # a prefix of one base: the last of its occurrences is the start
        out.append(("wide-prefix-%dx%d" % (n, m), S[:n], S[:m], (0, p, 0, p) if p > 1 else (last, last + 1, 0, 1) if m == 1 else (0, 1, last, last + 1)))
    return out


# ---- shapes at and one byte past a multiple of 256 bytes of codes

PACKING = {(5, 128): 256, (1, 257): 257, (13, 128): 512, (9, 171): 513, (13, 192): 768, (1, 769): 769, (29, 128): 1024, (1, 1025): 1025}
PACKING_2K = {(1, 2047): 2047, (2, 2047): 2048, (3, 2047): 2049}      # for a cap of 2 KB: the last two fill it exactly and exceed it


def end_aligned(rng, n, m):
    """The shorter string over ACG, the longer one T's and then the shorter: the trace runs into the LAST cell of the matrix, whose code
    is the last byte the alignment owns, and the first cell, a mismatch, has another code -- so a count of code bytes that is one short
    lets the next job's first byte change this job's result."""
    p = min(n, m)
    s = rand(rng, p, b"ACG")
    t = b"T" * (max(n, m) - p) + s
    return (s, t, (0, n, m - n, m)) if n <= m else (t, s, (n - m, n, 0, m))


@functools.lru_cache(maxsize=None)
def packing_cases():
    """one end-aligned pair per shape of PACKING and PACKING_2K, each followed by its transpose"""
    rng = np.random.default_rng(8700)
    out = []
    for n, m in list(PACKING) + list(PACKING_2K):
        for x, y in ((n, m), (m, n)):
            a, b, geometry = end_aligned(rng, x, y)
            out.append(("pack-%dx%d" % (x, y), a, b, geometry))
    return out


def packing_case(n, m):
    return next(c for c in packing_cases() if c[0] == "pack-%dx%d" % (n, m))


def greedy_launches(shapes, cap):
    """launches of one batch under a cap on the code bytes: a launch is closed when the next alignment would exceed the cap
    -> (launches, how many of them were filled to the last byte)"""
    launches, full, used = 0, 0, 0
    for n, m in shapes:
        need = rounded(n, m)
        assert need <= cap
        if used + need > cap:
            launches, full, used = launches + 1, full + (used == cap), 0
        used += need
    return launches + (used > 0), full + (used == cap)


FAMILIES = {"run": run_cases, "score": score_cases, "key": key_cases, "tie": tie_cases, "turn": turn_cases, "sweep": sweep_cases, "random": random_cases,
            "wide": wide_cases, "packing": packing_cases}
GEOMETRY = ("run", "score", "key", "tie", "turn", "wide", "packing")      # the families that go through one batch together
