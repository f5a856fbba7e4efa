"""A plain numpy restatement of the reference's --correctboundaries step, for the tests (never used by the product).

`align(a, b)`   localAlignment(align, Score<int>(25, -75, -75)) of SeqAn 1.3.1 as the reference calls it (reference
                src/postprocessor.cpp:257-277, src/include/seqan/align/align_local_dynprog.h:229-336, :545-648, :718-751):
                -> ((a_begin, a_end), (b_begin, b_end)).
`correct(...)`  Postprocessor::ImproveBlockBoundaries (src/postprocessor.cpp:156-348) on a block list.

The matrix is filled from the ends: M[i][j] is the best score of an alignment STARTING at a[i], b[j].  Every cell is pushed into a
heap whose sift-up is strict, with j descending outside and i descending inside, so the start cell is the first pushed cell that
holds the maximum: the largest j, then the largest i.  The trace walks forward from there until it meets a zero or an end.
"""
import numpy as np

MATCH, PENALTY = 25, 75
MAX_CORRECTION_RANGE = 1 << 10

_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")      # DNASequence::Translate (src/dnasequence.cpp:11-28): every other byte unchanged


def reverse_complement(s: bytes) -> bytes:
    return s.translate(_COMPLEMENT)[::-1]


def align(a: bytes, b: bytes):
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return (0, n), (0, m)
    A = np.frombuffer(a, dtype=np.uint8)
    Brev = np.frombuffer(b, dtype=np.uint8)[::-1]
    # skewed storage: K[i + j][i] = M[i][j]; the borders M[n][*] = M[*][m] = 0 are never written
    K = np.zeros((n + m + 1, n + 1), dtype=np.int32)
    for d in range(n + m - 2, -1, -1):
        lo, hi = max(0, d - (m - 1)), min(n - 1, d)
        eq = A[lo:hi + 1] == Brev[m - 1 - d + lo:m - d + hi]
        v = K[d + 1, lo + 1:hi + 2]          # M[i + 1][j]
        h = K[d + 1, lo:hi + 1]              # M[i][j + 1]
        g = K[d + 2, lo + 1:hi + 2]          # M[i + 1][j + 1]
        K[d, lo:hi + 1] = np.where(eq, g + MATCH, np.maximum(0, np.maximum(g, np.maximum(v, h)) - PENALTY))
    best = int(K.max())
    if best == 0:                            # no trace: the rows stay as assigned
        return (0, n), (0, m)
    dd, ii = np.nonzero(K == best)
    jj = dd - ii
    at = np.lexsort((ii, jj))[-1]            # largest j, then largest i
    i, j = int(ii[at]), int(jj[at])
    i0, j0 = i, j
    while i < n and j < m and K[i + j, i] != 0:
        if a[i] == b[j]:
            i += 1; j += 1
            continue
        v, g, h = int(K[i + j + 1, i + 1]) - PENALTY, int(K[i + j + 2, i + 1]) - PENALTY, int(K[i + j + 1, i]) - PENALTY
        gv, gh = v >= h or g >= h, h > v or g >= v
        i += gv; j += gh
    return (i0, i), (j0, j)


def windows(blocks, x, R, chr_size):
    """DetermineLeft / RightProbableBoundaries (src/postprocessor.cpp:199-238) of blocks[x] in the CURRENT list: (left, right) as
    half-open pairs.  blocks: lists [id, chr, start, end]."""
    _, c, start, end = blocks[x]
    prev_end = max((b[3] for k, b in enumerate(blocks) if k != x and b[1] == c and b[3] <= start), default=None)
    next_start = min((b[2] for k, b in enumerate(blocks) if k != x and b[1] == c and b[2] >= end), default=None)
    if prev_end is not None:
        left = (max(prev_end, start - R) + 1, start + R)      # start < R: signed here, undefined in the reference
    else:
        left = (start - R + 1 if start >= R else 0, start + R)
    right = (end - R + 1, min(next_start, end + R) if next_start is not None else min(end + R, chr_size[c]))
    return left, right


def hits_undefined_case(blocks, nref, min_block_size):
    """True if the pre-correction list reaches one of the two places where the reference is undefined (R == 0; start < R with a
    previous block present), or a window outside its record."""
    R = min(min_block_size, MAX_CORRECTION_RANGE)
    if R == 0:
        return True
    for x, (_, c, start, end) in enumerate(blocks):
        if start < R and any(k != x and b[1] == c and b[3] <= start for k, b in enumerate(blocks)):
            return True
        if end + 1 < R:
            return True
    return False


def boundary_sequences(seq, block, left, right):
    """GetBoundariesSequence (src/postprocessor.cpp:240-255)."""
    s = seq[block[1]]
    if block[0] > 0:
        return s[left[0]:left[1]], s[right[0]:right[1]]
    return reverse_complement(s[right[0]:right[1]]), reverse_complement(s[left[0]:left[1]])


def updated(block, left, right, start_coords, end_coords):
    """UpdateBlockBoundaries (src/postprocessor.cpp:279-293)."""
    if block[0] > 0:
        return [block[0], block[1], left[0] + start_coords[0], right[0] + end_coords[1]]
    return [block[0], block[1], left[1] - end_coords[1], right[1] - start_coords[0]]


def correct(blocks, seq, nref, min_block_size, aligner=align):
    """blocks: (id, chr, start, end) in any order; seq: the original records; chromosomes 0 .. nref - 1 are the reference set.
    Groups are visited by ascending |id| (the reference's unstable sort permutes instances of one id only).  -> new list."""
    R = min(min_block_size, MAX_CORRECTION_RANGE)
    assert R > 0
    chr_size = [len(s) for s in seq]
    cur = sorted(([int(v) for v in b] for b in blocks), key=lambda b: abs(b[0]))      # stable: order inside a group kept
    at = 0
    while at < len(cur):
        to = at
        while to < len(cur) and abs(cur[to][0]) == abs(cur[at][0]):
            to += 1
        in_ref = sum(1 for b in cur[at:to] if b[1] < nref)
        if in_ref == 1 and to - at - in_ref == 1:
            if cur[at][1] >= nref:
                cur[at], cur[at + 1] = cur[at + 1], cur[at]
            if cur[at][0] < 0:
                cur[at][0], cur[at + 1][0] = -cur[at][0], -cur[at + 1][0]
            w = [windows(cur, at, R, chr_size), windows(cur, at + 1, R, chr_size)]
            s = [boundary_sequences(seq, cur[at + k], *w[k]) for k in range(2)]
            ref_start, asm_start = aligner(s[0][0], s[1][0])
            ref_end, asm_end = aligner(s[0][1], s[1][1])
            cur[at] = updated(cur[at], w[0][0], w[0][1], ref_start, ref_end)
            cur[at + 1] = updated(cur[at + 1], w[1][0], w[1][1], asm_start, asm_end)
        at = to
    return cur


def parse_blocks_coords(text: str):
    """blocks_coords.txt (OutputGenerator::ListBlocksIndices) -> [(signed id, chr, start, end)], half-open 0-based."""
    out, block = [], None
    for line in text.splitlines():
        if line.startswith("Block #"):
            block = int(line[7:])
            continue
        f = line.split("\t")
        if block is None or len(f) != 5 or f[1] not in "+-" or not f[0].isdigit():
            continue
        c, a, b = int(f[0]) - 1, int(f[2]), int(f[3])
        out.append((block, c, a - 1, b) if f[1] == "+" else (-block, c, b - 1, a))
    return out
