"""A plain Python restatement of the multiple alignment of a group of instances (include/sibelia_amd.h), on top of
tests/galign_model.py, for the tests (never used by the product).

A group is a list of byte strings; the first is the centre c (n bases), the others are members.  Every member is aligned to the centre
with `galign_model.align(c, member)` (the unbanded matrix: the product's certificate makes its banded result equal to it).

`pair(c, s)`            -> (score, runs) of that alignment, runs = [(op, length)] with op in '=XID'.
`pair_banded(c, s)`     -> the same from band storage only, w = 64, 128, ... until galign_model.bound certifies it (or the band covers the
                           matrix): for instances of thousands of bases, where the full matrix of `pair` does not fit.  `msa` and `maf`
                           take either as `pair_fn`.
`slots(runs)`           -> {p: length} of the pair's 'D' runs by the centre index p at which they start.
`merge(n, all_slots)`   -> G, a list of n + 1 values: G[p] = the longest run any member has in slot p.
`msa(group)`            -> (rows, scores): the r rows of L = n + sum(G) columns and the r - 1 member scores.
`project(row_c, row_k)` -> the two rows without the columns where both hold '-'.
`maf(...)`              -> the MAF text --multimaf writes for aligned blocks.
"""
import numpy as np

import galign_model as GM

GAP = 45


def pair(c: bytes, s: bytes):
    score, steps = GM.align(c, s)
    return score, GM.runs(c, s, steps)


def _banded(a: bytes, b: bytes, w: int):
    """galign_model.align_banded with the band as the only storage: T[i, j - i - omin + 1], one column of minus infinity either side."""
    n, m = len(a), len(b)
    omin, omax = min(0, m - n) - w, max(0, m - n) + w
    W = omax - omin + 1
    A, B = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    T = np.full((n + 2, W + 2), GM.NEG, dtype=np.int64)
    for d in range(n + m, -1, -1):
        i_lo, i_hi = max(0, d - m, -((omax - d) // 2)), min(n, d, (d - omin) // 2)
        if i_lo > i_hi:
            continue
        i = np.arange(i_lo, i_hi + 1)
        j = d - i
        k = j - i - omin + 1
        sub = np.where(A[np.minimum(i, n - 1)] == B[np.minimum(j, m - 1)], GM.MATCH, -GM.PENALTY)
        v = np.maximum(T[i + 1, k] + sub, np.maximum(T[i + 1, k - 1], T[i, k + 1]) - GM.PENALTY)
        T[i, k] = np.where((i == n) | (j == m), -GM.PENALTY * ((n - i) + (m - j)), np.maximum(v, GM.NEG))

    def S(i, j):
        k = j - i - omin
        return int(T[i, k + 1]) if 0 <= k < W else GM.NEG
    i = j = 0
    out = []
    while i < n or j < m:                       # galign_model._trace
        if i == n:
            out.append("D"); j += 1
        elif j == m:
            out.append("I"); i += 1
        elif S(i + 1, j + 1) + (GM.MATCH if a[i] == b[j] else -GM.PENALTY) == S(i, j):
            out.append("M"); i += 1; j += 1
        elif S(i + 1, j) - GM.PENALTY == S(i, j):
            out.append("I"); i += 1
        else:
            assert S(i, j + 1) - GM.PENALTY == S(i, j)
            out.append("D"); j += 1
    return S(0, 0), "".join(out)


def pair_banded(c: bytes, s: bytes, w0: int = 64):
    n, m = len(c), len(s)
    if n == 0 or m == 0:
        return pair(c, s)
    w = w0
    while True:
        w = min(w, n, m)
        score, steps = _banded(c, s, w)
        if w >= min(n, m) or score > GM.bound(n, m, w):
            return score, GM.runs(c, s, steps)
        w *= 2


def slots(runs):
    """A slot holds at most one D run of a pair: runs are maximal, so between two D runs lies a run that consumes centre bases."""
    out, ai = {}, 0
    for op, n in runs:
        if op == "D":
            assert ai not in out
            out[ai] = n
        else:
            ai += n
    return out


def merge(n: int, all_slots):
    G = [0] * (n + 1)
    for d in all_slots:
        for p, ln in d.items():
            G[p] = max(G[p], ln)
    return G


def member_row(n: int, s: bytes, runs, G):
    """The member's row: per slot its inserted bases first, then '-' up to G[p]; per centre base its aligned base or '-'."""
    ins = [b""] * (n + 1)                       # inserted bases by slot
    col = [GAP] * n                             # the base under centre base p
    ai = bj = 0
    for op, ln in runs:
        if op == "D":
            ins[ai] = s[bj:bj + ln]
            bj += ln
        elif op == "I":
            ai += ln
        else:
            col[ai:ai + ln] = s[bj:bj + ln]
            ai += ln
            bj += ln
    assert ai == n and bj == len(s)
    out = bytearray()
    for p in range(n + 1):
        out += ins[p] + b"-" * (G[p] - len(ins[p]))
        if p < n:
            out.append(col[p])
    return bytes(out)


def msa(group, pair_fn=pair):
    c, members = bytes(group[0]), [bytes(s) for s in group[1:]]
    n = len(c)
    pairs = [pair_fn(c, s) for s in members]
    G = merge(n, [slots(runs) for _, runs in pairs])
    centre = bytearray()
    for p in range(n + 1):
        centre += b"-" * G[p]
        if p < n:
            centre.append(c[p])
    rows = [bytes(centre)] + [member_row(n, s, runs, G) for s, (_, runs) in zip(members, pairs)]
    assert all(len(r) == n + sum(G) for r in rows)
    return rows, [score for score, _ in pairs]


def project(row_c: bytes, row_k: bytes):
    keep = [i for i, (x, y) in enumerate(zip(row_c, row_k)) if x != GAP or y != GAP]
    return bytes(row_c[i] for i in keep), bytes(row_k[i] for i in keep)


_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def reverse_complement(s: bytes) -> bytes:
    return s.translate(_COMPLEMENT)[::-1]


def instance_text(records, chr_, start, end, rev) -> bytes:
    s = records[chr_][start:end]
    return reverse_complement(s) if rev else s


def block_groups(blocks, min_block_size=0):
    """Groups of a block list [(signed id, chr, start, end)]: per |id| with at least two instances of at least min_block_size bases,
    all of them by ascending (chr, start, end, rev) -> [(id, [(chr, start, end, rev)])] in ascending id."""
    by_id = {}
    for b, c, s, e in blocks:
        if e - s >= min_block_size:
            by_id.setdefault(abs(b), []).append((c, s, e, b < 0))
    return [(b, sorted(v)) for b, v in sorted(by_id.items()) if len(v) >= 2]


def maf(records, names, groups, pair_fn=pair) -> bytes:
    """`##maf version=1`, an empty line, then per group `a`, one `s` line per instance and an empty line."""
    out = [b"##maf version=1\n"]
    for _, insts in groups:
        rows, _ = msa([instance_text(records, *i) for i in insts], pair_fn)
        out.append(b"a")
        for (c, s, e, rev), row in zip(insts, rows):
            start, size, strand, total = GM.maf_fields(s, e, rev, len(records[c]))
            out.append(b"s %s %d %d %s %d %s" % (names[c].encode(), start, size, strand.encode(), total, row))
        out.append(b"")
    return b"\n".join(out) + b"\n"
