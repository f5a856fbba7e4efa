"""Crafted inputs that put the synteny stage (csrc/synteny.hip) at the limits of its small-block index.

Every case is a seeded, deterministic generator `make()` -> (records, ops).  An op is ("stage", k, D, iters) or
("blocks", k, trim_k, min_size, shared_only), run in order on ONE context.  Every case also carries its preconditions -- what makes
the input hit the limit it is named after -- as assertions on the first-iteration candidate blocks computed from the ORACLE's
edge list (`candidate_groups`), so that the inputs are verified on a machine without a GPU (tests/test_synteny_cases.py).  What
only the library can tell -- which path a block took -- is asserted on its path counters (BlockFinder.synteny_stats) by
tests/test_gpu_synteny_limits.py through `expect(stats per op)`.

The limits (csrc/synteny.hip): a candidate block goes to the small-block kernel when it has at most MAX_ELEM elements (bases +
sequences + 1) in at most MAX_REC sequences and trim_k <= MAX_TRIM_K; groups are speculated in chunks of CHUNK; the gather of the
general path clamps its grid at GATHER_RANGES ranges and GATHER_SPAN bases per range.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_ELEM, MAX_REC, MAX_TRIM_K, CHUNK = 1024, 16, 32, 8192
GATHER_RANGES, GATHER_SPAN = 1024, 1024 * 256

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def dna(rng, n: int) -> bytes:
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def revcomp(s: bytes) -> bytes:
    return s.translate(_RC)[::-1]


class Group(NamedTuple):
    elements: int                                   # sum of orig_len + instances + 1: the element count of the child index
    records: int                                    # instances
    edges: List[Tuple[int, int, int, int]]          # (chr, strand, orig_pos, orig_len)


def candidate_groups(edges: np.ndarray, min_size: int) -> Tuple[List[Group], int]:
    """The first-iteration candidate blocks of GenerateSyntenyBlocks(k, ., min_size) from list_edges(k) of any backend: edges of at least
    min_size original bases grouped by (start vertex, end vertex, first character); groups of at least two edges with one on the
    positive strand are resolved (occupancy by earlier blocks can only shrink them).  -> (those groups, number of ALL groups of at
    least two edges: the resolved ones and their mirror images on the negative strand)."""
    keep = edges[edges["orig_len"] >= min_size]
    if not len(keep):
        return [], 0
    fc = np.frombuffer(keep["first_char"].tobytes(), dtype=np.uint8)
    order = np.lexsort((fc, keep["end_vertex"], keep["start_vertex"]))
    e, fc = keep[order], fc[order]
    new = np.ones(len(e), dtype=bool)
    new[1:] = (e["start_vertex"][1:] != e["start_vertex"][:-1]) | (e["end_vertex"][1:] != e["end_vertex"][:-1]) | (fc[1:] != fc[:-1])
    first = np.flatnonzero(new)
    count = np.diff(np.append(first, len(e)))
    total = np.add.reduceat(e["orig_len"].astype(np.int64), first)
    positive = np.minimum.reduceat(e["strand"], first) == 0
    cols = np.stack([e["chr"], e["strand"], e["orig_pos"], e["orig_len"]], axis=1).astype(np.int64)
    out = [Group(int(total[i] + count[i] + 1), int(count[i]), [tuple(r) for r in cols[first[i]:first[i] + count[i]].tolist()])
           for i in np.flatnonzero((count >= 2) & positive)]
    return out, int((count >= 2).sum())


def tiny_by_size(g: Group) -> bool:
    return g.elements <= MAX_ELEM and g.records <= MAX_REC


def block_sequences(records: Sequence[bytes], g: Group) -> List[bytes]:
    """The sequences TrimBlocks indexes: the original ranges, forward strand (the index itself holds both strands)."""
    return [records[c][p:p + n] for c, _, p, n in g.edges]


def _plant(rng, copies: Sequence[bytes], spacer: int) -> bytes:
    """copies in the given order between random spacers; copy i is flanked by ACGT[i % 4] on the left and ACGT[(i + 1) % 4] on the
    right, so that copies of one repeat (given consecutive i by the callers) never extend it"""
    out = [dna(rng, spacer)]
    for i, c in enumerate(copies):
        out += [b"ACGT"[i % 4:i % 4 + 1], c, b"ACGT"[(i + 1) % 4:(i + 1) % 4 + 1], dna(rng, spacer)]
    return b"".join(out)


def mutate(rng, anc: bytes, snp: float, indel_every: int, indel_max: int = 3) -> bytes:
    """A related copy: substitutions at rate snp, one short insertion or deletion per indel_every bases."""
    g = np.frombuffer(anc, dtype=np.uint8).copy()
    m = rng.random(len(g)) < snp
    lut = np.zeros(256, np.uint8)
    lut[list(b"ACGT")] = [0, 1, 2, 3]
    g[m] = _ACGT[(lut[g[m]] + rng.integers(1, 4, int(m.sum()))) % 4]
    s, out, p = g.tobytes(), [], 0
    for q in sorted(int(x) for x in rng.choice(len(s), max(0, len(s) // indel_every), replace=False)) if indel_every else []:
        out.append(s[p:q])
        if rng.random() < 0.5:
            out.append(dna(rng, int(rng.integers(1, indel_max + 1))))
            p = q
        else:
            p = min(len(s), q + int(rng.integers(1, indel_max + 1)))
    out.append(s[p:])
    return b"".join(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# pre(records, ops, groups): groups[i] = (candidate groups, number of groups of >= 2 edges) before blocks op i on the oracle (None for a stage)
# expect(stats): stats[i] = the library's path counters after blocks op i (None for a stage)

def _blocks_ops(ops):
    return [i for i, o in enumerate(ops) if o[0] == "blocks"]


def make_elements():
    rng = np.random.default_rng(101)
    a, b, c = dna(rng, 510), dna(rng, 340), dna(rng, 511)
    rec = _plant(rng, [a, a, b, b, b, c, c], 200)      # 2 x 510 + 3 = 1023, 3 x 340 + 4 = 1024, 2 x 511 + 3 = 1025: the smallest above
    return [rec], [("blocks", 16, 12, 16, False), ("blocks", 16, 4, 16, False), ("blocks", 16, 32, 16, False)]


def pre_elements(records, ops, groups):
    for i in _blocks_ops(ops):
        sizes = sorted(g.elements for g in groups[i][0])
        assert sizes == [1023, 1024, 1025], sizes
        assert sorted(g.records for g in groups[i][0]) == [2, 2, 3]


def expect_elements(stats):
    for s in stats:
        assert s["tiny_max_elements"] == MAX_ELEM and s["tiny_max_records"] == 3, s       # 1023 and 1024 took the kernel ...
        assert s["speculated_used"] + s["single_launches"] == 2 and s["batch_indices"] == 2, s
        assert s["general_indices"] == 1 and s["general_max_elements"] == MAX_ELEM + 1 and s["general_max_records"] == 2, s      # ... 1025 did not
        assert s["batch_declines"] == s["single_declines"] == 0, s


def make_records():
    rng = np.random.default_rng(102)
    a, b = dna(rng, 40), dna(rng, 40)
    rec = _plant(rng, [a] * 16, 30) + _plant(rng, [b] * 17, 30)
    return [rec], [("blocks", 16, 12, 20, False), ("blocks", 16, 4, 20, False)]


def pre_records(records, ops, groups):
    for i in _blocks_ops(ops):
        got = sorted((g.records, g.elements) for g in groups[i][0])
        assert got == [(16, 16 * 41 + 1), (17, 17 * 41 + 1)], got      # both small enough by elements: only the instance count tells them apart


def expect_records(stats):
    for s in stats:
        assert s["tiny_max_records"] == MAX_REC and s["tiny_max_elements"] == 16 * 41 + 1, s
        assert s["general_indices"] == 1 and s["general_max_records"] == MAX_REC + 1 and s["general_max_elements"] == 17 * 41 + 1, s
        assert s["speculated_used"] + s["single_launches"] == 1, s


def make_gather_ranges():
    rng = np.random.default_rng(103)
    return [_plant(rng, [dna(rng, 24)] * 1100, 16)], [("blocks", 16, 12, 20, False)]


def pre_gather_ranges(records, ops, groups):
    gs = sorted(groups[0][0], key=lambda g: -g.records)      # (chance repeats between the spacers add a few groups of two)
    assert gs[0].records == 1100 > GATHER_RANGES and all(tiny_by_size(g) for g in gs[1:]), [g.records for g in gs]


def expect_gather_ranges(stats):
    s = stats[0]
    assert s["general_indices"] == 1 and s["general_max_records"] == 1100 and s["general_max_elements"] == 1100 * 25 + 1, s


def make_gather_span():
    rng = np.random.default_rng(104)
    shared = dna(rng, GATHER_SPAN + 257)
    return ([dna(rng, 100) + b"A" + shared + b"G" + dna(rng, 100), dna(rng, 100) + b"C" + shared + b"T" + dna(rng, 100)],
            [("blocks", 24, 12, 24, False)])


def pre_gather_span(records, ops, groups):
    gs = groups[0][0]
    assert len(gs) == 1 and gs[0].records == 2 and min(e[3] for e in gs[0].edges) == GATHER_SPAN + 257, [(g.records, g.elements) for g in gs]


def expect_gather_span(stats):
    s = stats[0]
    assert s["general_indices"] >= 1 and s["general_max_elements"] == 2 * (GATHER_SPAN + 257) + 3, s


def make_trimk():
    rng = np.random.default_rng(105)
    anc = dna(rng, 1500)
    recs = [mutate(rng, anc, 0.02, 0) for _ in range(3)]
    recs[2] = recs[2][:700] + revcomp(recs[2][700:1100]) + recs[2][1100:]
    return recs, [("blocks", 12, 2, 12, False), ("blocks", 12, 32, 40, False), ("blocks", 12, 33, 40, False), ("blocks", 40, 12, 40, False)]


def pre_trimk(records, ops, groups):
    for i in _blocks_ops(ops):
        gs = groups[i][0]
        assert len(gs) >= 8 and all(tiny_by_size(g) for g in gs), [(g.records, g.elements) for g in gs]
        assert any(any(s == 1 for _, s, _, _ in g.edges) for g in gs)      # a block with an instance on the negative strand


def expect_trimk(stats):
    for i, s in enumerate(stats):
        if i == 2:       # trim_k = 33: beyond the kernel's 64-bit codes, whatever the size
            assert s["general_indices"] > 0 and s["batch_indices"] == s["batch_launches"] == s["single_launches"] == s["speculated_used"] == 0, s
            assert s["tiny_max_elements"] == s["tiny_max_records"] == s["tiny_max_keys"] == 0, s
        else:
            assert s["general_indices"] == 0 and s["speculated_used"] > 0 and s["batch_launches"] == 1, s


def make_poly():
    rng = np.random.default_rng(106)
    rep = dna(rng, 60) + b"A" * 44 + dna(rng, 60) + b"T" * 41 + dna(rng, 60)
    return [_plant(rng, [rep, rep], 150), _plant(rng, [revcomp(rep)], 150)[:-1] + b"C"], [("blocks", 50, 32, 50, False)]


def pre_poly(records, ops, groups):
    gs = groups[0][0]       # the repeat and its mirror image: both groups hold a positive-strand edge, the second finds every position taken
    assert len(gs) == 2 and all(g.records == 3 and tiny_by_size(g) for g in gs), [(g.records, g.elements) for g in gs]
    seqs = block_sequences(records, gs[0])
    assert all(b"A" * 40 in s and b"T" * 40 in s for s in seqs)          # windows of 32 A (canonical code 0) and of 32 T (forward code all ones)
    assert {s for _, s, _, _ in gs[0].edges} == {0, 1}
    from oracle.oracle import Oracle
    keys, pos, _ = Oracle(seqs).enumerate(32)                            # the index TrimBlocks builds of that block
    assert keys == POLY_KEYS, keys
    runs = {seqs[x["chr"]][x["pos"]:x["pos"] + 32] for x in pos}
    assert b"A" * 32 in runs and b"T" * 32 in runs, runs              # both runs are bifurcations in it (one id: each is the other's complement)


POLY_KEYS = 8            # bifurcation ids of the oracle's index of the poly block (pre_poly); the only small-block index of the op


def expect_poly(stats):
    s = stats[0]
    assert s["batch_indices"] == 2 and s["speculated_used"] == 1 and s["general_indices"] == 0 and s["tiny_max_records"] == 3, s
    assert s["single_launches"] == 0 and s["tiny_max_keys"] == POLY_KEYS, s


PALINDROMES = [b"ACGT", b"TTAA", b"GAATTC", b"GGATCC", b"CATG", b"TGCGCA"]


def make_palindromes():
    rng = np.random.default_rng(107)
    rep = b"".join(dna(rng, 18) + p for p in PALINDROMES + PALINDROMES[::-1]) + dna(rng, 18)
    return [_plant(rng, [rep, rep, rep], 120)], [("blocks", 16, 4, 16, False), ("blocks", 16, 6, 16, False)]


def pre_palindromes(records, ops, groups):
    from oracle.oracle import Oracle
    for i in _blocks_ops(ops):
        gs, tk = groups[i][0], ops[i][2]
        assert len(gs) == 1 and gs[0].records == 3 and tiny_by_size(gs[0])
        seqs = block_sequences(records, gs[0])
        keys, pos, _ = Oracle(seqs).enumerate(tk)                        # the index TrimBlocks builds: a palindromic k-mer must be a bifurcation in it
        pal = [x for x in pos if seqs[x["chr"]][x["pos"]:x["pos"] + tk] == revcomp(seqs[x["chr"]][x["pos"]:x["pos"] + tk])]
        assert len(pal) >= 6, len(pal)
        assert keys == PALINDROME_KEYS[tk], (tk, keys)


PALINDROME_KEYS = {4: 142, 6: 76}      # bifurcation ids of the oracle's index of the block at that trim_k (pre_palindromes); the only index of the op


def expect_palindromes(stats):
    for s, tk in zip(stats, (4, 6)):
        assert s["speculated_used"] == 1 and s["single_launches"] == 0 and s["general_indices"] == 0, s
        assert s["tiny_max_keys"] == PALINDROME_KEYS[tk], s


def double_cover(rng, k: int, plan, depth: int = 3) -> bytes:
    """A sequence whose windows of k visit as many canonical k-mers as possible exactly TWICE with different neighbours -- every one of
    those is a bifurcation of an index at k, so their count approaches one per window instead of the one in three of random DNA.
    plan: ("free", n) -- n bases chosen greedily with `depth` bases of lookahead -- or ("fixed", bytes), in order."""
    cnt: Dict[bytes, int] = {}
    ctx: Dict[bytes, int] = {}
    s = bytearray()

    def canon(w):
        return min(w, revcomp(w))

    def gain(w, prev, used=()):
        c = canon(w)
        v = cnt.get(c, 0)
        if c in used or v >= 2:
            return -0.5
        return 1.0 if v == 0 else 1.2 if ctx.get(c) != prev else 0.3

    def look(tail, d, used):
        best = -9.0
        for ch in b"ACGT":
            w = tail[1:] + bytes([ch])
            g = gain(w, tail[0], used)
            if d > 1:
                g += 0.7 * look(w, d - 1, used | {canon(w)})
            best = max(best, g)
        return best

    def push(ch):
        s.append(ch)
        if len(s) > k:
            c = canon(bytes(s[-k:]))
            cnt[c] = cnt.get(c, 0) + 1
            ctx.setdefault(c, s[-k - 1])

    for kind, what in plan:
        if kind == "fixed":
            for ch in what:
                push(ch)
            continue
        for _ in range(what):
            tail, opts = bytes(s[-k:]), []
            for ch in b"ACGT":
                w = tail[1:] + bytes([ch])
                opts.append((gain(w, tail[0]) + 0.7 * look(w, depth - 1, {canon(w)}) + 1e-3 * rng.random(), ch))
            push(max(opts)[1])
    return bytes(s)


def make_dense_keys():
    """Three records whose instances of 340 bases share NOTHING but their first and last 12: one bulge of 316 bases a branch, which a
    stage with a large enough branch limit collapses into one block of exactly MAX_ELEM elements -- and its ORIGINAL sequences, which
    TrimBlocks indexes, are together a double cover of the 5-mers."""
    rng = np.random.default_rng(DENSE_SEED)
    x, y = dna(rng, 12), dna(rng, 12)
    s = double_cover(rng, 5, [("fixed", x), ("free", 316), ("fixed", y + x), ("free", 316), ("fixed", y + x), ("free", 316), ("fixed", y)])
    recs = [dna(rng, 30) + b"ACG"[i:i + 1] + s[340 * i:340 * i + 340] + b"CGT"[i:i + 1] + dna(rng, 30) for i in range(3)]
    return recs, [("stage", 12, 1500, 4)] + [("blocks", 12, tk, 12, False) for tk in (5, 4, 6, 8)]


DENSE_SEED, DENSE_KEYS = 43, 900


def _largest_tiny(records, groups, tk):
    from oracle.oracle import Oracle
    g = max((g for g in groups if tiny_by_size(g)), key=lambda g: g.elements)
    return g, Oracle(block_sequences(records, g)).enumerate(tk)[0]


def pre_dense_keys(records, ops, groups):
    g, keys = _largest_tiny(records, groups[1][0], 5)
    assert g.elements == 3 * 340 + 4 == MAX_ELEM and g.records == 3, g
    assert len(set(block_sequences(records, g))) == 3
    assert keys >= DENSE_KEYS, keys                  # the table of the kernel holds fewer than 2048: 1008 windows, two codes each


def expect_dense_keys(stats):
    assert stats[1]["tiny_max_elements"] == MAX_ELEM and stats[1]["tiny_max_records"] == 3 and stats[1]["tiny_max_keys"] >= DENSE_KEYS, stats[1]
    for s in stats[1:]:
        assert s["speculated_used"] >= 1 and s["general_indices"] == 0, s


def _related(rng, n, length, snp, indel_every, flank=40):
    anc = dna(rng, length)
    return [dna(rng, flank) + mutate(rng, anc, snp, indel_every) + dna(rng, flank) for _ in range(n)]


def make_diverged():
    """Three related records, one substitution in ten and a short indel per 60 bases: the stage collapses the bulges into one path, and
    the instances of its block differ wherever a bulge was -- the ranking of the small-block kernel works on every one of them."""
    recs = _related(np.random.default_rng(3), 3, 333, 0.1, 60)
    return recs, [("stage", 10, 300, 4)] + [("blocks", 10, tk, 10, False) for tk in (4, 5, 6, 8)] + [("blocks", 5, 12, 6, False), ("blocks", 6, 8, 7, False)]


DIVERGED_KEYS = 450      # records related by substitutions and indels share most windows: 466 here at 967 elements.  The bound of 900 keys
                         # on three records after a stage is held by make_dense_keys, whose instances are designed to share none


def pre_diverged(records, ops, groups):
    for i in range(1, 5):
        g, keys = _largest_tiny(records, groups[i][0], ops[i][2])
        assert g.elements >= 900 and g.records == 3, g
        assert len(set(block_sequences(records, g))) == 3
        if ops[i][2] == 5:
            assert keys >= DIVERGED_KEYS, keys
    for i in (5, 6):         # min_size < trim_k: an instance shorter than trim_k holds no k-mer and is dropped, what is left of its block is
        lens = [e[3] for g in groups[i][0] for e in g.edges]      # trimmed again through the one-block kernel
        assert min(lens) < ops[i][2] <= max(lens), (min(lens), max(lens))


def expect_diverged(stats):
    for s in stats[1:5]:
        assert s["tiny_max_elements"] >= 900 and s["speculated_used"] > 0 and s["general_indices"] == 0, s
    assert stats[2]["tiny_max_keys"] >= DIVERGED_KEYS, stats[2]
    for s in stats[5:]:      # speculation misses and further trim iterations
        assert s["single_launches"] > 0 and s["speculated_used"] > 0 and s["batch_indices"] > s["speculated_used"], s


def make_ambiguous():
    rng = np.random.default_rng(8)
    recs = [bytearray(r) for r in _related(rng, 3, 600, 0.03, 150)]
    for r in recs:
        for at in rng.choice(len(r), len(r) // 40, replace=False):
            r[int(at)] = b"NRY"[int(rng.integers(0, 3))]
    return [bytes(r) for r in recs], [("blocks", 8, 6, 8, False), ("blocks", 6, 8, 7, False), ("blocks", 8, 6, 8, False), ("blocks", 6, 8, 7, False)]


def pre_ambiguous(records, ops, groups):
    for i in _blocks_ops(ops):
        hit = [g for g in groups[i][0] if tiny_by_size(g) and any(set(s) - set(b"ACGT") for s in block_sequences(records, g))]
        assert len(hit) >= 5, len(hit)


def expect_ambiguous(stats):
    for s in stats:
        assert s["batch_declines"] > 0 and s["general_indices"] == s["single_declines"] >= s["batch_declines"], s
    # every batch decline is followed by a single one (the block is tried once more before the general path); a single decline WITHOUT a
    # batch one comes from a block that went through the one-block kernel only.  Here those are all speculation misses: on this input
    # no block that is trimmed again still holds an ambiguous byte (pre_ambiguous_retrim / expect_ambiguous_retrim pin that path)
    assert all(s["single_declines"] > s["batch_declines"] for s in stats), stats


RETRIM_K, RETRIM_TRIM_K, RETRIM_MIN = 12, 16, 13


def make_ambiguous_retrim():
    """Three planted groups of three instances each, one per record, far apart between random spacers (at k = 12 the spacers share
    nothing, so no candidate block overlaps another and every speculation holds).  A stage collapses what differs inside each:
    - z[:12] + a + GNT/CRA + b + z[2:] in two records and the 14 bases of z alone in the third: after the stage one edge from vertex
      z[:12] to vertex z[2:] with original lengths 71, 14, 71.  At trim_k = 16 > 14 >= min_size the short instance holds no k-mer and is
      dropped, and the other two, which still hold N and R, are trimmed again: a decline of the one-block kernel on a SECOND iteration;
    - u + GNT/CYA/TTG + v: ambiguous on the first iteration only (a decline of the batch kernel, then of the one-block kernel);
    - u2 + G/C/T + v2: no ambiguous byte (a speculated index is used).
    The op in the middle, at trim_k = 8 <= 14, drops nothing; the last repeats the first where the rand() stream has moved on."""
    rng = np.random.default_rng(0)
    k = RETRIM_K
    z, a, b = dna(rng, k + 2), dna(rng, 22), dna(rng, 22)
    u, v, u2, v2 = dna(rng, 16), dna(rng, 16), dna(rng, 16), dna(rng, 16)
    sp = [[dna(rng, 150) for _ in range(4)] for _ in range(3)]
    mid = [(z[:k] + a + b"GNT" + b + z[2:], u + b"GNT" + v, u2 + b"G" + v2),
           (z, u + b"CYA" + v, u2 + b"C" + v2),
           (z[:k] + a + b"CRA" + b + z[2:], u + b"TTG" + v, u2 + b"T" + v2)]
    recs = []
    for i in range(3):
        fl, fr = b"ACG"[i:i + 1], b"CGT"[i:i + 1]               # flanks that differ between the records: the planted pieces never extend
        recs.append(b"".join(sp[i][j] + fl + mid[i][j] + fr for j in range(3)) + sp[i][3])
    blocks = ("blocks", k, RETRIM_TRIM_K, RETRIM_MIN, False)
    return recs, [("stage", k, 80, 4), blocks, ("blocks", k, 8, RETRIM_MIN, False), blocks]


def oracle_trim_traces(records, ops):
    """Oracle.trim_trace() after every blocks op of the case run in full on one oracle (None for a stage)."""
    from oracle.oracle import Oracle
    o, out = Oracle(records), []
    try:
        for op in ops:
            if op[0] == "stage":
                o.simplify_stage(*op[1:])
                out.append(None)
            else:
                o.generate_blocks(*op[1:])
                out.append(o.trim_trace())
    finally:
        o.close()
    return out


def pre_ambiguous_retrim(records, ops, groups):
    for i in _blocks_ops(ops):
        got = sorted((g.records, g.elements, sorted(e[3] for e in g.edges)) for g in groups[i][0])
        assert got == [(3, 103, [33, 33, 33]), (3, 109, [35, 35, 35]), (3, 160, [14, 71, 71])], got
        assert RETRIM_MIN <= 14 < RETRIM_TRIM_K
    for i, tr in enumerate(oracle_trim_traces(records, ops)):
        if tr is None:
            continue
        calls = sorted((int(t["iteration"]), int(t["records"]), int(t["elements"]), int(t["ambiguous"])) for t in tr)
        first = [(1, 3, 103, 0), (1, 3, 109, 1), (1, 3, 160, 1)]
        # trim_k = 16: the block of 160 elements loses its short instance and is indexed again as two sequences that still hold N and R
        assert calls == (first + [(2, 2, 145, 1)] if ops[i][2] == RETRIM_TRIM_K else first), (ops[i], calls)
        assert all(t["elements"] <= MAX_ELEM and t["records"] <= MAX_REC for t in tr)


def expect_ambiguous_retrim(stats):
    for i, s in enumerate(stats):
        if s is None:
            continue
        again = 1 if i != 2 else 0                            # ambiguous blocks on a second trim iteration (pre_ambiguous_retrim)
        assert s["groups_resolved"] == s["batch_indices"] == 3 and s["batch_launches"] == 1, s
        assert s["batch_indices"] == s["speculated_used"] + s["batch_declines"], s          # no speculation miss: every single launch
        assert s["speculated_used"] == 1 and s["batch_declines"] == 2, s                     # beyond the batch declines is a further iteration
        assert s["single_declines"] == s["single_launches"] == s["batch_declines"] + again, s
        assert s["general_indices"] == s["single_declines"], s
    assert stats[1]["single_declines"] > stats[1]["batch_declines"] and stats[3]["single_declines"] > stats[3]["batch_declines"], stats


def make_chunk():
    rng = np.random.default_rng(9)
    anc = dna(rng, 320_000)
    return [anc, mutate(rng, anc, 0.04, 0)], [("blocks", 12, 12, 12, False)]


def pre_chunk(records, ops, groups):
    gs, multi = groups[0]
    assert multi >= 2 * (CHUNK + 1) and len(gs) >= 2 * CHUNK, (multi, len(gs))      # groups are taken largest first: the resolved half crosses a chunk


def expect_chunk(stats):
    s = stats[0]
    assert s["batch_launches"] >= 2 and s["groups_resolved"] >= CHUNK + 1, s
    assert s["speculated_used"] > CHUNK, s           # more than one chunk can hold: the speculation of a later chunk was used as well


class Case(NamedTuple):
    make: Callable[[], Tuple[List[bytes], list]]
    pre: Callable
    expect: Callable
    no_tiny_twin: bool = True        # also run under SBL_NO_TINY_INDEX (the chunk case would build ~15000 general child indices: oracle only)
    ambiguous: bool = False          # the input holds non-ACGT bytes: edge lists depend on the rand() stream


CASES: Dict[str, Case] = {
    "elements": Case(make_elements, pre_elements, expect_elements),
    "records": Case(make_records, pre_records, expect_records),
    "gather_ranges": Case(make_gather_ranges, pre_gather_ranges, expect_gather_ranges),
    "gather_span": Case(make_gather_span, pre_gather_span, expect_gather_span),
    "trimk": Case(make_trimk, pre_trimk, expect_trimk),
    "poly": Case(make_poly, pre_poly, expect_poly),
    "palindromes": Case(make_palindromes, pre_palindromes, expect_palindromes),
    "dense_keys": Case(make_dense_keys, pre_dense_keys, expect_dense_keys),
    "diverged": Case(make_diverged, pre_diverged, expect_diverged),
    "ambiguous": Case(make_ambiguous, pre_ambiguous, expect_ambiguous, ambiguous=True),
    "ambiguous_retrim": Case(make_ambiguous_retrim, pre_ambiguous_retrim, expect_ambiguous_retrim, ambiguous=True),
    "chunk": Case(make_chunk, pre_chunk, expect_chunk, no_tiny_twin=False),
}


def cmd_of(op) -> str:
    """The op as a command of tests/vectors.run_cmd and of the reference driver."""
    return "stage:%d:%d:%d" % op[1:] if op[0] == "stage" else "blocks:%d:%d:%d:%d" % (op[1], op[2], op[3], int(op[4]))


def oracle_groups(records, ops) -> List[Optional[Tuple[List[Group], int]]]:
    """Candidate groups before every blocks op, on an oracle that runs the stages only (list_edges consumes rand() like an index)."""
    from oracle.oracle import Oracle
    o, out = Oracle(records), []
    try:
        for op in ops:
            if op[0] == "stage":
                o.simplify_stage(op[1], op[2], op[3])
                out.append(None)
            else:
                out.append(candidate_groups(o.list_edges(op[1]), op[3]))
    finally:
        o.close()
    return out
