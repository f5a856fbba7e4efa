"""Inputs for the small-block index of the synteny stage called on its own (BlockFinder.tiny_index -> sbl_tiny_index, csrc/synteny.hip).

A case is a seeded, deterministic generator `make()` -> (records, jobs): a handful of records plus jobs (k, blocks), a block being a
list of (chr, start, end) ranges of the ORIGINAL records.  Every case states
- `counts[j]`: how many blocks of job j are indexed, declined (a byte other than A, C, G, T) and not eligible (no range, more than MAX_REC
  ranges, more than MAX_ELEM elements, k > MAX_TRIM_K) -- exact numbers, so that no test passes on an empty result;
- `pre(records, jobs, index)`: what makes the input reach the edge it is named after, asserted on the ORACLE's index of every block
  (index[(j, b)] = Oracle(sequences of block b of job j).enumerate(k), indexed blocks only) by tests/test_tiny_index_cases.py without
  a GPU;
- `general`: tests/test_gpu_tiny_index.py also compares with the general index on the GPU (BlockFinder(sequences).enumerate(k));
- `stage`: a (k, D, iterations) simplification run on the context before the index is asked for -- the index is over the ORIGINAL
  substrings whatever the stage did.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from tests import synteny_cases as S
from tests.synteny_cases import MAX_ELEM, MAX_REC, MAX_TRIM_K, dna, mutate, revcomp

INDEXED, DECLINED, NOT_ELIGIBLE = 0, 1, 2              # SBL_TINY_*
THREADS, WAVE = 256, 64                                # TE_THREADS of csrc/synteny.hip, lanes per wavefront
REAL_CAP = 200                                         # candidate blocks taken per case of synteny_cases.CASES (the first ones, in group order)

Block = List[Tuple[int, int, int]]
Job = Tuple[int, List[Block]]


def sequences(records: Sequence[bytes], block: Block) -> List[bytes]:
    return [records[c][s:e] for c, s, e in block]


def elements(block: Block) -> int:
    return sum(e - s for _, s, e in block) + len(block) + 1


def expected_status(records: Sequence[bytes], block: Block, k: int) -> int:
    """What the entry point must report for a block, from its definition (include/sibelia_amd.h)."""
    if not block or len(block) > MAX_REC or elements(block) > MAX_ELEM or k > MAX_TRIM_K:
        return NOT_ELIGIBLE
    return DECLINED if any(set(s) - set(b"ACGT") for s in sequences(records, block)) else INDEXED


def split(total: int, parts: int) -> List[int]:
    """`parts` lengths that sum to `total`, as equal as possible, the longer ones first"""
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


def family(rng, n: int, length: int, snp: float, flank: int = 0) -> List[bytes]:
    """n related records: copies of one ancestor with substitutions at rate snp (same length), between random flanks"""
    anc = dna(rng, length)
    return [dna(rng, flank) + mutate(rng, anc, snp, 0) + dna(rng, flank) for _ in range(n)]


def _none(records, jobs, index):
    pass


# ---- k range -------------------------------------------------------------------------------------------------------------------
K_RANGE = (2, 3, 16, 31, 32, 33)


def make_k_range():
    rng = np.random.default_rng(201)
    anc = dna(rng, 60)
    copies = [mutate(rng, anc, 0.03, 0), mutate(rng, anc, 0.03, 0), revcomp(mutate(rng, anc, 0.03, 0))]
    records = [dna(rng, 20) + c + dna(rng, 20) for c in copies]
    block = [(i, 20, 20 + len(c)) for i, c in enumerate(copies)]
    return records, [(k, [block]) for k in K_RANGE]


def pre_k_range(records, jobs, index):
    from oracle.oracle import Oracle
    o = Oracle(sequences(records, jobs[0][1][0]))
    try:
        for k in range(2, MAX_TRIM_K + 1):             # every k the kernel takes, not only the ones that are run
            assert o.enumerate(k)[0] > 0, k
    finally:
        o.close()
    assert (len(jobs) - 1, 0) not in index             # k = 33: not indexed


# ---- palindromes ---------------------------------------------------------------------------------------------------------------
def make_palindromes():
    rng = np.random.default_rng(202)
    half = dna(rng, 16)
    pals = S.PALINDROMES + [half + revcomp(half)]      # 4- and 6-mers and one 32-mer that are their own reverse complement
    records = [b"".join(dna(rng, 11) + p for p in order) + dna(rng, 11) for order in (pals, pals[::-1], pals[2:] + pals[:2])]
    block = [(i, 0, len(r)) for i, r in enumerate(records)]      # every palindrome three times, each time between other neighbours
    return records, [(k, [block]) for k in (4, 6, 32, 5)]


def self_paired(records, block, k, pos, neg):
    """ids that stand at (c, p) on the + strand and at (c, len_c - k - p) on the - strand: k-mers that are their own reverse complement"""
    lens = [e - s for _, s, e in block]
    mirror = {(int(x["id"]), int(x["chr"]), lens[int(x["chr"])] - k - int(x["pos"])) for x in pos}
    return mirror & {(int(x["id"]), int(x["chr"]), int(x["pos"])) for x in neg}


def pre_palindromes(records, jobs, index):
    for j, (k, blocks) in enumerate(jobs):
        _, pos, neg = index[(j, 0)]
        hit = self_paired(records, blocks[0], k, pos, neg)
        if k % 2 == 0:
            assert len(hit) >= 3, (k, len(hit))        # the planted palindrome of that length, in each of the three ranges
        else:
            assert not hit, (k, hit)                   # the contrast: no k-mer of odd length is its own reverse complement


# ---- strand order --------------------------------------------------------------------------------------------------------------
def make_strand_order():
    rng = np.random.default_rng(203)
    records = family(rng, 3, 80, 0.05, 15)
    return records, [(5, [[(i, 15, 95) for i in range(3)]])]


def pre_strand_order(records, jobs, index):
    _, _, neg = index[(0, 0)]
    mixed = [c for c in range(3) if len(set(neg["id"][neg["chr"] == c].tolist())) >= 2]
    assert len(mixed) >= 2, mixed                      # un-reversing the run of any of those records changes the list
    for c in mixed:
        run = neg["id"][neg["chr"] == c]
        assert run.tolist() != run[::-1].tolist(), c


# ---- short ranges --------------------------------------------------------------------------------------------------------------
SHORT_K = (2, 8, 32)


def make_short_ranges():
    rng = np.random.default_rng(204)
    records = family(rng, 4, 90, 0.04, 10)
    jobs = []
    for k in SHORT_K:
        # ranges of 1, k - 1, k and k + 1 bases cut out of the related part, next to two long ones: the short ones share their k-mers
        mixed = [(0, 30, 31), (1, 30, 30 + k - 1), (2, 30, 30 + k), (3, 30, 30 + k + 1), (0, 10, 100), (1, 10, 100)]
        below = [(0, 30, 31), (1, 30, 30 + k - 1), (2, 40, 40 + max(1, k // 2)), (3, 50, 50 + k - 1)]      # no range reaches k
        jobs.append((k, [mixed, below, [(2, 30, 30 + k)]]))      # ... and a single range of exactly k: one window, '$' on both sides
    return records, jobs


def pre_short_ranges(records, jobs, index):
    for j, (k, blocks) in enumerate(jobs):
        assert [e - s for _, s, e in blocks[0]][:4] == [1, k - 1, k, k + 1]
        bif, pos, neg = index[(j, 0)]
        assert bif > 0 and {2, 3} & set(pos["chr"].tolist()), (k, bif)      # instances inside the ranges of k and k + 1 bases
        bif, pos, neg = index[(j, 1)]
        assert max(e - s for _, s, e in blocks[1]) < k
        assert bif == 0 and len(pos) == 0 and len(neg) == 0, (k, bif)


# ---- limits --------------------------------------------------------------------------------------------------------------------
LIMIT_K, DENSE_K = 12, 5


def make_limits():
    rng = np.random.default_rng(205)
    dense, _ = S.make_dense_keys()                     # records 0..2: together a double cover of the 5-mers, 340 bases each from 31
    three = family(rng, 3, 345, 0.04)                  # records 3..5
    many = family(rng, 17, 70, 0.04)                   # records 6..22
    records = dense + three + many
    full3 = [(3 + i, 2, 2 + 340) for i in range(3)]                                          # 3 x 340 + 4 = 1024
    full16 = [(6 + i, 3, 3 + n) for i, n in enumerate(split(MAX_ELEM - MAX_REC - 1, MAX_REC))]      # 1007 bases + 17 = 1024
    over = [(3, 2, 342), (4, 2, 342), (5, 2, 343)]                                           # 1025
    seventeen = [(6 + i, 3, 13) for i in range(MAX_REC + 1)]                                 # small, but 17 ranges
    cover = [(i, 31, 371) for i in range(3)]
    return records, [(LIMIT_K, [full3, over, full16, seventeen, []]), (DENSE_K, [cover, over, cover])]


def pre_limits(records, jobs, index):
    b = jobs[0][1]
    assert [elements(x) for x in b[:4]] == [MAX_ELEM, MAX_ELEM + 1, MAX_ELEM, 10 * 17 + 18] and [len(x) for x in b[:4]] == [3, 3, MAX_REC, MAX_REC + 1]
    assert index[(0, 0)][0] > 0 and index[(0, 2)][0] > 0
    assert 15 in index[(0, 2)][1]["chr"].tolist()      # instances in the 16th range
    cover = jobs[1][1][0]
    assert elements(cover) == MAX_ELEM
    assert index[(1, 0)][0] >= S.DENSE_KEYS, index[(1, 0)][0]      # the far end of keys[] / payload[]: fewer than 2048 slots, two codes per k-mer


# ---- thread partition ----------------------------------------------------------------------------------------------------------
PARTITION_E, PARTITION_K = (255, 256, 257, 512, 513), 6


def make_partition():
    rng = np.random.default_rng(206)
    records = family(rng, 3, 180, 0.05)
    blocks = [[(i, 1, 1 + n) for i, n in enumerate(split(E - 4, 3))] for E in PARTITION_E]
    return records, [(PARTITION_K, blocks)]


def waves_of(block, pos) -> set:
    """wavefronts whose lanes write the instances: lane t of the workgroup owns elements [t * per, (t + 1) * per), per = ceil(E / 256)"""
    sep, e = [], 0
    for _, s, t in block:
        sep.append(e)
        e += t - s + 1
    per = (e + 1 + THREADS - 1) // THREADS
    return {(sep[int(x["chr"])] + 1 + int(x["pos"])) // per // WAVE for x in pos}


def pre_partition(records, jobs, index):
    blocks = jobs[0][1]
    assert [elements(b) for b in blocks] == list(PARTITION_E)
    for i, b in enumerate(blocks):
        w = waves_of(b, index[(0, i)][1])
        if elements(b) != 257:
            assert len(w) >= 3, (elements(b), w)
        else:
            # per = 2: lanes 0 .. 127 own elements 0 .. 255 and lane 128, the only busy lane of the third wavefront, owns element 256
            # alone -- the closing separator, where no window starts.  So the instances fill two wavefronts, the third adds a zero to the
            # prefix sum and the fourth is idle: that is the edge
            assert w == {0, 1} and (257 + THREADS - 1) // THREADS == 2, w


# ---- ranges as sbl_generate_blocks forms them -------------------------------------------------------------------------------------
FORMED_STAGE = (10, 300, 4)


def make_formed():
    records, _ = S.make_diverged()                     # three related records of ~410 bases whose bulges the stage collapses
    blocks = [[(1, 50, 150), (2, 60, 160)],                                  # from the middle of records, none of them record 0
              [(1, 50, 120), (1, 200, 280), (2, 55, 130)],                   # two ranges of one record
              [(1, 50, 150), (1, 100, 200), (0, 50, 150)],                   # overlapping ranges
              [(2, 0, len(records[2])), (1, 0, len(records[1]))]]            # whole records, in descending record order
    return records, [(8, blocks)]


def pre_formed(records, jobs, index):
    from oracle.oracle import Oracle
    o = Oracle(records)
    try:
        assert o.simplify_stage(*FORMED_STAGE) > 0
        assert o.state()[0] != list(records)           # the stage has changed the state the context holds
    finally:
        o.close()
    for b in range(4):
        assert index[(0, b)][0] > 0, b


# ---- declines ------------------------------------------------------------------------------------------------------------------
def make_declines():
    rng = np.random.default_rng(208)
    recs = [bytearray(r) for r in family(rng, 3, 100, 0.04)]
    recs[0][10], recs[2][89], recs[1][50] = ord("N"), ord("R"), ord("-")
    records = [bytes(r) for r in recs]
    blocks = [[(0, 10, 60), (1, 0, 40)],               # N: the first byte of the first range
              [(0, 11, 60), (1, 0, 40), (2, 0, 89)],   # clean: it ends right before the R
              [(0, 11, 60), (2, 40, 90)],              # R: the last byte of the last range
              [(0, 11, 60), (1, 30, 70), (2, 0, 40)],  # '-' in the middle
              [(1, 51, 100), (2, 0, 89)]]              # clean again
    return records, [(8, blocks)]


def pre_declines(records, jobs, index):
    b = jobs[0][1]
    assert sequences(records, b[0])[0][:1] == b"N" and sequences(records, b[2])[-1][-1:] == b"R" and b"-" in sequences(records, b[3])[1][1:-1]
    assert sorted(index) == [(0, 1), (0, 4)] and index[(0, 1)][0] > 0 and index[(0, 4)][0] > 0


# ---- batch layout --------------------------------------------------------------------------------------------------------------
BATCH_K = 6


def make_batch():
    rng = np.random.default_rng(209)
    fam = family(rng, 17, 420, 0.05)
    bad = bytearray(dna(rng, 420))
    bad[::37] = b"N" * len(bad[::37])
    records = fam + [bytes(bad)]                       # record 17 holds an N every 37 bases
    blocks: List[Block] = [[(0, 5, 6)], [(i, 0, 340) for i in range(3)]]      # the smallest block there is (3 elements) and a full one (1024)
    while len(blocks) < 320:
        i = len(blocks)
        if i % 10 == 4:
            blocks.append(list(blocks[int(rng.integers(0, i))]))                             # an exact duplicate of an earlier block
        elif i % 13 == 6:
            blocks.append([(int(rng.integers(0, 17)), 0, 50), (17, 0, 50)])                  # declined
        elif i % 17 == 9:
            blocks.append([(c, 0, 345) for c in range(3)] if i % 2 else [(c, 0, 9) for c in range(17)])      # not eligible: 1039 elements / 17 ranges
        else:
            n = int(rng.integers(1, MAX_REC + 1))
            budget = int(rng.integers(n, [40, 200, MAX_ELEM - n - 1][i % 3] + 1))
            lens = [max(1, min(400, x)) for x in split(max(budget, n), n)]
            at = [int(rng.integers(0, 420 - x + 1)) for x in lens]
            blocks.append([(int(rng.integers(0, 17)), a, a + x) for a, x in zip(at, lens)])
    return records, [(BATCH_K, blocks)]


def pre_batch(records, jobs, index):
    k, blocks = jobs[0]
    st = [expected_status(records, b, k) for b in blocks]
    assert len(blocks) >= 300
    sizes = [elements(b) for b, s in zip(blocks, st) if s == INDEXED]
    assert min(sizes) == 3 and max(sizes) == MAX_ELEM and len(set(sizes)) >= 100
    # not-eligible and declined blocks BETWEEN indexed ones: the slot of a block in the batch is not its number in the call
    assert any(st[i] == NOT_ELIGIBLE and INDEXED in st[:i] and INDEXED in st[i + 1:] for i in range(len(st)))
    assert any(st[i] == DECLINED and INDEXED in st[:i] and INDEXED in st[i + 1:] for i in range(len(st)))
    assert sum(blocks[i] in blocks[:i] for i in range(len(blocks))) >= 20
    # neighbours in the batch differ in result, so a stride that lands on the neighbour's result shows
    idx = [i for i, s in enumerate(st) if s == INDEXED]
    differ = sum(not _same(index[(0, a)], index[(0, b)]) for a, b in zip(idx, idx[1:]))
    assert differ >= len(idx) - 1 - 40, differ


def _same(x, y):
    return x[0] == y[0] and all(len(a) == len(b) and (a == b).all() for a, b in zip(x[1:], y[1:]))


# ---- real candidate blocks -----------------------------------------------------------------------------------------------------
def make_real(name: str):
    """The first-iteration candidate blocks of the first blocks op of a case of synteny_cases.CASES that the small-block index takes by
    size and content, the first REAL_CAP of them, at that op's trim_k"""
    def make():
        records, ops = S.CASES[name].make()
        i = next(i for i, op in enumerate(ops) if op[0] == "blocks")
        groups = S.oracle_groups(records, ops[:i + 1])[i][0]
        blocks = []
        for g in groups:
            if S.tiny_by_size(g) and not any(set(s) - set(b"ACGT") for s in S.block_sequences(records, g)):
                blocks.append([(c, p, p + n) for c, _, p, n in g.edges])
        return records, [(ops[i][2], blocks[:REAL_CAP])]
    return make


# (gather_span has one candidate block, far beyond the size limit: its call is the empty one)
REAL_COUNTS = {"elements": 2, "records": 1, "gather_ranges": 15, "gather_span": 0, "trimk": 132, "poly": 2, "palindromes": 1, "dense_keys": 1,
               "diverged": 3, "chunk": REAL_CAP}


class Case(NamedTuple):
    make: Callable[[], Tuple[List[bytes], List[Job]]]
    pre: Callable
    counts: List[Tuple[int, int, int]]               # per job: blocks indexed, declined, not eligible
    general: bool = False
    stage: Optional[Tuple[int, int, int]] = None


CASES: Dict[str, Case] = {
    "k_range": Case(make_k_range, pre_k_range, [(1, 0, 0)] * 5 + [(0, 0, 1)], general=True),
    "palindromes": Case(make_palindromes, pre_palindromes, [(1, 0, 0)] * 4, general=True),
    "strand_order": Case(make_strand_order, pre_strand_order, [(1, 0, 0)]),
    "short_ranges": Case(make_short_ranges, pre_short_ranges, [(3, 0, 0)] * 3, general=True),
    "limits": Case(make_limits, pre_limits, [(2, 0, 3), (2, 0, 1)], general=True),
    "partition": Case(make_partition, pre_partition, [(5, 0, 0)]),
    "formed": Case(make_formed, pre_formed, [(4, 0, 0)], stage=FORMED_STAGE),
    "declines": Case(make_declines, pre_declines, [(2, 3, 0)]),
    "batch": Case(make_batch, pre_batch, [(278, 26, 16)]),
}
for _n, _c in S.CASES.items():
    if not _c.ambiguous:
        CASES["real/" + _n] = Case(make_real(_n), _none, [(REAL_COUNTS[_n], 0, 0)])

_made: Dict[str, Tuple[List[bytes], List[Job]]] = {}
_index: Dict[str, dict] = {}


def made(name: str):
    if name not in _made:
        _made[name] = CASES[name].make()
    return _made[name]


def oracle_index(name: str) -> dict:
    """{(job, block): (bif_count, pos, neg)} of the oracle for every block of the case that must be indexed; computed once, shared"""
    if name not in _index:
        from oracle.oracle import Oracle
        records, jobs = made(name)
        out = {}
        for j, (k, blocks) in enumerate(jobs):
            for b, block in enumerate(blocks):
                if expected_status(records, block, k) == INDEXED:
                    o = Oracle(sequences(records, block))
                    out[(j, b)] = o.enumerate(k)
                    o.close()
        _index[name] = out
    return _index[name]


def inst_bytes(a: np.ndarray) -> bytes:
    """an instance list as the reference driver writes it: (id, chr, pos) as three little-endian u32 each"""
    return np.stack([a["id"], a["chr"], a["pos"]], axis=1).astype("<u4").tobytes() if len(a) else b""


def fixture_key(seqs: Sequence[bytes], k: int) -> str:
    from sibelia_amd import workloads as W
    return "%s:%d" % (W.input_digest(seqs), k)


LIST_MAX = 24                                          # the fixture keeps the lists themselves up to this many instances per strand


def as_fixture(bif: int, pos: np.ndarray, neg: np.ndarray) -> dict:
    """An index as tests/golden/tiny_index.json records it (tests/golden/gen/make_tiny_index_golden.py): equal entries = equal count,
    lengths and every (id, chr, pos) of both lists"""
    import hashlib
    p, q = inst_bytes(pos), inst_bytes(neg)
    e = {"bif": int(bif), "n": [len(pos), len(neg)], "sha256": [hashlib.sha256(p).hexdigest(), hashlib.sha256(q).hexdigest()]}
    if max(len(pos), len(neg)) <= LIST_MAX:
        e["pos"], e["neg"] = np.frombuffer(p, "<u4").tolist(), np.frombuffer(q, "<u4").tolist()
    return e
