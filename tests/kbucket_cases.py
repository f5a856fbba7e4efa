"""Inputs that take the k <= 32 k-mer table (k_bucket_classify, csrc/kmer_bucket_kernels.h) to its staging, direct and capacity edges.

A case is (label, sequences, k, env) plus `reaches`, a predicate on the host model's output (tests/kbucket_model.py) that asserts the
case arrives at the path it is named after -- tests/test_kbucket_cases.py runs it without a GPU, and checks the model's totals against
the CPU oracle; tests/test_gpu_kbucket.py runs every case on the device against the oracle.  Every input comes from a fixed seed and
stays below a few tens of kilobases: these are the smallest shapes that reach the paths.  Seeds and lengths were tuned with the
model; what a predicate asserts is the reason the numbers are what they are.

`env` holds the two test hooks of sbl_run_enumeration (SBL_TEST_BUCKET_BITS, SBL_TEST_MAXPAIRS).  `stage` asks the GPU test for one
simplification stage (k, 10 * k, 1) against the oracle on top of the enumeration.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Callable, Dict, List, NamedTuple

import numpy as np

from tests import kbucket_model as M

BITS, MAXPAIRS = "SBL_TEST_BUCKET_BITS", "SBL_TEST_MAXPAIRS"
HALF_MEM = M.KB_STAGE_MEM // 2
DIRECT_RECORDS = M.KB_REGS * M.KB_THREADS


class Case(NamedTuple):
    label: str
    sequences: List[bytes]
    k: int
    env: Dict[str, str]
    reaches: Callable[["Case", List[M.Attempt]], None]
    stage: bool = False


def dna(rng, n: int) -> bytes:
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def mutate(rng, s: bytes, rate: float) -> bytes:
    a = np.frombuffer(s, dtype=np.uint8).copy()
    hit = np.flatnonzero(rng.random(len(a)) < rate)
    a[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), a[hit]) + rng.integers(1, 4, len(hit))) % 4]
    return a.tobytes()


def kmer_of(code: int, k: int) -> bytes:
    return bytes(b"ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


@lru_cache(maxsize=None)
def _attempts(label: str) -> List[M.Attempt]:
    c = CASES[label]
    return M.model(c.sequences, c.k, int(c.env[BITS]) if BITS in c.env else None)


def attempts(case: Case) -> List[M.Attempt]:
    """the model's attempts for a case (one GPU), computed once"""
    return _attempts(case.label)


def workgroup(b: int) -> int:
    return b // M.KB_GROUP


def _one_attempt(at):
    assert len(at) == 1 and not at[0].overflow
    return at[0]


# ---- the direct path ----------------------------------------------------------------------------------------------------------
def make_direct_by_size():
    # two related records (bifurcations in most buckets: something to stage) around two homopolymer runs.  A^20 has the code 0 and
    # kmer_hash(0) = 0: its bucket is the FIRST of workgroup 0, nothing can be staged before it.  The run of C lands wherever
    # kmer_hash(0x5555555555) does: in the middle of a workgroup, with staged buckets on both sides.
    rng = np.random.default_rng(DIRECT_BY_SIZE_SEED)
    anc = dna(rng, 2400)
    return [mutate(rng, anc, 0.02) + b"A" * 6000 + dna(rng, 300), mutate(rng, anc, 0.02) + b"C" * 3000 + dna(rng, 300), mutate(rng, anc, 0.02)]


DIRECT_BY_SIZE_SEED = 1


def reaches_direct_by_size(case, at):
    a = _one_attempt(at)
    assert a.bits == M.start_bits(M.record_count(len(M.elements(case.sequences)))) and not case.env          # default bits, no hook
    big = [b for b, x in enumerate(a.buckets) if x.by_size]
    assert big and all(a.buckets[b].path == "direct" and a.buckets[b].records > DIRECT_RECORDS for b in big)
    assert 0 in big and a.buckets[0].members >= 5900                  # the run of A: bucket 0
    staged = [b for b, x in enumerate(a.buckets) if x.path == "staged"]
    mid = [b for b in big if a.buckets[b].distinct < 400
           and any(workgroup(s) == workgroup(b) and s < b for s in staged) and any(workgroup(s) == workgroup(b) and s > b for s in staged)]
    assert mid, "no bucket that is direct by size with staged buckets before and after it in its workgroup"
    # ... and what was staged before it is really there when the direct bucket flushes
    assert any(f.cause == "direct" and f.bucket in mid and f.s_nm > 0 and f.s_nk > 0 for f in a.flushes)
    assert not any(x.by_keys for x in a.buckets)


def make_direct_by_keys():
    # one random record at k = 7 under 16 buckets: about 400 sort keys per bucket, on both sides of KB_STAGE_KEYS, and about 700
    # records, on both sides of KB_REGS * KB_THREADS
    return [dna(np.random.default_rng(1), 11200)]


def reaches_direct_by_keys(case, at):
    a = _one_attempt(at)
    assert a.bits == 4
    keys_only = [b for b, x in enumerate(a.buckets) if x.path == "direct" and x.by_keys and not x.by_size]
    assert keys_only and all(a.buckets[b].records <= DIRECT_RECORDS and a.buckets[b].keys > M.KB_STAGE_KEYS for b in keys_only)
    assert any(x.by_size for x in a.buckets)
    assert max(x.distinct for x in a.buckets) < M.KB_MAX_DISTINCT - 200              # nowhere near the table limit
    # a bucket that is direct because of its keys alone comes after staged ones: its flush has something to write, and the staged
    # pair indices must not be touched by the direct reservation
    assert any(f.cause == "direct" and f.bucket in keys_only and f.s_nm > 0 and f.s_np > 0 for f in a.flushes)
    assert any(x.path == "staged" for x in a.buckets[min(keys_only):])               # ... and the workgroup stages again behind it


# ---- flushes in the middle of a workgroup -------------------------------------------------------------------------------------
def make_key_flush():
    return [dna(np.random.default_rng(1), 8180)]


def reaches_key_flush(case, at):
    a = _one_attempt(at)
    assert not any(x.path == "direct" for x in a.buckets) and all(x.path == "staged" for x in a.buckets)
    fl = [f for f in a.flushes if f.cause == "keys"]
    assert fl and all(f.s_nk > 0 and f.s_nm <= HALF_MEM for f in fl)                 # the key trigger, not the member trigger
    assert any(a.buckets[f.bucket].path == "staged" for f in fl)                      # the workgroup stages again afterwards
    assert not any(f.cause == "members" for f in a.flushes)


def make_member_flush():
    rng = np.random.default_rng(MEMBER_FLUSH_SEED)
    return [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, MEMBER_FLUSH_LEN, p=MEMBER_FLUSH_BASES)])]


# One random record at k = 4: every k-mer is a bifurcation, so a bucket's members are its valid records, about 480 of them.  A bucket is
# staged only while s_nm <= 768 and holds at most 768 records, so s_nm can never pass KB_STAGE_MEM = 1536; to come near it, a bucket of
# nearly 768 members has to follow a stage of nearly 768.  Of some 58 000 (seed, length, base composition) triples tried -- uniform bases
# came to 1364, 60 % G + C spreads the bucket sizes further -- this one stages the most: s_nm reaches 1482, 54 short of the 1536 the stage
# holds, and no bucket has more than 768 records (none is direct).
MEMBER_FLUSH_SEED, MEMBER_FLUSH_LEN, MEMBER_FLUSH_BASES, MEMBER_FLUSH_MAX_NM = 158, 7500, (0.2, 0.3, 0.3, 0.2), 1482


def reaches_member_flush(case, at):
    a = _one_attempt(at)
    assert not any(x.path == "direct" for x in a.buckets)
    fl = [f for f in a.flushes if f.cause == "members"]
    assert fl and all(f.s_nm > HALF_MEM and f.s_nk <= M.KB_STAGE_KEYS // 2 for f in fl)
    assert any(a.buckets[f.bucket].path == "staged" for f in fl)
    assert a.max_nm == MEMBER_FLUSH_MAX_NM <= M.KB_STAGE_MEM                          # the largest staged member count, recorded


# ---- palindromes --------------------------------------------------------------------------------------------------------------
def make_palindromes():
    rng = np.random.default_rng(PALINDROMES_SEED)
    return [dna(rng, 2500) + b"AT" * 900 + dna(rng, 1500) + b"CCGG" * 300 + dna(rng, 1100)]


PALINDROMES_SEED, PALINDROMES_K = 1, 6


def reaches_palindromes(case, at):
    a = _one_attempt(at)
    assert case.k % 2 == 0
    assert any(x.path == "staged" and x.palindromes for x in a.buckets), "no palindromic bifurcation k-mer in a staged bucket"
    assert any(x.path == "direct" and x.palindromes for x in a.buckets), "no palindromic bifurcation k-mer in a direct bucket"
    assert all(x.keys == 2 * x.pairs - x.palindromes for x in a.buckets)
    # ATATAT / TATATA (and CCGGCC's neighbours GGCC..) are their own reverse complement: the runs land in direct buckets
    rec = M.records(case.sequences, case.k)
    code = M.code_of(b"AT" * (case.k // 2))
    assert M.rc_of(code, case.k) == code
    b = int(M.kmer_hash([code])[0]) & ((1 << a.bits) - 1)
    assert a.buckets[b].path == "direct" and a.buckets[b].by_size and a.buckets[b].palindromes
    assert (rec.canon[rec.valid] == np.uint64(code)).sum() >= 850


# ---- the table limit ----------------------------------------------------------------------------------------------------------
TABLE_K, TABLE_OTHER = 16, 300


def _table_records(full: int) -> List[bytes]:
    """records of exactly k bases, each a single window between two separators (every k-mer a bifurcation): `full` distinct canonical
    k-mers whose hash has the low bit 0, TABLE_OTHER whose hash has the low bit 1"""
    rng = np.random.default_rng(16)
    want, got, seen = (full, TABLE_OTHER), ([], []), set()
    while len(got[0]) < want[0] or len(got[1]) < want[1]:
        code = int(rng.integers(0, 1 << (2 * TABLE_K), dtype=np.uint64))
        canon = min(code, M.rc_of(code, TABLE_K))
        side = int(M.kmer_hash([canon])[0]) & 1
        if canon in seen or len(got[side]) >= want[side]:
            continue
        seen.add(canon)
        got[side].append(kmer_of(code, TABLE_K))
    out = got[0] + got[1]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def reaches_table_exactly_full(case, at):
    a = _one_attempt(at)
    assert a.bits == 1 and [x.distinct for x in a.buckets] == [M.KB_MAX_DISTINCT, TABLE_OTHER]
    assert all(len(s) == case.k for s in case.sequences)
    assert a.pairs == M.KB_MAX_DISTINCT + TABLE_OTHER                                 # every k-mer is a bifurcation


def reaches_table_one_over(case, at):
    assert len(at) == 2 and at[0].overflow and not at[1].overflow
    assert at[0].bits == 1 and [x.distinct for x in at[0].buckets] == [M.KB_MAX_DISTINCT + 1, TABLE_OTHER]
    assert at[0].buckets[0].path == "overflow" and at[0].buckets[1].path == "unreached"      # (its workgroup left with the flag)
    assert at[1].bits == 3 and max(x.distinct for x in at[1].buckets) <= M.KB_MAX_DISTINCT
    assert all(len(s) == case.k for s in case.sequences)


# ---- output capacities --------------------------------------------------------------------------------------------------------
def _pairs_total() -> int:
    return M.model(make_direct_by_keys(), 7, 4)[-1].pairs


def reaches_pairs(case, at):
    # the input of direct_by_keys: staged flushes (bp + np <= maxpairs) and direct reservations (ki + 2 <= 2 * maxpairs) both run
    reaches_direct_by_keys(case, at)
    a, mp = at[-1], int(case.env[MAXPAIRS])
    assert a.keys == 2 * a.pairs - sum(x.palindromes for x in a.buckets)
    want = {"pairs_exact": a.pairs, "pairs_one_short": a.pairs - 1, "pairs_one": 1}[case.label]
    assert mp == want
    # exact: neither host condition (pairs > maxpairs, keys > 2 * maxpairs) holds, one pass; otherwise the buffers grow once
    assert (a.pairs > mp or a.keys > 2 * mp) == (case.label != "pairs_exact")


# ---- the ends of the k range --------------------------------------------------------------------------------------------------
def make_k_limits():
    rng = np.random.default_rng(32)
    body = dna(rng, 300)
    return [body, b"T" * 40 + dna(rng, 50) + b"A" * 40, b"G", dna(rng, 2), dna(rng, 31), dna(rng, 32), body[100:200] + dna(rng, 20)]


def reaches_k_limits(case, at):
    a = _one_attempt(at)
    k, rec = case.k, M.records(case.sequences, case.k)
    lens = [len(s) for s in case.sequences]
    assert min(lens) < k and k in lens                                               # a record shorter than k, one of exactly k
    # the record of exactly k: one window, a separator on both sides
    el = M.elements(case.sequences)
    start = 1 + sum(l + 1 for l in lens[:lens.index(k)])
    assert rec.valid[start] and not rec.valid[start - 1] and not rec.valid[start + 1] and el[start - 1] == 4 and el[start + k] == 4
    assert (int(rec.mask[start]) & 0x10) and (int(rec.mask[start]) >> 8 & 0x10)
    assert a.keys > 0 and a.members >= a.pairs > 0
    allt = np.uint64(M.EMPTY_CODE >> (64 - 2 * k))
    hit = rec.valid & (rec.fwd == allt)
    assert hit.sum() >= 40 - k + 1 and (rec.canon[hit] == 0).all()                   # the all-T windows are there; canonical: all-A
    if k == 32:
        # the all-T window has the code ~0, whose hash is the empty-slot key: never canonical, so no record carries that key
        assert int(allt) == M.EMPTY_CODE
        assert not (rec.canon[rec.valid] == np.uint64(M.EMPTY_CODE)).any()
        assert not (rec.key == M.kmer_hash([M.EMPTY_CODE])[0]).any()


# ---- tile edges ---------------------------------------------------------------------------------------------------------------
def make_tile_edges(sep_at: int, E: int):
    """three records; the separator behind the first lies at element sep_at, the element array has E entries; the third record repeats
    what straddles the tile boundary, so that the windows there are bifurcations at any k"""
    rng = np.random.default_rng(4096 + sep_at + E)
    first = dna(rng, sep_at - 1)
    rest = E - 4 - len(first) - 200
    second = dna(rng, rest)
    cut = min(max(M.TILE - sep_at - 1 - 50, 0), len(second) - 100)      # 50 bases before element 4096 in `second`, where it reaches that far
    third = mutate(rng, first[-50:] + second[:50] + second[cut:cut + 100], 0.03)
    seqs = [first, second, third]
    assert len(third) == 200 and len(M.elements(seqs)) == E
    return seqs


def reaches_tile_edges(sep_at: int, E: int):
    def check(case, at):
        a = _one_attempt(at)
        k, el, rec = case.k, M.elements(case.sequences), M.records(case.sequences, case.k)
        assert len(el) == E == rec.E and el[sep_at] == 4 and rec.n % M.TILE == 0 and rec.n >= E
        edge = M.TILE - 1
        # windows that start at element 4095 - j: for j = 0, 1, k - 1, k the window, its predecessor and its successor straddle the boundary in turn
        if sep_at == edge - 1:
            assert rec.valid[edge] and not rec.valid[edge - 1]                       # j = 0: the first window of a record, '#' before it
        if sep_at == edge - 2:
            assert rec.valid[edge - 1] and rec.valid[edge] and not rec.valid[edge - 2]      # j = 1
        if sep_at == edge:
            assert rec.valid[edge - k] and not rec.valid[edge - k + 1] and rec.valid[edge + 1]      # j = k: a record's last window ends at 4094
        if sep_at == edge + 1:
            assert rec.valid[edge - (k - 1)] and not rec.valid[edge - k + 2] and rec.valid[edge + 2]      # j = k - 1: ... at 4095
        if sep_at < edge - 100:
            assert all(rec.valid[edge - j] for j in (0, 1, k - 1, k))                # one record across the boundary: every j
        assert a.members > 0
    return check


def _build() -> Dict[str, Case]:
    cases: List[Case] = [
        Case("direct_by_size", make_direct_by_size(), 20, {}, reaches_direct_by_size, stage=True),
        Case("direct_by_keys", make_direct_by_keys(), 7, {BITS: "4"}, reaches_direct_by_keys, stage=True),
        Case("key_flush", make_key_flush(), 6, {}, reaches_key_flush),
        Case("member_flush", make_member_flush(), 4, {}, reaches_member_flush),
        Case("palindromes", make_palindromes(), PALINDROMES_K, {}, reaches_palindromes),
        Case("table_exactly_full", _table_records(M.KB_MAX_DISTINCT), TABLE_K, {BITS: "1"}, reaches_table_exactly_full),
        Case("table_one_over", _table_records(M.KB_MAX_DISTINCT + 1), TABLE_K, {BITS: "1"}, reaches_table_one_over),
    ]
    total = _pairs_total()
    for label, mp in (("pairs_exact", total), ("pairs_one_short", total - 1), ("pairs_one", 1)):
        cases.append(Case(label, make_direct_by_keys(), 7, {BITS: "4", MAXPAIRS: str(mp)}, reaches_pairs))
    for k in (2, 31, 32):
        cases.append(Case("k_limits_%d" % k, make_k_limits(), k, {}, reaches_k_limits))
    # separator at element 4093 .. 4096 of the first tile (a window starting at 4095 - j for j = 1, 0, k, k - 1), and element
    # counts with E % 4096 in {0, 1, 4095} and E % 32 in {0, 1, 31}; k = 5 (nearly every window a bifurcation) and k = 32 (two packed
    # words per window; the windows next to a separator and the repeated ones are the bifurcations)
    edge = M.TILE - 1
    for sep_at, E in ((edge - 2, 2 * M.TILE), (edge - 1, 2 * M.TILE + 1), (edge, 2 * M.TILE - 1), (edge + 1, M.TILE + 2080),
                      (edge, M.TILE + 2081), (edge + 1, M.TILE + 2079), (2000, 2 * M.TILE)):
        for k in (5, 32):
            cases.append(Case("tile_edges_sep%d_E%d_k%d" % (sep_at, E, k), make_tile_edges(sep_at, E), k, {}, reaches_tile_edges(sep_at, E)))
    assert len({c.label for c in cases}) == len(cases)
    return {c.label: c for c in cases}


CASES: Dict[str, Case] = _build()
