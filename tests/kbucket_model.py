"""Host model of the k <= 32 k-mer table's bucketing (csrc/kmer_bucket_kernels.h, sbl_run_enumeration in csrc/sbl_api.hip): which path
every bucket of an input takes through k_bucket_classify, in plain numpy and without a device.

The kernel has data-dependent paths that no counter of the product reports: buckets STAGED in LDS, flushes in the middle of a
workgroup (two triggers), buckets that go DIRECT (two reasons), and a bounded table that OVERFLOWS and makes the host re-bucket.  The
model restates, from the sources,
- the element array  '$' c0 '$' c1 '$' ...  (E = L + nchr + 1) and the record count n = ceil(ceil(E / 32) / KM_TILE_WORDS) * 4096;
- the bits rule of sbl_run_enumeration (start at 4, raise while n >> bits > KB_SLOTS * 9 / 16, minimum with SBL_TEST_BUCKET_BITS);
- the record keys of k_kmer_records: kmer_hash(min(fwd, rc)) for a valid position, kmer_hash(g) for an invalid one (a separator in
  the window, or g >= E); bucket = low `bits` bits of the key;
- per bucket: records, distinct canonical k-mers, bifurcation k-mers (13-bit mask as k_kmer_records builds it, both orientations of a
  palindrome included; the test of mask_is_bifurcation), sort keys (a palindrome yields one, every other bifurcation k-mer two) and
  member positions;
- the staging walk of a workgroup over its KB_GROUP consecutive buckets, the overflow rule and the re-bucket ladder.

What the model says is checked against the project's CPU oracle by tests/test_kbucket_cases.py: the summed sort keys are the oracle's
id count, the summed member positions the length of its instance lists.

With ranks > 1 the walk is that of shard.hip: the same bits (sized by the whole input), bucket b at the owner whose range
[ceil(p * nb / R), ceil((p + 1) * nb / R)) holds it, every owner walking all workgroups with the other owners' buckets empty, one
owner's overflow re-bucketing everybody.  The GPU tests rest their path claims on ranks = 1 only.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

# the constants of csrc/kmer_bucket_kernels.h and csrc/kmer_kernels.h, written down once (tests/test_kbucket_cases.py reads the
# #define lines of the two headers and fails when one has drifted)
KB_SLOTS = 1024
KB_THREADS = 256
KB_MAX_DISTINCT = KB_SLOTS * 23 // 32      # 736
KB_GROUP = 16
KB_REGS = 3
KB_STAGE_MEM = 1536
KB_STAGE_KEYS = 384
KM_TILE_WORDS = 128
CONSTANTS = dict(KB_SLOTS=KB_SLOTS, KB_THREADS=KB_THREADS, KB_MAX_DISTINCT=KB_MAX_DISTINCT, KB_GROUP=KB_GROUP, KB_REGS=KB_REGS,
                 KB_STAGE_MEM=KB_STAGE_MEM, KB_STAGE_KEYS=KB_STAGE_KEYS, KM_TILE_WORDS=KM_TILE_WORDS)
TILE = KM_TILE_WORDS * 32                  # records per tile
EMPTY_CODE = (1 << 64) - 1                 # ~0: the code whose hash marks an empty slot (KB_EMPTY_KEY)

U = np.uint64
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def kmer_hash(x):
    """murmur3 fmix64 (kmer_hash of csrc/kmer_kernels.h) on a uint64 array"""
    x = np.array(x, dtype=U, ndmin=1)
    x ^= x >> U(33); x *= U(0xff51afd7ed558ccd)
    x ^= x >> U(33); x *= U(0xc4ceb9fe1a85ec53)
    x ^= x >> U(33)
    return x


def code_of(kmer: bytes) -> int:
    c = 0
    for b in kmer:
        c = c << 2 | int(_CODE[b])
    return c


def rc_of(code: int, k: int) -> int:
    r = 0
    for _ in range(k):
        r = r << 2 | (3 - (code & 3))
        code >>= 2
    return r


def elements(seqs: Sequence[bytes]) -> np.ndarray:
    """'$' c0 '$' c1 '$' ...: 0..3 for A, C, G, T and 4 for a separator"""
    parts = [np.array([4], dtype=np.uint8)]
    for s in seqs:
        c = _CODE[np.frombuffer(bytes(s), dtype=np.uint8)]
        assert not (c == 255).any(), "the model takes A, C, G, T only"
        parts += [c, np.array([4], dtype=np.uint8)]
    return np.concatenate(parts)


def record_count(E: int) -> int:
    nwords = (E + 31) // 32
    return (nwords + KM_TILE_WORDS - 1) // KM_TILE_WORDS * TILE


def start_bits(n: int, bucket_bits_env: Optional[int] = None) -> int:
    bits = 4
    while bits < 30 and (n >> bits) > KB_SLOTS * 9 // 16:
        bits += 1
    if bucket_bits_env is not None:
        bits = min(bits, max(1, int(bucket_bits_env)))
    return bits


class Records(NamedTuple):
    k: int
    E: int
    n: int
    key: np.ndarray        # uint64[n]: the record keys
    valid: np.ndarray      # bool[n]
    canon: np.ndarray      # uint64[n]: canonical code of a valid position
    fwd: np.ndarray        # uint64[n]: code of the window as spelled on the + strand
    mask: np.ndarray       # uint32[n]: the 13-bit mask in canonical orientation


def records(seqs: Sequence[bytes], k: int) -> Records:
    """what k_kmer_records writes, one record per element slot of the tiles"""
    assert 2 <= k <= 32
    el = elements(seqs)
    E = len(el)
    n = record_count(E)
    pad = np.full(n + k + 1, 4, dtype=np.uint8)        # outside the array counts as separator
    pad[:E] = el
    sep = (pad == 4).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(sep)])
    g = np.arange(n)
    valid = (g < E) & (csum[g + k] - csum[g] == 0)
    base = np.where(pad == 4, 0, pad).astype(U)
    fwd, rev = np.zeros(n, dtype=U), np.zeros(n, dtype=U)
    for i in range(k):
        fwd = (fwd << U(2)) | base[g + i]
        rev |= (U(3) - base[g + i]) << U(2 * i)
    gv = g[valid]
    ps, ns = pad[gv - 1].astype(np.int64), pad[gv + k].astype(np.int64)      # 4: separator (a valid window never starts at element 0)
    cps, cns = np.where(ps == 4, 4, 3 - ps), np.where(ns == 4, 4, 3 - ns)
    f, r = fwd[valid], rev[valid]
    m = np.zeros(len(gv), dtype=np.int64)
    m |= np.where(f <= r, (1 << ps) | (1 << (8 + ns)), 0)
    m |= np.where(r <= f, (1 << cns) | (1 << (8 + cps)), 0)
    canon = np.zeros(n, dtype=U)
    canon[valid] = np.minimum(f, r)
    mask = np.zeros(n, dtype=np.uint32)
    mask[valid] = m
    key = kmer_hash(g.astype(U))
    key[valid] = kmer_hash(canon[valid])
    return Records(k, E, n, key, valid, canon, fwd, mask)


def mask_is_bifurcation(m: int) -> bool:
    p, q = m & 0x1F, (m >> 8) & 0x1F
    return bool((p & 0x10) or (q & 0x10) or bin(p & 0xF).count("1") > 1 or bin(q & 0xF).count("1") > 1)


class Bucket(NamedTuple):
    records: int
    distinct: int          # distinct canonical k-mers
    pairs: int             # bifurcation k-mers (canonical)
    palindromes: int       # ... of them their own reverse complement
    keys: int              # sort keys: 2 * pairs - palindromes
    members: int           # positions of the bifurcation k-mers
    path: str              # "empty" (no records), "plain" (no bifurcation), "staged", "direct", "overflow", "unreached" (behind an overflow)
    by_size: bool          # direct because records > KB_REGS * KB_THREADS
    by_keys: bool          # direct because keys > KB_STAGE_KEYS


class Flush(NamedTuple):
    rank: int
    bucket: int            # the bucket before which the workgroup flushed
    cause: str             # "members": s_nm > KB_STAGE_MEM / 2; "keys": s_nk + nkeys > KB_STAGE_KEYS; "direct": before a direct reservation
    s_np: int              # what was staged at that moment
    s_nk: int
    s_nm: int


class Attempt(NamedTuple):
    bits: int
    buckets: List[Bucket]
    flushes: List[Flush]   # the flushes before a bucket (the final flush of every workgroup is not listed)
    max_nm: int            # the largest s_nm / s_nk ever staged
    max_nk: int
    overflow: bool         # a bucket held more than KB_MAX_DISTINCT distinct k-mers: the host discards the attempt and re-buckets
    pairs: int             # totals over the buckets (what the counters hold after a kept attempt)
    keys: int
    members: int


def bucket_figures(rec: Records, bits: int) -> List[Dict]:
    nb = 1 << bits
    bucket = (rec.key & U(nb - 1)).astype(np.int64)
    nrec = np.bincount(bucket, minlength=nb)
    out = [dict(records=int(nrec[b]), distinct=0, pairs=0, palindromes=0, keys=0, members=0) for b in range(nb)]
    v = np.flatnonzero(rec.valid)
    if not len(v):
        return out
    canon, inv, cnt = np.unique(rec.canon[v], return_inverse=True, return_counts=True)
    ored = np.zeros(len(canon), dtype=np.uint32)
    np.bitwise_or.at(ored, inv, rec.mask[v])
    first = np.zeros(len(canon), dtype=np.int64)
    first[inv] = v
    k = rec.k
    for j, c in enumerate(canon.tolist()):
        d = out[int(bucket[first[j]])]
        d["distinct"] += 1
        if mask_is_bifurcation(int(ored[j])):
            pal = rc_of(c, k) == c
            d["pairs"] += 1
            d["palindromes"] += int(pal)
            d["keys"] += 1 if pal else 2
            d["members"] += int(cnt[j])
    return out


def walk(figs: List[Dict], bits: int, ranks: int = 1):
    """the staging walk of every workgroup of k_bucket_classify over figures per bucket"""
    nb = 1 << bits
    first = [(p * nb + ranks - 1) // ranks for p in range(ranks + 1)]
    buckets: List[Optional[Bucket]] = [None] * nb
    flushes: List[Flush] = []
    max_nm = max_nk = 0
    for r in range(ranks):
        for b0 in range(0, nb, KB_GROUP):
            s_np = s_nk = s_nm = 0
            for b in range(b0, min(b0 + KB_GROUP, nb)):
                if not first[r] <= b < first[r + 1]:
                    continue                                   # another owner's bucket: empty here
                f = figs[b]
                if not f["records"]:
                    buckets[b] = Bucket(path="empty", by_size=False, by_keys=False, **f)
                    continue
                if s_nm > KB_STAGE_MEM // 2:
                    flushes.append(Flush(r, b, "members", s_np, s_nk, s_nm))
                    s_np = s_nk = s_nm = 0
                if f["distinct"] > KB_MAX_DISTINCT:
                    buckets[b] = Bucket(path="overflow", by_size=False, by_keys=False, **f)
                    break                                      # the workgroup raises the flag and leaves
                if not f["pairs"]:
                    buckets[b] = Bucket(path="plain", by_size=False, by_keys=False, **f)
                    continue
                by_keys, by_size = f["keys"] > KB_STAGE_KEYS, f["records"] > KB_REGS * KB_THREADS
                if by_keys or by_size:
                    flushes.append(Flush(r, b, "direct", s_np, s_nk, s_nm))
                    s_np = s_nk = s_nm = 0
                    buckets[b] = Bucket(path="direct", by_size=by_size, by_keys=by_keys, **f)
                    continue
                if s_nk + f["keys"] > KB_STAGE_KEYS:
                    flushes.append(Flush(r, b, "keys", s_np, s_nk, s_nm))
                    s_np = s_nk = s_nm = 0
                s_np += f["pairs"]; s_nk += f["keys"]; s_nm += f["members"]
                assert s_nm <= KB_STAGE_MEM and s_nk <= KB_STAGE_KEYS
                max_nm, max_nk = max(max_nm, s_nm), max(max_nk, s_nk)
                buckets[b] = Bucket(path="staged", by_size=False, by_keys=False, **f)
    # (buckets behind an overflowing one in its workgroup are never looked at: they keep their figures and no path)
    done = [x if x is not None else Bucket(path="overflow" if figs[b]["distinct"] > KB_MAX_DISTINCT else "unreached", by_size=False, by_keys=False, **figs[b])
            for b, x in enumerate(buckets)]
    return done, flushes, max_nm, max_nk


def model(seqs: Sequence[bytes], k: int, bucket_bits_env: Optional[int] = None, ranks: int = 1) -> List[Attempt]:
    """the attempts of the host loop, the kept one last"""
    rec = records(seqs, k)
    bits = start_bits(rec.n, bucket_bits_env)
    attempts: List[Attempt] = []
    while True:
        assert len(attempts) < 8, "k-mer bucket classification did not converge"
        figs = bucket_figures(rec, bits)
        buckets, flushes, max_nm, max_nk = walk(figs, bits, ranks)
        over = any(f["distinct"] > KB_MAX_DISTINCT for f in figs)
        attempts.append(Attempt(bits, buckets, flushes, max_nm, max_nk, over, sum(f["pairs"] for f in figs), sum(f["keys"] for f in figs),
                                sum(f["members"] for f in figs)))
        if not over:
            return attempts
        assert bits < 28
        bits = min(bits + 2, 28)
