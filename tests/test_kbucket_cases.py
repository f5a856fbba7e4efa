"""The inputs of tests/kbucket_cases.py, checked where no GPU is needed: the host model (tests/kbucket_model.py) says every case reaches
the path of k_bucket_classify it is named after, the model's own totals agree with the project's CPU oracle on every case (that is what
the path predictions rest on), and the constants the model restates are still the ones of the two headers."""
import os
import re

import numpy as np
import pytest

from tests import kbucket_cases as K
from tests import kbucket_model as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sibelia_amd", "csrc")

# every row of the issue's table, by the labels that carry it
ROWS = {
    "direct_by_size": ["direct_by_size"], "direct_by_keys": ["direct_by_keys"], "key_flush": ["key_flush"], "member_flush": ["member_flush"],
    "palindromes": ["palindromes"], "table": ["table_exactly_full", "table_one_over"], "pairs": ["pairs_exact", "pairs_one_short", "pairs_one"],
    "k_limits": ["k_limits_2", "k_limits_31", "k_limits_32"],
}


def _defines(*headers):
    """the integer #define lines of the headers, evaluated (1024u, (KB_SLOTS * 23u / 32u), ...)"""
    text = {}
    for h in headers:
        for line in open(os.path.join(CSRC, h)):
            m = re.match(r"\s*#define\s+(\w+)\s+(.+)", line)
            if m:
                text[m.group(1)] = m.group(2).split("//")[0].strip()

    def value(name, depth=0):
        assert depth < 8
        expr = re.sub(r"\b(\d+)[uU]\b", r"\1", text[name])
        expr = re.sub(r"\b[A-Za-z_]\w*\b", lambda m: str(value(m.group(0), depth + 1)), expr)
        assert re.fullmatch(r"[\d\s()*/+-]+", expr), (name, expr)
        return int(eval(expr.replace("/", "//")))
    return value


def test_the_models_constants_are_the_headers():
    value = _defines("kmer_kernels.h", "kmer_bucket_kernels.h")
    for name, want in M.CONSTANTS.items():
        assert value(name) == want, name
    assert M.TILE == value("KM_TILE_WORDS") * 32 and value("KM_THREADS") * value("KM_PER_THREAD") == M.TILE
    # the empty-slot key is the hash of ~0
    text = open(os.path.join(CSRC, "kmer_bucket_kernels.h")).read()
    assert int(re.search(r"#define KB_EMPTY_KEY (0x[0-9a-fA-F]+)ull", text).group(1), 16) == int(M.kmer_hash([M.EMPTY_CODE])[0])
    # the bits rule and the ladder, as the two host loops spell them
    for f in ("sbl_api.hip", "shard.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert "unsigned bits = 4;" in src and "> KB_SLOTS * 9 / 16) bits++;" in src and "bits = std::min(bits + 2, 28u);" in src, f


def test_every_row_of_the_table_is_present():
    for row, labels in ROWS.items():
        assert all(x in K.CASES for x in labels), row
    tile = [c for c in K.CASES if c.startswith("tile_edges_")]
    assert sorted(set(K.CASES) - set(tile)) == sorted(x for labels in ROWS.values() for x in labels)
    # tile_edges: a separator at 4095 and at 4096, a record that starts at 4095 and at 4094 (windows at 4095 - j for j = 0, 1; the last
    # window of a record at j = k - 1, k), E % 4096 in {0, 1, 4095}, E % 32 in {0, 1, 31}
    seps = {int(re.search(r"sep(\d+)", c).group(1)) for c in tile}
    Es = {int(re.search(r"_E(\d+)", c).group(1)) for c in tile}
    assert {4093, 4094, 4095, 4096} <= seps
    assert {0, 1, 4095} <= {e % 4096 for e in Es} and {0, 1, 31} <= {e % 32 for e in Es if e % 4096 not in (0, 1, 4095)}
    assert all(sum(len(s) for s in c.sequences) <= 50_000 for c in K.CASES.values())


@pytest.mark.parametrize("label", list(K.CASES))
def test_the_case_reaches_its_path(label):
    case = K.CASES[label]
    case.reaches(case, K.attempts(case))


@pytest.mark.parametrize("label", list(K.CASES))
def test_the_model_agrees_with_the_oracle(label):
    from oracle.oracle import Oracle
    case = K.CASES[label]
    kept = K.attempts(case)[-1]
    assert not kept.overflow and all(a.overflow for a in K.attempts(case)[:-1])
    orc = Oracle(case.sequences)
    try:
        count, pos, neg = orc.enumerate(case.k)
    finally:
        orc.close()
    assert kept.keys == count
    assert kept.members == len(pos) == len(neg)
    assert kept.keys == sum(b.keys for b in kept.buckets) and kept.members == sum(b.members for b in kept.buckets)
    assert sum(b.records for b in kept.buckets) == M.record_count(len(M.elements(case.sequences)))


def test_the_model_hashes_like_the_library():
    # kmer_hash is murmur3's fmix64: the published test values of the finaliser
    assert int(M.kmer_hash([0])[0]) == 0
    assert int(M.kmer_hash([1])[0]) == 0xb456bcfc34c2cb2c
    assert M.rc_of(M.code_of(b"AACG"), 4) == M.code_of(b"CGTT")


def test_the_sharded_walk_covers_the_same_buckets():
    # ranks > 1: every bucket is walked by exactly one owner and keeps its figures; only what is staged together changes
    case = K.CASES["key_flush"]
    one = K.attempts(case)[-1]
    for R in (2, 3):
        many = M.model(case.sequences, case.k, None, ranks=R)[-1]
        assert [b[:6] for b in many.buckets] == [b[:6] for b in one.buckets]
        assert {f.rank for f in many.flushes} == set(range(R)) and 0 < many.max_nm <= M.KB_STAGE_MEM
