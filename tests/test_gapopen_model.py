"""tests/gapopen_model.py -- the alignment with a gap opening cost -- against tests/galign_model.py and against itself:
o = 0 is the linear alignment exactly, the rows re-score to the reported score, an opening cost can only merge gap runs, a certified
band equals the full matrix, and the centre-star merge keeps its consequences."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import galign_model as GM                          # noqa: E402
import gapopen_model as AM                         # noqa: E402
import msa_model as MM                             # noqa: E402

# the pair of DESIGN.md 0.5: a 9-base deletion with a substitution three bases before it
PAIR_A = b"CACTGGAGACACACCGAGTGGATAGTCCTATCCCATGAGC"
PAIR_B = b"CACTGGAGACACATCGTCCTATCCCATGAGC"


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def mutated(rng, a, rate=0.06, max_indel=12, alphabet=b"ACGT"):
    b = bytearray()
    i = 0
    while i < len(a):
        u = rng.random()
        if u < rate / 3:
            i += int(rng.integers(1, max_indel + 1))
        elif u < 2 * rate / 3:
            b += rand(rng, int(rng.integers(1, max_indel + 1)), alphabet)
        else:
            b += rand(rng, 1, alphabet) if rng.random() < rate else a[i:i + 1]
            i += 1
    return bytes(b)


def make_pairs(seed=31, count=150, longest=90):
    """every third pair over the alphabet AC: full of ties"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        alphabet = b"AC" if k % 3 == 2 else b"ACGT"
        a = rand(rng, int(rng.integers(1, longest + 1)), alphabet)
        b = (mutated(rng, a, alphabet=alphabet) or b"A")[:longest] if rng.random() < 0.85 else rand(rng, int(rng.integers(1, longest + 1)), alphabet)
        out.append((a, b))
    return out


@pytest.fixture(scope="module")
def pairs():
    return make_pairs()


@pytest.fixture(scope="module")
def linear(pairs):
    return [GM.align(a, b) for a, b in pairs]


@pytest.fixture(scope="module")
def affine(pairs):
    return [AM.align(a, b, 300) for a, b in pairs]


def test_no_opening_cost_is_the_linear_alignment_ties_included(pairs, linear):
    assert len(pairs) >= 150 and sum(set(a + b) <= set(b"AC") for a, b in pairs) >= 50
    for (a, b), want in zip(pairs, linear):
        assert AM.align(a, b, 0) == want, (a, b)
    for a, b in ((b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A" * 33, b"A" * 90), (b"A" * 90, b"A" * 33), (PAIR_A, PAIR_B)):
        assert AM.align(a, b, 0) == GM.align(a, b), (a, b)


def test_the_printed_pair():
    score, steps = GM.align(PAIR_A, PAIR_B)
    assert (score, GM.runs(PAIR_A, PAIR_B, steps)) == (0, [("=", 13), ("X", 1), ("=", 2), ("I", 2), ("=", 1), ("I", 7), ("=", 14)])
    score, steps = AM.align(PAIR_A, PAIR_B, 300)
    assert (score, GM.runs(PAIR_A, PAIR_B, steps)) == (-300, [("=", 13), ("X", 1), ("=", 2), ("I", 9), ("=", 15)])


def test_empty_sides():
    for o in (0, 1, 300):
        assert AM.align(b"", b"", o) == (0, "")
        assert AM.align(b"", b"ACGT", o) == (-(o + 300), "DDDD")
        assert AM.align(b"ACGT", b"", o) == (-(o + 300), "IIII")
        assert AM.align(b"A", b"ACGT", o) == (25 - o - 225, "MDDD")


def test_the_rows_rescore_to_the_reported_score(pairs, affine):
    for (a, b), (score, steps) in zip(pairs, affine):
        ra, rb = GM.rows(a, b, steps)
        assert ra.replace(b"-", b"") == a and rb.replace(b"-", b"") == b
        assert AM.score_of_rows(ra, rb, 300) == score, (a, b)
        assert AM.score_of_rows(ra, rb, 0) == GM.score_of_rows(ra, rb)


def test_an_opening_cost_only_merges_gap_runs(pairs, linear, affine):
    changed = fewer = 0
    for (a, b), (s0, steps0), (s1, steps1) in zip(pairs, linear, affine):
        assert s0 - 300 * AM.gap_runs(a, b, steps0) <= s1 <= s0, (a, b)      # the linear trace is a candidate; an opening cost only lowers a path
        if steps1 != steps0:
            changed += 1
            fewer += AM.gap_runs(a, b, steps1) < AM.gap_runs(a, b, steps0)
    assert changed >= 50 and fewer == changed, (changed, fewer)


@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_a_certified_band_equals_the_full_matrix(pairs, affine, w):
    certified = 0
    for (a, b), want in zip(pairs, affine):
        score, steps, ok = AM.align_banded(a, b, 300, w)
        if ok:
            certified += 1
            assert (score, steps) == want, (a, b, w)
        else:
            assert score <= want[0]
    assert certified >= 20, certified


def test_band_only_storage_gives_the_same(pairs, affine):
    for (a, b), want in list(zip(pairs, affine))[:60]:
        assert AM.pair_banded(a, b, 300, 2) == want, (a, b)
        assert AM.pair_banded(a, b, 0, 2) == GM.align(a, b), (a, b)


def test_doubling_ends_at_the_full_result(pairs, affine):
    for (a, b), want in list(zip(pairs, affine))[:40]:
        score, steps, w, passes = AM.align_doubling(a, b, 300, 1)
        assert (score, steps) == want and passes >= 1 and (w >= min(len(a), len(b)) or score > AM.bound(len(a), len(b), w))


def test_the_merge_keeps_its_consequences():
    rng = np.random.default_rng(32)
    for r in (1, 2, 3, 5):
        c = rand(rng, int(rng.integers(20, 120)))
        group = [c] + [mutated(rng, c, 0.08) or b"A" for _ in range(r - 1)]
        rows, scores = AM.msa(group, 300)
        assert len(rows) == r and len(scores) == r - 1
        assert all(any(row[x] != 45 for row in rows) for x in range(len(rows[0])))          # no all-gap column
        assert [row.replace(b"-", b"") for row in rows] == group                            # every row degapped is its instance
        for k in range(1, r):
            score, steps = AM.align(c, group[k], 300)
            assert MM.project(rows[0], rows[k]) == GM.rows(c, group[k], steps) and scores[k - 1] == score
