"""sbl_align_pairs (csrc/block_align.hip) -- the batched banded global alignment behind --maf / --variants -- against the numpy model
(tests/galign_model.py): status, score, runs and the two device-spelled rows must be equal to the UNBANDED model."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from galign_cases import Batch, mutated, rand      # noqa: E402

pytestmark = pytest.mark.gpu


def edge_pairs():
    rng = np.random.default_rng(21)
    x = rand(rng, 1000)
    pairs = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b""), (b"A", b"A"), (b"A", b"C"), (b"A", b"ACGT"), (b"ACGT", b"T")]
    pairs += [(x[:n], x[:n]) for n in (1, 63, 64, 65, 1000)]
    for at in (0, 500, 999):                                   # one substitution: first, middle, last position
        pairs.append((x, x[:at] + (b"A" if x[at:at + 1] != b"A" else b"C") + x[at + 1:]))
    pairs += [(x, x[3:]), (x[3:], x), (x, x[:-5]), (x[:-5], x), (x[:300], b"GG" + x[:300] + b"TTT")]      # an indel at either end
    return pairs


def test_edge_shapes():
    pairs = edge_pairs()
    b = Batch(pairs)
    got, st = b.run(0)
    b.check(got, b.want(0, linear=True))
    assert st["pairs"] == len(pairs) and st["skipped"] == 0 and st["launches"] >= 1 and st["cells"] > 0 and st["kernel_ms"] > 0 and st["spell_ms"] > 0


def test_length_differences_and_homopolymers():
    rng = np.random.default_rng(22)
    pairs = []
    for n, diff in ((200, 1), (700, 70), (1200, 300), (1500, 300)):
        a = rand(rng, n)
        cut = n // 3
        pairs += [(a, a[:cut] + a[cut + diff:]), (a[:cut] + a[cut + diff:], a)]      # |m - n| = diff, either way round
    pairs += [(b"A" * 70, b"A" * 70), (b"A" * 33, b"A" * 90), (b"A" * 90, b"A" * 33), (b"AC" * 40, b"AC" * 33), (b"T" * 600, b"T" * 590),
              (b"GATTACA" + b"T" * 200 + b"GATTACA", b"GATTACA" + b"T" * 180 + b"GATTACA")]
    b = Batch(pairs)
    got, _ = b.run(0)
    b.check(got, b.want(0, linear=True))
    assert got[8].runs == [("=", 70)] and got[9].runs == [("=", 33), ("D", 57)] and got[10].runs == [("=", 33), ("I", 57)]      # diagonal steps first


def test_reverse_ranges_and_bytes_outside_acgt():
    rng = np.random.default_rng(23)
    a = rand(rng, 500)
    b = mutated(rng, a)
    n1 = a[:100] + b"N" * 20 + a[120:]
    n2 = b[:90] + b"NNNNRYKM" + b[98:]
    pairs = [(a, b)] * 4 + [(n1, n2)] * 4 + [(rand(rng, 200, b"ACGTN"), rand(rng, 190, b"ACGTN")), (b"NNNN", b"TNNNNT")]
    revs = [(False, False), (True, False), (False, True), (True, True)] * 2 + [(True, False), (False, False)]
    bt = Batch(pairs, revs)
    got, _ = bt.run(0)
    bt.check(got, bt.want(0, linear=True))
    assert got[0].runs == got[1].runs == got[2].runs == got[3].runs


def random_pairs(seed=24, count=200):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(count):
        a = rand(rng, int(rng.integers(1, 401)))
        u = rng.random()
        b = (mutated(rng, a, 0.06, 30) or b"A")[:400] if u < 0.85 else rand(rng, int(rng.integers(1, 401)))
        pairs.append((a, b))
    return pairs


@pytest.fixture(scope="module")
def random_batch():
    return Batch(random_pairs())


def test_a_batch_of_random_pairs(random_batch):
    got, st = random_batch.run(0)
    random_batch.check(got, random_batch.want(0, linear=True))
    assert st["pairs"] == 200 and st["passes"] >= 200


def test_results_do_not_depend_on_the_first_band(random_batch, monkeypatch):
    passes = {}
    for w0 in (1, 8, 64):
        monkeypatch.setenv("SBL_TEST_GALIGN_W0", str(w0))
        got, st = random_batch.run(0)
        random_batch.check(got, random_batch.want(0, linear=True))
        passes[w0] = st["passes"]
    assert passes[1] > passes[8] > passes[64] >= 200, passes      # doubling ran


def tiny_pairs():
    """300 pairs of 0 .. 12 bases and their strands: empty and one-sided-empty pairs scattered through the batch, all four strand
    combinations, and stretches of at least three pairs in a row whose two rows together are shorter than 16 bytes -- among them pairs
    without any text -- so that the 16 bytes of one lane cross several groups and several empty ones; the text ends off a 16-byte boundary"""
    rng = np.random.default_rng(27)
    pairs, revs = [], []
    for k in range(300):
        n, m = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        if k % 20 < 5:                                          # five in a row of at most 3 + 3 bases: at most 12 bytes of text each
            n, m = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        a = rand(rng, n)
        b = rand(rng, m) if rng.random() < 0.4 else (mutated(rng, a, 0.2, 3)[:12] if n else b"")
        pairs.append((a, b))
        revs.append((bool(k & 1), bool(k & 2)))
    x = rand(rng, 7)
    for k, p in ((0, (b"", b"")), (21, (b"", b"")), (22, (x[:2], b"")), (23, (b"", b"")), (24, (b"", x[:3])), (77, (x, b"")), (150, (b"", x)), (151, (b"", b"")),
                 (299, (x[:5], x[:3] + x[4:5]))):
        pairs[k] = p
    return pairs, revs


def test_a_batch_of_tiny_pairs():
    pairs, revs = tiny_pairs()
    bt = Batch(pairs, revs)
    want = bt.want(0, linear=True)
    lens = [2 * len(rows[0]) for _, _, rows in want]
    assert len(pairs) == 300 and max(max(len(a), len(b)) for a, b in pairs) <= 12
    assert {(b"", b""), } <= set(pairs) and any(a and not b for a, b in pairs) and any(b and not a for a, b in pairs)
    assert set(revs) == {(False, False), (True, False), (False, True), (True, True)}
    assert lens[21] == lens[23] == 0 and sum(lens[20:25]) < 16               # one lane's 16 bytes: five groups, two of them without text
    assert any(all(0 < x < 16 for x in lens[k:k + 3]) for k in range(298))
    assert sum(lens) % 16 != 0 and lens[-1] > 0                               # the last pair ends off a 16-byte boundary
    got, st = bt.run(0)
    bt.check(got, bt.want(0, linear=True))
    assert st["pairs"] == 300 and st["skipped"] == 0


def test_wide_bands():
    """bands wider than one wave's registers: the score diagonal lives in LDS"""
    rng = np.random.default_rng(25)
    a = rand(rng, 3000)
    b = a[:1400] + rand(rng, 500) + a[1400:]                  # 3000 against 3500 bases: |m - n| + 2 w + 1 = 629 offsets at the first w
    c = a[:500] + rand(rng, 300) + a[500:2500] + a[2800:]     # equal lengths, the middle 300 off the main diagonal: w doubles up to 512
    u, v = b"A" * 2200, b"C" * 2200                           # nothing matches: -165000 clears U(w) = 55000 - 175 (w + 1) only at w = 2048 (4097 offsets)
    bt = Batch([(a, b), (b, a), (a, c), (u, v)])
    got, st = bt.run(0)
    bt.check(got, bt.want(0, linear=True))
    assert sum(n for op, n in got[0].runs if op == "D") == 500 and got[0].score == 3000 * 25 - 500 * 75
    assert got[2].passes == 4 and got[2].band_w == 512, (got[2].passes, got[2].band_w)
    assert got[3].band_w == 2048 and got[3].passes == 6 and got[3].runs == [("X", 2200)], (got[3].passes, got[3].band_w)


def test_the_per_alignment_cap_skips_long_pairs_only(monkeypatch):
    rng = np.random.default_rng(26)
    pairs, long_ones = [], set()
    for k in range(24):
        n = 900 if k % 4 == 1 else int(rng.integers(1, 60))      # 1800 diagonals * 17 bytes at w = 64: beyond 4 KiB
        a = rand(rng, n)
        pairs.append((a, mutated(rng, a) or b"C"))
        if n == 900:
            long_ones.add(k)
    bt = Batch(pairs)
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    got, st = bt.run(0)
    bt.check(got, bt.want(0, linear=True), skipped=long_ones)
    assert st["skipped"] == len(long_ones) == 6
    monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
    monkeypatch.setenv("SBL_TEST_GALIGN_TOTAL_KB", "64")         # a small total cap: several launches, the same results
    split, st2 = bt.run(0)
    monkeypatch.delenv("SBL_TEST_GALIGN_TOTAL_KB")
    single, st1 = bt.run(0)
    bt.check(single, bt.want(0, linear=True))
    assert st2["launches"] > st1["launches"] and st2["skipped"] == st1["skipped"] == 0
    for x, y in zip(split, single):
        assert (x.status, x.score, x.runs, x.row_a, x.row_b) == (y.status, y.score, y.runs, y.row_a, y.row_b)


def test_bad_arguments_leave_the_context_usable():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    bf = BlockFinder([b"ACGTACGTAC", b"ACGTTCGTAC"], device=0)
    try:
        for bad in [(0, 0, 11, False, 1, 0, 10, False), (0, 0, 10, False, 1, 5, 11, False), (0, 6, 5, False, 1, 0, 10, False),
                    (0, 0, 10, False, 1, 7, 3, False), (2, 0, 1, False, 1, 0, 1, False), (0, 0, 1, False, 2, 0, 1, False)]:
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.align_pairs([(0, 0, 10, False, 1, 0, 10, False), bad])
        got = bf.align_pairs([(0, 0, 10, False, 1, 0, 10, False)])
        assert got[0].status == 0 and got[0].runs == [("=", 4), ("X", 1), ("=", 5)] and got[0].score == 9 * 25 - 75
        assert (got[0].row_a, got[0].row_b) == (b"ACGTACGTAC", b"ACGTTCGTAC")
        assert bf.align_pairs([]) == []
    finally:
        bf.close()
