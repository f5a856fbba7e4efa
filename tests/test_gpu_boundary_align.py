"""sbl_align_windows (csrc/boundary_align.hip) -- the batched local alignment behind --correctboundaries -- against the numpy model
(tests/boundary_model.py, itself pinned to the reference program by tests/test_boundary_model.py): coordinates must be equal."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_model as BM                       # noqa: E402

pytestmark = pytest.mark.gpu


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def related(rng, n, m):
    """two strings that share a mutated stretch, so that the alignment has matches, mismatches and gaps"""
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


@pytest.fixture(scope="module")
def finder():
    from sibelia_amd import BlockFinder
    bf = BlockFinder([b"ACGT" * 8], device=0)
    yield bf
    bf.close()


def check(bf, pairs):
    got = bf.align_windows(pairs)
    for (a, b), g in zip(pairs, got):
        (ab, ae), (bb, be) = BM.align(a, b)
        assert tuple(int(x) for x in g) == (ab, ae, bb, be), (len(a), len(b), a[:60], b[:60])


def test_shapes(finder):
    rng = np.random.default_rng(11)
    pairs = [related(rng, n, m) for n, m in [(1, 1), (1, 5), (63, 64), (65, 64), (257, 255), (2047, 3), (3, 2047), (2047, 2047)]]
    pairs += [(b"A", b"A"), (b"A", b"C")]
    check(finder, pairs)
    assert finder.correct_stats()["alignments"] == len(pairs) and finder.correct_stats()["cells"] == sum(len(a) * len(b) for a, b in pairs)


def test_ties(finder):
    ac = b"AC" * 40
    check(finder, [(b"A" * 70, b"A" * 70), (b"A" * 33, b"A" * 90), (ac, ac[1:] + b"A"), (ac[:65], (b"CA" * 40)[:64]),
                   (b"ACGTTTTTTTTACGT", b"ACGT"), (b"ACGT", b"ACGTCCCCCCCACGT"), (b"GATTACA" + b"T" * 200 + b"GATTACA", b"CC" + b"GATTACA" + b"CC")])
    got = finder.align_windows([(b"ACGTTTTTTTTACGT", b"ACGT"), (b"ACGT", b"ACGTCCCCCCCACGT")])
    assert got.tolist() == [[11, 15, 0, 4], [0, 4, 11, 15]]                # equal maxima: largest j, then largest i


def test_no_common_character_and_empty_strings(finder):
    got = finder.align_windows([(b"A" * 100, b"C" * 37), (b"", b"ACGT"), (b"ACGT", b""), (b"ACAC", b"GTGT")])
    assert got.tolist() == [[0, 100, 0, 37], [0, 0, 0, 4], [0, 4, 0, 0], [0, 4, 0, 4]]


def test_bytes_are_compared_as_they_are(finder):
    rng = np.random.default_rng(5)
    a, b = related(rng, 300, 280)
    a = a[:100] + b"N" * 20 + a[120:]
    b = b[:90] + b"NNNNRYKM" + b[98:]
    check(finder, [(a, b), (b"NNNN", b"TNNNNT"), (rand(rng, 200, b"ACGTN"), rand(rng, 190, b"ACGTN"))])


def test_too_long_a_string_is_a_bad_argument(finder):
    from sibelia_amd.api import SibeliaError
    with pytest.raises(SibeliaError, match="bad argument|SBL_ALIGN_MAX_LEN"):
        finder.align_windows([(b"A" * 2048, b"A")])


def test_a_batch_that_crosses_chunk_boundaries(finder, monkeypatch):
    from sibelia_amd.api import SibeliaError
    monkeypatch.setenv("SBL_TEST_ALIGN_CAP_KB", "64")          # the cap on the trace codes is read when a batch starts
    rng = np.random.default_rng(3)
    pairs = [related(rng, int(rng.integers(1, 120)), int(rng.integers(1, 120))) for _ in range(300)]
    check(finder, pairs)
    st = finder.correct_stats()
    assert st["alignments"] == 300 and st["launches"] > 3, st
    with pytest.raises(SibeliaError, match="out of memory"):     # one alignment larger than the cap fails cleanly
        finder.align_windows([related(rng, 2047, 2047)])
    monkeypatch.delenv("SBL_TEST_ALIGN_CAP_KB")
    check(finder, pairs[:5])                                     # the context stays usable
