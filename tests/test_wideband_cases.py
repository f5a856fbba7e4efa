"""Preconditions of the tests of the global band class (tests/wideband_cases.py), without a GPU: what the CPU oracle makes of the crafted
FASTA pair, that its block and the crafted batches are beyond the limits of the LDS classes, and that both numpy models certify every
such pair at the first band -- so the device must end at band_w == 64 after one pass."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import galign_model as GM                          # noqa: E402
import gapopen_model as AM                         # noqa: E402
import wideband_cases as WC                        # noqa: E402

INSTANCES = WC.INSTANCES


@pytest.fixture(scope="module")
def oracle_built():
    from oracle import oracle as O
    O.build()


@pytest.mark.parametrize("ins", [5200, 12400])
def test_the_crafted_pair_is_one_block_beyond_the_limit(oracle_built, ins):
    (sa, ea), (sb, eb) = INSTANCES[ins]
    assert WC.oracle_blocks(ins) == [(1, 0, sa, ea), (1, 1, sb, eb)]
    n, m = ea - sa, eb - sb
    assert min(n, m) >= WC.MIN_BLOCK_SIZE and m - n >= ins - 1
    assert abs(m - n) + 129 == WC.offsets(n, m) > WC.LIMIT[WC.OPEN[ins]]
    assert WC.offsets(n, m) <= WC.LIMIT[0] or WC.OPEN[ins] == 0      # the 5200 case is within the limit without an opening cost


@pytest.mark.parametrize("ins", [5200, 12400])
def test_both_models_certify_the_crafted_block_at_the_first_band(ins):
    first, second = WC.crafted(ins)
    (sa, ea), (sb, eb) = INSTANCES[ins]
    a, b = first[sa:ea], second[sb:eb]
    assert GM.align_banded(a, b, WC.W0)[2]
    assert AM.align_banded(a, b, max(1, WC.OPEN[ins]), WC.W0)[2]


@pytest.mark.parametrize("o", [0, 1])
def test_both_models_certify_the_far_pairs_at_the_first_band(o):
    bt, far = WC.limit_batch(o)
    assert len(far) == (3 if o == 0 else 4) and len(bt.pairs) == len(far) + 1
    for k, (a, b) in enumerate(bt.pairs):
        assert (WC.offsets(len(a), len(b)) > WC.LIMIT[o]) == (k in far)
        assert GM.align_banded(a, b, WC.W0)[2] and AM.align_banded(a, b, o, WC.W0)[2], k
    quads = [(WC.offsets(len(a), len(b)) + 7) // 8 for a, b in bt.pairs]
    assert max(quads) > 1024                                    # more quads of cells a diagonal than a workgroup has lanes


def test_the_shapes_of_the_forced_batch():
    pairs, revs = WC.shape_pairs()
    lens = {(len(a), len(b)) for a, b in pairs}
    assert len(pairs) == 200 and max(max(x) for x in lens) <= 400
    assert {(n, m) for n in (1, 2, 7, 8, 9) for m in (1, 2, 7, 8, 9)} <= lens and {(n, 300) for n in (1, 2, 7, 8, 9)} <= lens
    assert (0, 9) in lens and (9, 0) in lens and set(revs) == {(False, False), (True, False), (False, True), (True, True)}
    need = [GM.required_w(a, b) for a, b in pairs if a and b]
    assert need.count(64) >= 50 and max(need) >= 256            # certified at once; doubled at least twice
    assert any(w == min(len(a), len(b)) and w > 64 for w, (a, b) in zip(need, [p for p in pairs if p[0] and p[1]]))      # the full-matrix end
