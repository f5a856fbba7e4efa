"""k_boundary_align (csrc/boundary_align.hip) at the edges of its 16-bit scores, of the 11-bit fields of its maximum key, of its one-wave
trace walk and of its code packing, against the numpy model (tests/boundary_model.py: align): all four coordinates equal.

Batch     the run, score, key-field, far-tie, wide and packing cases of tests/boundary_cases.py in one batch and in the reverse order:
          a job's result depends neither on its neighbours nor on where its codes lie.
Sweeps    every shape up to 16 x 16 and 1000 random pairs over `AC` in one launch each, and the first interleaved with empty strings.
Chunking  packing shapes under a cap of 1 KB and of 2 KB, in an order that fills launches to the last byte; one alignment of exactly the
          cap runs alone, one of a byte more (256 after the rounding) is refused.
History   the grow-only code and descriptor buffers hold what earlier batches left: results do not depend on it.

tests/test_boundary_cases.py holds the preconditions: which scores, start cells, ties and code bytes these cases have."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_cases as BC                        # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def finder():
    from sibelia_amd import BlockFinder
    bf = BlockFinder([b"ACGT" * 8], device=0)
    yield bf
    bf.close()


def cases_of(families):
    """-> (cases, the model's rows) of the families, in order"""
    return [c for f in families for c in BC.FAMILIES[f]()], [r for f in families for r in BC.model(f)]


def check(bf, cases, want):
    """one align_windows batch; every row equals the model's and the geometry the case claims"""
    got = bf.align_windows([(a, b) for _, a, b, _ in cases])
    assert got.shape == (len(cases), 4)
    wrong = [(name, tuple(int(x) for x in g), w) for (name, _, _, _), g, w in zip(cases, got, want) if tuple(int(x) for x in g) != w]
    assert not wrong, (len(wrong), wrong[:8])
    assert all(geometry in (None, w) for (_, _, _, geometry), w in zip(cases, want))
    return got


@pytest.mark.parametrize("family", BC.GEOMETRY)
def test_each_family_alone(finder, family):
    cases, want = cases_of([family])
    check(finder, cases, want)
    st = finder.correct_stats()
    assert st["alignments"] == len(cases) and st["launches"] == 1 and st["cells"] == sum(len(a) * len(b) for _, a, b, _ in cases)


def test_one_batch_and_its_reverse(finder):
    cases, want = cases_of(BC.GEOMETRY)
    first = check(finder, cases, want)
    assert finder.correct_stats()["launches"] == 1 and finder.correct_stats()["alignments"] == len(cases)
    second = check(finder, cases[::-1], want[::-1])
    assert (first == second[::-1]).all()
    # ... and with every job at another code_off than in either: the wide cases first, the rest rotated
    order = sorted(range(len(cases)), key=lambda k: (not cases[k][0].startswith("wide"), (k * 37) % len(cases)))
    check(finder, [cases[k] for k in order], [want[k] for k in order])


def test_the_16_x_16_sweep_in_one_launch(finder):
    cases, want = cases_of(["sweep"])
    check(finder, cases, want)
    st = finder.correct_stats()
    assert st["launches"] == 1 and st["alignments"] == 256 and st["cells"] == 136 * 136


def test_1000_random_pairs_in_one_launch(finder):
    cases, want = cases_of(["random"])
    check(finder, cases, want)
    st = finder.correct_stats()
    assert st["launches"] == 1 and st["alignments"] == 1000


def test_the_sweep_interleaved_with_empty_strings(finder):
    cases, want = cases_of(["sweep"])
    mixed, rows = [], []
    for k, (case, w) in enumerate(zip(cases, want)):
        name, a, b, _ = case
        empty = [("empty-a", b"", b, None), ("empty-b", a, b"", None), ("empty-both", b"", b"", None)][k % 3]
        if k % 2:
            mixed.append(empty); rows.append((0, len(empty[1]), 0, len(empty[2])))
        mixed.append(case); rows.append(w)
        if not k % 2:
            mixed.append(empty); rows.append((0, len(empty[1]), 0, len(empty[2])))
    # sweep, empty, empty, sweep, sweep, empty, ...: an empty job first in its pair, last in it, and two in a row
    assert len(mixed) == 512 and [c[0][:5] for c in mixed[:6]] == ["sweep", "empty", "empty", "sweep", "sweep", "empty"]
    assert {c[0] for c in mixed if c[0].startswith("empty")} == {"empty-a", "empty-b", "empty-both"}
    check(finder, mixed, rows)
    st = finder.correct_stats()
    assert st["launches"] == 1 and st["alignments"] == 256 and st["cells"] == 136 * 136      # the empty ones are no alignments
    check(finder, [c for c in mixed if c[0].startswith("empty")], [r for c, r in zip(mixed, rows) if c[0].startswith("empty")])
    assert finder.correct_stats()["launches"] == 0 and finder.correct_stats()["alignments"] == 0


# the packing shapes in an order whose sums of rounded() land on the cap: 256 + 768 | 512 + 512 | 768 + 256 | 1024 | 1024 | 512 + 256
# | 768 | 768 | 512 + 512 | 1024 | 1024 | 256 x 4 under 1 KB (tests/test_boundary_cases.py has the bytes of each)
ORDER_1K = [(5, 128), (9, 171), (13, 128), (1, 257), (13, 192), (128, 5), (29, 128), (1, 769), (128, 13), (5, 128), (171, 9), (192, 13),
            (257, 1), (128, 13), (128, 29), (769, 1), (128, 5), (5, 128), (128, 5), (5, 128)]
# ... and with the shapes of 1280 and 2048 bytes under 2 KB: 1280 + 768 | 2048 | 1280 + 512 + 256 | 2048 | 1024 + 1024 | 768 + 1280 | the rest
ORDER_2K = [(1, 1025), (9, 171), (1, 2047), (1025, 1), (13, 128), (5, 128), (2047, 2), (29, 128), (1, 769), (13, 192), (1, 1025), (2, 2047),
            (2047, 1)] + ORDER_1K


def chunked(finder, monkeypatch, kb, order, alone, refused, refused_bytes):
    from sibelia_amd.api import SibeliaError
    cap = kb << 10
    monkeypatch.setenv("SBL_TEST_ALIGN_CAP_KB", str(kb))       # the cap on the trace codes is read when a batch starts
    by_name = dict(zip((c[0] for c in BC.packing_cases()), zip(BC.packing_cases(), BC.model("packing"))))
    cases = [by_name["pack-%dx%d" % s][0] for s in order]
    want = [by_name["pack-%dx%d" % s][1] for s in order]
    launches, full = BC.greedy_launches(order, cap)
    assert full >= 4 and launches < len(order)                 # several prefix sums land exactly on the cap
    check(finder, cases, want)
    st = finder.correct_stats()
    assert st["launches"] == launches and st["alignments"] == len(order), (st, launches)
    check(finder, cases[::-1], want[::-1])
    assert finder.correct_stats()["launches"] == BC.greedy_launches(order[::-1], cap)[0]
    for shape in alone:                                        # exactly the cap: alone in its launch, and it succeeds
        assert BC.rounded(*shape) == cap
        case, w = by_name["pack-%dx%d" % shape]
        check(finder, [case, case], [w, w])
        assert finder.correct_stats()["launches"] == 2
        check(finder, [case], [w])
        assert finder.correct_stats()["launches"] == 1
    assert cap < BC.rounded(*refused) == refused_bytes
    case, w = by_name["pack-%dx%d" % refused]
    with pytest.raises(SibeliaError, match=r"out of memory.*\(%d bytes\) exceed the cap of %d bytes" % (refused_bytes, cap)):
        finder.align_windows([cases[0][1:3], case[1:3]])
    check(finder, cases[:3], want[:3])                          # the context stays usable under the cap ...
    monkeypatch.delenv("SBL_TEST_ALIGN_CAP_KB")
    check(finder, cases + [case], want + [w])                  # ... and without it, where one launch takes them all
    assert finder.correct_stats()["launches"] == 1


def test_chunking_at_equality_under_1_kb(finder, monkeypatch):
    assert set(ORDER_1K) == {s for n, m in BC.PACKING for s in ((n, m), (m, n))} - {(1, 1025), (1025, 1)}
    chunked(finder, monkeypatch, 1, ORDER_1K, [(29, 128), (128, 29), (1, 769)], (1, 1025), 1280)


def test_chunking_at_equality_under_2_kb(finder, monkeypatch):
    chunked(finder, monkeypatch, 2, ORDER_2K, [(2, 2047), (2047, 2), (1, 2047)], (3, 2047), 2304)


def test_results_do_not_depend_on_what_ran_before(finder):
    wide = [c for c in BC.score_cases() if c[0] == "score-2047"]
    assert wide[0][3] == (0, 2047, 0, 2047)
    sweep, want = cases_of(["sweep"])
    check(finder, wide, [wide[0][3]])
    check(finder, sweep, want)                                 # in buffers that hold the wide pair's codes and descriptor
    check(finder, wide, [wide[0][3]])
    check(finder, sweep[::-1], want[::-1])
