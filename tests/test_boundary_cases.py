"""Preconditions of the boundary alignment's edge cases (tests/boundary_cases.py), without a GPU, on the numpy model alone
(tests/boundary_model.py: align, pinned to the reference program by tests/test_boundary_model.py): every case has the geometry it was
built for, the score cases pass 2^15 and 3 * 2^14, the key-field cases start at 2046, the far ties really are ties and their start is
the largest j, then the largest i, and the packing shapes have the code bytes they are named for.  So on the device
(tests/test_gpu_boundary_edges.py) a narrowed score, a swapped key field, a wrong count in a walk window or a short count of code bytes
changes a result."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_cases as BC                        # noqa: E402
import boundary_model as BM                        # noqa: E402


ENDINGS_AT_ZERO = ("sub", "igap", "jgap", "stop", "enda", "endb")      # the run cases whose start cell has ilo = 0


@pytest.mark.parametrize("family", BC.GEOMETRY)
def test_every_claimed_geometry_is_the_models(family):
    cases, kept = BC.FAMILIES[family](), BC.model(family)
    assert len(cases) == len(kept) and len({name for name, _, _, _ in cases}) == len(cases)
    claimed = 0
    for (name, a, b, geometry), got in zip(cases, kept):
        assert 1 <= len(a) <= BC.MAXLEN and 1 <= len(b) <= BC.MAXLEN, name
        if geometry is not None:
            assert got == geometry, name
            claimed += 1
    assert claimed == (len(cases) if family != "wide" else len(BC.WIDE))      # only the related wide pairs have none


def test_run_cases_cover_every_length_ending_and_position_in_a_code_byte():
    cases = BC.run_cases()
    assert len(cases) == 6 * 7 * 4
    assert [name for name, _, _, _ in cases] == ["run-%s-%d-%d" % (e, L, s) for L in (63, 64, 65, 127, 128, 129)
                                                 for e in ("sub", "igap", "jgap", "stop", "enda", "endb", "deep") for s in range(4)]
    for name, a, b, (ab, ae, bb, be) in cases:
        _, ending, L, s = name.split("-")
        L, s, n, m = int(L), int(s), len(a), len(b)
        assert bb == 0 and a[ab:ab + L] == b[:L], name                     # the run of L matches comes first ...
        # ... and ends as the name says: in a mismatch with the alignment going on in one of three ways, in a zero cell, or at an end
        if ending in ("stop", "enda", "endb"):
            assert (ae, be) == (ab + L, L), name
            assert {"stop": ae < n and be < m and a[ae] != b[be], "enda": ae == n and be < m, "endb": ae < n and be == m}[ending], name
        else:
            assert (ae, be) == (n, m) and a[ab + L] != b[L] and (n - ab) - m == {"sub": 0, "igap": 1, "jgap": -1, "deep": 1}[ending], name
        # the start cell: its place in its code byte, and which half of the matrix it is in
        ilo = max(0, ab + bb - (m - 1))
        assert ab == s + (BC.DEEP if ending == "deep" else 0) and (ilo > 0) == (ending == "deep"), name
        # the leading bases do not extend the alignment: without them the result is the same, moved
        if s:
            same = BC.model("run")[[c[0] for c in cases].index("run-%s-%d-0" % (ending, L))]
            assert (ab - s, ae - s, bb, be) == same, name
    # over the four shifts the start cell takes every 2-bit position of a byte where ilo = 0 ...
    for ending in ENDINGS_AT_ZERO:
        for L in BC.RUN_L:
            assert {ab % BC.CELLS for name, _, _, (ab, _, _, _) in cases if name.startswith("run-%s-%d-" % (ending, L))} == {0, 1, 2, 3}, (ending, L)
    # ... and where ilo > 0 the position is m - 1 - j whatever i is: there every diagonal step of the trace moves it by one
    for name, a, b, (ab, _, bb, _) in cases:
        if "deep" in name:
            assert ab - max(0, ab + bb - (len(b) - 1)) == len(b) - 1, name


def test_score_cases_pass_15_bits_and_three_quarters_of_16():
    cases = BC.score_cases()
    scores = {name: BC.max_score(a, b) for name, a, b, _ in cases}
    assert scores == BC.SCORES and [name for name, _, _, _ in cases] == list(BC.SCORES)
    assert [scores[name] for name in list(BC.SCORES)[:4]] == [32750, 32775, 51175, 51075]
    assert max(scores.values()) == BC.MAXLEN * BM.MATCH < 1 << 16
    assert sum(s < 32768 for s in scores.values()) == 1 and sum(s > 49152 for s in scores.values()) == len(scores) - 2
    name, a, b, _ = cases[3]
    mid = BC.MAXLEN // 2
    assert len(a) == len(b) == BC.MAXLEN and [k for k in range(BC.MAXLEN) if a[k] != b[k]] == [mid]
    # With ONE mismatch the matrix is symmetric about the main diagonal and nothing beside it reaches it: the scores are plain sums.
    # In the middle the score beside the mismatch is still below 2^15 -- the matrix is filled from the ends -- so a score type that
    # breaks at 2^15 only when the penalty is taken off it, or when it is compared, passes that case.  The early ones are for that.
    assert BM.MATCH * (BC.MAXLEN - 1 - mid) == 25575 < 32768
    for (name, a, b, _), p in zip(cases[4:6], BC.EARLY):
        K = BC.matrix(a, b)
        assert [k for k in range(BC.MAXLEN) if a[k] != b[k]] == [p], name
        assert int(K[2 * p + 2, p + 1]) == BM.MATCH * (BC.MAXLEN - 1 - p) >= 32768 and int(K[2 * p, p]) == int(K[2 * p + 2, p + 1]) - BM.PENALTY, name
    assert BM.MATCH * (BC.MAXLEN - 1 - BC.EARLY[1]) == 32775 and BM.MATCH * (BC.MAXLEN - 1 - (BC.EARLY[1] + 1)) < 32768      # the last such p
    for name, a, b, _ in cases[6:]:
        p, (long, short) = BC.EARLY[0], (a, b) if len(a) > len(b) else (b, a)
        assert len(long) == BC.MAXLEN and long[:p] + long[p + 1:] == short, name
    assert BC.max_score(b"A", b"A") == 25 and BC.max_score(b"", b"A") == 0 and BC.max_score(b"A", b"C") == 0


def test_key_field_cases_start_at_2046():
    starts = [(got[0], got[2]) for got in BC.model("key")]
    assert starts == [(2046, 2046), (0, 2046), (2046, 0)]
    for name, a, b, _ in BC.key_cases():
        assert BC.maxima(a, b) == (25, [(len(a) - 1 if a[-1:] == b"A" else 0, len(b) - 1 if b[-1:] == b"A" else 0)]), name


def test_far_ties_are_ties_and_start_at_the_largest_j_then_the_largest_i():
    waves, diagonals = {}, {}
    for (name, a, b, geometry), got in zip(BC.tie_cases(), BC.model("tie")):
        best, at = BC.maxima(a, b)
        assert best == BM.MATCH * BC.WORD and len(at) >= 2, name
        start = max(at, key=lambda ij: (ij[1], ij[0]))
        assert (got[0], got[2]) == start == (geometry[0], geometry[2]), name
        assert (got[1] - got[0], got[3] - got[2]) == (BC.WORD, BC.WORD), name
        rest = [ij for ij in at if ij != start]
        assert min(abs(i - start[0]) + abs(j - start[1]) for i, j in rest) >= BC.NEAR, name      # far apart
        w = BC.wave_of(*start, len(a), len(b))
        waves[name] = (w, [BC.wave_of(i, j, len(a), len(b)) for i, j in rest])
        diagonals[name] = (sum(start), sorted({i + j for i, j in at}))
    assert [len(BC.maxima(a, b)[1]) for _, a, b, _ in BC.tie_cases()] == [2, 2, 4, 2, 2, 4, 2, 2]
    # the three of the issue: start i = 1920, start j = 1920, and (1920, 1520)
    assert [g[:1] + g[2:3] for g in BC.model("tie")[:3]] == [(1920, 0), (0, 1920), (1920, 1520)]
    # two maxima on ONE diagonal: there the winner, with the larger j, is in the lower lane
    for name in ("tie-diag", "tie-diag-t"):
        assert diagonals[name] == (1920, [1920]) and waves[name] == (0, [7]), name
    assert diagonals["tie-diag-ij"][1] == [0, 1920, 3840]
    # ... both orders of wave: the winner's wave below another maximum's, and above
    assert waves["tie-diag"][0] < max(waves["tie-diag"][1]) and waves["tie-ij"] == (0, [0, 0, 6])
    assert waves["tie-wave-up"] == (7, [0])
    # the first two of the issue live in one wave (a diagonal of 20 cells is 5 lanes): the key alone decides them
    assert waves["tie-i"] == (0, [0]) and waves["tie-j"] == (0, [0])


def test_turn_cases_stand_on_equal_gap_neighbours():
    cases = BC.turn_cases()
    assert len(cases) == 2 * len(BC.TURN_K) * len(BC.TURN_LEAD) and {len(a) % 4 for _, a, _, _ in cases} == {0, 1, 2, 3}
    for (name, a, b, geometry), got in zip(cases, BC.model("turn")):
        k, p = int(name.split("-")[1]), int(name.split("-")[2])
        K = BC.matrix(a, b)
        M = lambda i, j: int(K[i + j, i])                                   # noqa: E731
        assert a[:p] == b[:p] and a[p] != b[p] and BC.maxima(a, b)[1] == [(0, 0)], name      # the trace comes down the diagonal to (p, p)
        v, h, g = M(p + 1, p), M(p, p + 1), M(p + 1, p + 1)
        assert v == h == BM.MATCH * (2 * k - 1) > g and v > BM.PENALTY, name
        assert got == geometry == (0, len(a), 0, len(b) - 1), name          # the step taken was i: with j it would end at (n - 1, m)


def test_code_bytes_of_the_packing_shapes():
    assert BC.PACKING == {(5, 128): 256, (1, 257): 257, (13, 128): 512, (9, 171): 513, (13, 192): 768, (1, 769): 769, (29, 128): 1024, (1, 1025): 1025}
    for table in (BC.PACKING, BC.PACKING_2K):
        for (n, m), want in table.items():
            assert BC.code_bytes(n, m) == BC.code_bytes(m, n) == want, (n, m)
            assert BC.rounded(n, m) == BC.rounded(m, n) == -(-want // 256) * 256, (n, m)
    assert [BC.rounded(*s) for s in BC.PACKING_2K] == [2048, 2048, 2304]
    assert (BC.code_bytes(1, 1), BC.code_bytes(4, 4), BC.code_bytes(5, 5), BC.code_bytes(2, 3)) == (1, 7, 10, 4)      # by hand
    assert BC.code_bytes(BC.MAXLEN, BC.MAXLEN) == 2 * sum(-(-k // 4) for k in range(1, BC.MAXLEN)) + 512
    names = [name for name, _, _, _ in BC.packing_cases()]
    assert names == [x for n, m in list(BC.PACKING) + list(BC.PACKING_2K) for x in ("pack-%dx%d" % (n, m), "pack-%dx%d" % (m, n))]
    for name, a, b, (ab, ae, bb, be) in BC.packing_cases():
        assert (ae, be) == (len(a), len(b)) and a[0] != b[0], name            # the trace ends in the last cell; the first cell is no match


def test_wide_shapes_cover_the_residues_and_the_three_orders():
    assert {min(n, m) % 4 for n, m in BC.WIDE if n == m} == {0, 1, 2, 3}
    assert {(n > m) - (n < m) for n, m in BC.WIDE} == {-1, 0, 1}
    assert {-(-min(n, m) // 4) for n, m in BC.WIDE if n == m} == {511, 512}       # code bytes of the longest diagonal; 512: one per lane
    assert [(len(a), len(b)) for _, a, b, _ in BC.wide_cases()] == [s for s in BC.WIDE for _ in range(2)]


def test_the_sweeps_are_complete_and_dense_in_distinct_results():
    sweep = BC.sweep_cases()
    assert [(len(a), len(b)) for _, a, b, _ in sweep] == [(n, m) for n in range(1, 17) for m in range(1, 17)] and len(sweep) == 256
    rnd = BC.random_cases()
    assert len(rnd) == 1000 and all(1 <= len(a) <= 40 and 1 <= len(b) <= 40 and set(a + b) <= set(b"AC") for _, a, b, _ in rnd)
    assert {len(a) for _, a, _, _ in rnd} == set(range(1, 41)) == {len(b) for _, _, b, _ in rnd}
    assert len(set(BC.model("random"))) >= 500                              # a condition on the seed, not a measurement


def test_greedy_launches_counts_the_launches_filled_to_the_last_byte():
    assert BC.greedy_launches([(5, 128)] * 4, 1024) == (1, 1)
    assert BC.greedy_launches([(5, 128)] * 5, 1024) == (2, 1)
    assert BC.greedy_launches([(9, 171), (1, 257)], 1024) == (2, 0)
    assert BC.greedy_launches([(29, 128), (128, 29)], 1024) == (2, 2)
    with pytest.raises(AssertionError):
        BC.greedy_launches([(1, 1025)], 1024)
