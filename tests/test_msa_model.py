"""The definition of the multiple alignment as tests/msa_model.py states it: the consequences the definition names, on
crafted and seeded random groups.  Device-free."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import galign_model as GM                          # noqa: E402
import msa_cases as MC                             # noqa: E402
import msa_model as MM                             # noqa: E402


def check_consequences(group):
    rows, scores = MM.msa(group)
    c, n = group[0], len(group[0])
    assert len(rows) == len(group) and len(scores) == len(group) - 1
    G = MM.merge(n, [MM.slots(MM.pair(c, s)[1]) for s in group[1:]])
    L = n + sum(G)
    assert all(len(r) == L for r in rows)                                       # L = n + sum G
    for col in range(L):
        assert any(r[col] != MM.GAP for r in rows), (group, col)                # no column is all gaps
    for s, r in zip(group, rows):
        assert r.replace(b"-", b"") == s                                        # every row, degapped, is its instance
    for s, r, score in zip(group[1:], rows[1:], scores):
        want_score, steps = GM.align(c, s)
        assert MM.project(rows[0], r) == GM.rows(c, s, steps) and score == want_score      # the pair projection
    return rows


@pytest.mark.parametrize("name", sorted(MC.CRAFTED))
def test_crafted_groups(name):
    group, want = MC.CRAFTED[name]
    rows = check_consequences(group)
    if want is not None:
        assert rows == want


def test_the_crafted_rows_hold_what_their_names_say():
    rows, _ = MM.msa(MC.CRAFTED["slots_0_and_n"][0])
    assert MM.slots(MM.pair(*MC.CRAFTED["slots_0_and_n"][0])[1]) == {0: 2, 8: 2}
    g = MC.CRAFTED["same_slot_different_lengths"][0]
    assert [MM.slots(MM.pair(g[0], s)[1]) for s in g[1:]] == [{4: 2}, {4: 3}, {}]
    g = MC.CRAFTED["i_run_spans_a_slot"][0]
    assert MM.pair(g[0], g[1])[1] == [("=", 4), ("I", 4), ("=", 4)] and MM.slots(MM.pair(g[0], g[2])[1]) == {6: 1}
    assert len(MM.msa(MC.CRAFTED["short_group"][0])[0][0]) < 16
    assert len(rows[0]) == 12


def test_seeded_random_groups():
    groups = MC.random_groups(seed=31, count=60, rmin=1, rmax=6, max_len=120, max_indel=20)
    assert {len(g) for g in groups} == {1, 2, 3, 4, 5, 6}
    assert any(len(g[0]) == 0 or any(len(s) == 0 for s in g[1:]) for g in groups)
    shared = 0
    for g in groups:
        check_consequences(g)
        slot_lists = [MM.slots(MM.pair(g[0], s)[1]) for s in g[1:]]
        shared += any(len({d.get(p, 0) for d in slot_lists}) > 1 for d in slot_lists for p in d) and len(g) > 2
    assert shared >= 10                                                         # slots that members fill to different lengths


def test_a_group_of_one_member_is_the_pair():
    """What lets one kernel spell both: the rows of msa([a, b]) are the two rows of the pair alignment of a and b, for the edge shapes of
    tests/test_gpu_block_align.py (empty and one-sided-empty pairs among them) and for 200 pairs of its random generator."""
    import test_gpu_block_align as BA
    pairs = BA.edge_pairs() + BA.random_pairs()
    assert len(pairs) == 221 and (b"", b"") in pairs and (b"", b"ACGT") in pairs and (b"ACGT", b"") in pairs
    for a, b in pairs:
        score, steps = GM.align(a, b)
        rows, scores = MM.msa([a, b])
        assert tuple(rows) == GM.rows(a, b, steps) and scores == [score], (a, b)


def test_the_banded_pair_equals_the_full_matrix():
    groups = MC.random_groups(seed=32, count=25, rmin=2, rmax=3, max_len=300, max_indel=20)
    groups.append([b"A" * 150, b"C" * 150])                                     # nothing matches: the band has to double up to the matrix
    groups.append([MC.rand(np.random.default_rng(33), 250)] * 2)
    groups[-1] = [groups[-1][0], groups[-1][0][:100] + b"ACGT" * 30 + groups[-1][0][100:]]      # 120 bases more: beyond the first band
    for g in groups:
        for s in g[1:]:
            for w0 in (1, 64):
                assert MM.pair_banded(g[0], s, w0) == MM.pair(g[0], s), (g[0], s, w0)


def test_block_groups_order_and_filter():
    blocks = [(2, 1, 50, 90), (-1, 0, 10, 40), (1, 1, 5, 35), (1, 0, 10, 40), (3, 0, 0, 30), (-2, 0, 60, 100), (2, 0, 200, 204), (1, 0, 10, 39)]
    assert MM.block_groups(blocks) == [(1, [(0, 10, 39, False), (0, 10, 40, False), (0, 10, 40, True), (1, 5, 35, False)]),
                                       (2, [(0, 60, 100, True), (0, 200, 204, False), (1, 50, 90, False)])]
    assert MM.block_groups(blocks, 30) == [(1, [(0, 10, 40, False), (0, 10, 40, True), (1, 5, 35, False)]), (2, [(0, 60, 100, True), (1, 50, 90, False)])]
    assert MM.block_groups(blocks, 41) == []


def test_maf_text_of_a_small_list():
    records = [b"GGACGTACGTCC", b"TTACGAACGTAA"]
    text = MM.maf(records, ["one", "two"], MM.block_groups([(1, 0, 2, 10), (-1, 1, 2, 10)]))
    rc = MM.reverse_complement(records[1][2:10])
    rows, _ = MM.msa([records[0][2:10], rc])
    assert text == b"##maf version=1\n\na\ns one 2 8 + 12 " + rows[0] + b"\ns two 2 8 - 12 " + rows[1] + b"\n\n"
