"""tests/parsimony_model.py against DESIGN.md 0.14 without a device: expectations written by hand, the predicates of the crafted cases,
the minimum over all assignments by brute force, and the tree reader against sibelia_amd/tree.py's writer."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parsimony_cases as PC                       # noqa: E402
import parsimony_model as PM                       # noqa: E402

A, C, T, G = 0, 1, 2, 3


def test_the_codes_are_those_of_the_packed_sites():
    assert [PM.code(ch) for ch in b"ACTG"] == [0, 1, 2, 3] and PM.BASES == "ACTG"


def test_the_star_of_three_files_by_hand():
    c = PC.CASES["star_top_excludes_file_0"]
    counts, steps, least, changes = PC.model(c)
    # "ACG": the top node holds {C, G}, not file 0's A: two steps; it takes C, the lowest code, and G hangs off it
    # "TCA": {A, C} -> A (code 0): T -> A above it, A -> C to file 1.  "GAT": {A, T} -> A: G -> A, A -> T to file 2
    assert steps == [2, 2, 2] and least == [2, 2, 2]
    assert changes == [(0, 0, A, C), (0, 2, C, G), (1, 0, T, A), (1, 1, A, C), (2, 0, G, A), (2, 2, A, T)]
    assert counts[0][A][C] == counts[0][T][A] == counts[0][G][A] == 1 and sum(sum(r) for r in counts[0]) == 3
    assert sum(sum(r) for r in counts[1]) == 1 and sum(sum(r) for r in counts[2]) == 2


def test_the_tie_by_hand():
    c = PC.CASES["tie_lowest_code"]
    assert c["edges"] == [(4, 0), (4, 1), (5, 4), (5, 2), (5, 3)]
    counts, steps, least, changes = PC.model(c)
    # "AACT": node 5 holds {C, T} and its parent's A is not among them: C; so A -> C above node 5 (edge 2) and C -> T to file 3 (edge 4)
    # "AATC": the same sets, the same choice: A -> C on edge 2, C -> T to file 2 (edge 3).  "GGTC": G -> C on edge 2, C -> T on edge 3
    assert changes == [(0, 2, A, C), (0, 4, C, T), (1, 2, A, C), (1, 3, C, T), (2, 2, G, C), (2, 3, C, T)]
    assert steps == least == [2, 2, 2]


def test_a_homoplasic_site_by_hand():
    # files 0 and 2 hold A, 1 and 3 hold C on the tree (0, 1 | 2, 3): two bases, two steps.  Node 5 holds {A, C}, the top node 4 only
    # file 1's C: A -> C above the top node (edge 0), node 5 keeps C and file 2 turns back, C -> A (edge 3)
    counts, steps, least, changes = PM.fitch([b"A", b"C", b"A", b"C"], None, PC.CASES["tie_lowest_code"]["edges"])
    assert (steps, least) == ([2], [1]) and changes == [(0, 0, A, C), (0, 3, C, A)]


def test_an_absent_leaf_by_hand():
    c = PC.CASES["one_absent_leaf"]
    _, steps, least, changes = PC.model(c)
    assert c["edges"] == [(5, 0), (5, 1), (6, 5), (6, 2), (7, 6), (7, 3), (7, 4)]
    # "AC-CA": node 7 holds {A, C}, node 6 -- file 2 is absent -- the same, the top node 5 only C: not file 0's A.  Two steps for two bases:
    # A -> C above the top node (edge 0) and C -> A to file 4 (edge 6); the absent file takes its parent's C
    assert (steps[0], least[0]) == (2, 1) and [x for x in changes if x[0] == 0] == [(0, 0, A, C), (0, 6, C, A)]
    assert all(e != 3 for _, e, _, _ in changes)                                 # edge 3 leads to file 2


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_every_case_is_what_its_name_says(name):
    c = PC.CASES[name]
    assert c["hits"](c), name
    counts, steps, least, changes = PC.model(c)
    assert sum(x for e in counts for r in e for x in r) == sum(steps) == len(changes)
    assert all(a >= b for a, b in zip(steps, least)) and len(steps) == len(least) == len(c["columns"])
    assert changes == sorted(changes) and all(a != b for _, _, a, b in changes)
    assert all(e[k][k] == 0 for e in counts for k in range(4))


def test_the_cases_cover_the_word_edges_and_the_site_counts():
    assert {c["n"] for c in PC.CASES.values()} >= set(PC.LEAF_COUNTS) == {3, 4, 5, 32, 33, 64}
    assert {len(c["columns"]) for c in PC.CASES.values()} >= set(PC.SITE_COUNTS) == {0, 1, 63, 64, 65, 255, 256, 257}
    assert [n for n, c in PC.CASES.items() if not c["device"]] == ["top_children_absent"]
    # leaf 0 next to the first-made and to the last-made internal node
    for n in PC.LEAF_COUNTS[1:]:
        assert PM.rooted(PC.caterpillar(n), n)[0] == n and PM.rooted(PC.caterpillar(n, first=False), n)[0] == 2 * n - 3


def random_tree(rng, n):
    return PC.joined(n, lambda live, s: [int(x) for x in rng.choice(len(live), 2, replace=False)])


def test_steps_are_the_minimum_and_the_changes_reach_it():
    rng = np.random.default_rng(1414)
    done = 0
    for absent in (0.0, 0.3):
        for _ in range(100):
            n = int(rng.integers(3, 8))
            edges = PC.permuted(random_tree(rng, n), n, int(rng.integers(1 << 30)))
            col = [b"ACGT"[int(x)] for x in rng.integers(0, 4, n)]
            held = [rng.random() >= absent for _ in range(n)]
            counts, steps, least, changes = PM.fitch([bytes([x]) for x in col], [[h] for h in held], edges)
            best = PM.brute_steps(col, held, edges)
            assert steps == [best] and len(changes) == best and steps[0] >= least[0]
            for root in range(n):                                                # the number of steps does not depend on the leaf the tree is read from
                assert PM.site_steps(col, held, edges, root) == best
            done += 1
    assert done == 200


def test_what_is_not_a_binary_tree_is_refused():
    good = PC.CASES["tie_lowest_code"]["edges"]
    PM.rooted(good, 4)
    for edges, n in ((good, 3), (good[:-1], 4), (good[:-1] + [(5, 6)], 4), (good[:-1] + [(5, 2)], 4), ([(4, 0), (4, 1), (4, 5), (5, 5), (2, 3)], 4),
                     ([(4, 1), (4, 2), (4, 5), (5, 3), (5, 3)], 4), ([(1, 0), (4, 2), (4, 3), (4, 5), (5, 5)], 4), ([(2, 0), (2, 1)], 2)):
        with pytest.raises(PM.Refused):
            PM.rooted(edges, n)
    with pytest.raises(PM.TooLarge):
        PM.rooted(PC.caterpillar(65), 65)


def test_the_reader_reads_what_the_writer_writes():
    from sibelia_amd import tree
    rng = np.random.default_rng(7)
    for n in (3, 4, 7, 12):
        D = rng.random((n, n))
        D = D + D.T
        np.fill_diagonal(D, 0)
        t = tree.neighbour_joining(D)
        names = ["f%d.fa" % k for k in range(n)]
        held = {b: int(rng.integers(0, 11)) for b in tree.bipartitions(t)}
        for text in (tree.newick(t, names), tree.newick(t, names, held, 10)):
            got_names, edges, labels = PM.read_newick(text)
            assert sorted(got_names) == sorted(names) and got_names[0] == names[0] and len(edges) == 2 * n - 3
            assert PM.write_newick(got_names, edges, labels, lambda v, e, length: length) == text
            PM.rooted([(names.index(got_names[u]) if u < n else u, names.index(got_names[v]) if v < n else v) for u, v, _ in edges], n)
        order = tree.branches(t)
        assert [v for v, _, _, _ in order][0] == 0 and sorted(e for _, e, _, _ in order) == list(range(2 * n - 3))
