"""sibelia_amd/tree.py: distances, neighbour joining, bipartitions, bootstrap support and the canonical Newick text,
against known answers and against random additive trees, which neighbour joining recovers exactly.  Device-free."""
import re

import numpy as np
import pytest

from sibelia_amd import tree as T

TEXTBOOK = [[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]]


def names(n):
    return ["f%d" % i for i in range(n)]


def test_the_textbook_matrix():
    assert T.newick(T.neighbour_joining(TEXTBOOK), list("abcde")) == "(a:2.000000000,b:3.000000000,(c:4.000000000,(d:2.000000000,e:1.000000000):2.000000000):3.000000000);\n"
    p = [3, 0, 4, 1, 2]                                                          # the files in the order d a e b c
    D = np.array(TEXTBOOK)[np.ix_(p, p)]
    assert T.newick(T.neighbour_joining(D), list("daebc")) == "(d:2.000000000,((a:2.000000000,b:3.000000000):3.000000000,c:4.000000000):2.000000000,e:1.000000000);\n"


def random_tree(rng, n):
    """a random unrooted binary tree over n leaves whose edge lengths are multiples of 1/8 (0 excluded): edges and the leaf distances"""
    edges = [(n, 0, None), (n, 1, None), (n, 2, None)]
    nxt = n + 1
    for leaf in range(3, n):
        u, v, _ = edges.pop(int(rng.integers(0, len(edges))))
        edges += [(u, nxt, None), (nxt, v, None), (nxt, leaf, None)]
        nxt += 1
    edges = [(u, v, int(rng.integers(1, 41)) / 8) for u, v, _ in edges]
    adj = {}
    for u, v, ln in edges:
        adj.setdefault(u, []).append((v, ln))
        adj.setdefault(v, []).append((u, ln))
    D = np.zeros((n, n))
    for a in range(n):
        dist, stack = {a: 0.0}, [a]
        while stack:
            x = stack.pop()
            for y, ln in adj[x]:
                if y not in dist:
                    dist[y] = dist[x] + ln
                    stack.append(y)
        D[a] = [dist[b] for b in range(n)]
    return T.Tree(n, edges), D


def splits_with_lengths(tree):
    """bipartition -> length for the internal edges; leaf -> length for the others"""
    r = T._Rooted(tree)
    return {r.mask[v]: r.length[v] for v in r.internal}, {v: r.length[v] for v in range(tree.n)}


def test_additive_trees_come_back_exactly():
    rng = np.random.default_rng(5)
    for n in range(3, 21):
        for _ in range(5):
            want, D = random_tree(rng, n)
            got = T.neighbour_joining(D)
            gi, gl = splits_with_lengths(got)
            wi, wl = splits_with_lengths(want)
            assert set(gi) == set(wi) and len(gi) == n - 3
            assert all(abs(gi[b] - wi[b]) <= 1e-9 for b in wi) and all(abs(gl[v] - wl[v]) <= 1e-9 for v in range(n))
            # the text of the tree that was put in and of the one that came out: the same but for the last digits of a length
            a, b = T.newick(want, names(n)), T.newick(got, names(n))
            assert re.sub(r":[0-9.]+", ":", a) == re.sub(r":[0-9.]+", ":", b)
            assert all(abs(float(x) - float(y)) <= 1e-9 for x, y in zip(re.findall(r":([0-9.]+)", a), re.findall(r":([0-9.]+)", b)))


def test_the_bipartitions_do_not_depend_on_the_order_of_the_files():
    rng = np.random.default_rng(6)
    for n in (4, 5, 9, 16):
        _, D = random_tree(rng, n)
        base = {frozenset(i for i in range(n) if b >> i & 1) for b in T.bipartitions(T.neighbour_joining(D))}
        base = {s if 0 not in s else frozenset(range(n)) - s for s in base}
        for _ in range(4):
            p = [int(x) for x in rng.permutation(n)]                             # new file k is old file p[k]
            got = {frozenset(p[i] for i in range(n) if b >> i & 1) for b in T.bipartitions(T.neighbour_joining(D[np.ix_(p, p)]))}
            got = {s if 0 not in s else frozenset(range(n)) - s for s in got}
            assert got == base and len(base) == n - 3


def test_three_files():
    t = T.neighbour_joining([[0, 3, 4], [3, 0, 5], [4, 5, 0]])
    assert T.bipartitions(t) == [] and T.support(t, [t, t]) == {}
    assert T.newick(t, names(3)) == "(f0:1.000000000,f1:2.000000000,f2:3.000000000);\n"
    assert T.newick(t, names(3), {}, 10) == "(f0:1.000000000,f1:2.000000000,f2:3.000000000);\n"
    # the three-point formula gives -1 for file 0: set to 0, the others stay
    assert T.newick(T.neighbour_joining([[0, 1, 1], [1, 0, 4], [1, 4, 0]]), names(3)) == "(f0:0.000000000,f1:2.000000000,f2:2.000000000);\n"
    for bad in ([[0, 1], [1, 0]], [[0]], np.zeros((3, 4))):
        with pytest.raises(ValueError):
            T.neighbour_joining(bad)


def test_a_negative_length_becomes_0_and_the_other_takes_the_distance():
    # files 0 and 1 are joined first (Q = -22, the smallest); l_0 = 1/2 + (8 - 14) / 4 = -1: 0, and file 1 gets D(0, 1) = 1
    D = [[0, 1, 3, 4], [1, 0, 6, 7], [3, 6, 0, 2], [4, 7, 2, 0]]
    text = T.newick(T.neighbour_joining(D), names(4))
    assert text.startswith("(f0:0.000000000,f1:1.000000000,(f2:") and "-" not in text


def test_ties_go_to_the_first_pair():
    for n in (4, 5, 6):
        D = np.ones((n, n)) - np.eye(n)
        text = T.newick(T.neighbour_joining(D), names(n))
        assert text == T.newick(T.neighbour_joining(D.copy()), names(n))
        assert text.startswith("(f0:0.500000000,f1:0.500000000,")                # files 0 and 1: the first of the smallest Q
    assert T.newick(T.neighbour_joining(np.ones((4, 4)) - np.eye(4)), names(4)) == "(f0:0.500000000,f1:0.500000000,(f2:0.500000000,f3:0.500000000):0.000000000);\n"


def quartet(a, b):
    """the matrix of four files in which files a and b are neighbours"""
    D = np.full((4, 4), 4.0) - 4 * np.eye(4)
    c, d = [x for x in range(4) if x not in (a, b)]
    D[a, b] = D[b, a] = D[c, d] = D[d, c] = 2.0
    return D


def test_support_counts_the_replicates_that_hold_an_edge():
    main = T.neighbour_joining(quartet(2, 3))
    assert T.bipartitions(main) == [0b1100]
    same, other, also = T.neighbour_joining(quartet(0, 1)), T.neighbour_joining(quartet(1, 3)), T.neighbour_joining(quartet(1, 2))
    assert T.bipartitions(same) == [0b1100] and T.bipartitions(other) == [0b1010] and T.bipartitions(also) == [0b0110]
    assert T.support(main, []) == {0b1100: 0}
    assert T.support(main, [other, also, other]) == {0b1100: 0}
    assert T.support(main, [same, other, main, also]) == {0b1100: 2}
    assert T.support(main, [same] * 5) == {0b1100: 5}
    text = T.newick(main, names(4), {0b1100: 2}, 4)
    assert text == "(f0:1.000000000,f1:1.000000000,(f2:1.000000000,f3:1.000000000)50:2.000000000);\n"
    assert T.newick(main, names(4)) == text.replace(")50:", "):") == T.newick(main, names(4), {0b1100: 2}, 0)
    assert ")0:" in T.newick(main, names(4), {0b1100: 0}, 4) and ")100:" in T.newick(main, names(4), {0b1100: 4}, 4)
    assert ")0:" in T.newick(main, names(4), {}, 4)


def test_the_percentage_rounds_half_up():
    main = T.neighbour_joining(quartet(2, 3))
    label = lambda k, B: re.search(r"\)(\d+):", T.newick(main, names(4), {0b1100: k}, B)).group(1)      # noqa: E731
    assert [label(k, 8) for k in range(9)] == ["0", "13", "25", "38", "50", "63", "75", "88", "100"]      # 12.5 -> 13, 37.5 -> 38, 62.5 -> 63
    assert label(1, 200) == "1" and label(1, 3) == "33" and label(2, 3) == "67" and label(1, 1000) == "0" and label(5, 1000) == "1" and label(99999, 100000) == "100"


def test_distances_and_the_correction():
    M = np.array([[0, 10, 30], [10, 0, 74], [30, 74, 0]], dtype=np.uint64)
    p = T.distances(M, 100, "p")
    assert p.dtype == np.float64 and p.tolist() == [[0.0, 0.1, 0.3], [0.1, 0.0, 0.74], [0.3, 0.74, 0.0]]
    jc = T.distances(M, 100, "jc")
    assert jc.tolist() == (-0.75 * np.log(1 - 4 * (M.astype(np.float64) / 100) / 3)).tolist()
    assert jc[0, 0] == 0 and abs(jc[0, 1] - 0.107325632) < 1e-9 and abs(jc[0, 2] - 0.383119218) < 1e-9 and (jc >= p).all()
    M[1, 2] = M[2, 1] = 75
    assert T.distances(M, 100, "p")[1, 2] == 0.75
    with pytest.raises(T.Saturated) as e:
        T.distances(M, 100, "jc")
    assert e.value.pair == (1, 2) and "files 1 and 2" in str(e.value)
    with pytest.raises(ValueError):
        T.distances(M, 100, "k2p")


def test_tree_text_puts_it_together():
    counts = np.array([quartet(2, 3), quartet(2, 3), quartet(1, 3), quartet(0, 1)], dtype=np.uint64)
    assert T.tree_text(counts, 8, "p", names(4)) == "(f0:0.125000000,f1:0.125000000,(f2:0.125000000,f3:0.125000000)67:0.250000000);\n"
    assert T.tree_text(counts[:1], 8, "p", names(4)) == "(f0:0.125000000,f1:0.125000000,(f2:0.125000000,f3:0.125000000):0.250000000);\n"
    with pytest.raises(T.Saturated):
        T.tree_text(counts, 5, "jc", names(4))


@pytest.mark.parametrize("bad", ["a(b", "a)b", "a[b", "a]b", "a:b", "a;b", "a,b", "a'b", 'a"b', "a b", "a\tb", "a\nb", ""])
def test_a_name_newick_cannot_hold_is_refused(bad):
    t = T.neighbour_joining(TEXTBOOK)
    with pytest.raises(ValueError):
        T.newick(t, ["a", "b", bad, "d", "e"])
    with pytest.raises(ValueError):
        T.check_names([bad])
    T.check_names(["a.fa", "x_1-2.fasta", "é"])
    with pytest.raises(ValueError):
        T.newick(t, list("abcd"))
