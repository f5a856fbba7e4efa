"""sibelia_amd/tree.py's tally of the replicates' bipartitions, the majority-rule consensus and tree_files against texts
written out by hand and against the functions that were there before.  Device-free."""
import math

import numpy as np
import pytest

from sibelia_amd import tree as T


def names(n):
    return ["f%d" % i for i in range(n)]


def quartet(a, b):
    """the matrix of four files in which files a and b are neighbours (tests/test_tree.py): every leaf edge 1, the inner edge 2"""
    D = np.full((4, 4), 4.0) - 4 * np.eye(4)
    c, d = [x for x in range(4) if x not in (a, b)]
    D[a, b] = D[b, a] = D[c, d] = D[d, c] = 2.0
    return D


def records_of(trees):
    return np.array([t.edges for t in trees], dtype=T.EDGE_RECORD)


def text(replicates, n):
    tree, held = T.consensus(replicates, len(replicates))
    return T.newick(tree, names(n), held, len(replicates))


Q23, Q13, Q12 = (T.neighbour_joining(quartet(a, b)) for a, b in ((2, 3), (1, 3), (1, 2)))
STAR4 = "(f0:1.000000000,f1:1.000000000,f2:1.000000000,f3:1.000000000);\n"


def both(trees):
    """the consensus text from the trees and from their edge records: one text"""
    a, b = text(trees, trees[0].n), text(records_of(trees), trees[0].n)
    assert a == b
    return a


def test_three_of_five_replicates_hold_the_branch():
    assert both([Q23, Q13, Q23, Q12, Q23]) == "(f0:1.000000000,f1:1.000000000,(f2:1.000000000,f3:1.000000000)60:2.000000000);\n"
    assert both([Q13] * 5) == "(f0:1.000000000,(f1:1.000000000,f3:1.000000000)100:2.000000000,f2:1.000000000);\n"


def test_exactly_half_is_no_majority_and_none_gives_the_star():
    assert both([Q23, Q13, Q23, Q12]) == STAR4                                   # 2 of 4: the majority is strict
    assert both([Q23, Q13, Q12]) == STAR4
    assert both([Q23, Q13]) == STAR4
    tree, held = T.consensus([Q23, Q13], 2)
    assert held == {} and len(tree.edges) == 4 and T.bipartitions(tree) == []
    assert both([Q23, Q23, Q13]) != STAR4                                        # 2 of 3 is one


def six(order, inner, leaf=1.0):
    """the caterpillar (order[0], order[1], (order[2], (order[3], (order[4], order[5])))) with file 0 first: inner = the lengths of the three
    inner edges from the outermost in"""
    a, b, c, d, e, f = order
    return T.Tree(6, [(6, e, leaf), (6, f, leaf), (7, d, leaf), (7, 6, inner[2]), (8, c, leaf), (8, 7, inner[1]), (9, a, leaf), (9, b, leaf), (9, 8, inner[0])])


def test_a_nested_pair_of_branches_on_six_files():
    # all hold {4, 5} inside {3, 4, 5}; around them two hold {2, 3, 4, 5} and two {1, 3, 4, 5}: exactly half each, so neither is a branch
    reps = [six((0, 1, 2, 3, 4, 5), (0.5, 2.0, 0.25)), six((0, 2, 1, 3, 4, 5), (1.5, 3.0, 0.5)), six((0, 1, 2, 3, 5, 4), (7.0, 1.0, 0.75)), six((0, 2, 1, 3, 4, 5), (2.5, 2.0, 0.5))]
    assert [sorted(T.bipartitions(t)) for t in reps] == [[0b110000, 0b111000, 0b111100], [0b110000, 0b111000, 0b111010]] * 2
    assert both(reps) == "(f0:1.000000000,f1:1.000000000,f2:1.000000000,(f3:1.000000000,(f4:1.000000000,f5:1.000000000)100:0.500000000)100:2.000000000);\n"
    # the first three: {2, 3, 4, 5} is held by two of three, a third branch around the pair; a length is the mean over the holders alone
    assert both(reps[:3]) == ("(f0:1.000000000,f1:1.000000000,(f2:1.000000000,(f3:1.000000000,(f4:1.000000000,f5:1.000000000)100:0.500000000)100:2.000000000)"
                              "67:3.750000000);\n")
    # a replicate with {4, 5} in {2, 4, 5} in {2, 3, 4, 5} holds only the inner one of the pair
    reps[3] = six((0, 1, 3, 2, 4, 5), (1.0, 1.0, 1.0))
    assert sorted(T.bipartitions(reps[3])) == [0b110000, 0b110100, 0b111100]
    assert both(reps) == ("(f0:1.000000000,f1:1.000000000,(f2:1.000000000,(f3:1.000000000,(f4:1.000000000,f5:1.000000000)100:0.625000000)75:2.000000000)"
                          "75:2.833333333);\n")


def test_the_mean_is_taken_with_fsum():
    lengths = [1e16, 1.0, 1.0]                                                   # left to right the two 1.0 are lost
    assert sum(lengths) != math.fsum(lengths)
    reps = [six((0, 1, 2, 3, 4, 5), (ln, 1.0, 1.0), leaf=ln) for ln in lengths]
    mean = "%.9f" % (math.fsum(lengths) / 3)
    assert mean != "%.9f" % (sum(lengths) / 3)
    for order in ([0, 1, 2], [2, 1, 0], [1, 0, 2]):
        s = both([reps[k] for k in order])
        assert s.startswith("(f0:%s,f1:%s,(f2:%s," % (mean, mean, mean)) and s.endswith(")100:%s);\n" % mean)


def random_trees(seed, n, B, bound=40):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        M = np.triu(rng.integers(0, bound, size=(n, n)), 1)
        out.append(T.neighbour_joining(T.distances(M + M.T, 1000, "p")))
    return out


@pytest.mark.parametrize("n, B", [(5, 9), (7, 25), (12, 10), (64, 3)])
def test_the_text_does_not_depend_on_the_order_of_the_replicates(n, B):
    rng = np.random.default_rng(n)
    M = np.triu(rng.integers(5, 60, size=(n, n)), 1)
    base = T.distances(M + M.T, 1000, "p")
    reps = [T.neighbour_joining((lambda U: base + U + U.T)(np.triu(rng.integers(0, 4, size=(n, n)), 1) / 1000.0)) for _ in range(B)]
    s = both(reps)
    assert s.count("\n") == 1 and s.startswith("(f0:")
    for _ in range(3):
        assert both([reps[k] for k in rng.permutation(B)]) == s
    # every labelled branch is a majority one and is compatible with the others
    tree, held = T.consensus(reps, B)
    assert all(2 * k > B for k in held.values()) and sorted(held) == sorted(T.bipartitions(tree))
    assert all(a & b in (0, a, b) for a in held for b in held)


def test_split_tally_is_support():
    reps = random_trees(3, 8, 30, bound=6)
    main = random_trees(4, 8, 1, bound=6)[0]
    tally = T.split_tally([T.bipartitions(t) for t in reps])
    assert sum(tally.values()) == 30 * 5 and all(isinstance(b, int) and isinstance(k, int) for b, k in tally.items())
    assert T.support(main, reps) == {b: tally.get(b, 0) for b in T.bipartitions(main)}
    assert T.support(reps[0], reps) == {b: tally[b] for b in T.bipartitions(reps[0])} and min(T.support(reps[0], reps).values()) >= 1
    assert T.split_tally(np.zeros((7, 0), dtype=np.uint64)) == {} and T.split_tally([]) == {}
    wide = np.array([[1 << 63, 6], [6, 1 << 63]], dtype=np.uint64)              # the top bit of a 64-file mask
    assert T.split_tally(wide) == {6: 2, 1 << 63: 2}


def test_a_tree_comes_back_from_its_records():
    t = random_trees(8, 9, 1)[0]
    back = T.Tree.of_records(records_of([t])[0])
    assert back.n == 9 and back.edges == t.edges and all(type(u) is int and type(ln) is float for u, _, ln in back.edges)
    assert T.EDGE_RECORD.itemsize == 16 and T.EDGE_RECORD.names == ("parent", "child", "length")


def counts_of(seed, n, B):
    rng = np.random.default_rng(seed)
    base = np.triu(rng.integers(20, 200, size=(n, n)), 1)
    out = []
    for _ in range(B + 1):
        M = base + np.triu(rng.integers(0, 12, size=(n, n)), 1)
        out.append(M + M.T)
    return np.array(out, dtype=np.uint64)


def host_nj(calls):
    def nj(D):
        calls.append(D.shape)
        trees = [T.neighbour_joining(d) for d in D]
        return records_of(trees), np.array([T.bipartitions(t) for t in trees], dtype=np.uint64).reshape(len(D), D.shape[1] - 3)
    return nj


@pytest.mark.parametrize("n, B, model", [(4, 5, "p"), (9, 20, "jc"), (3, 4, "p"), (6, 0, "p")])
def test_tree_files_without_nj_gives_the_bytes_of_tree_text(n, B, model):
    counts = counts_of(n, n, B)
    main, majority, lines = T.tree_files(counts, 5000, model, names(n))
    assert main == T.tree_text(counts, 5000, model, names(n))
    reps = [T.neighbour_joining(T.distances(counts[r], 5000, model)) for r in range(1, B + 1)]
    if B == 0:
        assert majority is None and lines is None
        return
    assert majority == text(reps, n) and lines == "".join(T.newick(t, names(n)) for t in reps) and lines.count("\n") == B
    # a callable that joins like neighbour_joining gets every matrix in one call and changes no byte; only the wanted texts are made
    calls = []
    assert T.tree_files(counts, 5000, model, names(n), host_nj(calls)) == (main, majority, lines) and calls == [(B + 1, n, n)]
    assert T.tree_files(counts, 5000, model, names(n), host_nj(calls), ["consensus"]) == (None, majority, None)
    assert T.tree_files(counts, 5000, model, names(n), None, ["tree", "boottrees"]) == (main, None, lines)
    K = np.full((n, n), 5000)
    assert T.tree_files(counts, K, model, names(n), host_nj(calls)) == (main, majority, lines)


def test_tree_files_above_64_files_joins_on_the_host():
    counts = counts_of(65, 65, 1)

    def never(D):
        raise AssertionError("65 files do not go to the callable")
    main, majority, lines = T.tree_files(counts, 5000, "p", names(65), never)
    assert main == T.tree_text(counts, 5000, "p", names(65)) and lines.count("\n") == 1 and majority.endswith(");\n")


def test_tree_files_raises_what_tree_text_raises():
    counts = counts_of(4, 4, 3)
    with pytest.raises(T.Saturated):
        T.tree_files(counts, 100, "jc", names(4))
    K = np.full((4, 4), 5000)
    K[1, 2] = K[2, 1] = 0
    with pytest.raises(T.NoSharedColumn) as e:
        T.tree_files(counts, K, "p", names(4), host_nj([]))
    assert e.value.pair == (1, 2)
    with pytest.raises(ValueError):
        T.consensus([Q23], 2)
    with pytest.raises(ValueError):
        T.consensus([], 0)
