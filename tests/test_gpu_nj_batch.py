"""sbl_nj_batch (csrc/tree_nj.hip: k_nj_batch) through BlockFinder.nj_batch against sibelia_amd/tree.py on tests/nj_cases.py: every edge
bit for bit the edge of tree.neighbour_joining, in its order, and the splits the bipartitions of that tree; the batches, the calls around
it and every refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BM                            # noqa: E402
import nj_cases as NC                              # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, TOO_LARGE = 1, 5                          # SBL_ERR_BAD_ARG, SBL_ERR_TOO_LARGE


@pytest.fixture(scope="module")
def finder():
    from sibelia_amd import BlockFinder
    bf = BlockFinder([b"ACGTTGCAAC" * 4], device=0)      # the call needs no groups: any records do
    yield bf
    bf.close()


def same(edges, splits, label):
    want_edges, want_splits = NC.reference(label)
    assert [(int(u), int(v), NC.bits(float(ln))) for u, v, ln in edges.tolist()] == want_edges, label
    assert sorted(splits.tolist()) == want_splits, label


def joined(bf, labels):
    by = dict(NC.CASES)
    D = np.array([by[label] for label in labels])
    n = D.shape[1]
    edges, splits = bf.nj_batch(D)
    assert edges.shape == (len(labels), 2 * n - 3) and splits.shape == (len(labels), n - 3) and splits.dtype == np.uint64
    assert edges.dtype.itemsize == 16 and edges.dtype.names == ("parent", "child", "length")
    for k, label in enumerate(labels):
        same(edges[k], splits[k], label)
    kernel, copy = bf.nj_batch_times()
    assert kernel > 0 and copy > 0
    return edges, splits


@pytest.mark.parametrize("label", NC.LABELS)
def test_every_case_alone(finder, label):
    joined(finder, [label])


@pytest.mark.parametrize("n", sorted({len(D) for _, D in NC.CASES}))
def test_all_cases_of_one_size_in_one_call(finder, n):
    labels = [label for label, D in NC.CASES if len(D) == n]
    joined(finder, labels + labels[::-1])


def test_no_tree_and_one_tree(finder):
    joined(finder, ["n9_all_equal"])
    edges, splits = finder.nj_batch(np.zeros((0, 5, 5)))
    assert edges.shape == (0, 7) and splits.shape == (0, 2)
    assert finder.nj_batch_times() == (0.0, 0.0)
    edges, splits = joined(finder, ["n3_all_zero"])
    assert splits.shape == (1, 0) and edges["parent"].tolist() == [[3, 3, 3]] and edges["child"].tolist() == [[0, 1, 2]]
    # the complement of a mask of 64 files: the split of the first join that holds file 0 keeps its 64 bits
    edges, splits = joined(finder, ["n64_all_equal"])
    assert edges[0, 0]["child"] == 0 and edges[0, 1]["child"] == 1 and int(splits[0, 0]) == 2 ** 64 - 4


def pool64():
    """32 different matrices of 64 files and the records and splits of tree.py for them"""
    from sibelia_amd import tree as T
    rng = np.random.default_rng(64)
    pool = np.array([T.distances(NC.counts(rng, 64, 50), NC.K, "jc" if k % 2 else "p") for k in range(32)])
    trees = [T.neighbour_joining(D) for D in pool]
    return pool, np.array([t.edges for t in trees], dtype=T.EDGE_RECORD), np.array([sorted(T.bipartitions(t)) for t in trees], dtype=np.uint64)


def test_a_call_of_more_than_one_batch(finder):
    """2049 matrices of 64 files: the first batch holds 2048 of them (64 MiB), the last tree is a launch of its own"""
    pool, records, masks = pool64()
    pick = np.arange(2049) % 32
    pick[2048] = 7                                                               # not the matrix that opens a batch
    edges, splits = finder.nj_batch(pool[pick])
    assert edges.shape == (2049, 125) and splits.shape == (2049, 61)
    assert np.array_equal(edges.view(np.uint8), records[pick].view(np.uint8))    # bit for bit
    assert np.array_equal(np.sort(splits, axis=1), masks[pick])
    assert len({records[k].tobytes() for k in range(32)}) == 32


def test_two_calls_in_a_row_and_a_bootstrap_between(finder):
    from sibelia_amd import BlockFinder
    first = joined(finder, ["n17_below50_jc", "n17_below3_p"])
    second = joined(finder, ["n8_below5000_p"])
    joined(finder, ["n17_below50_jc", "n17_below3_p"])
    # between two calls the bootstrap of a groups call on the same finder: neither changes the other
    b = Groups([[b"ACGTACGTACGTACGTAGCA", b"ACGTACCTACGTACGTAGCA", b"ACGAACGTACGTACGTAGCT"]])
    bf = BlockFinder(b.records, device=0)
    try:
        aligned = bf.align_groups(b.desc)
        rows = [al.rows for al in aligned]
        assert aligned[0].status == 0 and aligned[0].L == 20
        before = joined(bf, ["n33_below50_p"])
        M, sites, clean = bf.group_bootstrap([0, 1, 2], 3, 7, 5)
        after = joined(bf, ["n33_below50_p", "n33_below3_jc"])
        M2, sites2, clean2 = bf.group_bootstrap([0, 1, 2], 3, 7, 5)
        wM, wC, wK = BM.counts(rows, [0, 1, 2], 3, 7, 5, 0, None)
        assert (sites, clean) == (sites2, clean2) == (wC, wK) == (3, 20) and (M == wM).all() and (M2 == wM).all()
        assert before[0][0].tobytes() == after[0][0].tobytes()
    finally:
        bf.close()
    assert first[0].tobytes() != second[0].tobytes()


def test_every_refused_argument_leaves_the_earlier_result(finder):
    from sibelia_amd.api import NjEdge, SibeliaError
    L, h = finder.L, finder.h
    label = "n9_three_identical"
    good = np.ascontiguousarray(dict(NC.CASES)[label])
    edges, splits = C.POINTER(NjEdge)(), C.POINTER(C.c_uint64)()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                      # noqa: E731
    assert L.sbl_nj_batch(h, ptr(good), 9, 1, C.byref(edges), C.byref(splits)) == 0
    held = (C.cast(edges, C.c_void_p).value, C.cast(splits, C.c_void_p).value)

    def earlier_result_is_there():
        assert (C.cast(edges, C.c_void_p).value, C.cast(splits, C.c_void_p).value) == held
        want_edges, want_splits = NC.reference(label)
        assert [(edges[k].parent, edges[k].child, NC.bits(edges[k].length)) for k in range(15)] == want_edges
        assert sorted(splits[k] for k in range(6)) == want_splits

    earlier_result_is_there()

    def bad(cell, value, n=9):
        D = np.array([good, good, good])
        D[(1,) + cell] = value
        return D

    nan_pair = bad((2, 5), np.nan)
    nan_pair[1, 5, 2] = np.nan                                                   # symmetric: refused as not finite, not as asymmetric
    inf_pair = bad((0, 8), np.inf)
    inf_pair[1, 8, 0] = np.inf
    minus = bad((3, 4), -np.inf)
    minus[1, 4, 3] = -np.inf
    refused = [(np.zeros((1, 2, 2)), 2, BAD_ARG, "three or more"), (np.zeros((1, 65, 65)), 65, TOO_LARGE, "at most 64"),
               (nan_pair, 9, BAD_ARG, "matrix 1, cell (2, 5) is not finite"), (inf_pair, 9, BAD_ARG, "matrix 1, cell (0, 8) is not finite"),
               (minus, 9, BAD_ARG, "matrix 1, cell (3, 4) is not finite"),
               (bad((6, 1), np.nextafter(good[6, 1], 1.0)), 9, BAD_ARG, "matrix 1, cell (1, 6) differs from its mirror"),
               (bad((4, 4), 1e-300), 9, BAD_ARG, "matrix 1, cell (4, 4) is not 0"), (bad((0, 0), np.nan), 9, BAD_ARG, "matrix 1, cell (0, 0) is not 0")]
    for D, n, status, words in refused:
        D = np.ascontiguousarray(D, dtype=np.float64)
        assert L.sbl_nj_batch(h, ptr(D), n, len(D), C.byref(edges), C.byref(splits)) == status, words
        assert words in L.sbl_last_error(h).decode(), (words, L.sbl_last_error(h))
        earlier_result_is_there()
        with pytest.raises(SibeliaError):
            finder.nj_batch(D)
        earlier_result_is_there()
    for args in ((None, 9, 1, C.byref(edges), C.byref(splits)), (ptr(good), 9, 1, None, C.byref(splits)), (ptr(good), 9, 1, C.byref(edges), None)):
        assert L.sbl_nj_batch(h, *args) == BAD_ARG
        earlier_result_is_there()
    assert L.sbl_nj_batch(h, None, 9, 0, C.byref(edges), C.byref(splits)) == 0  # no matrix: nothing to point at, and a result
    with pytest.raises(SibeliaError):
        finder.nj_batch(np.zeros((2, 4, 5)))
    joined(finder, [label])
