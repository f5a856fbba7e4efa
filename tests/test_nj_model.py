"""tests/nj_model.py, the scalar restatement of sbl_nj_batch's arithmetic, is tree.neighbour_joining bit for bit on
tests/nj_cases.py; and its row-sum rule alone is numpy's sum over a row, so that a numpy that adds in another order shows up here and
not as a mismatch on the device.  Device-free."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nj_cases as NC                              # noqa: E402
import nj_model as NM                              # noqa: E402


@pytest.mark.parametrize("label", NC.LABELS)
def test_the_model_is_neighbour_joining_bit_for_bit(label):
    D = dict(NC.CASES)[label]
    edges, splits = NM.neighbour_joining(D.tolist())
    want_edges, want_splits = NC.reference(label)
    assert [(u, v, NC.bits(ln)) for u, v, ln in edges] == want_edges
    assert sorted(splits) == want_splits and len(splits) == len(D) - 3


def test_the_cases_are_what_they_say():
    by = dict(NC.CASES)
    assert len(by) == len(NC.CASES)
    for label, D in NC.CASES:
        assert D.dtype == np.float64 and D.shape == (len(D), len(D)) and np.isfinite(D).all()
        assert (D == D.T).all() and not D.diagonal().any()
    assert {len(D) for _, D in NC.CASES} >= set(NC.SIZES)
    # ties: among the smallest counts most steps have more than one smallest Q, among the largest few have
    D = by["n16_below3_p"]
    r = D.sum(axis=1)
    Q = 14 * D - r[:, None] - r[None, :]
    assert (Q[np.triu_indices(16, 1)] == Q[np.triu_indices(16, 1)].min()).sum() >= 1
    assert len(np.unique(by["n16_below3_p"])) <= 3 and len(np.unique(by["n16_below5000_p"])) > 100
    assert (by["n6_two_identical"][1] == by["n6_two_identical"][4]).all() and by["n9_three_identical"][0, 8] == 0
    # the negative length of tests/test_tree.py is there: the model clamps it as the tree does
    edges, _ = NM.neighbour_joining(by["n4_negative_length"].tolist())
    assert edges[0] == (4, 0, 0.0) and edges[1] == (4, 1, 1.0)


def test_the_row_sum_is_numpys():
    rng = np.random.default_rng(29)
    for m in range(3, 65):
        for scale in (1.0, 1e-5, 1e7):
            A = rng.random((5, m)) * scale
            A[0] = rng.integers(0, 3, size=m) / NC.K                             # many equal entries
            got = [NM.row_sum(row) for row in A.tolist()]
            assert [NC.bits(x) for x in got] == [NC.bits(float(x)) for x in A.sum(axis=1)], m
    # rows of zeros of either sign: the reduction starts from +0.0
    for m in (3, 7, 8, 20):
        assert NC.bits(NM.row_sum([-0.0] * m)) == NC.bits(float(np.full((2, m), -0.0).sum(axis=1)[0]))
