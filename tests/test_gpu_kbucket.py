"""k_bucket_classify (csrc/kmer_bucket_kernels.h) at its staging, direct and capacity edges, against the CPU oracle (needs an MI355X:
-m gpu).

The inputs are those of tests/kbucket_cases.py.  The host model (tests/kbucket_model.py) says which path each of them takes --
buckets that go direct by size and by keys, flushes in the middle of a workgroup by either trigger, a table exactly full and one
over, output buffers exactly large enough and one pair short -- and tests/test_kbucket_cases.py checks those predictions and the model
itself without a GPU.  Here every case is enumerated on the device and compared with Oracle(seqs).enumerate(k): the id count and both
instance lists, field for field.

The model predicts paths for ONE GPU only: on several ranks (shard.hip) every owner runs the same kernel over its own buckets, so what
is staged together differs.  The sharded runs assert equality with the oracle and nothing more.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import kbucket_cases as K

pytestmark = pytest.mark.gpu

LABELS = list(K.CASES)
STAGE = [c.label for c in K.CASES.values() if c.stage]


@lru_cache(maxsize=None)
def _want(label):
    """the oracle's enumeration of a case, computed once and shared (read-only)"""
    from oracle.oracle import Oracle
    case = K.CASES[label]
    orc = Oracle(case.sequences)
    try:
        count, pos, neg = orc.enumerate(case.k)
    finally:
        orc.close()
    for a in (pos, neg):
        a.setflags(write=False)
    assert count > 0 and len(pos) == len(neg) > 0                    # no case passes on an empty result
    return count, pos, neg


def _same(got, want, what):
    assert got[0] == want[0], "%s: %d ids, the oracle has %d" % (what, got[0], want[0])
    for name, a, b in (("positive", got[1], want[1]), ("negative", got[2], want[2])):
        assert len(a) == len(b), "%s: %d %s instances, the oracle has %d" % (what, len(a), name, len(b))
        for f in ("id", "chr", "pos"):
            bad = np.flatnonzero(a[f] != b[f])
            assert not len(bad), "%s: %s instance %d differs in %s (%d of %d differ): %r, the oracle has %r" % (what, name, bad[0], f, len(bad), len(a), a[bad[0]], b[bad[0]])


def _run(case, make, monkeypatch):
    want = _want(case.label)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    bf = make(case.sequences)
    try:
        _same(bf.enumerate(case.k), want, "first call")
        # the member list reuses the record buffer: a second call on the same finder shows a stale buffer
        _same(bf.enumerate(case.k), want, "second call")
        if case.env:
            for name in case.env:
                monkeypatch.delenv(name)
            _same(bf.enumerate(case.k), want, "without the hooks")
    finally:
        bf.close()


@pytest.mark.parametrize("label", LABELS)
def test_one_gpu_equals_the_oracle(label, monkeypatch):
    from sibelia_amd import BlockFinder
    _run(K.CASES[label], lambda seqs: BlockFinder(seqs, device=0), monkeypatch)


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("label", LABELS)
def test_sharded_equals_the_oracle(label, nranks, monkeypatch):
    from sibelia_amd.dist import LocalShardedFinder
    _run(K.CASES[label], lambda seqs: LocalShardedFinder(seqs, [0] * nranks), monkeypatch)


@pytest.mark.parametrize("label", STAGE)
def test_marks_of_the_direct_path_carry_a_stage(label, monkeypatch):
    """one simplification stage (k, 10 * k, 1) on the two direct cases: the bulge count and the state after it, against the oracle (which
    takes 0.1 s for it)"""
    from oracle.oracle import Oracle
    from sibelia_amd import BlockFinder
    case = K.CASES[label]
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    bf, orc = BlockFinder(case.sequences, device=0), Oracle(case.sequences)
    try:
        got, want = bf.simplify_stage(case.k, 10 * case.k, 1), orc.simplify_stage(case.k, 10 * case.k, 1)
        assert got == want and want > 0
        (sa, pa), (sb, pb) = bf.state(), orc.state()
        assert sa == sb and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    finally:
        bf.close()
        orc.close()
