"""The small-block index of the synteny stage, entry by entry (needs an MI355X: -m gpu).

BlockFinder.tiny_index (sbl_tiny_index) runs the host code and the kernels that sbl_generate_blocks indexes its candidate blocks with
(csrc/synteny.hip: k_tiny_enumerate through tiny_index, k_tiny_enumerate_batch through batch_add / batch_run, then tiny_result) and
hands out what TrimBlocks would read.  For every case of tests/tiny_index_cases.py (preconditions verified on the oracle by
tests/test_tiny_index_cases.py) and every block: status as defined, and for an indexed block the bifurcation count, both list lengths
and every (id, chr, pos) of both lists equal -- exactly, there is no tolerance -- between the one-block launch, the batched launch, the
oracle's index of the block's sequences and the unmodified reference's (tests/golden/tiny_index.json); for the cases marked `general`
also the general index on the GPU (BlockFinder(sequences).enumerate(k)), which pins that path at the same small-record edges."""
import json
import os

import numpy as np
import pytest

from tests import synteny_cases as S
from tests import tiny_index_cases as T
from tests import vectors as V

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(V.GOLDEN, "tiny_index.json")))["index"]


def same_list(a, b):
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in ("id", "chr", "pos"))


def check_index(what, got, want):
    assert got[0] == want[0], "%s: bifurcation count %d, expected %d" % (what, got[0], want[0])
    assert len(got[1]) == len(want[1]) and len(got[2]) == len(want[2]), "%s: list lengths" % what
    assert same_list(got[1], want[1]), "%s: + strand instances differ" % what
    assert same_list(got[2], want[2]), "%s: - strand instances differ" % what


@pytest.mark.parametrize("name", list(T.CASES))
def test_single_and_batched_index_equal_oracle_and_reference(name):
    from sibelia_amd import BlockFinder
    case, (records, jobs), want = T.CASES[name], T.made(name), T.oracle_index(name)
    bf = BlockFinder(records, device=0)
    try:
        if case.stage:
            assert bf.simplify_stage(*case.stage) > 0
        for j, (k, blocks) in enumerate(jobs):
            single, batched = bf.tiny_index(blocks, k, False), bf.tiny_index(blocks, k, True)
            for path, got in (("single", single), ("batched", batched)):
                assert len(got) == len(blocks)
                st = [g[0] for g in got]
                print(name, k, path, [st.count(x) for x in (0, 1, 2)])
                assert tuple(st.count(x) for x in (T.INDEXED, T.DECLINED, T.NOT_ELIGIBLE)) == case.counts[j], (name, k, path)
                for b, (status, bif, pos, neg) in enumerate(got):
                    what = "%s k=%d block %d (%s)" % (name, k, b, path)
                    assert status == T.expected_status(records, blocks[b], k), what
                    if status != T.INDEXED:
                        assert bif == 0 and len(pos) == 0 and len(neg) == 0, what
                        continue
                    check_index(what + " against the oracle", (bif, pos, neg), want[(j, b)])
                    assert T.as_fixture(bif, pos, neg) == GOLD[T.fixture_key(T.sequences(records, blocks[b]), k)], what + " against the reference"
            for b in range(len(blocks)):
                if single[b][0] == T.INDEXED:
                    check_index("%s k=%d block %d: batched against single" % (name, k, b), batched[b][1:], single[b][1:])
    finally:
        bf.close()


@pytest.mark.parametrize("name", [n for n, c in T.CASES.items() if c.general])
def test_general_index_equals_oracle_and_small_block_index(name):
    from sibelia_amd import BlockFinder
    (records, jobs), want = T.made(name), T.oracle_index(name)
    assert want
    bf = BlockFinder(records, device=0)
    try:
        for (j, b), w in want.items():
            k, blocks = jobs[j]
            g = BlockFinder(T.sequences(records, blocks[b]), device=0)
            try:
                got = g.enumerate(k)
            finally:
                g.close()
            what = "%s k=%d block %d: general index" % (name, k, b)
            check_index(what + " against the oracle", got, w)
            tiny = bf.tiny_index([blocks[b]], k, True)[0]
            assert tiny[0] == T.INDEXED
            check_index(what + " against the small-block index", got, tiny[1:])
    finally:
        bf.close()


def test_bad_arguments_are_refused_before_any_launch():
    from sibelia_amd import BlockFinder, SibeliaError
    records, jobs = T.made("k_range")
    good = jobs[0][1][0]
    n0 = len(records[0])
    bf = BlockFinder(records, device=0)
    try:
        for blocks, k in (([good], 1), ([good], 0), ([[(3, 0, 10)]], 8), ([[(0, 5, 5)]], 8), ([[(0, 6, 5)]], 8), ([[(0, n0 - 3, n0 + 1)]], 8),
                          ([good, [(1, 0, 10), (2, 10, 2 ** 40)]], 8), ([[(0, n0, n0 + 1)]], 8)):
            for batched in (False, True):
                with pytest.raises(SibeliaError, match="bad argument"):
                    bf.tiny_index(blocks, k, batched)
        assert bf.tiny_index([], 8, True) == [] and bf.tiny_index([], 8, False) == []
        assert bf.tiny_index([[(0, n0 - 1, n0)]], 8, True)[0][0] == T.INDEXED      # the last base of a record is a range
    finally:
        bf.close()


def test_the_switch_that_turns_the_small_block_index_off_is_ignored(monkeypatch):
    from sibelia_amd import BlockFinder
    monkeypatch.setenv("SBL_NO_TINY_INDEX", "1")
    records, jobs = T.made("strand_order")
    k, blocks = jobs[0]
    bf = BlockFinder(records, device=0)
    try:
        for batched in (False, True):
            got = bf.tiny_index(blocks, k, batched)[0]
            assert got[0] == T.INDEXED
            check_index("strand_order with the switch set", got[1:], T.oracle_index("strand_order")[(0, 0)])
    finally:
        bf.close()


def test_the_call_leaves_blocks_counters_and_the_rand_stream_alone():
    # an input with ambiguous bytes: its block lists depend on where the rand() stream stands.  The ops of the case with a tiny_index
    # call after every one of them must still give the oracle's block lists, and the counters and the block list stay as they were
    from oracle.oracle import Oracle
    from sibelia_amd import BlockFinder
    records, ops = S.CASES["ambiguous_retrim"].make()
    ranges = [[(0, 100, 180), (1, 90, 170), (2, 120, 200)], [(0, 0, 300)], [(1, 0, 40)] * 17]
    o, bf = Oracle(records), BlockFinder(records, device=0)
    names = ["seq%d" % i for i in range(len(records))]
    try:
        for op in ops:
            if op[0] == "stage":
                assert bf.simplify_stage(*op[1:]) == o.simplify_stage(*op[1:])
                continue
            got, want = bf.generate_blocks(*op[1:]), o.generate_blocks(*op[1:])
            assert len(got) == len(want) and all((got[f] == want[f]).all() for f in ("id", "chr", "start", "end")), op
            stats, coords = bf.synteny_stats(), bf.blocks_coords(None, names)
            assert stats["batch_indices"] > 0
            for batched in (False, True):
                res = bf.tiny_index(ranges, 8, batched)
                assert [r[0] for r in res] == [T.expected_status(records, r, 8) for r in ranges]
            assert bf.synteny_stats() == stats and bf.blocks_coords(None, names) == coords
    finally:
        o.close()
        bf.close()
