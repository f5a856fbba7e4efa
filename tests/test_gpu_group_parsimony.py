"""sbl_group_parsimony (csrc/group_parsimony.hip: k_fitch_steps, the scan, k_fitch_changes) through BlockFinder.align_groups,
BlockFinder.group_bootstrap and BlockFinder.group_parsimony against tests/parsimony_model.py on the sites of the rows the groups call
returned, exactly: the counts per edge, the steps, the least steps and every change."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BM                            # noqa: E402
import gmask_cases as KC                           # noqa: E402
import gmask_model as KM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
import parsimony_cases as PC                       # noqa: E402
import parsimony_model as PM                       # noqa: E402
import softcore_model as SM                        # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402

pytestmark = pytest.mark.gpu


def sites_of(rows, cls, n, partial):
    """the site matrix of the rows a groups call returned -> (S, present or None) as the model takes them"""
    if partial:
        S, H, _, _ = SM.site_matrix_partial(rows, cls, n)
        return [bytes(r) for r in S.tolist()], H.tolist()
    return [bytes(r) for r in BM.site_matrix(rows, cls, n)[0].tolist()], None


def same(got, want):
    counts, steps, least, changes = got
    wcounts, wsteps, wleast, wchanges = want
    assert counts.dtype == np.uint64 and counts.tolist() == wcounts
    assert steps.dtype == least.dtype == np.uint8 and steps.tolist() == wsteps and least.tolist() == wleast
    assert list(zip(changes["site"].tolist(), changes["edge"].tolist(), changes["from"].tolist(), changes["to"].tolist())) == wchanges
    assert not changes["pad_"].any()


class Run:
    """a finder over the groups of a case, aligned; .rows: the rows the device made"""

    def __init__(self, groups, cls, n, partial=False):
        from sibelia_amd import BlockFinder
        self.b, self.cls, self.n, self.partial = Groups(groups), list(cls), n, partial
        self.bf = BlockFinder(self.b.records, device=0)
        aligned = self.bf.align_groups(self.b.desc)
        assert [al.status for al in aligned] == [0] * len(groups)
        self.rows = [al.rows for al in aligned]
        self.bf.set_partial(partial)

    def boot(self, replicates=0):
        return self.bf.group_bootstrap(self.cls, self.n, replicates, 1)

    def want(self, edges, rows=None):
        S, present = sites_of(rows or self.rows, self.cls, self.n, self.partial)
        return PM.fitch(S, present, edges)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bf.close()


@pytest.mark.parametrize("name", sorted(n for n, c in PC.CASES.items() if c["device"]))
def test_crafted_cases(name):
    c = PC.CASES[name]
    groups, cls = PC.groups_of(c)
    with Run(groups, cls, c["n"], c["partial"]) as r:
        assert r.rows == groups
        _, nsites, _ = r.boot()
        S, present = sites_of(r.rows, cls, c["n"], c["partial"])
        wS, wpresent = PC.rows_of(c["columns"], c["n"])
        assert nsites == len(c["columns"])
        if c["columns"]:                                                         # the sites are the case's: its predicate holds for what the device read
            assert [[chr(x) if h else "-" for x, h in zip(row, held)] for row, held in zip(S, present or wpresent)] == [list(map(chr, row)) for row in wS]
        got = r.bf.group_parsimony(c["edges"])
        same(got, PC.model(c))
        k, d = r.bf.group_parsimony_times()
        assert k >= 0 and d >= 0 and (k > 0) == bool(c["columns"])


def random_tree(rng, n):
    return PC.joined(n, lambda live, s: [int(x) for x in rng.choice(len(live), 2, replace=False)])


def test_seeded_random_cases_with_joined_and_random_trees():
    rng = np.random.default_rng(1440)
    for k in range(40):
        n = int(rng.choice([3, 4, 6, 9, 17, 31, 32, 33, 40, 64]))
        partial = k % 2 == 1
        cols = PC.variable_columns(rng, n, int(rng.integers(1, 70)), 0.25 if partial else 0.0)
        if partial:
            cols.sort(key=lambda col: [ch == "-" for ch in col])
        c = PC.case(n, [], cols, None, partial)
        groups, cls = PC.groups_of(c, rng)
        with Run(groups, cls, n, partial) as r:
            M, nsites, nclean = r.boot()
            assert nsites == len(cols)
            if k % 4 < 2:                                                        # the tree neighbour joining makes of these very sites
                D = M[0].astype(np.float64) / nclean
                records, _ = r.bf.nj_batch(D[None])
                edges = records[0]
                pairs = list(zip(edges["parent"].tolist(), edges["child"].tolist()))
            else:
                edges = pairs = PC.permuted(random_tree(rng, n), n, k)
            same(r.bf.group_parsimony(edges), r.want(pairs))


def test_twice_in_a_row_and_with_the_other_calls_in_between():
    c = PC.CASES["balanced_33"]
    groups, cls = PC.groups_of(c)
    other = PC.CASES["permuted_33"]["edges"]
    headers = [b">%d\n" % f for f in range(33)]
    with Run(groups, cls, 33) as r:
        M, _, nclean = r.boot(2)
        want, want_other = PC.model(c), r.want(other)
        same(r.bf.group_parsimony(c["edges"]), want)
        same(r.bf.group_parsimony(c["edges"]), want)
        same(r.bf.group_parsimony(other), want_other)
        r.bf.group_concat(cls, 33, headers, 1)
        r.bf.group_distances(cls, 33)
        r.bf.group_variants()
        r.bf.nj_batch(np.stack([M[0], M[1]]).astype(np.float64) / nclean)
        r.bf.group_mask(10, 1)
        same(r.bf.group_parsimony(c["edges"]), want)
        assert sum(want[1]) > 0 and want[3] != want_other[3]


def test_masked_rows():
    """after a mask with the setting on the sites are those of the masked rows"""
    rng = np.random.default_rng(78)
    c = MC.rand(rng, 400)
    groups = [[c, KC.subst(c, [10, 12, 14, 100, 200, 300]), KC.subst(c, [50, 150, 250, 252, 254, 256, 350]), KC.subst(c, [100, 150, 380])]]
    cls = [0, 2, 1, 3]
    edges = PC.CASES["tie_lowest_code"]["edges"]
    with Run(groups, cls, 4) as r:
        assert r.rows == groups
        r.boot()
        plain = r.want(edges)
        same(r.bf.group_parsimony(edges), plain)
        intervals, masked = KM.mask(groups, 10, 2)
        assert r.bf.group_mask(10, 2) == intervals and len(intervals) == 2
        same(r.bf.group_parsimony(edges), plain)                                 # the packed sites of the bootstrap call stay
        r.bf.set_masked(True)
        _, nsites, _ = r.boot()
        hidden = r.want(edges, masked)
        assert nsites == len(hidden[1]) == len(plain[1]) - 7
        same(r.bf.group_parsimony(edges), hidden)
        r.bf.set_masked(False)
        same(r.bf.group_parsimony(edges), hidden)                                # ... whatever the setting is now


def test_a_second_bootstrap_call_with_other_classes():
    c = PC.CASES["partial_5"]
    groups, cls = PC.groups_of(c)
    swap = [4 - f for f in cls]
    with Run(groups, cls, 5, True) as r:
        r.boot()
        same(r.bf.group_parsimony(c["edges"]), PC.model(c))
        r.cls = swap
        r.boot(3)
        second = r.want(c["edges"])
        same(r.bf.group_parsimony(c["edges"]), second)
        assert second[3] != PC.model(c)[3]
        r.bf.set_partial(False)                                                  # the setting of the bootstrap call counts, not the one now
        same(r.bf.group_parsimony(c["edges"]), second)


def raw(bf, edges, n, null=None):
    """the entry point itself, with a null pointer in place of `null` (edges, or the k-th result) -> (status, the results)"""
    from sibelia_amd.api import NjEdge, ParsimonyChange
    arr = (NjEdge * max(1, len(edges)))(*[(u, v, 0.0) for u, v in edges])
    outs = [C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.POINTER(ParsimonyChange)(), C.c_uint64()]
    fn = bf.L.sbl_group_parsimony
    saved = fn.argtypes
    fn.argtypes = None
    try:
        return fn(bf.h, None if null == "edges" else arr, C.c_uint32(n), *[None if null == k else C.byref(o) for k, o in enumerate(outs)]), outs
    finally:
        fn.argtypes = saved


def test_refused_arguments_leave_an_earlier_result_valid(monkeypatch):
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    c = PC.CASES["tie_lowest_code"]
    good = c["edges"]
    groups, cls = PC.groups_of(c)
    b = Groups(groups)
    bf = BlockFinder(b.records, device=0)
    try:
        bf.align_groups(b.desc)
        with pytest.raises(SibeliaError, match="bad argument"):                  # before any bootstrap call
            bf.group_parsimony(good)
        bf.group_bootstrap(cls, 4, 0, 1)
        want = PC.model(c)

        def held():
            """a successful call -> a check of the arrays it handed out, which stay the context's until the next successful call"""
            status, (counts, steps, least, changes, nchanges) = raw(bf, good, 4)
            assert status == 0

            def still_valid():
                assert nchanges.value == len(want[3]) and [steps[k] for k in range(3)] == want[1] and [least[k] for k in range(3)] == want[2]
                assert [(changes[k].site, changes[k].edge, changes[k].from_, changes[k].to) for k in range(nchanges.value)] == want[3]
                assert [counts[k] for k in range(5 * 16)] == [x for e in want[0] for row in e for x in row]
            still_valid()
            return still_valid
        still_valid = held()
        bad_trees = [good[:-1] + [(5, 6)],                                       # a node that is not below 2 n - 2
                     good[:-1] + [(5, 2)],                                       # file 2 twice, file 3 never
                     [(4, 0), (4, 1), (4, 5), (5, 5), (2, 3)],                   # a loop
                     [(4, 1), (4, 2), (4, 5), (5, 3), (5, 3)],                   # file 0 never, an edge twice
                     [(1, 0), (4, 2), (4, 3), (4, 5), (5, 5)]]                   # file 0 on file 1
        for edges in bad_trees:
            with pytest.raises(PM.Refused):
                PM.rooted(edges, 4)
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_parsimony(edges)
            still_valid()
        for edges in ([(3, 0), (3, 1), (3, 2)], PC.caterpillar(5), [(2, 0), (2, 1)]):      # n is not the classes of the bootstrap call; n < 3
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_parsimony(edges)
        with pytest.raises(SibeliaError, match="exceeds.*at most 64"):
            bf.group_parsimony(PC.caterpillar(65))
        for null in ("edges", 0, 1, 2, 3, 4):
            assert raw(bf, good, 4, null)[0] == 1
        assert raw(bf, good, 2)[0] == 1 and raw(bf, PC.caterpillar(65), 65)[0] not in (0, 1)
        still_valid()
        monkeypatch.setenv("SBL_TEST_PARSIMONY_MAX_CHANGES", "5")               # the case has six changes: refused after the first pass
        with pytest.raises(SibeliaError, match="exceeds.*too many changes"):
            bf.group_parsimony(good)
        still_valid()
        monkeypatch.setenv("SBL_TEST_PARSIMONY_MAX_CHANGES", "6")
        same(bf.group_parsimony(good), want)
        monkeypatch.delenv("SBL_TEST_PARSIMONY_MAX_CHANGES")
        still_valid = held()
        with pytest.raises(SibeliaError, match="bad argument"):                  # a refused bootstrap call leaves the sites of the one before
            bf.group_bootstrap(cls, 5, 0, 1)
        still_valid()
        same(bf.group_parsimony(good), want)
    finally:
        bf.close()
