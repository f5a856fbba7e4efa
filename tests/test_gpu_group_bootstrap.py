"""sbl_group_bootstrap (csrc/group_boot.hip: k_site_flags<true>, k_boot_clean, k_boot_pack, k_boot_count) through BlockFinder.align_groups
and BlockFinder.group_bootstrap against tests/boot_model.py on the rows the groups call returned, exactly: every cell of every slab, the
number of sites and the number of clean columns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_cases as BC                            # noqa: E402
import boot_model as BM                            # noqa: E402
import concat_model as CM                          # noqa: E402
import gdist_cases as DC                           # noqa: E402
import gdist_model as DM                           # noqa: E402
import gmask_cases as KC                           # noqa: E402
import gmask_model as KM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402  (the layout of groups of strings as ranges of three records)

pytestmark = pytest.mark.gpu


def rows_of(aligned, groups):
    """the rows a groups call returned, as the models take them: a skipped group is its number of instances"""
    return [al.rows if al.status == 0 else len(g) for al, g in zip(aligned, groups)]


def same(got, want):
    (M, C_, K), (wM, wC, wK) = got, want
    assert (C_, K) == (wC, wK)
    assert M.shape == wM.shape and M.dtype == np.uint64 and (M == wM).all(), np.argwhere(M != wM)[:5]


def check(groups, cls, nclass, replicates, seed, draws=0, want=None, revs=None, wide=False):
    from sibelia_amd import BlockFinder
    b = Groups(groups, revs)
    bf = BlockFinder(b.records, device=0)
    try:
        bf.set_wide(wide)
        aligned = bf.align_groups(b.desc)
        got = bf.group_bootstrap(cls, nclass, replicates, seed, draws, want)
        k, c = bf.group_bootstrap_times()
        assert k >= 0 and c >= 0
        same(got, BM.counts(rows_of(aligned, groups), cls, nclass, replicates, seed, draws, want))
        return aligned, got
    finally:
        bf.close()


@pytest.mark.parametrize("name", sorted(n for n, c in BC.CASES.items() if not c["refused"]))
def test_crafted_calls_one_by_one(name):
    c = BC.CASES[name]
    aligned, (M, nsites, _) = check(c["groups"], c["cls"], c["nclass"], c["replicates"], c["seed"], c["draws"], c["want"])
    if c["sites"] is not None:                                                   # the case is what it says on the rows the device made
        assert nsites == c["sites"] and [al.rows for al in aligned] == c["groups"]
    if name == "draws_70000_on_one_site":
        assert M[1].tolist() == M[2].tolist() == [[0, 70000], [70000, 0]]
    if name == "draws_70000_on_two_sites":
        assert M[1][1][2] == M[2][1][2] == 70000 and min(int(M[1][0][1]), int(M[1][0][2])) > 255


def test_crafted_groups_of_equal_nclass_in_one_call():
    """sites on the first and the last column of groups of 1, 2, 3, 15, 16 and 17 columns next to each other, and every other crafted
    group of two and of three classes: sites of several groups in one 16-column piece"""
    by_n = {}
    for name in sorted(BC.CASES):
        c = BC.CASES[name]
        if c["refused"] or c["want"] is not None or c["nclass"] not in (2, 3) or len(c["groups"][0][0]) > 3000:
            continue
        groups, cls = by_n.setdefault(c["nclass"], ([], []))
        groups += c["groups"]
        cls += c["cls"]
    assert len(by_n[2][0]) > 10 and len(by_n[3][0]) > 10
    for n, (groups, cls) in sorted(by_n.items()):
        _, (M, nsites, _) = check(groups, cls, n, 5, 3)
        assert nsites > 20


def test_one_wide_group():
    """4 x 200 kbp with about 50 000 sites: many workgroups per phase, several chunks of draws per replicate.  Every member differs from
    the centre in every twelfth column, the three of them in columns of their own, by a base the centre holds neither there nor next to
    it: lone substitutions that no shift repays.  Members 8 % away from the centre need a band beyond the LDS classes: aligned with
    the wide band setting.  The counts are compared on the rows the device made, whatever they are"""
    rng = np.random.default_rng(94)
    base = np.frombuffer(MC.rand(rng, 200000), dtype=np.uint8)
    group = [base.tobytes()]
    for k in range(3):
        b = base.copy()
        at = np.arange(12 + 4 * k, len(base) - 12, 12)
        for y in b"ACGT":
            b[at] = np.where((base[at - 1] != y) & (base[at] != y) & (base[at + 1] != y), y, b[at])
        assert (b[at] != base[at]).all()
        group.append(b.tobytes())
    aligned, (M, nsites, nclean) = check([group], [3, 1, 0, 2], 4, 3, 1, wide=True)
    assert aligned[0].status == 0 and aligned[0].L >= 200000
    assert 45000 < nsites < 52500 and nsites < nclean <= aligned[0].L and 30000 < int(M[1][0][1]) < 40000


def test_replicates_on_both_sides_of_a_batch(monkeypatch):
    """the count slabs of one batch fit a budget of device memory; with 1 KiB of it two slabs of 8 x 8 do"""
    from sibelia_amd import BlockFinder
    c = BC.CASES["replicates_1000_on_few_sites"]
    b = Groups(c["groups"])
    bf = BlockFinder(b.records, device=0)
    try:
        rows = rows_of(bf.align_groups(b.desc), c["groups"])
        whole = BM.counts(rows, c["cls"], 8, 7, 9)
        for budget in ("1", "2", None):
            if budget:
                monkeypatch.setenv("SBL_TEST_BOOT_BUDGET_KB", budget)
            else:
                monkeypatch.delenv("SBL_TEST_BOOT_BUDGET_KB")
            for B in (0, 1, 2, 3, 4, 5, 7):
                M, nsites, K = bf.group_bootstrap(c["cls"], 8, B, 9)
                same((M, nsites, K), (whole[0][:B + 1], whole[1], whole[2]))
    finally:
        bf.close()


def test_two_calls_in_a_row_with_different_seeds():
    from sibelia_amd import BlockFinder
    c = BC.CASES["seed_1"]
    b = Groups(c["groups"])
    bf = BlockFinder(b.records, device=0)
    try:
        rows = rows_of(bf.align_groups(b.desc), c["groups"])
        first = bf.group_bootstrap(c["cls"], 4, 4, 1)
        second = bf.group_bootstrap(c["cls"], 4, 6, 2, 33)
        third = bf.group_bootstrap(c["cls"], 4, 4, 1)
        same(first, BM.counts(rows, c["cls"], 4, 4, 1))
        same(second, BM.counts(rows, c["cls"], 4, 6, 2, 33))
        same(third, first)
        assert first[0][1].tolist() != second[0][1].tolist() and first[0][0].tolist() == second[0][0].tolist()
    finally:
        bf.close()


def test_want_mask_and_a_skipped_group(monkeypatch):
    rng = np.random.default_rng(45)
    groups = [DC.indel_group(rng, 4, 60) for _ in range(9)]
    c = MC.rand(rng, 50)
    groups[4] = [c, MC.mutated(rng, c, 0.05, 5), MC.rand(rng, 900), c[:30]]      # as tests/test_gpu_multi_align.py: the second member is beyond a cap of 4 KiB
    b = Groups(groups)
    cls = [0, 1, 2, 3] * 9
    from sibelia_amd import BlockFinder
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    bf = BlockFinder(b.records, device=0)
    try:
        capped = bf.align_groups(b.desc)
        monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
        assert [g.status for g in capped] == [0, 0, 0, 0, 1, 0, 0, 0, 0]
        rows = rows_of(capped, groups)
        seen = []
        for want in (None, [k not in (1, 7) for k in range(9)], [k == 4 for k in range(9)], [False] * 9):
            got = bf.group_bootstrap(cls, 4, 3, 1, 0, want)
            same(got, BM.counts(rows, cls, 4, 3, 1, 0, want))
            seen.append(got[1])
        assert seen[0] > seen[1] > 0 and seen[2:] == [0, 0] and not got[0].any() and got[2] == 0
        with pytest.raises(ValueError):
            bf.group_bootstrap(cls, 4, 3, 1, 0, [True] * 8)
    finally:
        bf.close()


def test_reverse_centre_and_reverse_members():
    rng = np.random.default_rng(41)
    c = MC.rand(rng, 150)
    g = [c, MC.mutated(rng, c), MC.mutated(rng, c), b"TT" + c[:70] + b"GAG" + c[70:]]
    revs = [[True, False, False, False], [False, True, True, True], [True, True, False, True], [False] * 4]
    _, (_, nsites, _) = check([g, g, g, g], [0, 1, 2, 3] * 4, 4, 3, 1, revs=revs)
    assert nsites > 8


def test_seeded_random_groups_with_n_and_indels():
    rng = np.random.default_rng(195)
    groups = []
    for _ in range(40):
        c = MC.rand(rng, int(rng.integers(0, 301)), b"ACGTACGTACGTN")
        groups.append([c] + [MC.mutated(rng, c, 0.05, 8)[:300] for _ in range(4)])
    cls = [int(x) for _ in groups for x in rng.permutation(5)]
    aligned, (_, nsites, nclean) = check(groups, cls, 5, 4, 2 ** 64 - 1)
    assert [g.status for g in aligned] == [0] * 40 and 50 < nsites < nclean < sum(g.L for g in aligned)


def test_masked_rows_and_back():
    """after sbl_group_mask with the setting on the counts are those of the masked rows, with it off again those of the rows"""
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    rng = np.random.default_rng(77)
    c = MC.rand(rng, 400)
    groups = [[c, KC.subst(c, [10, 12, 14, 100, 200, 300]), KC.subst(c, [50, 150, 250, 252, 254, 256, 350])], [c[:90], KC.subst(c[:90], [5, 40]), KC.subst(c[:90], [41, 80])]]
    b = Groups(groups)
    cls = [2, 0, 1, 0, 1, 2]
    bf = BlockFinder(b.records, device=0)
    try:
        aligned = bf.align_groups(b.desc)
        assert [al.rows for al in aligned] == groups
        plain = BM.counts(groups, cls, 3, 5, 1)
        same(bf.group_bootstrap(cls, 3, 5, 1), plain)
        bf.set_masked(True)
        with pytest.raises(SibeliaError, match="bad argument"):                  # no mask yet
            bf.group_bootstrap(cls, 3, 5, 1)
        bf.set_masked(False)
        intervals, masked = KM.mask(groups, 10, 2)
        assert bf.group_mask(10, 2) == intervals and len(intervals) == 2
        same(bf.group_bootstrap(cls, 3, 5, 1), plain)                            # a mask with the setting off changes nothing
        bf.set_masked(True)
        hidden = BM.counts(masked, cls, 3, 5, 1)
        same(bf.group_bootstrap(cls, 3, 5, 1), hidden)
        assert hidden[1] == plain[1] - 7 and hidden[2] == plain[2] - 12          # the columns 10 .. 14 and 250 .. 256 hold an N now
        bf.set_masked(False)
        same(bf.group_bootstrap(cls, 3, 5, 1), plain)
    finally:
        bf.close()


def test_any_order_with_the_other_readers():
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(96)
    groups = [DC.indel_group(rng, 4, 120), DC.indel_group(rng, 4, 90), [MC.rand(rng, 30)] + [MC.rand(rng, 30)] * 3]
    b = Groups(groups)
    cls = [0, 1, 2, 3] * 3
    h = [b">class %d\n" % f for f in range(4)]
    seen = []
    for order in ("bvdc", "cbdv", "dcvb", "vdc"):
        bf = BlockFinder(b.records, device=0)
        try:
            rows = rows_of(bf.align_groups(b.desc), groups)
            out = {}
            for step in order:
                if step == "v":
                    out["v"] = bf.group_variants()
                elif step == "d":
                    out["d"] = bf.group_distances(cls, 4).tolist()
                elif step == "c":
                    out["c"] = [bf.group_concat(cls, 4, h, mode) for mode in (CM.ALL, CM.VARIABLE)]
                else:
                    out["b"] = bf.group_bootstrap(cls, 4, 3, 7)
                    same(out["b"], BM.counts(rows, cls, 4, 3, 7))
            seen.append((out["v"], out["d"], out["c"]))
        finally:
            bf.close()
    assert seen[0] == seen[1] == seen[2] == seen[3] and len(seen[0][0]) > 0      # the last order is without the new call
    assert seen[0][1] == DM.fold([DM.rows_counts(r) for r in rows], cls, 4).tolist()
    assert seen[0][2] == [CM.concat(rows, cls, 4, h, 80, mode) for mode in (CM.ALL, CM.VARIABLE)]


def test_refused_crafted_calls_name_the_group():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    names = sorted(n for n, c in BC.CASES.items() if c["refused"] and c["replicates"] <= 100000)
    assert len(names) == 3
    for name in names:
        c = BC.CASES[name]
        b = Groups(c["groups"])
        bf = BlockFinder(b.records, device=0)
        try:
            bf.align_groups(b.desc)
            at, bad = 0, None
            for g, group in enumerate(c["groups"]):                               # the first group that breaks the class rule
                if bad is None and sorted(c["cls"][at:at + len(group)]) != list(range(c["nclass"])):
                    bad = g
                at += len(group)
            with pytest.raises(SibeliaError, match="bad argument.*group %d .*a used group holds every class exactly once" % bad):
                bf.group_bootstrap(c["cls"], c["nclass"], 3, 1)
        finally:
            bf.close()


def raw_bootstrap(bf, want, cls, nclass, replicates, seed, draws, counts=True):
    out, nsites, nclean = C.POINTER(C.c_uint64)(), C.c_uint64(), C.c_uint64()
    fn = bf.L.sbl_group_bootstrap
    saved = fn.argtypes
    fn.argtypes = None                                                         # null pointers where the mirror has typed ones
    try:
        return fn(bf.h, want, cls, C.c_uint32(nclass), C.c_uint32(replicates), C.c_uint64(seed), C.c_uint32(draws), C.byref(out) if counts else None,
                  C.byref(nsites), C.byref(nclean))
    finally:
        fn.argtypes = saved


def test_bad_arguments_leave_the_context_usable(monkeypatch):
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    c = BC.CASES["sites_17"]
    b = Groups(c["groups"])
    bf = BlockFinder(b.records, device=0)
    try:
        good = BM.counts(c["groups"], c["cls"], 3, 2, 1)
        ok = lambda: same(bf.group_bootstrap(c["cls"], 3, 2, 1), good)          # noqa: E731
        with pytest.raises(SibeliaError, match="bad argument"):                  # before any groups call
            bf.group_bootstrap(c["cls"], 3, 2, 1)
        d = b.desc[0]
        bf.align_groups(b.desc)
        ok()
        bf.align_pairs([d[0] + d[1]])
        with pytest.raises(SibeliaError, match="bad argument"):                  # the last call was a pairs call
            bf.group_bootstrap(c["cls"], 3, 2, 1)
        bf.align_groups(b.desc)
        ok()
        for cls, nclass, replicates in (([0, 0, 0], 0, 2), ([0, 1, 2], 1025, 0), ([0, 1, 3], 3, 2), ([0, 1, 1], 3, 2), ([0, 1, 2], 4, 2), ([0, 1, 2], 2, 2), ([0, 1, 2], 3, 100001)):
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_bootstrap(cls, nclass, replicates, 1)
            ok()
        for replicates, seed, draws in ((2 ** 32, 1, 0), (2, 2 ** 64, 0), (2, -1, 0), (2, 1, 2 ** 32)):      # beyond their widths: never reach the library
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_bootstrap(c["cls"], 3, replicates, seed, draws)
        cls = (C.c_uint32 * 3)(*c["cls"])
        assert raw_bootstrap(bf, None, cls, 3, 2, 1, 0) == 0
        assert raw_bootstrap(bf, None, None, 3, 2, 1, 0) == 1
        assert raw_bootstrap(bf, None, cls, 3, 2, 1, 0, counts=False) == 1
        assert raw_bootstrap(bf, None, cls, 3, 100001, 1, 0) == 1
        ok()
        # the two limits, neither allocated for: 129 slabs of 1024 x 1024 cells are more than 2^27, refused before the groups are looked at;
        # the limit on the sites through its test switch
        with pytest.raises(SibeliaError, match="exceeds.*2\\^27 cells"):
            bf.group_bootstrap(c["cls"], 1024, 128, 1)
        with pytest.raises(SibeliaError, match="bad argument"):                  # 128 slabs are within it: the class rule speaks
            bf.group_bootstrap(c["cls"], 1024, 127, 1)
        monkeypatch.setenv("SBL_TEST_BOOT_MAX_SITES", "16")
        with pytest.raises(SibeliaError, match="exceeds.*too many variable columns"):
            bf.group_bootstrap(c["cls"], 3, 2, 1)
        monkeypatch.setenv("SBL_TEST_BOOT_MAX_SITES", "17")
        ok()
        monkeypatch.delenv("SBL_TEST_BOOT_MAX_SITES")
        ok()
    finally:
        bf.close()
