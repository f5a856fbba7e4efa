"""sbl_group_set_partial (csrc/sbl_groups.h, group_concat.hip, group_boot.hip: the partial instantiations of k_site_flags,
k_concat_text, k_boot_pack and k_boot_count, and k_boot_clean_groups) through BlockFinder against tests/softcore_model.py on the rows the
groups call returned, exactly: text, parts, sites, every cell of every slab, the sites, the clean columns and the clean columns per pair."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_cases as BC                            # noqa: E402
import boot_model as BM                            # noqa: E402
import concat_model as CM                          # noqa: E402
import gmask_cases as KC                           # noqa: E402
import gmask_model as KM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
import softcore_cases as SC                        # noqa: E402
import softcore_model as SM                        # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402

pytestmark = pytest.mark.gpu


def rows_of(aligned, groups):
    return [al.rows if al.status == 0 else len(g) for al, g in zip(aligned, groups)]


def same_counts(bf, got, want):
    (M, C_, K), (wM, wC, wK, wclean) = got, want
    assert (C_, K) == (wC, wK)
    assert M.shape == wM.shape and M.dtype == np.uint64 and (M == wM).all(), np.argwhere(M != wM)[:5]
    clean = bf.group_bootstrap_pairs()
    assert clean.shape == wclean.shape and clean.dtype == np.uint64 and (clean == wclean).all(), np.argwhere(clean != wclean)[:5]


def compare(bf, rows, c, want="case"):
    """every output of both readers with the setting on, against the model on `rows`"""
    want = c["want"] if want == "case" else want
    for width in c["widths"]:
        for mode in (SM.ALL, SM.VARIABLE):
            assert bf.group_concat(c["cls"], c["nclass"], c["headers"], mode, width, want) == SM.concat_partial(rows, c["cls"], c["nclass"], c["headers"], width, mode, want), (width, mode)
    got = bf.group_bootstrap(c["cls"], c["nclass"], c["replicates"], c["seed"], c["draws"], want)
    model = SM.counts_partial(rows, c["cls"], c["nclass"], c["replicates"], c["seed"], c["draws"], want)
    same_counts(bf, got, model)
    return got, model


class Finder:
    """a finder with the groups of strings aligned and the setting on"""

    def __init__(self, groups, revs=None, partial=True):
        from sibelia_amd import BlockFinder
        self.groups = groups
        self.b = Groups(groups, revs)
        self.bf = BlockFinder(self.b.records, device=0)
        self.partial = partial

    def __enter__(self):
        try:
            self.bf.set_partial(self.partial)
            self.aligned = self.bf.align_groups(self.b.desc)
            self.rows = rows_of(self.aligned, self.groups)
        except BaseException:
            self.bf.close()
            raise
        return self

    def __exit__(self, *a):
        self.bf.close()


@pytest.mark.parametrize("name", sorted(n for n, c in SC.CASES.items() if not c["refused"]))
def test_crafted_calls_one_by_one(name):
    c = SC.CASES[name]
    with Finder(c["groups"]) as f:
        (M, nsites, _), _ = compare(f.bf, f.rows, c)
        if name == "draws_70000_one_site_class_1_absent":
            assert nsites == 1 and M[1].tolist() == [[0, 0, 70000], [0, 0, 0], [70000, 0, 0]]
        if name == "gap_fill_next_to_a_neighbour":
            assert f.rows == c["groups"]


def test_crafted_calls_of_three_classes_together():
    groups, cls = [], []
    for name in sorted(SC.CASES):
        c = SC.CASES[name]
        if not c["refused"] and c["nclass"] == 3:
            groups += c["groups"]
            cls += c["cls"]
    assert len(groups) > 20
    c = SC.case(groups, cls, 3, widths=(80, 16, 1), replicates=5, seed=3)
    with Finder(groups) as f:
        (_, nsites, _), _ = compare(f.bf, f.rows, c)
        assert nsites > 15


@pytest.mark.parametrize("L", [15, 16, 17, 255, 256, 257, 4095, 4096, 4097])
def test_columns_on_either_side_of_a_piece_a_wave_and_a_workgroup_with_the_second_class_absent(L):
    rng = np.random.default_rng(L)
    centre = BC.rand(rng, L)
    member = bytearray(centre)
    for at in [0, L - 1] + list(range(4, L - 4, 7)):                             # apart from each other: no shift repays two of them
        member[at] = BC.other(centre[at])
    c = SC.case([[centre, bytes(member)], SC._SETS[0], [centre[:9]]], [0, 2, 2, 1, 0, 1], 3, widths=(80, 17), replicates=2)
    with Finder(c["groups"]) as f:
        assert f.rows == c["groups"]
        (_, nsites, nclean), (_, _, _, clean) = compare(f.bf, f.rows, c)
        assert nsites >= 3 and clean[0][2] == L + 20 and clean[1][1] == 20 + 9 and clean[0][1] == 20


def test_two_copies_of_a_wide_group_each_without_one_class():
    """4 x 20 kbp twice over five classes: the first copy lacks class 4, the second class 1; every member differs from the centre in every
    fiftieth column, in columns of its own"""
    rng = np.random.default_rng(1203)
    base = np.frombuffer(MC.rand(rng, 20000), dtype=np.uint8)
    group = [base.tobytes()]
    for k in range(3):
        b = base.copy()
        at = np.arange(50 + 7 * k, len(base) - 50, 50)
        for y in b"ACGT":
            b[at] = np.where((base[at - 1] != y) & (base[at] != y) & (base[at + 1] != y), y, b[at])
        group.append(b.tobytes())
    c = SC.case([group, group], [3, 1, 0, 2, 0, 4, 2, 3], 5, widths=(80,), replicates=3)
    with Finder(c["groups"]) as f:
        assert [al.status for al in f.aligned] == [0, 0]
        (M, nsites, nclean), (_, _, _, clean) = compare(f.bf, f.rows, c)
        assert nsites > 2000 and clean[1][4] == 0 and clean[0][0] == nclean and 0 < clean[1][1] < nclean and M[0][1][4] == 0 and M[0][0][1] > 300


@pytest.mark.parametrize("seed", [1204, 1205])
def test_forty_random_calls(seed):
    """forty calls laid out in ONE groups call: call k is the want mask of its groups, and the other groups' instances get class 0 (an
    unwanted group is not looked at)"""
    rng = np.random.default_rng(seed)
    calls = [SC.random_call(rng, full=k % 5 == 0) for k in range(40)]
    groups = [g for c in calls for g in c["groups"]]
    with Finder(groups) as f:
        g0 = i0 = partial = 0
        ninst = sum(len(g) for g in groups)
        for c in calls:
            want = [g0 <= g < g0 + len(c["groups"]) for g in range(len(groups))]
            cls = [0] * ninst
            cls[i0:i0 + len(c["cls"])] = c["cls"]
            compare(f.bf, f.rows, dict(c, cls=cls), want)
            partial += any(len(g) < c["nclass"] for g in c["groups"])
            g0 += len(c["groups"])
            i0 += len(c["cls"])
        assert partial >= 20


def test_replicates_in_several_batches(monkeypatch):
    """33 x 33 cells are more than the budget of 1 KiB: one slab per batch"""
    c = dict(SC.CASES["classes_33_absent_31"], replicates=5, widths=[80])
    with Finder(c["groups"]) as f:
        whole, _ = compare(f.bf, f.rows, c)
        monkeypatch.setenv("SBL_TEST_BOOT_BUDGET_KB", "1")
        again, _ = compare(f.bf, f.rows, c)
        assert (whole[0] == again[0]).all() and whole[0][1:].any()


def test_reverse_instances():
    c = SC.CASES["presence_sets_permuted_rows"]
    revs = [[True, False, True], [False, True], [True, True], [False, False], [True]]
    with Finder(c["groups"], revs) as f:
        assert f.rows == c["groups"]
        compare(f.bf, f.rows, c)


def test_masked_rows_with_the_setting_on():
    rng = np.random.default_rng(77)
    s = MC.rand(rng, 400)
    groups = [[s, KC.subst(s, [10, 12, 14, 100, 200, 300]), KC.subst(s, [50, 150, 250, 252, 254, 256, 350])], [s[:90], KC.subst(s[:90], [5, 40])], [s[:33]]]
    c = SC.case(groups, [2, 0, 1, 0, 2, 1], 3, widths=(80,), replicates=3)
    with Finder(groups) as f:
        assert f.rows == groups
        plain, _ = compare(f.bf, f.rows, c)
        intervals, masked = KM.mask(groups, 10, 2)
        assert f.bf.group_mask(10, 2) == intervals and len(intervals) == 2
        compare(f.bf, f.rows, c)                                                 # a mask with the masked setting off changes nothing
        f.bf.set_masked(True)
        hidden, _ = compare(f.bf, masked, c)
        assert hidden[1] == plain[1] - 7 and hidden[2] == plain[2] - 12
        f.bf.set_masked(False)
        compare(f.bf, f.rows, c)


def test_want_mask_and_a_skipped_group(monkeypatch):
    rng = np.random.default_rng(45)
    groups = [list(g) for g in SC.CASES["presence_sets"]["groups"]]
    s = MC.rand(rng, 50)
    groups.insert(2, [s, MC.mutated(rng, s, 0.05, 5), MC.rand(rng, 900)])          # as tests/test_gpu_multi_align.py: beyond a cap of 4 KiB
    cls = [0, 1, 2, 0, 2, 0, 1, 2, 0, 1, 1, 2, 2]
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    with Finder(groups) as f:
        monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
        assert [al.status for al in f.aligned] == [0, 0, 1, 0, 0, 0]
        c = SC.case(groups, cls, 3, widths=(80, 5))
        seen = []
        for want in (None, [k != 1 for k in range(6)], [k == 2 for k in range(6)], [False] * 6):
            (_, nsites, _), _ = compare(f.bf, f.rows, c, want)
            seen.append(nsites)
        assert seen[0] > seen[1] > 0 and seen[2:] == [0, 0]


def test_full_calls_answer_alike_with_the_setting_on_and_off():
    """on calls whose groups all hold every class the partial instantiations give what the strict ones give, byte for byte"""
    from sibelia_amd import BlockFinder
    names = ["classes_in_permuted_row_order", "codes_gap_and_edges", "header_lengths", "thirty_three_classes", "centre_of_length_0", "short_groups_width_80", "one_class"]
    names += ["classes_%d" % n for n in (9, 33, 65, 70)] + ["sites_257", "replicates_65", "draws_70000_on_two_sites"]
    for name in names:
        c = BC.CASES[name]
        h = [b">class %d\n" % k for k in range(c["nclass"])]
        b = Groups(c["groups"])
        bf = BlockFinder(b.records, device=0)
        try:
            bf.align_groups(b.desc)
            out = []
            for on in (False, True):
                bf.set_partial(on)
                texts = [bf.group_concat(c["cls"], c["nclass"], h, mode, w, c["want"]) for mode in (CM.ALL, CM.VARIABLE) for w in (80, 16)]
                M, nsites, nclean = bf.group_bootstrap(c["cls"], c["nclass"], c["replicates"], c["seed"], c["draws"], c["want"])
                clean = bf.group_bootstrap_pairs()
                assert (clean == nclean).all()
                out.append((texts, M.tolist(), nsites, nclean))
            assert out[0] == out[1], name
        finally:
            bf.close()


def test_the_setting_off_refuses_a_partial_group_as_before():
    from sibelia_amd.api import SibeliaError
    c = SC.CASES["presence_sets"]
    with Finder(c["groups"], partial=False) as f:
        for call in (lambda: f.bf.group_concat(c["cls"], 3, c["headers"], CM.ALL), lambda: f.bf.group_bootstrap(c["cls"], 3, 2, 1)):
            with pytest.raises(SibeliaError, match="bad argument.*group 1 has fewer instances than there are classes: a used group holds every class exactly once"):
                call()
        f.bf.set_partial(True)
        compare(f.bf, f.rows, c)


@pytest.mark.parametrize("name", sorted(n for n, c in SC.CASES.items() if c["refused"]))
def test_refused_crafted_calls_name_the_group(name):
    from sibelia_amd.api import SibeliaError
    c = SC.CASES[name]
    what = {"group_with_a_class_twice": "group 1 holds a class twice", "four_rows_for_three_classes": "group 0 has more instances than there are classes"}[name]
    with Finder(c["groups"]) as f:
        for call in (lambda: f.bf.group_concat(c["cls"], 3, c["headers"], CM.VARIABLE), lambda: f.bf.group_bootstrap(c["cls"], 3, 2, 1)):
            with pytest.raises(SibeliaError, match="bad argument.*%s: a used group holds every class exactly once" % what):
                call()
        with pytest.raises(SibeliaError, match="bad argument.*a class is not below"):
            f.bf.group_bootstrap([3] + c["cls"][1:], 3, 2, 1)


def test_the_other_readers_do_not_look_at_the_setting():
    c = SC.CASES["presence_sets"]
    s = MC.rand(np.random.default_rng(5), 200)
    groups = c["groups"] + [[s, KC.subst(s, [10, 12, 14, 100]), KC.subst(s, [50, 150])]]
    cls = c["cls"] + [0, 1, 2]
    with Finder(groups, partial=False) as f:
        seen = []
        for on in (False, True, False):
            f.bf.set_partial(on)
            seen.append((f.bf.group_distances(cls, 3).tolist(), f.bf.group_variants(), f.bf.group_mask(10, 2)))
        assert seen[0] == seen[1] == seen[2] and seen[0][1] and seen[0][2]


def test_the_setting_survives_a_groups_call_and_bad_values_leave_it():
    from sibelia_amd.api import SibeliaError
    c = SC.CASES["presence_sets"]
    with Finder(c["groups"], partial=False) as f:
        assert f.bf.partial == 0
        for bad in (2, 2 ** 32 - 1, 2 ** 32, -1):
            with pytest.raises(SibeliaError, match="bad argument"):
                f.bf.set_partial(bad)
        assert f.bf.partial == 0
        f.bf.set_partial(True)
        with pytest.raises(SibeliaError, match="bad argument"):
            f.bf.set_partial(2)
        assert f.bf.partial == 1
        f.bf.align_groups(f.b.desc)
        assert f.bf.partial == 1
        compare(f.bf, f.rows, c)
        f.bf.set_partial(False)
        assert f.bf.partial == 0


def test_two_bootstrap_calls_in_a_row_on_and_then_off():
    from sibelia_amd.api import SibeliaError
    c, full = SC.CASES["presence_sets"], BC.CASES["seed_1"]
    groups = c["groups"] + full["groups"]
    with Finder(groups) as f:
        with pytest.raises(SibeliaError, match="bad argument"):                  # no bootstrap call yet
            f.bf.group_bootstrap_pairs()
        first = [k < len(c["groups"]) for k in range(len(groups))]
        cls3 = c["cls"] + [0] * 4
        same_counts(f.bf, f.bf.group_bootstrap(cls3, 3, 3, 1, 0, first), SM.counts_partial(f.rows, cls3, 3, 3, 1, 0, first))
        f.bf.set_partial(False)
        cls4 = [0] * len(c["cls"]) + full["cls"]
        rest = [not x for x in first]
        M, nsites, nclean = f.bf.group_bootstrap(cls4, 4, 4, 1, 0, rest)
        wM, wC, wK = BM.counts(f.rows, cls4, 4, 4, 1, 0, rest)
        assert (M == wM).all() and (nsites, nclean) == (wC, wK) and f.bf.group_bootstrap_pairs().tolist() == [[wK] * 4] * 4
        with pytest.raises(SibeliaError, match="bad argument"):                  # a refused call ...
            f.bf.group_bootstrap(cls3, 3, 3, 1, 0, first)
        f.bf.set_partial(True)
        same_counts(f.bf, f.bf.group_bootstrap(cls3, 3, 3, 1, 0, first), SM.counts_partial(f.rows, cls3, 3, 3, 1, 0, first))
