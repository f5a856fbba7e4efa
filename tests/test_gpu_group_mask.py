"""sbl_group_mask / sbl_group_set_masked (csrc/group_mask.hip: k_diff_flags, k_diff_fill, k_dense_start, k_dense_ends, k_mask_fill,
k_mask_rows) through BlockFinder.align_groups, BlockFinder.group_mask and the three readers against tests/gmask_model.py, exactly: every
interval, and every byte of the masked rows as group_concat(..., CONCAT_ALL) with identity classes spells them under set_masked(True)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import concat_model as CM                          # noqa: E402
import gdist_cases as DC                           # noqa: E402
import gdist_model as DM                           # noqa: E402
import gmask_cases as KC                           # noqa: E402
import gmask_model as KM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
import mvariants_model as MV                       # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402  (the layout of groups of strings as ranges of three records)

pytestmark = pytest.mark.gpu


def headers_of(n):
    return [b">row %d\n" % f for f in range(n)]


def rows_through_concat(bf, model_groups):
    """the rows the readers see, group by group: one CONCAT_ALL call per number of rows, the class of an instance its row.  Compared with
    the same call of the model on `model_groups`"""
    for r in sorted({CM.ninst(g) for g in model_groups}):
        want = [CM.ninst(g) == r for g in model_groups]
        cls = [i if CM.ninst(g) == r else 0 for g in model_groups for i in range(CM.ninst(g))]
        assert bf.group_concat(cls, r, headers_of(r), CM.ALL, 80, want) == CM.concat(model_groups, cls, r, headers_of(r), 80, CM.ALL, want), r


def check_on(bf, rows, W, T, want=None):
    """one mask call on the finder's last groups call, whose rows are `rows`: the intervals, then the masked rows"""
    intervals, masked = KM.mask(rows, W, T, want)
    assert bf.group_mask(W, T, want) == intervals
    k, c = bf.group_mask_times()
    assert k >= 0 and c >= 0
    bf.set_masked(True)
    try:
        rows_through_concat(bf, masked)
    finally:
        bf.set_masked(False)
    return intervals, masked


def check(groups, W, T, want=None, rows=None, revs=None):
    from sibelia_amd import BlockFinder
    rows = CM.rows_of(groups) if rows is None else rows
    b = Groups(groups, revs)
    bf = BlockFinder(b.records, device=0)
    try:
        got = bf.align_groups(b.desc)
        assert [al.rows for al in got] == rows                                   # the case's precondition, on the rows the device made
        return got, check_on(bf, rows, W, T, want)
    finally:
        bf.close()


@pytest.mark.parametrize("name", sorted(KC.CASES))
def test_crafted_cases_one_by_one(name):
    c = KC.CASES[name]
    got, (intervals, masked) = check(c["groups"], c["W"], c["T"], rows=KC.rows_of(c))
    assert intervals == KC.BY_HAND.get(name, intervals)
    if name == "word_bounds":
        assert got[0].row_off == 0 and got[0].L == 48
    if name == "short_rows":
        assert got[0].row_off == 0 and got[0].L == 5                             # rows 1 .. 3 share the word of bytes 0 .. 15 and the next
    if name == "column_edges":
        assert any(g.row_off % 16 for g in got)


def test_crafted_groups_in_one_call_per_parameter_pair():
    """the groups of every case with the same (W, T) in one call: rows that start anywhere in a word, intervals of many groups"""
    by_wt = {}
    for name in sorted(KC.CASES):
        c = KC.CASES[name]
        groups, rows = by_wt.setdefault((c["W"], c["T"]), ([], []))
        groups += c["groups"]
        rows += KC.rows_of(c)
    assert len(by_wt[(12, 2)][0]) == 3 and len(by_wt[(4, 1)][0]) > 10
    for (W, T), (groups, rows) in sorted(by_wt.items()):
        check(groups, W, T, rows=rows)


def test_reverse_centre_and_reverse_members():
    c = KC.CASES["insertion_inside"]
    g = c["groups"][0]
    rows = KC.rows_of(c)
    revs = [[True, False, False], [False, True, True], [True, True, False], [False] * 3]
    _, (intervals, _) = check([g, g, g, g], c["W"], c["T"], rows=rows * 4, revs=revs)
    assert len(intervals) == 8


def test_more_rows_than_a_wave():
    c = KC._centre(70, 200)
    g = [c] + [KC.subst(c, [(i * 7) % 180 + d for d in ((0, 3, 6) if i % 3 else (0, 9))]) for i in range(1, 70)]
    _, (intervals, _) = check([g], 8, 2, rows=[g])
    assert len(intervals) == sum(1 for i in range(1, 70) if i % 3) and {iv[1] for iv in intervals} == {i for i in range(1, 70) if i % 3}


def wide_group():
    """4 x 200 kbp: in every member 30 clusters of 4 differences 3 columns apart and 40 lone differences, all at least 50 columns apart"""
    rng = np.random.default_rng(93)
    c = MC.rand(rng, 200000)
    group = [c]
    for _ in range(3):
        at = sorted(int(x) * 50 + 10 for x in rng.choice(3990, 70, replace=False))
        rng.shuffle(at)
        group.append(KC.subst(c, [x + d for x in at[:30] for d in (0, 3, 6, 9)] + at[30:]))
    return group


def test_one_wide_group():
    """many workgroups per row in every pass"""
    group = wide_group()
    got, (intervals, masked) = check([group], 12, 3, rows=[group])
    assert got[0].status == 0 and got[0].L == 200000
    assert len(intervals) == 90 and all(iv[6] == 4 and iv[3] - iv[2] == 9 for iv in intervals)
    assert sum(r.count(b"N") for r in masked[0]) == 900


def test_seeded_random_groups():
    groups = MC.random_groups(195, 40, 1, 5, 300, 8)
    rows = CM.rows_of(groups)
    from sibelia_amd import BlockFinder
    b = Groups(groups)
    bf = BlockFinder(b.records, device=0)
    try:
        got = bf.align_groups(b.desc)
        assert [al.rows for al in got] == rows
        for W, T in ((20, 2), (50, 4)):
            intervals, masked = check_on(bf, rows, W, T)                          # two masks in a row with different parameters
            inside = sum(iv[6] for iv in intervals)
            total = sum(len(KM.differences(r, i)) for r in rows for i in range(1, len(r)))
            assert len(intervals) >= 1 and total > inside                         # at least one interval, at least one unmasked difference
    finally:
        bf.close()


def test_want_mask_one_row_a_skipped_group_and_an_empty_centre(monkeypatch):
    rng = np.random.default_rng(45)
    c = KC.C64
    dense = [c, KC.subst(c, [10, 12, 14, 40]), KC.subst(c, [30, 33, 36])]
    groups = [dense, [c], dense, [b"", b"ACG", b""], [c, KC.subst(c, [5, 6]), MC.rand(rng, 900)], dense, [b"", b""]]
    b = Groups(groups)
    from sibelia_amd import BlockFinder
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")                             # as tests/test_gpu_group_concat.py: the second member of group 4 is beyond the cap
    bf = BlockFinder(b.records, device=0)
    try:
        got = bf.align_groups(b.desc)
        monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
        assert [g.status for g in got] == [0, 0, 0, 0, 1, 0, 0] and got[3].L == 3 and got[6].L == 0
        rows = [dense, [c], dense, [b"---", b"ACG", b"---"], 3, dense, [b"", b""]]
        assert [al.rows for al in got if al.status == 0] == [r for r in rows if r != 3]
        for want in (None, [k not in (0, 5) for k in range(7)], [k in (1, 3, 4, 6) for k in range(7)], [False] * 7):
            intervals, masked = check_on(bf, rows, 8, 2, want)
            assert {iv[0] for iv in intervals} == {g for g in (0, 2, 5) if want is None or want[g]}
        assert masked == rows
        with pytest.raises(ValueError):
            bf.group_mask(8, 2, [True] * 6)
    finally:
        bf.close()


def readers(bf, cls, nclass, h):
    return {"v": bf.group_variants(), "d": bf.group_distances(cls, nclass).tolist(), "c": [bf.group_concat(cls, nclass, h, mode) for mode in (CM.ALL, CM.VARIABLE)]}


def readers_model(rows, cls, nclass, h):
    return {"v": [(g, s, e, before, lead, slices) for g, r in enumerate(rows) for s, e, before, lead, _, slices in MV.segments(r)],
            "d": DM.fold([DM.rows_counts(r) for r in rows], cls, nclass).tolist(),
            "c": [CM.concat(rows, cls, nclass, h, 80, mode) for mode in (CM.ALL, CM.VARIABLE)]}


def test_the_setting_off_is_today_and_on_is_the_model_on_the_masked_rows():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import GroupInst
    rng = np.random.default_rng(96)
    c = KC.C200
    groups = [DC.indel_group(rng, 4, 120), [c, KC.subst(c, [20, 23, 26, 100]), KC.subst(c, [60, 150, 152, 154]), KC.subst(c, [5])], DC.indel_group(rng, 4, 90)]
    b = Groups(groups)
    cls, h = [0, 1, 2, 3, 2, 0, 3, 1, 3, 2, 1, 0], headers_of(4)
    rows = CM.rows_of(groups)
    intervals, masked = KM.mask(rows, 10, 2)
    assert len(intervals) >= 2 and masked != rows
    plain, hidden = readers_model(rows, cls, 4, h), readers_model(masked, cls, 4, h)
    first = [0]
    for d in b.desc:
        first.append(first[-1] + len(d))
    assert plain["v"] != hidden["v"] and plain["d"] != hidden["d"] and plain["c"] != hidden["c"]
    for order in ("vdc", "cdv", "dcv"):
        bf = BlockFinder(b.records, device=0)
        try:
            inst = (GroupInst * len(cls))()
            for d, i in zip(inst, [i for g in b.desc for i in g]):
                d.chr, d.start, d.end, d.rev = [int(x) for x in i]
            res, members, text, text_len = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
            assert bf.L.sbl_align_groups(bf.h, len(groups), (C.c_uint64 * len(first))(*first), inst, C.byref(res), C.byref(members), C.byref(text), C.byref(text_len)) == 0
            got = bf._group_alignments(first, res, members, text, text_len)
            held = C.string_at(text.value, text_len.value)                       # the rows of the groups call, where the library left them
            assert [al.rows for al in got] == rows and bf.masked == 0
            assert readers(bf, cls, 4, h) == plain
            assert bf.group_mask(10, 2) == intervals
            assert readers(bf, cls, 4, h) == plain                               # a mask with the setting off changes nothing
            assert C.string_at(text.value, text_len.value) == held
            bf.set_masked(True)
            assert bf.masked == 1
            out = {}
            for step in order:
                out[step] = {"v": bf.group_variants, "d": lambda: bf.group_distances(cls, 4).tolist(),
                             "c": lambda: [bf.group_concat(cls, 4, h, mode) for mode in (CM.ALL, CM.VARIABLE)]}[step]()
            assert out == hidden, order
            bf.set_masked(False)
            assert readers(bf, cls, 4, h) == plain
            assert C.string_at(text.value, text_len.value) == held
        finally:
            bf.close()


def test_two_masks_in_a_row_and_a_new_groups_call():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    c = KC.C64
    groups = [[c, KC.subst(c, [10, 12, 14, 30, 40, 50])]]
    b = Groups(groups)
    cls, h = [0, 1], headers_of(2)
    bf = BlockFinder(b.records, device=0)
    try:
        bf.align_groups(b.desc)
        first, _ = check_on(bf, groups, 6, 2)
        second, _ = check_on(bf, groups, 21, 1)
        third, _ = check_on(bf, groups, 6, 2)
        assert first == third == [(0, 1, 10, 14, 10, 14, 3)] and second == [(0, 1, 10, 50, 10, 50, 6)]
        bf.set_masked(True)
        bf.align_groups(b.desc)                                                  # new rows: the mask of the old ones is gone
        for call in (bf.group_variants, lambda: bf.group_distances(cls, 2), lambda: bf.group_concat(cls, 2, h, CM.ALL)):
            with pytest.raises(SibeliaError, match="bad argument"):
                call()
        bf.set_masked(False)
        assert bf.group_concat(cls, 2, h, CM.ALL) == CM.concat(groups, cls, 2, h, 80, CM.ALL)
        check_on(bf, groups, 6, 2)
    finally:
        bf.close()


def test_bad_arguments_leave_the_context_usable():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    c = KC.C64
    groups = [[c, KC.subst(c, [10, 12, 14])]]
    b = Groups(groups)
    cls, h = [0, 1], headers_of(2)
    bf = BlockFinder(b.records, device=0)
    try:
        with pytest.raises(SibeliaError, match="bad argument"):                  # before any groups call
            bf.group_mask(6, 2)
        d = b.desc[0]
        bf.align_groups(b.desc)
        first, masked = check_on(bf, groups, 6, 2)
        assert first == [(0, 1, 10, 14, 10, 14, 3)]
        bf.set_masked(True)
        for W, T in ((0, 2), (6, 0), (0, 0)):
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_mask(W, T)
            rows_through_concat(bf, masked)                                      # a refused call leaves the earlier mask valid
        for W, T in ((2 ** 32, 2), (6, 2 ** 32), (-1, 2)):                       # beyond 32 bits: never reaches the library
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_mask(W, T)
        for on in (2, 2 ** 32 - 1, 2 ** 32, -1):
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.set_masked(on)
            assert bf.masked == 1
        bf.set_masked(False)
        assert bf.group_mask(2 ** 32 - 1, 2 ** 32 - 1) == [] and bf.group_mask(2 ** 32 - 1, 2) == first
        bf.align_pairs([d[0] + d[1]])
        with pytest.raises(SibeliaError, match="bad argument"):                  # the last call was a pairs call
            bf.group_mask(6, 2)
        bf.set_masked(True)
        bf.align_groups(b.desc)
        for call in (bf.group_variants, lambda: bf.group_distances(cls, 2), lambda: bf.group_concat(cls, 2, h, CM.ALL)):
            with pytest.raises(SibeliaError, match="bad argument"):              # the setting on without a mask
                call()
        assert bf.group_mask(6, 2) == first
        rows_through_concat(bf, masked)
    finally:
        bf.close()
