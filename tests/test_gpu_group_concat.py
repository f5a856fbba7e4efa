"""sbl_group_concat (csrc/group_concat.hip: k_site_flags, k_site_fill, k_concat_text) through BlockFinder.align_groups and
BlockFinder.group_concat against tests/concat_model.py, exactly: every byte of the text, every part, every site."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import concat_cases as CC                          # noqa: E402
import concat_model as CM                          # noqa: E402
import gdist_cases as DC                           # noqa: E402
import gdist_model as DM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402  (the layout of groups of strings as ranges of three records)

pytestmark = pytest.mark.gpu
MODES = (CM.ALL, CM.VARIABLE)


def headers_of(n):
    return [b">class %d\n" % f for f in range(n)]


def both_modes(b, cls, nclass, headers, width=80, want=None):
    """(alignments, [result of mode ALL, result of mode VARIABLE]) of the groups b on a context of its own"""
    from sibelia_amd import BlockFinder
    bf = BlockFinder(b.records, device=0)
    try:
        got = bf.align_groups(b.desc)
        out = []
        for mode in MODES:
            out.append(bf.group_concat(cls, nclass, headers, mode, width, want))
            k, c = bf.group_concat_times()
            assert k >= 0 and c >= 0
        return got, out
    finally:
        bf.close()


def check(groups, cls, nclass, headers, width=80, want=None, rows=None, revs=None, what=""):
    rows = CM.rows_of(groups) if rows is None else rows
    got, out = both_modes(Groups(groups, revs), cls, nclass, headers, width, want)
    for mode, res in zip(MODES, out):
        assert res == CM.concat(rows, cls, nclass, headers, width, mode, want), (what, mode)
    return got, out


@pytest.mark.parametrize("name", sorted(n for n, c in CC.CASES.items() if not c["refused"]))
def test_crafted_calls_one_by_one(name):
    c = CC.CASES[name]
    _, out = check(c["groups"], c["cls"], c["nclass"], c["headers"], c["width"], c["want"], what=name)
    if name in CC.BY_HAND:
        assert (out[0][0], out[1][0], out[1][2]) == CC.BY_HAND[name]


def test_crafted_groups_of_equal_nclass_in_one_call():
    by_n = {}
    for name in sorted(CC.CASES):
        c = CC.CASES[name]
        if c["refused"] or c["want"] is not None:
            continue
        groups, cls = by_n.setdefault(c["nclass"], ([], []))
        groups += c["groups"]
        cls += c["cls"]
    assert set(by_n) >= {1, 2, 3, 33} and len(by_n[2][0]) > 40
    for n, (groups, cls) in sorted(by_n.items()):
        for width in (13, 80):
            got, _ = check(groups, cls, n, headers_of(n), width, what=n)
        assert any(g.row_off % 16 for g in got) or len(got) == 1


def test_refused_crafted_calls_name_the_group():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    for name in sorted(n for n, c in CC.CASES.items() if c["refused"]):
        c = CC.CASES[name]
        b = Groups(c["groups"])
        bf = BlockFinder(b.records, device=0)
        try:
            bf.align_groups(b.desc)
            at, bad = 0, None
            for g, group in enumerate(c["groups"]):                               # the first group that breaks the class rule
                if bad is None and sorted(c["cls"][at:at + len(group)]) != list(range(c["nclass"])):
                    bad = g
                at += len(group)
            for mode in MODES:
                with pytest.raises(SibeliaError, match="bad argument.*group %d " % bad):
                    bf.group_concat(c["cls"], c["nclass"], c["headers"], mode, c["width"])
            want = [g != bad for g in range(len(c["groups"]))]                      # without the offending group the call stands
            if c["nclass"] == 2:
                assert bf.group_concat(c["cls"], 2, c["headers"], CM.ALL, 80, want) == CM.concat(CM.rows_of(c["groups"]), c["cls"], 2, c["headers"], 80, CM.ALL, want)
        finally:
            bf.close()


def other(base: int) -> int:
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def test_column_edges():
    """one group of three rows without indels, L on either side of 16 bytes, of a workgroup's flags (4096 columns) and of 256"""
    rng = np.random.default_rng(191)
    for n in (15, 16, 17, 255, 256, 257, 4095, 4096, 4097):
        c = MC.rand(rng, n)
        two, three = bytearray(c), bytearray(c)
        for at in range(7, n - 8, 50):                                           # lone substitutions, far from each other: the alignment is the identity
            two[at] = other(c[at])
        for at in range(11, n - 8, 60):
            three[at] = other(c[at])
        two[n - 1] = other(c[n - 1])                                             # the last column is a site: a byte more or less shows
        three[0] = other(c[0])                                                   # ... and so is the first
        g = [c, bytes(two), bytes(three)]
        got, out = check([g], [1, 2, 0], 3, headers_of(3), 80, rows=[g], what=n)
        assert got[0].L == n and out[1][2][0][:2] == (0, 0) and out[1][2][-1][:2] == (0, n - 1)


def test_more_rows_than_a_wave():
    rng = np.random.default_rng(192)
    c = MC.rand(rng, 200)
    g = [c]
    for i in range(1, 70):
        b = bytearray(c)
        b[(i * 17) % 200] = other(c[(i * 17) % 200])
        if i == 40:
            b[100] = ord("N")
        g.append(bytes(b))
    cls = [int(x) for x in rng.permutation(70)]
    got, out = check([g], cls, 70, headers_of(70), 61, rows=[g])
    assert got[0].L == 200 and len(out[1][2]) > 40


def test_one_wide_group():
    """4 x 200 kbp as tests/test_gpu_group_distances.py builds it: many workgroups per class row, both modes"""
    rng = np.random.default_rng(93)
    c = MC.rand(rng, 200000)
    group = [c]
    for n in (50, 70, 90):
        b = bytearray(c)
        for at in rng.choice(len(c), n, replace=False):
            b[at] = other(c[at])
        group.append(bytes(b))
    got, out = check([group], [3, 1, 0, 2], 4, headers_of(4), 80, rows=[group])
    assert got[0].status == 0 and got[0].L == len(c)
    assert 150 < len(out[1][2]) <= 210 and len(out[0][0]) == 4 * (len(b">class 0\n") + 200000 + 2500)


def test_reverse_centre_and_reverse_members():
    rng = np.random.default_rng(41)
    c = MC.rand(rng, 150)
    g = [c, MC.mutated(rng, c), MC.mutated(rng, c), b"TT" + c[:70] + b"GAG" + c[70:]]
    revs = [[True, False, False, False], [False, True, True, True], [True, True, False, True], [False] * 4]
    check([g, g, g, g], [0, 1, 2, 3] * 4, 4, headers_of(4), 80, revs=revs)


def test_want_mask_and_a_skipped_group(monkeypatch):
    rng = np.random.default_rng(45)
    groups = [DC.indel_group(rng, 4, 60) for _ in range(9)]
    c = MC.rand(rng, 50)
    groups[4] = [c, MC.mutated(rng, c, 0.05, 5), MC.rand(rng, 900), c[:30]]      # as tests/test_gpu_multi_align.py: the second member is beyond a cap of 4 KiB
    b = Groups(groups)
    cls = [0, 1, 2, 3] * 9
    h = headers_of(4)
    from sibelia_amd import BlockFinder
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    bf = BlockFinder(b.records, device=0)
    try:
        capped = bf.align_groups(b.desc)
        monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
        assert [g.status for g in capped] == [0, 0, 0, 0, 1, 0, 0, 0, 0]
        rows = CM.rows_of(groups, skipped=(4,))
        for want in (None, [k not in (1, 7) for k in range(9)], [k == 4 for k in range(9)], [False] * 9):
            for mode in MODES:
                res = bf.group_concat(cls, 4, h, mode, 80, want)
                assert res == CM.concat(rows, cls, 4, h, 80, mode, want)
        assert res == (b"".join(h), [], [])
        with pytest.raises(ValueError):
            bf.group_concat(cls, 4, h, CM.ALL, 80, [True] * 8)
    finally:
        bf.close()


def test_seeded_random_groups():
    rng = np.random.default_rng(195)
    groups = []
    for _ in range(40):
        c = MC.rand(rng, int(rng.integers(0, 301)), b"ACGTACGTACGTN")
        groups.append([c] + [MC.mutated(rng, c, 0.05, 8)[:300] for _ in range(4)])
    cls = [int(x) for _ in groups for x in rng.permutation(5)]
    got, out = check(groups, cls, 5, headers_of(5), 80)
    assert [g.status for g in got] == [0] * 40 and len(out[1][2]) > 50


def test_any_order_with_variants_and_distances_leaves_the_rows():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import GroupInst
    rng = np.random.default_rng(96)
    groups = [DC.indel_group(rng, 4, 120), DC.indel_group(rng, 4, 90), [MC.rand(rng, 30)] + [MC.rand(rng, 30)] * 3]
    b = Groups(groups)
    cls = [0, 1, 2, 3] * 3
    h = headers_of(4)
    first = [0]
    for d in b.desc:
        first.append(first[-1] + len(d))
    seen = []
    for order in ("vdc", "cdv", "dcv"):
        bf = BlockFinder(b.records, device=0)
        try:
            inst = (GroupInst * len(cls))()
            for d, i in zip(inst, [i for g in b.desc for i in g]):
                d.chr, d.start, d.end, d.rev = [int(x) for x in i]
            res, members, rows, rows_len = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
            assert bf.L.sbl_align_groups(bf.h, len(groups), (C.c_uint64 * len(first))(*first), inst, C.byref(res), C.byref(members), C.byref(rows), C.byref(rows_len)) == 0
            bf._group_alignments(first, res, members, rows, rows_len)
            before = C.string_at(rows.value, rows_len.value)
            out = {}
            for step in order:
                if step == "v":
                    out["v"] = bf.group_variants()
                elif step == "d":
                    out["d"] = bf.group_distances(cls, 4).tolist()
                else:
                    out["c"] = [bf.group_concat(cls, 4, h, mode) for mode in MODES]
            assert C.string_at(rows.value, rows_len.value) == before              # the rows of the groups call, where the library left them
            seen.append((out["v"], out["d"], out["c"], before))
        finally:
            bf.close()
    assert seen[0] == seen[1] == seen[2] and len(seen[0][0]) > 0
    all_rows = CM.rows_of(groups)
    assert seen[0][1] == DM.fold([DM.rows_counts(r) for r in all_rows], cls, 4).tolist()
    assert seen[0][2] == [CM.concat(all_rows, cls, 4, h, 80, mode) for mode in MODES]


def test_readers_with_different_masks_share_their_tables():
    """variants, concat VARIABLE, variants, distances, concat ALL on the rows of ONE groups call, with two masks in turn: the table of
    used groups and the prefix of their padded columns are one set of device buffers for all readers, and one left over from the call
    before has the wrong length and the wrong prefix.  Four groups of three rows with 15, 16, 17 and 33 columns, substitutions only:
    the rows are the strings."""
    import mvariants_model as MV
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(198)
    groups = []
    for n in (15, 16, 17, 33):
        c = MC.rand(rng, n)
        two, three = bytearray(c), bytearray(c)
        two[n - 1], three[0], three[n // 2] = other(c[n - 1]), other(c[0]), other(c[n // 2])
        groups.append([c, bytes(two), bytes(three)])
    b = Groups(groups)
    cls, h = [0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 2, 1], headers_of(3)
    A, B = [True, False, True, True], [False, True, True, False]
    segments = lambda want: [(g, s, e, before, lead, slices) for g, rows in enumerate(groups) if want[g]      # noqa: E731
                             for s, e, before, lead, _, slices in MV.segments(rows)]
    bf = BlockFinder(b.records, device=0)
    try:
        assert [al.rows for al in bf.align_groups(b.desc)] == groups
        v1 = bf.group_variants(A)
        c1 = bf.group_concat(cls, 3, h, CM.VARIABLE, 80, B)
        v2 = bf.group_variants(A)
        d = bf.group_distances(cls, 3, B)
        c2 = bf.group_concat(cls, 3, h, CM.ALL, 80, A)
    finally:
        bf.close()
    assert v1 == v2 == segments(A) and {s[0] for s in v1} == {0, 2, 3}
    assert c1 == CM.concat(groups, cls, 3, h, 80, CM.VARIABLE, B) and len(c1[2]) == 6
    assert c2 == CM.concat(groups, cls, 3, h, 80, CM.ALL, A)
    assert d.tolist() == DM.fold([DM.rows_counts(r) if w else DM.skipped(3) for r, w in zip(groups, B)], cls, 3).tolist()


def test_two_calls_in_a_row():
    """ALL then VARIABLE on one context: the first result was copied, the second replaces what the context owns"""
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(197)
    groups = [DC.indel_group(rng, 3, 500), DC.indel_group(rng, 3, 40)]
    b = Groups(groups)
    cls, h = [2, 0, 1, 0, 1, 2], headers_of(3)
    rows = CM.rows_of(groups)
    bf = BlockFinder(b.records, device=0)
    try:
        bf.align_groups(b.desc)
        first = bf.group_concat(cls, 3, h, CM.ALL, 70)
        second = bf.group_concat(cls, 3, h, CM.VARIABLE, 70)
        third = bf.group_concat(cls, 3, h, CM.ALL, 70)
        assert first == third == CM.concat(rows, cls, 3, h, 70, CM.ALL)
        assert second == CM.concat(rows, cls, 3, h, 70, CM.VARIABLE) and len(second[0]) < len(first[0])
    finally:
        bf.close()


def raw_concat(bf, want, cls, nclass, mode, width, headers, header_first):
    parts, sites, text = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nparts, nsites, ln = C.c_uint64(), C.c_uint64(), C.c_uint64()
    fn = bf.L.sbl_group_concat
    saved = fn.argtypes
    fn.argtypes = None                                                         # null pointers where the mirror has typed ones
    try:
        return fn(bf.h, want, cls, C.c_uint32(nclass), C.c_uint32(mode), C.c_uint32(width), headers, header_first,
                  C.byref(parts), C.byref(nparts), C.byref(sites), C.byref(nsites), C.byref(text), C.byref(ln))
    finally:
        fn.argtypes = saved


def test_bad_arguments_leave_the_context_usable():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    g = [b"ACGTACGTAC", b"ACGTTCGTAC", b"ACGTACGAC"]
    b = Groups([g])
    h = headers_of(3)
    rows = CM.rows_of([g])
    want = [CM.concat(rows, [0, 1, 2], 3, h, 80, mode) for mode in MODES]
    bf = BlockFinder(b.records, device=0)
    try:
        ok = lambda: [bf.group_concat([0, 1, 2], 3, h, mode) for mode in MODES] == want      # noqa: E731
        with pytest.raises(SibeliaError, match="bad argument"):                  # before any groups call
            bf.group_concat([0, 1, 2], 3, h, CM.ALL)
        d = b.desc[0]
        bf.align_groups(b.desc)
        assert ok()
        bf.align_pairs([d[0] + d[1]])
        with pytest.raises(SibeliaError, match="bad argument"):                  # the last call was a pairs call
            bf.group_concat([0, 1, 2], 3, h, CM.ALL)
        bf.align_groups(b.desc)
        assert ok()
        for cls, nclass, heads, mode, width in (([0, 0, 0], 0, [], CM.ALL, 80), ([0, 1, 2], 1025, [b">\n"] * 1025, CM.ALL, 80), ([0, 1, 3], 3, h, CM.ALL, 80),
                                                ([0, 1, 2], 3, h, CM.ALL, 0), ([0, 1, 2], 3, h, 2, 80), ([0, 1, 1], 3, h, CM.VARIABLE, 80),
                                                ([0, 1, 2], 4, h + [b">\n"], CM.VARIABLE, 80), ([0, 1, 2], 2, h[:2], CM.ALL, 80)):
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_concat(cls, nclass, heads, mode, width)
            assert ok()
        with pytest.raises(SibeliaError, match="bad argument"):                  # a width beyond 32 bits never reaches the library
            bf.group_concat([0, 1, 2], 3, h, CM.ALL, 2 ** 32)
        # null pointers and descending header offsets, through the C interface itself
        cls = (C.c_uint32 * 3)(0, 1, 2)
        blob = b"".join(h)
        hf = (C.c_uint64 * 4)(0, 9, 18, 27)
        assert raw_concat(bf, None, cls, 3, 0, 80, blob, hf) == 0
        assert raw_concat(bf, None, None, 3, 0, 80, blob, hf) != 0
        assert raw_concat(bf, None, cls, 3, 0, 80, None, hf) != 0
        assert raw_concat(bf, None, cls, 3, 0, 80, blob, None) != 0
        assert raw_concat(bf, None, cls, 3, 0, 80, blob, (C.c_uint64 * 4)(0, 18, 9, 27)) != 0
        assert b"bad argument" in bf.L.sbl_strerror(raw_concat(bf, None, cls, 3, 0, 0, blob, hf))
        assert ok()
        wide = bf.group_concat([0, 1, 2], 3, h, CM.ALL, 2 ** 32 - 1)
        assert wide == CM.concat(rows, [0, 1, 2], 3, h, 2 ** 32 - 1, CM.ALL)
    finally:
        bf.close()
