"""sbl_group_variants (csrc/group_variants.hip: k_column_classes, k_segment_bounds, k_gather_slices) against tests/mvariants_model.py
applied to the rows the SAME groups call returned -- the rows themselves are pinned to tests/msa_model.py by tests/test_gpu_multi_align.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_cases as MC                             # noqa: E402
import mvariants_model as MV                       # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_LANE, BOUNDS_GROUP, CLASS_GROUP = 16, 256, 256 * 16      # columns per lane / per workgroup of k_segment_bounds / of k_column_classes


def layout(groups):
    """groups of strings as ranges of three records, instance after instance in turn -> (records, descriptors)"""
    recs = [bytearray(b"G"), bytearray(b"T"), bytearray(b"CA")]
    desc, at = [], 0
    for g in groups:
        d = []
        for s in g:
            r = recs[at % 3]
            d.append((at % 3, len(r), len(r) + len(s), False))
            r += s
            at += 1
        desc.append(d)
    return [bytes(r) + b"C" for r in recs], desc


def expected(aligned, want=None):
    """the model on the rows of every aligned group -> ([(group, s, e, before, lead, slices)], [gapped])"""
    segs, gapped = [], []
    for g, al in enumerate(aligned):
        if al.status != 0 or (want is not None and not want[g]):
            continue
        for s, e, before, lead, gap, slices in MV.segments(al.rows):
            segs.append((g, s, e, before, lead, slices))
            gapped.append(gap)
    return segs, gapped


def run(groups, want=None):
    from sibelia_amd import BlockFinder
    records, desc = layout(groups)
    bf = BlockFinder(records, device=0)
    try:
        aligned = bf.align_groups(desc)
        got = bf.group_variants(want)
        return aligned, got, [int(x) for x in bf.last_group_segments["gapped"]], bf.group_variants_times()
    finally:
        bf.close()


def check(groups, want=None):
    aligned, got, gapped, _ = run(groups, want)
    segs, gaps = expected(aligned, want)
    assert got == segs
    assert gapped == gaps
    return aligned, got


def test_crafted_groups():
    names = sorted(MC.CRAFTED)
    aligned, got = check([MC.CRAFTED[n][0] for n in names])
    assert min(a.L for a in aligned) == 0 and min(len(a.rows) for a in aligned) == 1 and 0 < min(a.L for a in aligned if a.L) < 16
    by_name = {n: [s[1:] for s in got if s[0] == k] for k, n in enumerate(names)}
    assert by_name["one_instance"] == by_name["nothing_at_all"] == []
    assert by_name["slots_0_and_n"] == [(0, 12, 0, 0, [b"--ACGTACGT--", b"TTACGTACGTGG"])]      # 8 equal columns between: merged
    assert by_name["same_slot_different_lengths"] == [(4, 7, 4, 1, [b"A---", b"AGG-", b"ATTT", b"A---"])]
    assert by_name["empty_centre"] == [(0, 7, 0, 0, [b"-------", b"-------", b"ACG----", b"ACGTACG"])]
    for name in names:                                                          # alone: one group, a text of a few bytes
        check([MC.CRAFTED[name][0]])


@pytest.fixture(scope="module")
def random_groups():
    return MC.random_groups(7, 40, 2, 6, 1500, 40)


def test_seeded_random_groups(random_groups):
    aligned, got = check(random_groups)
    assert all(a.status == 0 for a in aligned) and len(got) >= len(random_groups)      # not vacuous: a segment per group on average
    assert {s[4] for s in got} == {0, 1} and max(s[2] - s[1] for s in got) > CLASS_LANE


def test_a_want_mask_drops_every_second_group(random_groups):
    want = [g % 2 == 0 for g in range(len(random_groups))]
    aligned, got = check(random_groups, want)
    assert got and {s[0] % 2 for s in got} == {0}
    check(random_groups, [False] * len(random_groups))                          # nothing wanted: no segments, an empty text


def substituted(rng, n, columns):
    """a centre of n bases and three members with substitutions only: column i of `columns` (ascending) goes to member i % 3"""
    c = MC.rand(rng, n)
    members = [bytearray(c) for _ in range(3)]
    for i, p in enumerate(columns):
        members[i % 3][p] = b"ACGT".replace(c[p:p + 1], b"")[int(rng.integers(0, 3))]
    return [c] + [bytes(m) for m in members]


@pytest.mark.parametrize("n", [15, 16, 17, BOUNDS_GROUP + 1, 1023, 1024, 1025, CLASS_GROUP + 1])
def test_substitutions_around_every_boundary_of_the_kernels(n):
    """Substitutions only: a mismatch costs 75, the two gap columns that would avoid it 150 -- the rows are the strings, L = n.  One
    group with substitutions at columns 0 and n - 1 and on both sides of every multiple of 16; one with 29, 30 and 31 equal columns
    between substitutions, counted from column 0 and from column n."""
    rng = np.random.default_rng(n)
    sixteens = sorted({0, n - 1} | {p for k in range(16, n, 16) for p in (k - 1, k)})
    chain = [0, 40, 70, 101, 133]                                               # 39, then 29, 30 and 31 equal columns between
    spaced = sorted({p for p in chain if p < n} | {n - 1 - p for p in chain if p < n} | ({n // 2, n // 2 + 30} if n > 400 else set()))
    groups = [substituted(rng, n, sixteens), substituted(rng, n, spaced), [b"ACGTT", b"ACTT"]]
    aligned, got = check(groups)
    for al, columns, g in zip(aligned, (sixteens, spaced), groups):
        assert al.rows == g                                                      # no gaps: the columns are the ones planted
        assert [i for i, c in enumerate(MV.classes(al.rows)) if c] == columns
    mine = [s for s in got if s[0] == 1]
    if n > 400:                                                                  # 29 equal columns merge, 30 and 31 do not
        assert [(s, e) for _, s, e, _, _, _ in mine][:4] == [(0, 1), (40, 71), (101, 102), (133, 134)]
        assert [(s, e) for _, s, e, _, _, _ in mine][-4:] == [(n - 134, n - 133), (n - 102, n - 101), (n - 71, n - 40), (n - 1, n)]
        assert (n // 2, n // 2 + 31) in [(s, e) for _, s, e, _, _, _ in mine]
    for g, s, e, before, lead, _ in got:
        if g < 2:                                                                # no gaps: every centre byte counts, one column is one substitution
            assert (before, lead) == (s, 0 if s == 0 or e - s == 1 else 1)


def test_a_skipped_group_gives_no_segments_and_leaves_the_others_alone(monkeypatch):
    rng = np.random.default_rng(45)
    groups = MC.random_groups(seed=46, count=9, rmin=2, rmax=4, max_len=55, max_indel=5)      # the recipe of tests/test_gpu_multi_align.py
    c = MC.rand(rng, 50)
    groups[4] = [c, MC.mutated(rng, c, 0.05, 5), MC.rand(rng, 900), c[:30]]
    plain, got0 = check(groups)
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    capped, got = check(groups)
    assert [a.status for a in capped] == [0, 0, 0, 0, 1, 0, 0, 0, 0] and plain[4].status == 0
    assert [s for s in got0 if s[0] == 4] and not [s for s in got if s[0] == 4]
    assert got == [s for s in got0 if s[0] != 4]


def test_the_rows_of_the_groups_call_stay_where_they_are(random_groups):
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import GroupInst
    records, desc = layout(random_groups[:8])
    bf = BlockFinder(records, device=0)
    try:
        first = [0]
        for d in desc:
            first.append(first[-1] + len(d))
        inst = (GroupInst * first[-1])()
        for x, i in zip(inst, [i for d in desc for i in d]):
            x.chr, x.start, x.end, x.rev = [int(v) for v in i]
        res, members, rows, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert bf.L.sbl_align_groups(bf.h, len(desc), (C.c_uint64 * len(first))(*first), inst, C.byref(res), C.byref(members), C.byref(rows), C.byref(n)) == 0
        before = C.string_at(rows.value, n.value)
        segs, text, ns, nt = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        for _ in range(2):
            assert bf.L.sbl_group_variants(bf.h, None, C.byref(segs), C.byref(ns), C.byref(text), C.byref(nt)) == 0
            assert ns.value > 0 and nt.value > 0
            assert not (rows.value <= text.value < rows.value + n.value) and not (text.value <= rows.value < text.value + nt.value)
            assert C.string_at(rows.value, n.value) == before
        k, d = bf.group_variants_times()
        assert k > 0 and d > 0
    finally:
        bf.close()


def test_bad_argument_without_rows_of_groups_on_the_device():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    bf = BlockFinder([b"ACGTACGTAC", b"ACGTTCGTAC"], device=0)
    good = [(0, 0, 10, False), (1, 0, 10, False)]
    try:
        with pytest.raises(SibeliaError, match="bad argument"):                 # no groups call yet
            bf.group_variants()
        assert bf.align_groups([good])[0].rows == [b"ACGTACGTAC", b"ACGTTCGTAC"]
        assert bf.group_variants() == [(0, 4, 5, 4, 0, [b"A", b"T"])]
        bf.align_pairs([good[0] + good[1]])
        with pytest.raises(SibeliaError, match="bad argument"):                 # the pairs were spelled through the same buffers
            bf.group_variants()
        assert bf.align_groups([]) == [] and bf.group_variants() == []          # no groups is a result
        bf.align_groups([good])
        assert bf.group_variants([True]) == [(0, 4, 5, 4, 0, [b"A", b"T"])] and bf.group_variants([False]) == []
    finally:
        bf.close()
