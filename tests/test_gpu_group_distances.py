"""sbl_group_distances (csrc/group_distances.hip: the item list of the host, k_group_distances) through BlockFinder.align_groups and
BlockFinder.group_distances against tests/gdist_model.py, exactly: every count of every cell."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gdist_cases as DC                           # noqa: E402
import gdist_model as DM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
from test_gpu_multi_align import Groups            # noqa: E402  (the layout of groups of strings as ranges of three records)

pytestmark = pytest.mark.gpu


def flat_classes(groups):
    return list(range(sum(len(g) for g in groups)))


def distances(b, cls, nclass, want=None, env=None, monkeypatch=None):
    """(alignments, matrix) of the groups b on a context of its own"""
    from sibelia_amd import BlockFinder
    bf = BlockFinder(b.records, device=0)
    try:
        got = bf.align_groups(b.desc)
        if env:
            monkeypatch.setenv(*env)
        M = bf.group_distances(cls, nclass, want)
        if env:
            monkeypatch.delenv(env[0])
        k, c = bf.group_distances_times()
        assert k >= 0 and c >= 0
        return got, M
    finally:
        bf.close()


def model_counts(groups):
    return [DM.group_counts(g) for g in groups]


def direct_counts(group):
    """the counts of a group whose alignment is known to be the identity (assert L == n first): position by position"""
    return DM.rows_counts(group)


def substituted(rng, c, n, alphabet=b"ACGT"):
    b = bytearray(c)
    for at in rng.choice(len(c), n, replace=False):
        b[at] = [x for x in alphabet if x != c[at]][int(rng.integers(0, len(alphabet) - 1))]
    return bytes(b)


def other(base: int) -> int:
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def test_crafted_groups_one_by_one_and_in_one_call():
    names = sorted(DC.CRAFTED)
    for name in names:
        g = DC.CRAFTED[name]
        _, M = distances(Groups([g]), flat_classes([g]), len(g))
        assert M.dtype == np.uint64 and M.shape == (len(g), len(g), 4)
        assert M.tolist() == DM.group_counts(g).tolist(), name
    groups = [DC.CRAFTED[n] for n in names]
    cls = flat_classes(groups)
    got, M = distances(Groups(groups), cls, len(cls))
    assert 0 not in {g.L % 16 for g in got if g.L} and any(g.row_off % 16 for g in got)      # no L is a multiple of 16, texts start unaligned
    assert M.tolist() == DM.fold(model_counts(groups), cls, len(cls)).tolist()


def test_column_edges():
    """three rows without indels, L on either side of 16 bytes, of a tile (256) and of the smallest span (4096)"""
    rng = np.random.default_rng(91)
    groups = []
    for n in (15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097):
        c = MC.rand(rng, n)
        two, three = bytearray(c), bytearray(c)
        for at in range(7, n - 8, 50):                                           # lone substitutions, far from each other: the alignment is the identity
            two[at] = other(c[at])
        for at in range(11, n - 8, 60):
            three[at] = other(c[at])
        two[n - 1] = ord("N")                                                    # the last column counts as ambiguous: a byte more or less shows
        three[0] = other(c[0])                                                   # ... and so does the first
        groups.append([c, bytes(two), bytes(three)])
    cls = flat_classes(groups)
    got, M = distances(Groups(groups), cls, len(cls))
    assert [g.L for g in got] == [len(g[0]) for g in groups]
    assert M.tolist() == DM.fold([direct_counts(g) for g in groups], cls, len(cls)).tolist()


def test_row_block_edges():
    """groups of r rows on either side of one and of two row blocks of 32"""
    rng = np.random.default_rng(92)
    groups = [DC.indel_group(rng, r) for r in (2, 3, 31, 32, 33, 64, 65, 70)]
    cls = flat_classes(groups)
    assert len(cls) <= 1024
    _, M = distances(Groups(groups), cls, len(cls))
    want = DM.fold(model_counts(groups), cls, len(cls))
    assert want[:, :, 3].sum() > 0 and want[:, :, 2].sum() > 0 and want[:, :, 1].sum() > 0
    assert M.tolist() == want.tolist()


def test_spans_and_atomics(monkeypatch):
    """one wide group: cut into spans by the host, many workgroups add to one cell; the same matrix with spans of 4096 columns"""
    rng = np.random.default_rng(93)
    c = MC.rand(rng, 200000)
    group = [c] + [substituted(rng, c, n) for n in (50, 70, 90)]
    b = Groups([group])
    got, M = distances(b, [0, 1, 2, 3], 4)
    assert got[0].status == 0 and got[0].L == len(c)
    want = direct_counts(group)
    assert [int(want[0, k, 1]) for k in (1, 2, 3)] == [50, 70, 90]
    assert M.tolist() == want.tolist()
    _, M2 = distances(b, [0, 1, 2, 3], 4, env=("SBL_TEST_GDIST_SPAN", "4096"), monkeypatch=monkeypatch)
    assert M2.tolist() == M.tolist()
    _, M3 = distances(b, [0, 0, 0, 0], 1, env=("SBL_TEST_GDIST_SPAN", "4096"), monkeypatch=monkeypatch)      # every workgroup into one cell
    assert M3.tolist() == DM.fold([want], [0, 0, 0, 0], 1).tolist()


def test_fold():
    rng = np.random.default_rng(94)
    groups = [DC.indel_group(rng, 5), DC.indel_group(rng, 4), DC.CRAFTED["codes_other_than_acgt"]]
    per = model_counts(groups)
    b = Groups(groups)
    n = sum(len(g) for g in groups)
    _, M = distances(b, [0] * n, 1)                                             # one class: only the diagonal, every unordered pair twice
    assert M.tolist() == DM.fold(per, [0] * n, 1).tolist() and all(int(v) % 2 == 0 for v in M[0, 0, :3]) and M[0, 0, 0] > 0
    cls = [0, 1, 2, 3, 4] + [0, 1, 2, 3] + [4, 3, 2, 1, 0]                    # the groups add into the same cells
    _, M = distances(b, cls, 5)
    assert M.tolist() == DM.fold(per, cls, 5).tolist()
    _, big = distances(b, cls, 9)                                                # classes nobody has: zero rows and columns
    assert big[:5, :5].tolist() == M.tolist() and big[5:].sum() == 0 and big[:, 5:].sum() == 0
    perm = [3, 0, 4, 1, 2]
    _, P = distances(b, [perm[x] for x in cls], 5)
    assert all(P[perm[f], perm[g]].tolist() == M[f, g].tolist() for f in range(5) for g in range(5))


def test_want_mask_and_a_skipped_group(monkeypatch):
    rng = np.random.default_rng(45)
    groups = MC.random_groups(seed=46, count=9, rmin=2, rmax=4, max_len=55, max_indel=5)
    c = MC.rand(rng, 50)
    groups[4] = [c, MC.mutated(rng, c, 0.05, 5), MC.rand(rng, 900), c[:30]]      # as tests/test_gpu_multi_align.py: the second member is beyond a cap of 4 KiB
    b = Groups(groups)
    cls = flat_classes(groups)
    per = model_counts(groups)
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    capped, M = distances(b, cls, len(cls))
    monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
    assert [g.status for g in capped] == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert M.tolist() == DM.fold([DM.skipped(len(groups[k])) if k == 4 else per[k] for k in range(9)], cls, len(cls)).tolist()
    want = [k not in (1, 7) for k in range(9)]
    _, M = distances(b, cls, len(cls), want)
    assert M.tolist() == DM.fold([per[k] if want[k] else DM.skipped(len(groups[k])) for k in range(9)], cls, len(cls)).tolist()
    _, M = distances(b, cls, len(cls), [False] * 9)
    assert M.sum() == 0
    with pytest.raises(ValueError):
        distances(b, cls, len(cls), [True] * 8)


def test_reverse_centre_and_reverse_members():
    rng = np.random.default_rng(41)
    c = MC.rand(rng, 150)
    g = [c, MC.mutated(rng, c), MC.mutated(rng, c), b"TT" + c[:70] + b"GAG" + c[70:]]
    revs = [[True, False, False, False], [False, True, True, True], [True, True, False, True], [False] * 4]
    cls = flat_classes([g] * 4)
    _, M = distances(Groups([g, g, g, g], revs), cls, 16)
    one = DM.group_counts(g)
    assert M.tolist() == DM.fold([one] * 4, cls, 16).tolist()


def test_seeded_random_groups():
    rng = np.random.default_rng(95)
    groups = []
    for _ in range(40):
        c = MC.rand(rng, int(rng.integers(0, 301)), b"ACGTACGTACGTN")
        groups.append([c] + [MC.mutated(rng, c, 0.05, 8)[:300] for _ in range(int(rng.integers(2, 10)) - 1)])
    cls = [int(x) for x in rng.integers(0, 7, sum(len(g) for g in groups))]
    got, M = distances(Groups(groups), cls, 7)
    assert [g.status for g in got] == [0] * 40
    assert M.tolist() == DM.fold(model_counts(groups), cls, 7).tolist()


def test_variants_and_distances_in_either_order_leave_the_rows():
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(96)
    groups = [DC.indel_group(rng, 4, 120), DC.indel_group(rng, 3, 90), [MC.rand(rng, 30)]]
    b = Groups(groups)
    cls = flat_classes(groups)
    first = [0]
    for d in b.desc:
        first.append(first[-1] + len(d))
    seen = []
    for order in ("vd", "dv"):
        bf = BlockFinder(b.records, device=0)
        try:
            from sibelia_amd.api import GroupInst
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
                else:
                    out["d"] = bf.group_distances(cls, len(cls)).tolist()
            assert C.string_at(rows.value, rows_len.value) == before              # the rows of the groups call, where the library left them
            seen.append((out["v"], out["d"], before))
        finally:
            bf.close()
    assert seen[0] == seen[1] and len(seen[0][0]) > 0
    assert seen[0][1] == DM.fold(model_counts(groups), cls, len(cls)).tolist()


def test_bad_arguments_leave_the_context_usable():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    g = [b"ACGTACGTAC", b"ACGTTCGTAC", b"ACGTACGAC"]
    b = Groups([g])
    want = DM.group_counts(g).tolist()
    bf = BlockFinder(b.records, device=0)
    try:
        with pytest.raises(SibeliaError, match="bad argument"):                  # before any groups call
            bf.group_distances([0, 1, 2], 3)
        d = b.desc[0]
        bf.align_groups(b.desc)
        assert bf.group_distances([0, 1, 2], 3).tolist() == want
        bf.align_pairs([d[0] + d[1]])
        with pytest.raises(SibeliaError, match="bad argument"):                  # the last call was a pairs call
            bf.group_distances([0, 1, 2], 3)
        bf.align_groups(b.desc)
        assert bf.group_distances([0, 1, 2], 3).tolist() == want
        for cls, nclass in (([0, 0, 0], 0), ([0, 1, 2], 1025), ([0, 1, 3], 3)):
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.group_distances(cls, nclass)
            assert bf.group_distances([0, 1, 2], 3).tolist() == want
        assert bf.group_distances([0, 1023, 5], 1024)[0, 1023].tolist() == want[0][1]
    finally:
        bf.close()
