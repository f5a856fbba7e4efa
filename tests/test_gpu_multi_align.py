"""sbl_align_groups (csrc/block_align.hip: the pair passes, the host merge of the gap slots, k_spell_groups) against tests/msa_model.py,
byte for byte: status, L, row offsets, rows and member scores."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_cases as MC                             # noqa: E402
import msa_model as MM                             # noqa: E402

pytestmark = pytest.mark.gpu


class Groups:
    """groups of strings laid out as ranges of three records, instance after instance in turn; a reverse range holds the reverse
    complement, so that the strings the kernels read are the ones given"""

    def __init__(self, groups, revs=None):
        self.groups = [[bytes(s) for s in g] for g in groups]
        self.revs = revs or [[False] * len(g) for g in groups]
        recs = [bytearray(b"G"), bytearray(b"T"), bytearray(b"CA")]
        self.desc, at = [], 0
        for g, rv in zip(self.groups, self.revs):
            d = []
            for s, v in zip(g, rv):
                r = recs[at % 3]
                d.append((at % 3, len(r), len(r) + len(s), v))
                r += MM.reverse_complement(s) if v else s
                at += 1
            self.desc.append(d)
        self.records = [bytes(r) + b"C" for r in recs]
        self._want = None

    def want(self):
        if self._want is None:
            self._want = [MM.msa(g) for g in self.groups]
        return self._want

    def run(self):
        from sibelia_amd import BlockFinder
        bf = BlockFinder(self.records, device=0)
        try:
            return bf.align_groups(self.desc), bf.align_stats()
        finally:
            bf.close()

    def check(self, got, skipped=()):
        assert len(got) == len(self.groups)
        off = 0
        for k, (g, (rows, scores)) in enumerate(zip(got, self.want())):
            if k in skipped:
                assert (g.status, g.L, g.rows) == (1, 0, []) and all(m[0] is None for m in g.members) and len(g.members) == len(self.groups[k]) - 1, k
                continue
            assert g.status == 0, k
            assert (g.L, g.row_off) == (len(rows[0]), off), (k, g.L, g.row_off, off)
            assert g.rows == rows, (k, self.groups[k], g.rows, rows)
            assert [m[0] for m in g.members] == scores, k
            off += len(rows) * len(rows[0])


def test_crafted_groups_one_by_one_and_in_one_call():
    names = sorted(MC.CRAFTED)
    for name in names:                                                          # alone: a text of fewer than 16 bytes among them
        b = Groups([MC.CRAFTED[name][0]])
        got, _ = b.run()
        b.check(got)
        if MC.CRAFTED[name][1] is not None:
            assert got[0].rows == MC.CRAFTED[name][1], name
    b = Groups([MC.CRAFTED[n][0] for n in names])                               # together: no L is a multiple of 16 -- a lane's 16 bytes cross rows and groups
    got, st = b.run()
    b.check(got)
    assert {g.L % 16 for g in got} != {0} and min(g.L for g in got) == 0 and st["skipped"] == 0 and st["spell_ms"] > 0
    assert st["pairs"] == sum(len(MC.CRAFTED[n][0]) - 1 for n in names)


def test_reverse_centre_and_reverse_members():
    rng = np.random.default_rng(41)
    c = MC.rand(rng, 150)
    g = [c, MC.mutated(rng, c), MC.mutated(rng, c), b"TT" + c[:70] + b"GAG" + c[70:]]
    b = Groups([g, g, g, g], [[True, False, False, False], [False, True, True, True], [True, True, False, True], [False] * 4])
    got, _ = b.run()
    b.check(got)
    assert got[0].rows == got[1].rows == got[2].rows == got[3].rows


def test_a_group_longer_than_one_workgroup_writes():
    rng = np.random.default_rng(42)
    c = MC.rand(rng, 1200)                                                       # 256 lanes of 16 bytes: 4096 bytes; this group has 5 rows of more than 1200
    g = [c] + [MC.mutated(rng, c, 0.02, 20) for _ in range(4)]
    b = Groups([[b"ACGTT", b"ACTT"], g, [b"GGA", b"GA", b"GGGA"]])
    got, _ = b.run()
    b.check(got)
    assert got[1].L > 1200 and got[1].L % 16 != 0


@pytest.fixture(scope="module")
def random_groups():
    groups = MC.random_groups(seed=43, count=200, rmin=2, rmax=6, max_len=400, max_indel=20)
    rng = np.random.default_rng(44)
    return Groups(groups, [[bool(rng.random() < 0.3) for _ in g] for g in groups])


def test_seeded_random_groups(random_groups):
    got, st = random_groups.run()
    assert [g.status for g in got] == [0] * 200 and st["skipped"] == 0           # no limit binds at these sizes: a skip cannot hide a mismatch
    random_groups.check(got)
    assert st["pairs"] == sum(len(g) - 1 for g in random_groups.groups) and st["passes"] > 0


def test_rows_do_not_depend_on_the_first_band(random_groups, monkeypatch):
    monkeypatch.setenv("SBL_TEST_GALIGN_W0", "1")
    got, st = random_groups.run()
    assert [g.status for g in got] == [0] * 200
    random_groups.check(got)
    assert st["passes"] > 2 * st["pairs"]                                        # doubling ran


def test_pair_projection_against_align_pairs(random_groups):
    from sibelia_amd import BlockFinder
    picks = [k for k, g in enumerate(random_groups.groups) if len(g) >= 3][:6]
    bf = BlockFinder(random_groups.records, device=0)
    try:
        groups = bf.align_groups([random_groups.desc[k] for k in picks])
        for k, g in zip(picks, groups):
            d = random_groups.desc[k]
            pairs = bf.align_pairs([d[0] + m for m in d[1:]])
            for row, p, (score, _, _) in zip(g.rows[1:], pairs, g.members):
                assert MM.project(g.rows[0], row) == (p.row_a, p.row_b) and score == p.score
    finally:
        bf.close()


def test_calls_on_one_context_carry_nothing_over():
    """align_groups, align_pairs and align_groups again on ONE context -- every call spells through the same device tables -- give what
    each gives on a fresh context"""
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(47)
    c = MC.rand(rng, 90)
    five = [c] + [MC.mutated(rng, c, 0.05, 6) for _ in range(4)]
    b = Groups([five, [b"ACGTT", b"ACTT"], [MC.rand(rng, 40)], [b"GGA", b"GA", b"GGGA"], five[::-1], [b"", b"AC"]],
               [[False, True, False, True, False], [False, False], [True], [False] * 3, [True, False, False, True, True], [False, False]])
    first, second = b.desc[:3], b.desc[3:]
    pairs = [first[0][0] + m for m in first[0][1:]] + [(0, 0, 0, False, 1, 0, 0, False), second[0][0] + second[0][2]]
    calls = [lambda bf: bf.align_groups(first), lambda bf: bf.align_pairs(pairs), lambda bf: bf.align_groups(second)]

    def flat(results):
        return [(r.status, r.L, r.row_off, r.rows, r.members) if hasattr(r, "rows") else (r.status, r.score, r.band_w, r.passes, r.runs, r.row_a, r.row_b)
                for r in results]
    want = []
    for call in calls:                                                          # each on a context of its own
        bf = BlockFinder(b.records, device=0)
        try:
            want.append(flat(call(bf)))
        finally:
            bf.close()
    bf = BlockFinder(b.records, device=0)
    try:
        got = [flat(call(bf)) for call in calls]
    finally:
        bf.close()
    assert got == want
    assert [g[3] for g in got[0] + got[2]] == [rows for rows, _ in b.want()] and len(got[0][0][3]) == 5      # ... and what the model gives
    assert [p[0] for p in got[1]] == [0] * 6 and (got[1][0][5], got[1][0][6]) == MM.project(got[0][0][3][0], got[0][0][3][1]) and got[1][4][5:] == (b"", b"")


def test_one_member_beyond_the_cap_skips_its_group_only(monkeypatch):
    rng = np.random.default_rng(45)
    groups = MC.random_groups(seed=46, count=9, rmin=2, rmax=4, max_len=55, max_indel=5)      # at most 111 diagonals of at most 14 bytes: below 4 KiB
    c = MC.rand(rng, 50)
    groups[4] = [c, MC.mutated(rng, c, 0.05, 5), MC.rand(rng, 900), c[:30]]      # the second member: 951 band offsets, 951 diagonals of 119 bytes
    b = Groups(groups)
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    capped, st = b.run()
    monkeypatch.delenv("SBL_TEST_GALIGN_CAP_KB")
    plain, st0 = b.run()
    b.check(plain)
    assert (st["skipped"], st0["skipped"]) == (1, 0)                             # exactly one pair
    assert (capped[4].status, capped[4].L, capped[4].rows) == (1, 0, []) and [m[0] for m in capped[4].members] == [None] * 3
    gone = plain[4].L * 4
    for k in range(9):
        if k != 4:
            assert (capped[k].status, capped[k].rows, capped[k].members) == (0, plain[k].rows, plain[k].members), k
            assert capped[k].row_off == plain[k].row_off - (gone if k > 4 else 0), k


def test_bad_arguments_leave_the_context_usable():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    bf = BlockFinder([b"ACGTACGTAC", b"ACGTTCGTAC"], device=0)
    good = [(0, 0, 10, False), (1, 0, 10, False)]
    try:
        for bad in [[good, []], [[], good], [good, [(0, 0, 11, False)]], [good, [(0, 0, 10, False), (1, 5, 11, False)]], [good, [(0, 6, 5, False)]],
                    [good, [(2, 0, 1, False)]]]:
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.align_groups(bad)
        got = bf.align_groups([good])
        assert got[0].rows == [b"ACGTACGTAC", b"ACGTTCGTAC"] and got[0].members == [(9 * 25 - 75, 10, 1)]
        assert bf.align_groups([]) == []
    finally:
        bf.close()


def test_no_records_loaded_is_a_bad_argument():
    from sibelia_amd import load_library
    from sibelia_amd.api import GroupInst
    L = load_library()
    h = C.c_void_p()
    assert L.sbl_create(C.byref(h), 0) == 0
    first, inst = (C.c_uint64 * 2)(0, 1), (GroupInst * 1)()
    res, members, rows, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert L.sbl_align_groups(h, 1, first, inst, C.byref(res), C.byref(members), C.byref(rows), C.byref(n)) == 1      # SBL_ERR_BAD_ARG
    assert b"no records loaded" in L.sbl_last_error(h)
    L.sbl_destroy(h)
