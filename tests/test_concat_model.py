"""tests/concat_model.py held to its invariants, and tests/concat_cases.py to what its cases say they are: the GPU tests
of sbl_group_concat compare against this model, so it is checked here against hand-written texts and against the other models."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import concat_cases as CC                          # noqa: E402
import concat_model as CM                          # noqa: E402
import gdist_model as DM                           # noqa: E402
import msa_cases as MC                             # noqa: E402

ACCEPTED = sorted(n for n, c in CC.CASES.items() if not c["refused"])
_ROWS = {}


def rows(name):
    if name not in _ROWS:
        _ROWS[name] = CM.rows_of(CC.CASES[name]["groups"])
    return _ROWS[name]


def run(name, mode):
    c = CC.CASES[name]
    return CM.concat(rows(name), c["cls"], c["nclass"], c["headers"], c["width"], mode, c["want"])


def check_invariants(groups, all_rows, cls, nclass, headers, width, want=None):
    """what holds for every accepted call, in both modes"""
    first = [0]
    for g in groups:
        first.append(first[-1] + len(g))
    for mode in (CM.ALL, CM.VARIABLE):
        text, parts, sites = CM.concat(all_rows, cls, nclass, headers, width, mode, want)
        C = sum(n for _, _, n in parts)
        assert [g for g, _, _ in parts] == CM.used(all_rows, want)
        at = 0
        for _, f0, n in parts:                                                       # the parts tile [0, C)
            assert f0 == at
            at += n
        assert len(text) == sum(len(h) for h in headers) + nclass * (C + (C + width - 1) // width)
        if all(h.startswith(b">") for h in headers):
            out = CM.split_fasta(text, headers)
            assert [len(r) for r in out] == [C] * nclass                             # every row holds C bytes once line feeds are removed
            lines = [ln for ln in text.split(b"\n")[:-1] if not ln.startswith(b">")]
            assert all(0 < len(ln) <= width for ln in lines)
        else:
            out = None
        if mode == CM.ALL:
            assert sites == [] and all(n == len(all_rows[g][0]) for g, _, n in parts)
            for g, f0, n in parts:                                                   # row f of a part without gaps is the instance of class f
                for i, s in enumerate(groups[g]):
                    if out is not None:
                        assert out[cls[first[g] + i]][f0:f0 + n].replace(b"-", b"") == s
        else:
            assert len(sites) == C and sites == sorted(sites)
            per_group = {}
            for k, (g, col, before) in enumerate(sites):
                column = bytes(r[col] for r in all_rows[g])
                assert set(column) <= set(b"ACGT") and len(set(column)) > 1
                assert groups[g][0][before] == column[0]                             # the centre's base in that column, by its index in the instance
                per_group[g] = per_group.get(g, 0) + 1
                if out is not None:
                    assert bytes(out[cls[first[g] + i]][k] for i in range(nclass)) == column
            assert [(g, per_group.get(g, 0)) for g, _, _ in parts] == [(g, n) for g, _, n in parts]
            for g, _, n in parts:                                                    # against the pairwise counts: a site gives some pair a mismatch
                counts = DM.rows_counts(all_rows[g])
                mismatch = sum(int(counts[i, j, 1]) for i in range(nclass) for j in range(i + 1, nclass))
                assert n == mismatch if nclass == 2 else n <= mismatch


@pytest.mark.parametrize("name", sorted(CC.BY_HAND))
def test_texts_written_out_by_hand(name):
    text_all, text_var, sites = CC.BY_HAND[name]
    got_all, got_var = run(name, CM.ALL), run(name, CM.VARIABLE)
    assert got_all[0] == text_all and got_all[2] == []
    assert got_var[0] == text_var and got_var[2] == sites
    assert got_all[1] == [(g, sum(len(r[0]) for r in rows(name)[:g]), len(r[0])) for g, r in enumerate(rows(name))]


@pytest.mark.parametrize("name", ACCEPTED)
def test_invariants_on_the_crafted_calls(name):
    c = CC.CASES[name]
    check_invariants(c["groups"], rows(name), c["cls"], c["nclass"], c["headers"], c["width"], c["want"])


@pytest.mark.parametrize("name", sorted(n for n, c in CC.CASES.items() if c["refused"]))
def test_refused_calls(name):
    for mode in (CM.ALL, CM.VARIABLE):
        with pytest.raises(CM.Refused, match="group"):
            run(name, mode)


def test_refused_arguments():
    r = [[b"ACGT", b"AGGT"]]
    h = [b">a\n", b">b\n"]
    assert CM.concat(r, [0, 1], 2, h, 80, CM.ALL)[0] == b">a\nACGT\n>b\nAGGT\n"
    for args in ((r, [0, 1], 2, h, 0, CM.ALL), (r, [0, 1], 2, h, 2 ** 32, CM.ALL), (r, [0, 0], 0, [], 80, CM.ALL), (r, [0, 1], 1025, [b""] * 1025, 80, CM.ALL),
                 (r, [0, 2], 2, h, 80, CM.ALL), (r, None, 2, h, 80, CM.ALL), (r, [0, 1], 2, None, 80, CM.ALL), (r, [0, 1], 2, h, 80, 2)):
        with pytest.raises(CM.Refused):
            CM.concat(*args)


def test_seeded_random_groups():
    """200 groups from a fixed seed, each a call of its own with its rows in a random order of classes, and ten calls of twenty"""
    rng = np.random.default_rng(97)
    groups = MC.random_groups(seed=98, count=200, rmin=1, rmax=5, max_len=120, max_indel=8)
    all_rows = CM.rows_of(groups)
    sites = 0
    for g, r in zip(groups, all_rows):
        cls = [int(x) for x in rng.permutation(len(g))]
        width = int(rng.integers(1, 40))
        check_invariants([g], [r], cls, len(g), [b">c%d\n" % f for f in range(len(g))], width)
        sites += len(CM.concat([r], cls, len(g), [b""] * len(g), width, CM.VARIABLE)[2])
    assert sites > 100
    by_r = {}
    for g, r in zip(groups, all_rows):
        by_r.setdefault(len(g), []).append((g, r))
    for n, members in sorted(by_r.items()):
        cls = [int(x) for _ in members for x in rng.permutation(n)]
        check_invariants([g for g, _ in members], [r for _, r in members], cls, n, [b">c%d\n" % f for f in range(n)], 60)


def test_the_crafted_cases_are_what_they_say():
    c = CC.CASES["codes_gap_and_edges"]
    (r,) = rows("codes_gap_and_edges")
    assert len(r[0]) == 32 and r[0] == c["groups"][0][0] and r[1] == c["groups"][0][1] and r[2][17:18] == b"-" and r[2].count(b"-") == 1
    _, parts_all, _ = run("codes_gap_and_edges", CM.ALL)
    _, _, sites = run("codes_gap_and_edges", CM.VARIABLE)
    cols = [col for _, col, _ in sites]
    assert parts_all == [(0, 0, 32)]
    assert cols == [0, 12, 31]                                                      # first and last column; the column in which every row differs
    column = lambda x: bytes(row[x] for row in r)                                    # noqa: E731
    assert b"N" in column(5) and column(9) == b"CgC" and len(set(column(12))) == 3 and column(17) == b"GT-"
    assert all(x not in cols for x in (5, 9, 17))                                    # variable, in ALL, out of VARIABLE
    # consecutive short groups: their L, every one with its first and last column variable
    for w in (1, 15, 16, 17, 80, 100):
        name = "short_groups_width_%d" % w
        assert CC.CASES[name]["width"] == w
        assert [len(x[0]) for x in rows(name)] == CC.SHORT_L
    _, parts, sites = run("short_groups_width_16", CM.VARIABLE)
    assert [n for _, _, n in parts] == [1, 2, 2, 2, 2, 2] and sum(CC.SHORT_L) == 54 and 100 > 54
    assert [(g, col) for g, col, _ in sites] == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 2), (3, 0), (3, 14), (4, 0), (4, 15), (5, 0), (5, 16)]
    # C an exact multiple of the width
    text, parts, _ = run("columns_a_multiple_of_width", CM.ALL)
    assert parts == [(0, 0, 32)] and CC.CASES["columns_a_multiple_of_width"]["width"] == 16 and text.count(b"\n") == 2 * (1 + 2)
    assert [len(h) for h in CC.CASES["header_lengths"]["headers"]] == CC.HEADER_LENGTHS == [2, 15, 16, 17, 300]
    assert {CC.CASES[n]["nclass"] for n in ACCEPTED} >= {1, 2, 3, 33}
    assert {CC.CASES[n]["width"] for n in ACCEPTED} >= {1, 15, 16, 17, 80, 100}
    assert run("no_site", CM.VARIABLE)[2] == [] and run("no_site", CM.VARIABLE)[0] == b">s0\n>s1\n"
    z = rows("centre_of_length_0")
    assert z[0][0] == b"-" * 6 and run("centre_of_length_0", CM.ALL)[1] == [(0, 0, 6), (1, 6, 4)]
    assert any(sorted(c["cls"][:len(c["groups"][0])]) == list(range(c["nclass"])) and c["cls"][:c["nclass"]] != list(range(c["nclass"]))
               for c in (CC.CASES[n] for n in ACCEPTED))                              # classes in permuted row order
    u = CC.CASES["unwanted_group_breaks_the_class_rule"]
    assert u["want"] == [True, False, True] and [g for g, _, _ in run("unwanted_group_breaks_the_class_rule", CM.ALL)[1]] == [0, 2]
    with pytest.raises(CM.Refused):
        CM.concat(rows("unwanted_group_breaks_the_class_rule"), u["cls"], 2, u["headers"], 80, CM.ALL)
