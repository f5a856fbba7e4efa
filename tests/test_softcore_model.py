"""tests/softcore_model.py held to texts and matrices written out by hand and to its invariants, and
tests/softcore_cases.py to what its cases say they are: the GPU tests of the partial setting compare against this model."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BM                            # noqa: E402
import concat_model as CM                          # noqa: E402
import softcore_cases as SC                        # noqa: E402
import softcore_model as SM                        # noqa: E402

ACCEPTED = sorted(n for n, c in SC.CASES.items() if not c["refused"])
_ROWS = {}


def rows(name):
    if name not in _ROWS:
        _ROWS[name] = CM.rows_of(SC.CASES[name]["groups"])
    return _ROWS[name]


def test_a_call_written_out_by_hand():
    groups, cls, h = [[b"ACGT", b"AGGT"], [b"TTA"]], [0, 2, 1], [b">a\n", b">b\n", b">c\n"]
    assert SM.concat_partial(groups, cls, 3, h, 80, SM.ALL) == (b">a\nACGT---\n>b\n----TTA\n>c\nAGGT---\n", [(0, 0, 4), (1, 4, 3)], [])
    assert SM.concat_partial(groups, cls, 3, h, 3, SM.ALL)[0] == b">a\nACG\nT--\n-\n>b\n---\n-TT\nA\n>c\nAGG\nT--\n-\n"
    assert SM.concat_partial(groups, cls, 3, h, 80, SM.VARIABLE) == (b">a\nC\n>b\n-\n>c\nG\n", [(0, 0, 1), (1, 1, 0)], [(0, 1, 1)])
    M, C, nclean, clean = SM.counts_partial(groups, cls, 3, 2, 5)
    assert (C, nclean) == (1, 7)
    assert M.tolist() == [[[0, 0, 1], [0, 0, 0], [1, 0, 0]]] * 3                     # one site: every draw is that site
    assert clean.tolist() == [[4, 0, 4], [0, 3, 0], [4, 0, 4]]
    # a class that no group holds; a centre with a gap gives `before` by the centre's bases
    groups = [[b"AC-GT", b"ACTGA"]]
    assert SM.concat_partial(groups, [3, 1], 4, [b""] * 4, 80, SM.VARIABLE) == (b"-\nA\n-\nT\n", [(0, 0, 1)], [(0, 4, 3)])
    M, C, nclean, clean = SM.counts_partial(groups, [3, 1], 4, 0, 0)
    assert (C, nclean) == (1, 4) and M[0].tolist() == [[0] * 4, [0, 0, 0, 1], [0] * 4, [0, 1, 0, 0]]
    assert clean.tolist() == [[0] * 4, [0, 4, 0, 4], [0] * 4, [0, 4, 0, 4]]


def check_invariants(all_rows, c, width):
    cls, nclass = c["cls"], c["nclass"]
    M, C, nclean, clean = SM.counts_partial(all_rows, cls, nclass, c["replicates"], c["seed"], c["draws"], c["want"])
    n = c["draws"] or C
    assert M.shape == (c["replicates"] + 1, nclass, nclass) and clean.shape == (nclass, nclass)
    for slab in M:
        assert (slab == slab.T).all() and not slab.diagonal().any()
    assert (M[1:] <= n).all() and (clean == clean.T).all()
    d = clean.diagonal()
    assert (M[0] <= clean).all() and (clean <= np.minimum(d[:, None], d[None, :])).all() and clean.max(initial=0) <= nclean
    texts = {}
    for mode in (SM.ALL, SM.VARIABLE):
        text, parts, sites = texts[mode] = SM.concat_partial(all_rows, cls, nclass, c["headers"], width, mode, c["want"])
        K = sum(k for _, _, k in parts)
        assert [g for g, _, _ in parts] == CM.used(all_rows, c["want"])
        assert len(text) == sum(len(h) for h in c["headers"]) + nclass * (K + (K + width - 1) // width)
        if all(h.startswith(b">") for h in c["headers"]):
            out = CM.split_fasta(text, c["headers"])
            assert [len(r) for r in out] == [K] * nclass                             # every text row has equal length
            if mode == SM.VARIABLE:
                assert K == C == len(sites)
                for k in range(K):                                                   # no column whose bytes other than '-' are all equal
                    column = bytes(r[k] for r in out).replace(b"-", b"")
                    assert len(set(column)) > 1 and set(column) <= set(b"ACGT")
                got = np.zeros((nclass, nclass), dtype=np.uint64)                    # slab 0 again, from the text alone
                for f in range(nclass):
                    for g in range(nclass):
                        got[f, g] = sum(1 for x, y in zip(out[f], out[g]) if x != y and x != 45 and y != 45)
                assert (got == M[0]).all()
    held = SM._classes(all_rows, cls, nclass, c["want"])
    if all(len(v) == nclass for v in held.values()):                                 # the strict core: the models of 0.9 and 0.11
        for mode in (SM.ALL, SM.VARIABLE):
            assert texts[mode] == CM.concat(all_rows, cls, nclass, c["headers"], width, mode, c["want"])
        sM, sC, sK = BM.counts(all_rows, cls, nclass, c["replicates"], c["seed"], c["draws"], c["want"])
        assert (M == sM).all() and (C, nclean) == (sC, sK) and (clean == nclean).all()
        return True
    return False


@pytest.mark.parametrize("name", ACCEPTED)
def test_invariants_on_the_crafted_calls(name):
    c = SC.CASES[name]
    for width in c["widths"]:
        check_invariants(rows(name), c, width)


def test_invariants_on_200_random_calls():
    rng = np.random.default_rng(1202)
    strict = partial = 0
    for k in range(200):
        c = SC.random_call(rng, full=k % 4 == 0)
        if check_invariants(CM.rows_of(c["groups"]), c, c["widths"][0]):
            strict += 1
        else:
            partial += 1
    assert strict >= 50 and partial >= 100


@pytest.mark.parametrize("name", sorted(n for n, c in SC.CASES.items() if c["refused"]))
def test_refused_calls(name):
    c = SC.CASES[name]
    with pytest.raises(SM.Refused, match="group"):
        SM.concat_partial(rows(name), c["cls"], c["nclass"], c["headers"], 80, SM.ALL)
    with pytest.raises(SM.Refused, match="group"):
        SM.counts_partial(rows(name), c["cls"], c["nclass"], 2, 1)


def test_refused_arguments():
    r, h = [[b"ACGT", b"AGGT"]], [b">a\n", b">b\n", b">c\n"]
    assert SM.concat_partial(r, [0, 2], 3, h, 80, SM.ALL)[0] == b">a\nACGT\n>b\n----\n>c\nAGGT\n"
    for args in ((r, [0, 2], 3, h, 0, SM.ALL), (r, [0, 2], 0, [], 80, SM.ALL), (r, [0, 3], 3, h, 80, SM.ALL), (r, None, 3, h, 80, SM.ALL), (r, [0, 2], 3, None, 80, SM.ALL),
                 (r, [0, 2], 3, h, 80, 2), (r, [2, 2], 3, h, 80, SM.ALL), (r, [0, 1], 1, h[:1], 80, SM.ALL)):
        with pytest.raises(SM.Refused):
            SM.concat_partial(*args)
    for args in ((r, [0, 2], 3, 100001, 1), (r, [0, 2], 3, 1, 2 ** 64), (r, [0, 2], 3, 1, 1, 2 ** 32), (r, [1, 1], 3, 1, 1), (r, [0, 1], 1, 1, 1)):
        with pytest.raises(SM.Refused):
            SM.counts_partial(*args)
    with pytest.raises(SM.TooLarge):
        SM.counts_partial(r, [0, 2], 1024, 128, 1)


def test_the_crafted_cases_are_what_they_say():
    held = lambda name: [sorted(v) for _, v in sorted(SM._classes(rows(name), SC.CASES[name]["cls"], SC.CASES[name]["nclass"], None).items())]      # noqa: E731
    assert held("presence_sets") == held("presence_sets_permuted_rows") == [[0, 1, 2], [0, 2], [0, 1], [1, 2], [2]]
    assert SC.CASES["presence_sets_permuted_rows"]["cls"][:3] != [0, 1, 2]
    for name in ("presence_sets", "gap_fill_next_to_a_neighbour", "site_around_an_absent_class", "not_variable_by_the_absent_row"):
        assert rows(name) == SC.CASES[name]["groups"]                                # no indels: the rows are the strings
    c = SC.CASES["gap_fill_next_to_a_neighbour"]
    assert [len(g[0]) for g in c["groups"]] == [1, 2, 3, 15, 16, 17] and c["widths"] == list(range(1, 101))
    assert held("gap_fill_next_to_a_neighbour") == [[0, 1], [0, 2]] * 3
    out = CM.split_fasta(SM.concat_partial(rows("gap_fill_next_to_a_neighbour"), c["cls"], 3, c["headers"], 100, SM.ALL)[0], c["headers"])
    assert out[1] == b"C--TCA" + b"-" * 15 + b"CCGTACGTACGTACGA" + b"-" * 17 and out[2] == b"-GT---" + b"CCGTACGTACGTACT" + b"-" * 16 + b"CCGTACGTACGTACGTC"
    for name, n in (("class_without_a_group_empty_header", 0), ("class_without_a_group_header_300", 300)):
        c = SC.CASES[name]
        lone = [f for f in range(3) if not any(f in h for h in held(name))]
        assert len(lone) == 1 and len(c["headers"][lone[0]]) == n
        M, C, _, clean = SM.counts_partial(rows(name), c["cls"], 3, 1, 1)
        assert C == 2 and not clean[lone[0]].any() and not M[:, lone[0]].any()
    c = SC.CASES["site_around_an_absent_class"]
    assert SM.concat_partial(rows("site_around_an_absent_class"), c["cls"], 3, [b""] * 3, 80, SM.VARIABLE)[0] == b"G\n-\nT\n"
    c = SC.CASES["not_variable_by_the_absent_row"]
    M, C, nclean, clean = SM.counts_partial(rows("not_variable_by_the_absent_row"), c["cls"], 3, 1, 1)
    assert (C, nclean) == (0, 20) and clean.tolist() == [[20, 0, 20], [0, 0, 0], [20, 0, 20]]
    r = rows("codes_and_a_centre_gap")
    assert b"N" in r[0][1] and any(x in r[0][1] for x in b"acgt") and r[1][0].count(b"-") == 3
    sites = SM.concat_partial(r, SC.CASES["codes_and_a_centre_gap"]["cls"], 3, [b""] * 3, 80, SM.VARIABLE)[2]
    assert [col for g, col, _ in sites if g == 0] == [0, 12, 17, 31] and any(col != before for g, col, before in sites if g == 1)
    c = SC.CASES["draws_70000_one_site_class_1_absent"]
    M, C, _, _ = SM.counts_partial(rows("draws_70000_one_site_class_1_absent"), c["cls"], 3, 2, 1, 70000)
    assert C == 1 and M[1].tolist() == M[2].tolist() == [[0, 0, 70000], [0, 0, 0], [70000, 0, 0]]
    assert held("one_row_groups_only") == [[1], [0]]
    seen = set()
    for name in ACCEPTED:
        if name.startswith("classes_"):
            n = SC.CASES[name]["nclass"]
            h = held(name)
            assert len(h[1]) == n and len(h[0]) < n
            seen |= {(n, f) for f in range(n) if f not in h[0]}
    assert seen >= {(33, 31), (33, 32), (65, 31), (65, 32), (65, 63), (65, 64), (70, 31), (70, 32), (70, 63), (70, 64)}
