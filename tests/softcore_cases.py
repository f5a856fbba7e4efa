"""Crafted calls for the tests of the soft core, shared by tests/test_softcore_model.py and
tests/test_gpu_group_softcore.py.  A case: groups (lists of byte strings, centre first -- a group holds the classes its instances are
given, at most once each), cls (flat, one class per instance), nclass, headers, widths (every line width the case is run with),
replicates, seed, draws, want (None: all) and refused (the call is SBL_ERR_BAD_ARG with the setting on).  What each case is for stands
next to it; tests/test_softcore_model.py checks that it does what it says."""
import numpy as np

import boot_cases as BC
import concat_cases as CC


def case(groups, cls, nclass, headers=None, widths=(80,), replicates=3, seed=1, draws=0, want=None, refused=False):
    if headers is None:
        headers = [b">s%d\n" % f for f in range(nclass)]
    assert len(cls) == sum(len(g) for g in groups)
    return dict(groups=[[bytes(s) for s in g] for g in groups], cls=list(cls), nclass=nclass, headers=list(headers), widths=list(widths), replicates=replicates,
                seed=seed, draws=draws, want=want, refused=refused)


_C20 = b"ACGTTGCAACGTTGCAACGT"


def _sub(s: bytes, *cols) -> bytes:
    b = bytearray(s)
    for x in cols:
        b[x] = BC.other(s[x])
    return bytes(b)


# five groups of 20 columns that hold {0,1,2}, {0,2}, {0,1}, {1,2} and {2}; every group of two rows or more has a site in a column of its own
_SETS = [[_C20, _sub(_C20, 3), _sub(_C20, 3, 9)], [_C20, _sub(_C20, 5)], [_C20, _sub(_C20, 0)], [_C20, _sub(_C20, 19)], [_C20]]
# the short groups of concat_cases (L = 1, 2, 3, 15, 16, 17, two rows, first and last column variable): every one holds class 0, the
# even ones class 1 and the odd ones class 2, so that in rows 1 and 2 a gap fill lies next to a present row of the neighbouring group
_SHORT_CLS = [x for k in range(len(CC._SHORT)) for x in (0, 1 + k % 2)]


def _absent_at(nclass: int, absent, rng):
    """two groups of 40 and 24 columns; the first holds every class but `absent`, the second every class: scattered differences"""
    held = [f for f in range(nclass) if f not in absent]
    g0, g1 = BC.scattered_group(rng, len(held), 40, 3), BC.scattered_group(rng, nclass, 24, 2)
    order = [int(x) for x in rng.permutation(len(held))]
    return case([g0, g1], [held[k] for k in order] + [int(x) for x in rng.permutation(nclass)], nclass, replicates=2)


_RNG = np.random.default_rng(1201)

CASES = {
    "presence_sets": case(_SETS, [0, 1, 2, 0, 2, 0, 1, 1, 2, 2], 3, widths=(80, 7)),
    "presence_sets_permuted_rows": case(_SETS, [2, 0, 1, 2, 0, 1, 0, 2, 1, 2], 3, widths=(80, 16)),
    "gap_fill_next_to_a_neighbour": case(CC._SHORT, _SHORT_CLS, 3, [b">first\n", b">second file\n", b">3\n"], widths=range(1, 101)),
    "class_without_a_group_empty_header": case(_SETS[1:3], [0, 1, 0, 1], 3, [b">a\n", b">b\n", b""], widths=(80, 3)),
    "class_without_a_group_header_300": case(_SETS[1:3], [0, 2, 0, 2], 3, [b">a\n", CC._header(300), b">c\n"], widths=(80, 16, 17)),
    # the rows of classes 0 and 2 differ in column 5 and class 1, which lies between them, is absent
    "site_around_an_absent_class": case([[_C20, _sub(_C20, 5)]], [0, 2], 3),
    # rows equal: with the absent row taken as a row of '-' every column would vary; none is kept, all are clean
    "not_variable_by_the_absent_row": case([[_C20, _C20]], [0, 2], 3),
    # present rows with N and lower case (columns 5, 9: clean for nobody), a centre with a gap (the member holds three bases more)
    "codes_and_a_centre_gap": case([[CC._C32, CC._R1], [_C20, _C20[:8] + b"GAG" + _sub(_C20, 15)[8:]]], [0, 1, 2, 0], 3, widths=(80, 16)),
    "draws_70000_one_site_class_1_absent": case([[_C20, _sub(_C20, 5)]], [0, 2], 3, replicates=2, draws=70000),
    "one_row_groups_only": case([[_C20], [_C20[:7]]], [1, 0], 2, widths=(80, 5)),
    "group_with_a_class_twice": case([_SETS[0], [_C20, _sub(_C20, 5)]], [0, 1, 2, 2, 2], 3, refused=True),
    "four_rows_for_three_classes": case([_SETS[0] + [_sub(_C20, 7)]], [0, 1, 2, 0], 3, refused=True),
}
for _n, _absent in ((33, (31,)), (33, (32,)), (65, (31, 32)), (65, (63,)), (65, (64,)), (70, (63, 64)), (70, (31, 32, 63, 64))):
    CASES["classes_%d_absent_%s" % (_n, "_".join(map(str, _absent)))] = _absent_at(_n, _absent, _RNG)


def random_call(rng, full=False):
    """a call of 1 .. 6 groups over 2 .. 6 classes: every group holds a random non-empty subset of the classes (all of them with `full`)
    in a random row order; rows without indels, up to 60 columns, with an N now and then -- strings, to be aligned by the caller"""
    nclass = int(rng.integers(2, 7))
    groups, cls = [], []
    for _ in range(int(rng.integers(1, 7))):
        r = nclass if full else int(rng.integers(1, nclass + 1))
        L = int(rng.integers(1, 61))
        c = BC.rand(rng, L)
        rows = [c]
        for _ in range(1, r):
            b = bytearray(c)
            for at in rng.choice(L, min(L, 3), replace=False):
                b[at] = b"ACGTN"[int(rng.integers(0, 5))]
            rows.append(bytes(b))
        groups.append(rows)
        cls += [int(x) for x in rng.permutation(nclass)[:r]]
    return case(groups, cls, nclass, widths=(int(rng.integers(1, 40)),), replicates=2, seed=int(rng.integers(0, 2 ** 63)))
