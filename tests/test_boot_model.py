"""tests/boot_model.py, the restatement of the bootstrap pair counts (include/sibelia_amd.h) that the GPU tests of
sbl_group_bootstrap compare against, checked here against known answers, a plain-integer restatement of the draw rule, the texts of
tests/concat_model.py and the properties a count matrix has; and tests/boot_cases.py, checked to hold what it says."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_cases as BC                            # noqa: E402
import boot_model as BM                            # noqa: E402
import concat_model as CM                          # noqa: E402


def rows_of(c):
    """the rows of a case: a group of rows of one length without indels is its own alignment"""
    if all(len({len(r) for r in g}) == 1 for g in c["groups"]):
        return c["groups"]
    return CM.rows_of(c["groups"])


def model(c):
    return BM.counts(rows_of(c), c["cls"], c["nclass"], c["replicates"], c["seed"], c["draws"], c["want"])


def test_the_known_draws():
    assert BM.draw(1, 1, np.arange(10), 1000).tolist() == [88, 459, 719, 254, 99, 168, 881, 400, 994, 398]
    assert BM.draw(2 ** 64 - 1, 3, np.arange(5), 7).tolist() == [4, 0, 3, 0, 0]
    assert [BM.draw_int(1, 1, i, 1000) for i in range(10)] == [88, 459, 719, 254, 99, 168, 881, 400, 994, 398]
    assert [BM.draw_int(2 ** 64 - 1, 3, i, 7) for i in range(5)] == [4, 0, 3, 0, 0]
    w = BM.weights(1, 1, 250000, 250000)
    assert w.max() == 8 and w.sum() == 250000 and round(100 * float((w == 0).mean()), 1) == 36.8


def test_numpy_against_plain_integers():
    rng = np.random.default_rng(7)
    cases = [(2 ** 64 - 1, 1, 0, 1), (2 ** 64 - 1, 100000, 2 ** 32 - 1, 2 ** 32 - 1), (0, 1, 0, 2 ** 32 - 1), (1, 100000, 2 ** 32 - 1, 1)]
    while len(cases) < 1000:
        C = int(rng.choice([1, 2, 3, 7, 1000, 250000, 2 ** 31, 2 ** 32 - 1, int(rng.integers(1, 2 ** 32))]))
        cases.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(1, 100001)), int(rng.integers(0, 2 ** 32)), C))
    for seed, r, i, C in cases:
        got = int(BM.draw(seed, r, i, C))
        assert got == BM.draw_int(seed, r, i, C) and 0 <= got < C, (seed, r, i, C)
    i = np.arange(5000, dtype=np.uint64)
    assert BM.draw(12345, 77, i, 977).tolist() == [BM.draw_int(12345, 77, int(x), 977) for x in i]


def pair_counts_of_text(text: bytes, headers):
    rows = [np.frombuffer(r, dtype=np.uint8) for r in CM.split_fasta(text, headers)]
    return [[int((a != b).sum()) for b in rows] for a in rows]


@pytest.mark.parametrize("name", sorted(n for n, c in BC.CASES.items() if not c["refused"]))
def test_a_case_has_the_properties_of_its_counts(name):
    c = BC.CASES[name]
    M, C, K = model(c)
    n, B = c["nclass"], c["replicates"]
    assert M.shape == (B + 1, n, n) and M.dtype == np.uint64
    if c["sites"] is not None:
        assert C == c["sites"]
    headers = [b">%d\n" % f for f in range(n)]
    snps = CM.concat(rows_of(c), c["cls"], n, headers, 80, CM.VARIABLE, c["want"])
    assert M[0].tolist() == pair_counts_of_text(snps[0], headers) and C == len(snps[2])
    full = CM.split_fasta(CM.concat(rows_of(c), c["cls"], n, headers, 80, CM.ALL, c["want"])[0], headers)
    assert K == sum(all(r[x] in b"ACGT" for r in full) for x in range(len(full[0]))) and C <= K
    assert (M == M.transpose(0, 2, 1)).all() and all((M[r].diagonal() == 0).all() for r in range(B + 1))
    nd = c["draws"] or C
    S, _ = BM.site_matrix(rows_of(c), c["cls"], n, c["want"])
    for r in range(1, min(B, 3) + 1):
        if C == 0:
            assert not M[r].any()
            continue
        w = BM.weights(c["seed"], r, nd, C)
        assert w.sum() == nd and len(w) == C
        # every draw lands on a site, and a site parts at least one pair: the upper triangle counts every draw at least once
        assert int(np.triu(M[r]).sum()) >= nd
        by_hand = np.zeros((n, n), dtype=np.int64)
        for site in BM.draw(c["seed"], r, np.arange(nd, dtype=np.uint64), C).tolist()[:2000] if nd <= 2000 else []:
            col = S[:, site]
            by_hand += col[:, None] != col[None, :]
        if nd <= 2000:
            assert by_hand.tolist() == M[r].tolist()


def test_the_cases_hold_what_they_say():
    assert {c["sites"] for n, c in BC.CASES.items() if n.startswith("sites_")} == set(BC.SITE_COUNTS)
    assert {c["nclass"] for n, c in BC.CASES.items() if n.startswith("classes_")} == set(BC.CLASS_COUNTS)
    assert {c["replicates"] for n, c in BC.CASES.items() if n.startswith("replicates_")} == set(BC.REPLICATE_COUNTS) | {1000}
    assert {c["seed"] for n, c in BC.CASES.items() if n.startswith("seed_")} == set(BC.SEEDS)
    # the first and the last column of a group are sites
    for n in (15, 4097):
        c = BC.CASES["sites_%d" % n]
        S = CM.concat(c["groups"], c["cls"], 3, [b">\n"] * 3, 80, CM.VARIABLE)[2]
        assert S[0][1] == 0 and S[-1][1] == len(c["groups"][0][0]) - 1
    # all draws on one site pass 8 and 16 bits; on two sites one pair counts every draw and the other two share them
    one, _, _ = model(BC.CASES["draws_70000_on_one_site"])
    assert one[1].tolist() == one[2].tolist() == [[0, 70000], [70000, 0]] and one[0].tolist() == [[0, 1], [1, 0]]
    two, C, _ = model(BC.CASES["draws_70000_on_two_sites"])
    assert C == 2 and two[0].tolist() == [[0, 1, 1], [1, 0, 2], [1, 2, 0]]
    for r in (1, 2):
        assert two[r][1][2] == 70000 and two[r][0][1] + two[r][0][2] == 70000 and min(two[r][0][1], two[r][0][2]) > 255
    # replicates differ from each other and from seed to seed
    a, _, _ = model(BC.CASES["seed_0"])
    assert a[1].tolist() != a[2].tolist()
    c = dict(BC.CASES["seed_0"], seed=5)
    assert model(c)[0][1].tolist() != a[1].tolist() and model(c)[0][0].tolist() == a[0].tolist()


def test_what_the_model_refuses():
    ok = BC.CASES["draws_70000_on_one_site"]
    for change in (dict(replicates=100001), dict(replicates=-1), dict(seed=2 ** 64), dict(nclass=0), dict(nclass=1025), dict(cls=[0, 2]), dict(cls=[0, 0]), dict(nclass=3)):
        with pytest.raises(BM.Refused):
            model(dict(ok, **change))
    for name in sorted(n for n, c in BC.CASES.items() if c["refused"]):
        with pytest.raises(BM.Refused):
            model(BC.CASES[name])
    with pytest.raises(BM.TooLarge):
        BM.counts([[b"A"] * 1024], list(range(1024)), 1024, 128, 1)
    assert BM.counts([[b"A"] * 1024], list(range(1024)), 1024, 0, 1)[1:] == (0, 1)
