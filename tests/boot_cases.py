"""Crafted calls for the tests of the bootstrap pair counts, shared by tests/test_boot_model.py and
tests/test_gpu_group_bootstrap.py.  A case: groups (lists of byte strings, centre first), cls (flat, one class per instance), nclass,
replicates, seed, draws (0: as many as sites), want (None: all), refused (the call is SBL_ERR_BAD_ARG) and sites (the number of sites
the case is made to have, None where it is not pinned).  What each case is for stands next to it; tests/test_boot_model.py checks that
it does what it says."""
import numpy as np

import concat_cases as CC

SEEDS = (0, 1, 2 ** 64 - 1)
SITE_COUNTS = (0, 1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)
CLASS_COUNTS = (2, 3, 8, 9, 31, 32, 33, 64, 65, 70)
REPLICATE_COUNTS = (0, 1, 2, 63, 64, 65)
SPACING = 8


def case(groups, cls, nclass, replicates=3, seed=1, draws=0, want=None, refused=False, sites=None):
    return dict(groups=[[bytes(s) for s in g] for g in groups], cls=list(cls), nclass=nclass, replicates=replicates, seed=seed, draws=draws, want=want,
                refused=refused, sites=sites)


def other(base: int, step: int = 1) -> int:
    return b"ACGT"[(b"ACGT".index(base) + step) % 4]


def rand(rng, n: int) -> bytes:
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def spaced_group(rng, nrows: int, nsites: int):
    """nrows rows without indels and exactly nsites sites, SPACING columns apart, the first one on column 0 and the last one on the last
    column: site k changes row 1 + k % (nrows - 1), every fifth one a second row to a third base (two pairs more differ there)"""
    L = max(20, SPACING * (nsites - 1) + 1) if nsites != 1 else 20
    c = rand(rng, L)
    rows = [bytearray(c) for _ in range(nrows)]
    for k in range(nsites):
        at = SPACING * k if nsites > 1 else 7
        rows[1 + k % (nrows - 1)][at] = other(c[at])
        if k % 5 == 4 and nrows > 2:
            rows[1 + (k + 1) % (nrows - 1)][at] = other(c[at], 2)
    return [bytes(r) for r in rows]


def scattered_group(rng, nrows: int, L: int, per_row: int):
    """nrows rows without indels: every member row differs from the centre in per_row columns of its own choice (some shared by chance)"""
    c = rand(rng, L)
    rows = [c]
    for _ in range(1, nrows):
        b = bytearray(c)
        for at in rng.choice(L, per_row, replace=False):
            b[at] = other(c[at], int(rng.integers(1, 4)))
        rows.append(bytes(b))
    return rows


_RNG = np.random.default_rng(1101)
_C20 = b"ACGTTGCAACGTTGCAACGT"
_ONE = [_C20, _C20[:5] + b"A" + _C20[6:]]                                          # C = 1, two classes
_TWO = [_C20, _C20[:5] + b"A" + _C20[6:], _C20[:14] + b"T" + _C20[15:]]            # C = 2, three classes: site 0 parts class 1, site 1 class 2

CASES = {name: case(c["groups"], c["cls"], c["nclass"], want=c["want"], refused=c["refused"]) for name, c in CC.CASES.items() if not name.startswith("short_groups_width_") or name.endswith("_80")}
for _n in SITE_COUNTS:
    CASES["sites_%d" % _n] = case([spaced_group(_RNG, 3, _n)], [1, 2, 0], 3, replicates=3, sites=_n)
for _n in CLASS_COUNTS:
    CASES["classes_%d" % _n] = case([scattered_group(_RNG, _n, 120, 3), scattered_group(_RNG, _n, 40, 2)],
                                    [int(x) for _ in range(2) for x in _RNG.permutation(_n)], _n, replicates=2)
for _b in REPLICATE_COUNTS:
    CASES["replicates_%d" % _b] = case([spaced_group(_RNG, 4, 40)], [0, 1, 2, 3], 4, replicates=_b, sites=40)
CASES["replicates_1000_on_few_sites"] = case([spaced_group(_RNG, 8, 30)], [3, 1, 4, 0, 5, 7, 2, 6], 8, replicates=1000, sites=30)
for _s in SEEDS:
    CASES["seed_%d" % _s] = case([spaced_group(_RNG, 4, 100)], [0, 1, 2, 3], 4, replicates=4, seed=_s, sites=100)
for _d in (1, 39, 41):                                                              # one draw, C - 1, C + 1
    CASES["draws_%d_of_40_sites" % _d] = case([spaced_group(_RNG, 3, 40)], [0, 1, 2], 3, replicates=5, draws=_d, sites=40)
# all draws on one site: its weight passes 255 and 65535; on two sites the pair (1, 2) differs in both and counts all 70000 draws
CASES["draws_70000_on_one_site"] = case([_ONE], [0, 1], 2, replicates=2, draws=70000, sites=1)
CASES["draws_70000_on_two_sites"] = case([_TWO], [0, 1, 2], 3, replicates=2, draws=70000, sites=2)
CASES["no_replicate_too_many"] = case([_ONE], [0, 1], 2, replicates=100001, refused=True)
