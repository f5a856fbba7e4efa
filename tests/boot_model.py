"""The bootstrap pair counts of the core-genome alignment (include/sibelia_amd.h) restated in numpy on the kept columns
of concat_model, for tests/test_boot_model.py and the GPU tests of sbl_group_bootstrap (never used by the product).

`draw(seed, r, i, C)`                      -> the site of draw i of replicate r: numpy uint64, i a scalar or an array.
`draw_int(seed, r, i, C)`                  -> the same in plain Python integers.
`site_matrix(groups, cls, nclass, want)`   -> (uint8 array (nclass, C): the bytes of the sites, row f the class f; K); Refused where the
                                              library answers SBL_ERR_BAD_ARG.
`counts(groups, cls, nclass, replicates, seed, draws, want)` -> (uint64 array (replicates + 1, nclass, nclass), C, K).
`counts_of_sites(S, replicates, seed, draws)` -> the same array from a site matrix, e.g. the rows of a SNP text.
`weights(seed, r, n, C)`                   -> how often every site is drawn in replicate r.
"""
import numpy as np

import concat_model as CM

Refused = CM.Refused
MAX_REPLICATES = 100000
MAX_CELLS = 2 ** 27
_M64 = (1 << 64) - 1
_GOLD, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


class TooLarge(ValueError):
    """what the library answers with SBL_ERR_TOO_LARGE"""


def draw(seed, r, i, C):
    u = np.uint64
    with np.errstate(over="ignore"):
        ctr = (u(r) << u(32)) | np.asarray(i, dtype=np.uint64)
        z = u(seed) + u(_GOLD) * (ctr + u(1))
        z = (z ^ (z >> u(30))) * u(_M1)
        z = (z ^ (z >> u(27))) * u(_M2)
        z = z ^ (z >> u(31))
        return ((z >> u(32)) * u(C)) >> u(32)


def draw_int(seed, r, i, C):
    ctr = (r << 32) | i
    z = (seed + _GOLD * (ctr + 1)) & _M64
    z = ((z ^ (z >> 30)) * _M1) & _M64
    z = ((z ^ (z >> 27)) * _M2) & _M64
    z ^= z >> 31
    return ((z >> 32) * C) >> 32


def weights(seed, r, n, C):
    return np.bincount(draw(seed, r, np.arange(n, dtype=np.uint64), C).astype(np.int64), minlength=C)


def site_matrix(groups, cls, nclass, want=None):
    total = sum(CM.ninst(g) for g in groups)
    if not 1 <= nclass <= CM.MAX_CLASS or (cls is None and total):
        raise Refused("classes")
    if any(not 0 <= x < nclass for x in (cls or [])):
        raise Refused("a class is not below the number of classes")
    first = [0]
    for g in groups:
        first.append(first[-1] + CM.ninst(g))
    parts, K = [], 0
    for g in CM.used(groups, want):
        rows = groups[g]
        classes = cls[first[g]:first[g + 1]]
        if sorted(classes) != list(range(nclass)):
            raise Refused("group %d does not hold every class exactly once" % g)
        a = np.array([np.frombuffer(r, dtype=np.uint8) for r in rows]).reshape(len(rows), len(rows[0]))
        K += int(CM._BASE[a].all(axis=0).sum())
        by_class = np.empty_like(a)
        by_class[list(classes)] = a
        parts.append(by_class[:, CM.kept_columns(rows, CM.VARIABLE)])
    S = np.concatenate(parts, axis=1) if parts else np.zeros((nclass, 0), dtype=np.uint8)
    return S, K


def counts_of_sites(S, replicates, seed, draws=0):
    n, C = S.shape
    M = np.zeros((replicates + 1, n, n), dtype=np.uint64)
    if C == 0:
        return M
    D = (S[:, None, :] != S[None, :, :]).reshape(n * n, C).astype(np.float64)      # sums below 2^53: exact
    M[0] = D.sum(axis=1).reshape(n, n).astype(np.uint64)
    nd = draws if draws else C
    for r in range(1, replicates + 1):
        M[r] = (D @ weights(seed, r, nd, C).astype(np.float64)).reshape(n, n).astype(np.uint64)
    return M


def counts(groups, cls, nclass, replicates, seed, draws=0, want=None):
    if not 0 <= replicates <= MAX_REPLICATES or not 0 <= seed <= _M64 or not 0 <= draws <= 2 ** 32 - 1:
        raise Refused("replicates, seed or draws")
    S, K = site_matrix(groups, cls, nclass, want)
    if (replicates + 1) * nclass * nclass > MAX_CELLS:
        raise TooLarge("cells")
    return counts_of_sites(S, replicates, seed, draws), S.shape[1], K
