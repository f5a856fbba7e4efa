"""The soft core -- sbl_group_concat and sbl_group_bootstrap under sbl_group_set_partial (include/sibelia_amd.h) --
restated in numpy on the rows of msa_model.msa, for tests/test_softcore_model.py and the GPU tests (never used by the product).

A call is what concat_model takes: groups given by their ROWS (centre first) or by an int (a skipped group of that many instances), and
`cls`, one class per instance, flat.  A used group holds every class AT MOST once; its rows are the rows of the classes it holds.

`present(groups, cls, want)`                                      -> {used group: its classes in row order}
`concat_partial(groups, cls, nclass, headers, width, mode, want)` -> (text, parts, sites) as sbl_group_concat returns them with the setting on
`counts_partial(groups, cls, nclass, replicates, seed, draws, want)` -> (M, C, nclean, clean) as sbl_group_bootstrap and
                                                                     sbl_group_bootstrap_pairs return them with the setting on
Both raise Refused where the library answers SBL_ERR_BAD_ARG, counts_partial TooLarge where it answers SBL_ERR_TOO_LARGE.
"""
import numpy as np

import boot_model as BM
import concat_model as CM

Refused, TooLarge = CM.Refused, BM.TooLarge
ALL, VARIABLE = CM.ALL, CM.VARIABLE


def _classes(groups, cls, nclass, want):
    """the class rule with the setting on, group after group in call order: {used group: its classes in row order}"""
    total = sum(CM.ninst(g) for g in groups)
    if not 1 <= nclass <= CM.MAX_CLASS or (cls is None and total):
        raise Refused("classes")
    if any(not 0 <= x < nclass for x in (cls or [])):
        raise Refused("a class is not below the number of classes")
    first = [0]
    for g in groups:
        first.append(first[-1] + CM.ninst(g))
    out = {}
    for g in CM.used(groups, want):
        classes = list(cls[first[g]:first[g + 1]])
        if len(classes) > nclass:
            raise Refused("group %d has more instances than there are classes" % g)
        if len(set(classes)) != len(classes):
            raise Refused("group %d holds a class twice" % g)
        out[g] = classes
    return out


def present(groups, cls, want=None):
    return _classes(groups, cls, max([1] + [x + 1 for x in cls or []]), want)


def _array(rows):
    return np.array([np.frombuffer(r, dtype=np.uint8) for r in rows]).reshape(len(rows), len(rows[0]))


def concat_partial(groups, cls, nclass, headers, width, mode, want=None):
    if mode not in (ALL, VARIABLE) or not 1 <= width <= 2 ** 32 - 1 or not 1 <= nclass <= CM.MAX_CLASS:
        raise Refused("mode, width or number of classes")
    if headers is None or len(headers) != nclass:
        raise Refused("headers missing")
    held = _classes(groups, cls, nclass, want)
    out_rows = [bytearray() for _ in range(nclass)]
    parts, sites = [], []
    for g in sorted(held):
        rows = groups[g]
        cols = CM.kept_columns(rows, mode)                   # on the present rows: clean and not all equal; one row keeps nothing
        parts.append((g, len(out_rows[0]), len(cols)))
        for f in range(nclass):
            out_rows[f] += bytes(rows[held[g].index(f)][x] for x in cols) if f in held[g] else b"-" * len(cols)
        if mode == VARIABLE:
            sites += [(g, x, x - rows[0][:x].count(b"-")) for x in cols]
    text = b"".join(bytes(h) + CM.wrap(bytes(r), width) for h, r in zip(headers, out_rows))
    return text, parts, sites


def site_matrix_partial(groups, cls, nclass, want=None):
    """-> (S: uint8 (nclass, C), the bytes of the sites, 0 where the class is absent; H: bool (nclass, C), the class is held there;
    clean: uint64 (nclass, nclass); nclean)"""
    held = _classes(groups, cls, nclass, want)
    S, H = [], []
    clean, nclean = np.zeros((nclass, nclass), dtype=np.uint64), 0
    for g in sorted(held):
        a = _array(groups[g])
        k = int(CM._BASE[a].all(axis=0).sum())
        nclean += k
        here = np.zeros(nclass, dtype=bool)
        here[held[g]] = True
        clean += np.uint64(k) * np.outer(here, here).astype(np.uint64)
        cols = CM.kept_columns(groups[g], VARIABLE)
        s = np.zeros((nclass, len(cols)), dtype=np.uint8)
        s[held[g]] = a[:, cols]
        S.append(s)
        H.append(np.repeat(here[:, None], len(cols), axis=1))
    if not S:
        return np.zeros((nclass, 0), dtype=np.uint8), np.zeros((nclass, 0), dtype=bool), clean, nclean
    return np.concatenate(S, axis=1), np.concatenate(H, axis=1), clean, nclean


def counts_partial(groups, cls, nclass, replicates, seed, draws=0, want=None):
    if not 0 <= replicates <= BM.MAX_REPLICATES or not 0 <= seed <= 2 ** 64 - 1 or not 0 <= draws <= 2 ** 32 - 1:
        raise Refused("replicates, seed or draws")
    if 1 <= nclass <= CM.MAX_CLASS and (replicates + 1) * nclass * nclass > BM.MAX_CELLS:
        raise TooLarge("cells")
    S, H, clean, nclean = site_matrix_partial(groups, cls, nclass, want)
    n, C = S.shape
    M = np.zeros((replicates + 1, n, n), dtype=np.uint64)
    if C:
        D = ((S[:, None, :] != S[None, :, :]) & H[:, None, :] & H[None, :, :]).reshape(n * n, C).astype(np.float64)      # sums below 2^53: exact
        M[0] = D.sum(axis=1).reshape(n, n).astype(np.uint64)
        nd = draws if draws else C
        for r in range(1, replicates + 1):
            M[r] = (D @ BM.weights(seed, r, nd, C).astype(np.float64)).reshape(n, n).astype(np.uint64)
    return M, C, nclean, clean
