"""Distance matrices for the neighbour joining of a batch (tests/nj_model.py, csrc/tree_nj.hip): what the bootstrap makes -- integer
counts over K columns, both models, with counts so small that the criterion ties constantly, sometimes and rarely -- at every size at
which the row sum or the launch takes another path, and the matrices that are all ties or all zeros, hold identical files, come from a
tree or give a negative length.  CASES: (label, float64 matrix); the references of tree.neighbour_joining are made once (reference)."""
import struct

import numpy as np

from sibelia_amd import tree as T

K = 100003
SIZES = (3, 4, 5, 7, 8, 9, 10, 12, 15, 16, 17, 31, 32, 33, 63, 64)
BOUNDS = (3, 50, 5000)                              # counts below: ties constantly, sometimes, rarely
NEGATIVE = [[0, 1, 3, 4], [1, 0, 6, 7], [3, 6, 0, 2], [4, 7, 2, 0]]      # tests/test_tree.py: l_0 = -1 at the first join


def counts(rng, n, bound):
    M = np.triu(rng.integers(0, bound, size=(n, n)), 1)
    return (M + M.T).astype(np.uint64)


def additive(rng, n):
    """the leaf distances of a random unrooted binary tree over n leaves with integer edge lengths 1 .. 40"""
    edges = [(n, 0), (n, 1), (n, 2)]
    nxt = n + 1
    for leaf in range(3, n):
        u, v = edges.pop(int(rng.integers(0, len(edges))))
        edges += [(u, nxt), (nxt, v), (nxt, leaf)]
        nxt += 1
    adj = {}
    for u, v in edges:
        ln = float(rng.integers(1, 41))
        adj.setdefault(u, []).append((v, ln))
        adj.setdefault(v, []).append((u, ln))
    D = np.zeros((n, n))
    for a in range(n):
        dist, stack = {a: 0.0}, [a]
        while stack:
            x = stack.pop()
            for y, ln in adj[x]:
                if y not in dist:
                    dist[y] = dist[x] + ln
                    stack.append(y)
        D[a] = [dist[b] for b in range(n)]
    return D


def with_copies(rng, n, copies):
    """counts in which the files `copies` are one file several times: distance 0 between them, equal rows otherwise"""
    M = counts(rng, n, 50)
    for c in copies[1:]:
        M[c, :] = M[copies[0], :]
        M[:, c] = M[:, copies[0]]
    for c in copies:
        for d in copies:
            M[c, d] = 0
    M[np.diag_indices(n)] = 0
    return M


def _cases():
    rng = np.random.default_rng(13)
    out = []
    for n in SIZES:
        for bound in BOUNDS:
            M = counts(rng, n, bound)
            for model in T.MODELS:
                out.append(("n%d_below%d_%s" % (n, bound, model), T.distances(M, K, model)))
    for n in (4, 9, 64):
        out.append(("n%d_all_equal" % n, (np.ones((n, n)) - np.eye(n)) * (7 / K)))
    out.append(("n6_two_identical", T.distances(with_copies(rng, 6, [1, 4]), K, "p")))
    out.append(("n9_three_identical", T.distances(with_copies(rng, 9, [0, 3, 8]), K, "jc")))
    out.append(("n17_three_identical", T.distances(with_copies(rng, 17, [2, 3, 16]), K, "p")))
    for n in (3, 5, 12):
        out.append(("n%d_all_zero" % n, np.zeros((n, n))))
    for n in (5, 8, 13, 20):
        out.append(("n%d_additive" % n, additive(rng, n)))
    out.append(("n4_negative_length", np.array(NEGATIVE, dtype=np.float64)))
    return out


CASES = _cases()
LABELS = [label for label, _ in CASES]
_REFERENCE = {}


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def reference(label):
    """(edges of tree.neighbour_joining with the length as its 8 bytes, its bipartitions sorted), made once per case"""
    if label not in _REFERENCE:
        t = T.neighbour_joining(dict(CASES)[label])
        _REFERENCE[label] = ([(u, v, bits(ln)) for u, v, ln in t.edges], sorted(T.bipartitions(t)))
    return _REFERENCE[label]
