"""The tree of the input files from the pair counts of the core-genome alignment (--coretree / --corefilteredtree):
distances from counts, neighbour joining (Studier and Keppler's form of Saitou and Nei's method), the bipartitions of a tree, bootstrap
support and the canonical Newick text.  numpy only: matrices of files x files belong on the host.  Everything is one fixed sequence of
float64 operations on integers, so the same counts give the same text, byte for byte.

A tree is unrooted: leaves 0 .. n - 1 (the files), internal nodes n .., and `edges`, a list of (node, node, length)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

MODELS = ("p", "jc")
BAD_NAME_BYTES = "()[]:;,'\""


class Saturated(ValueError):
    """a pair of files too far apart for the Jukes-Cantor correction; .pair = (f, g)"""

    def __init__(self, f: int, g: int, p: float):
        ValueError.__init__(self, "files %d and %d differ in %.6f of the columns: no Jukes-Cantor distance at 0.75 and beyond" % (f, g, p))
        self.pair = (f, g)


class NoSharedColumn(ValueError):
    """a pair of files without a column to compare them in (a denominator of 0 in a matrix K); .pair = (f, g)"""

    def __init__(self, f: int, g: int, names: Optional[Sequence[str]] = None):
        a, b = (names[f], names[g]) if names is not None else ("%d" % f, "%d" % g)
        ValueError.__init__(self, "files %s and %s share no column in which both hold one of A C G T: they have no distance" % (a, b))
        self.pair = (f, g)


class Tree:
    def __init__(self, n: int, edges):
        self.n, self.edges = n, list(edges)


def check_names(names: Sequence[str]) -> None:
    """Newick takes a name as it is only without its own punctuation, quotes and white space"""
    for name in names:
        if not name or any(ch in BAD_NAME_BYTES or ch.isspace() for ch in name):
            raise ValueError("the name %r cannot stand in a Newick tree: it is empty or holds one of ( ) [ ] : ; , a quote or white space" % name)


def distances(M, K, model: str = "p", names: Optional[Sequence[str]] = None) -> np.ndarray:
    """counts of differing columns M (files x files) over K columns -> distances: the proportion p, or Jukes and Cantor's correction.
    K: one number, or a matrix files x files with the columns of every pair (the soft core): a pair of two files with
    K[f][g] == 0 raises NoSharedColumn, which names them (by `names` where given)"""
    if model not in MODELS:
        raise ValueError("unknown model %r" % (model,))
    if np.ndim(K) == 0:
        p = np.asarray(M).astype(np.float64) / K
    else:
        K = np.asarray(K).astype(np.float64)
        if K.shape != np.shape(M):
            raise ValueError("the columns per pair must have the shape of the counts")
        bad = np.argwhere((K == 0) & ~np.eye(len(K), dtype=bool))
        if len(bad):
            raise NoSharedColumn(int(bad[0][0]), int(bad[0][1]), names)
        p = np.asarray(M).astype(np.float64) / np.where(K == 0, 1.0, K)              # a diagonal cell: 0 over anything
    if model == "p":
        return p
    bad = np.argwhere(p >= 0.75)
    if len(bad):
        f, g = (int(x) for x in bad[0])
        raise Saturated(f, g, float(p[f, g]))
    return -0.75 * np.log(1 - 4 * p / 3)


def neighbour_joining(D) -> Tree:
    D = np.array(D, dtype=np.float64)
    n = len(D)
    if n < 3 or D.shape != (n, n):
        raise ValueError("neighbour joining takes a square matrix over three or more files")
    ids = list(range(n))
    edges, nxt = [], n
    while len(ids) > 3:
        m = len(ids)
        r = D.sum(axis=1)
        Q = (m - 2) * D - r[:, None] - r[None, :]
        Q[np.tril_indices(m)] = np.inf
        i, j = divmod(int(np.argmin(Q)), m)                                      # the first of the smallest, row-major over i < j
        dij = D[i, j]
        li = dij / 2 + (r[i] - r[j]) / (2 * (m - 2))
        lj = dij - li
        if li < 0:
            li, lj = 0.0, dij
        elif lj < 0:
            li, lj = dij, 0.0
        edges += [(nxt, ids[i], float(li)), (nxt, ids[j], float(lj))]
        row = (D[i] + D[j] - dij) / 2
        D[i, :] = row
        D[:, i] = row
        D[i, i] = 0.0
        D = np.delete(np.delete(D, j, axis=0), j, axis=1)
        ids[i] = nxt
        del ids[j]
        nxt += 1
    a, b, c = ids
    edges += [(nxt, a, max(0.0, float((D[0, 1] + D[0, 2] - D[1, 2]) / 2))), (nxt, b, max(0.0, float((D[0, 1] + D[1, 2] - D[0, 2]) / 2))),
              (nxt, c, max(0.0, float((D[0, 2] + D[1, 2] - D[0, 1]) / 2)))]
    return Tree(n, edges)


class _Rooted:
    """the tree hung from the internal node next to leaf 0: per node its children in canonical order (by the smallest leaf below), the
    length of the edge to its parent and the leaves below it as a bit mask"""

    def __init__(self, tree: Tree):
        adj: Dict[int, list] = {}
        for u, v, ln in tree.edges:
            adj.setdefault(u, []).append((v, ln))
            adj.setdefault(v, []).append((u, ln))
        self.top = adj[0][0][0]
        self.children: Dict[int, List[int]] = {}
        self.length: Dict[int, float] = {}
        self.mask: Dict[int, int] = {}
        self.least: Dict[int, int] = {}
        order, stack, parent = [], [self.top], {self.top: -1}
        while stack:
            v = stack.pop()
            order.append(v)
            for w, ln in adj[v]:
                if w != parent[v]:
                    parent[w] = v
                    self.length[w] = ln
                    stack.append(w)
        for v in reversed(order):
            kids = [w for w, _ in adj[v] if w != parent[v]]
            if v < tree.n:
                self.mask[v], self.least[v] = 1 << v, v
            else:
                kids.sort(key=lambda w: self.least[w])
                self.mask[v] = sum(self.mask[w] for w in kids)
                self.least[v] = self.least[kids[0]]
            self.children[v] = kids
        self.internal = [v for v in order if v >= tree.n and v != self.top]      # one per internal edge: the node below it


def bipartitions(tree: Tree) -> List[int]:
    """per internal edge the files on the side that does not hold file 0, as a bit mask"""
    r = _Rooted(tree)
    return [r.mask[v] for v in r.internal]


def support(tree: Tree, replicate_trees) -> Dict[int, int]:
    """bipartition of an internal edge of `tree` -> the number of replicate trees that hold it"""
    out = {b: 0 for b in bipartitions(tree)}
    for t in replicate_trees:
        for b in set(bipartitions(t)):
            if b in out:
                out[b] += 1
    return out


def newick(tree: Tree, names: Sequence[str], support: Optional[Dict[int, int]] = None, B: int = 0) -> str:
    """the canonical text: from the internal node next to file 0, children by their smallest file, lengths %.9f; with B > 0 every internal
    node but the top one carries its edge's support in percent, ties going up.  One line, ';' and a line feed"""
    check_names(names)
    if len(names) != tree.n:
        raise ValueError("%d names for %d files" % (len(names), tree.n))
    r = _Rooted(tree)
    text: Dict[int, str] = {}
    stack = [(r.top, False)]
    while stack:
        v, done = stack.pop()
        if v < tree.n:
            text[v] = "%s:%.9f" % (names[v], r.length[v])
        elif not done:
            stack.append((v, True))
            stack += [(w, False) for w in r.children[v]]
        else:
            inner = "(" + ",".join(text.pop(w) for w in r.children[v]) + ")"
            if v == r.top:
                text[v] = inner + ";\n"
            else:
                label = "%d" % ((200 * (support or {}).get(r.mask[v], 0) + B) // (2 * B)) if B > 0 else ""
                text[v] = "%s%s:%.9f" % (inner, label, r.length[v])
    return text[r.top]


def tree_text(counts, K, model: str, names: Sequence[str]) -> str:
    """counts: (B + 1, files, files), slab 0 of all sites and one slab per replicate; K: the columns they were taken from, one number
    or one per pair of files (distances) -> the Newick text of slab 0's tree with the support of the B replicate trees"""
    B = len(counts) - 1
    main = neighbour_joining(distances(counts[0], K, model, names))
    reps = [neighbour_joining(distances(counts[r], K, model, names)) for r in range(1, B + 1)]
    return newick(main, names, support(main, reps) if B else None, B)
