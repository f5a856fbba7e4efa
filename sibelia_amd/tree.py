"""The tree of the input files from the pair counts of the core-genome alignment (--coretree / --corefilteredtree):
distances from counts, neighbour joining (Studier and Keppler's form of Saitou and Nei's method), the bipartitions of a tree, bootstrap
support and the canonical Newick text.  numpy only: matrices of files x files belong on the host.  Everything is one fixed sequence of
float64 operations on integers, so the same counts give the same text, byte for byte.
--coreconsensus / --coreboottrees: the tally of the replicates' bipartitions, the majority-rule consensus and tree_files,
which makes every text of one set of counts and may be handed a callable that joins all matrices at once (BlockFinder.nj_batch, the
same float64 operations on the device); this module never loads the library itself.

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

    @classmethod
    def of_records(cls, records) -> "Tree":
        """the tree of one tree's edge records (EDGE_RECORD: 2 n - 3 of them, in the order of `edges`)"""
        return cls((len(records) + 3) // 2, [(int(u), int(v), float(ln)) for u, v, ln in zip(records["parent"].tolist(), records["child"].tolist(), records["length"].tolist())])


# one edge of a tree as the neighbour joining of a batch hands it out (BlockFinder.nj_batch): parent, child, length
EDGE_RECORD = np.dtype([("parent", "<u4"), ("child", "<u4"), ("length", "<f8")])
NJ_BATCH_MAX_FILES = 64                            # a callable `nj` takes matrices of at most this many files: its splits are 64-bit masks


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


def support_label(held: int, B: int) -> str:
    """the label of an internal edge that `held` of B replicates hold: the percentage, a tie going up"""
    return "%d" % ((200 * held + B) // (2 * B))


def newick(tree: Tree, names: Sequence[str], support: Optional[Dict[int, int]] = None, B: int = 0, lengths: Optional[Dict[int, int]] = None) -> str:
    """the canonical text: from the internal node next to file 0, children by their smallest file, lengths %.9f; with B > 0 every internal
    node but the top one carries its edge's support in percent, ties going up.  One line, ';' and a line feed.  lengths: node -> an
    integer written in place of the length of the edge above it (--coresnptree: the changes of branches)"""
    check_names(names)
    if len(names) != tree.n:
        raise ValueError("%d names for %d files" % (len(names), tree.n))
    r = _Rooted(tree)
    above = (lambda v: "%.9f" % r.length[v]) if lengths is None else (lambda v: "%d" % lengths[v])
    text: Dict[int, str] = {}
    stack = [(r.top, False)]
    while stack:
        v, done = stack.pop()
        if v < tree.n:
            text[v] = "%s:%s" % (names[v], above(v))
        elif not done:
            stack.append((v, True))
            stack += [(w, False) for w in r.children[v]]
        else:
            inner = "(" + ",".join(text.pop(w) for w in r.children[v]) + ")"
            if v == r.top:
                text[v] = inner + ";\n"
            else:
                label = support_label((support or {}).get(r.mask[v], 0), B) if B > 0 else ""
                text[v] = "%s%s:%s" % (inner, label, above(v))
    return text[r.top]


def branches(tree: Tree):
    """the edges of a tree in the order its newick text visits the node below them -- preorder from the internal node next to file 0,
    children by their smallest file, so the edge to file 0 comes first -- as (node below the edge, index of the edge in tree.edges, the
    files on the side away from the top node as a bit mask, length).  Branch k + 1 of --corebranches is entry k"""
    r = _Rooted(tree)
    index = {}
    for e, (u, v, _) in enumerate(tree.edges):
        index[(u, v)] = index[(v, u)] = e
    parent = {w: v for v, kids in r.children.items() for w in kids}
    out, stack = [], list(reversed(r.children[r.top]))
    while stack:
        v = stack.pop()
        out.append((v, index[(parent[v], v)], r.mask[v], r.length[v]))
        stack += reversed(r.children[v])
    return out


def tree_text(counts, K, model: str, names: Sequence[str]) -> str:
    """counts: (B + 1, files, files), slab 0 of all sites and one slab per replicate; K: the columns they were taken from, one number
    or one per pair of files (distances) -> the Newick text of slab 0's tree with the support of the B replicate trees"""
    B = len(counts) - 1
    main = neighbour_joining(distances(counts[0], K, model, names))
    reps = [neighbour_joining(distances(counts[r], K, model, names)) for r in range(1, B + 1)]
    return newick(main, names, support(main, reps) if B else None, B)


def split_tally(splits) -> Dict[int, int]:
    """the bipartitions of a set of trees, one row of masks per tree (bipartitions' convention: the side without file 0; a tree holds a
    bipartition once) -> bipartition -> the number of trees that hold it"""
    flat = np.asarray(splits).ravel()
    if not len(flat):
        return {}
    masks, held = np.unique(flat, return_counts=True)
    return {int(b): int(k) for b, k in zip(masks.tolist(), held.tolist())}


def _edge_lengths_of_records(records):
    """edge records of shape (trees, 2 n - 3), n <= 64 -> (n, per internal edge of every tree its bipartition as uint64 and its length,
    both of shape (trees, n - 3); the lengths of the leaf edges, (trees, n)).  Join s = 0 .. n - 4 of a tree is records 2 s and 2 s + 1, whose
    parent is node n + s: the leaves below a node are those below the two children of its join"""
    B, ne = records.shape
    n = (ne + 3) // 2
    child = records["child"].astype(np.int64)
    rows = np.arange(B)
    below = np.zeros((B, 2 * n - 2), dtype=np.uint64)
    below[:, :n] = np.uint64(1) << np.arange(n, dtype=np.uint64)
    for s in range(n - 3):
        below[:, n + s] = below[rows, child[:, 2 * s]] | below[rows, child[:, 2 * s + 1]]
    full = np.uint64((1 << n) - 1)
    side = np.take_along_axis(below, child, axis=1)
    side = np.where(side & np.uint64(1) != 0, full ^ side, side)                # the side without file 0
    order = np.argsort(child, axis=1, kind="stable")                            # the leaf edges by leaf, then the internal edges by node
    length = np.take_along_axis(records["length"], order, axis=1)
    return n, np.take_along_axis(side, order, axis=1)[:, n:], length[:, n:], length[:, :n]


def consensus(replicates, B: int):
    """The majority-rule consensus of B replicate trees: `replicates` is a sequence of B Trees or their edge records of shape
    (B, 2 n - 3) (EDGE_RECORD).  Its internal edges are the bipartitions that strictly more than half of the replicates hold
    (2 * count > B); they are pairwise compatible, so they nest by inclusion under a top node that carries file 0.  An edge is as long as
    the mean of its length in the replicates that hold it (a leaf edge: in all of them), the sum taken with math.fsum, which does not
    depend on the order of the replicates.  No such bipartition: the star.
    -> (the tree, {bipartition: the replicates that hold it} for its internal edges): what newick takes as tree and support"""
    import math
    if B < 1 or len(replicates) != B:
        raise ValueError("a consensus takes the %d replicate trees" % B if B >= 1 else "a consensus takes one replicate at least")
    held: Dict[int, list] = {}                          # a majority bipartition -> its lengths
    if isinstance(replicates, np.ndarray):
        n, masks, lengths, leaf_lengths = _edge_lengths_of_records(replicates)
        uniq, inverse, count = np.unique(masks.ravel(), return_inverse=True, return_counts=True)
        inverse = np.asarray(inverse).ravel()
        flat = lengths.ravel()
        for u in np.nonzero(2 * count > B)[0].tolist():
            held[int(uniq[u])] = flat[inverse == u].tolist()
        leaves = [leaf_lengths[:, f].tolist() for f in range(n)]
    else:
        n = replicates[0].n
        leaves = [[] for _ in range(n)]
        every: Dict[int, list] = {}
        for t in replicates:
            r = _Rooted(t)
            for v in r.internal:
                every.setdefault(r.mask[v], []).append(r.length[v])
            for f in range(n):
                leaves[f].append(r.length[f])
        held = {b: ls for b, ls in every.items() if 2 * len(ls) > B}
    inner = sorted(held, key=lambda b: (bin(b).count("1"), b))                  # a bipartition lies inside a later one or beside it
    node = {b: n + k for k, b in enumerate(inner)}
    top = n + len(inner)

    def parent(b: int, after: int) -> int:
        return next((node[c] for c in inner[after:] if b & c == b), top)
    edges = [(parent(1 << f, 0) if f else top, f, math.fsum(leaves[f]) / B) for f in range(n)]
    edges += [(parent(b, k + 1), node[b], math.fsum(held[b]) / len(held[b])) for k, b in enumerate(inner)]
    return Tree(n, edges), {b: len(held[b]) for b in inner}


def tree_files(counts, K, model: str, names: Sequence[str], nj=None, want: Sequence[str] = ("tree", "consensus", "boottrees"), keep: Optional[dict] = None):
    """counts, K, model, names: as for tree_text -> (the text of tree_text; the consensus of the B replicate trees as newick writes it
    with their support; B lines, the unlabelled newick of replicate 1 .. B), None for a text that `want` does not name, and for the
    consensus without replicates.  nj: a callable, matrices of shape (trees, files, files) -> (edge records (trees, 2 files - 3),
    bipartitions (trees, files - 3)) that joins like neighbour_joining, bit for bit (BlockFinder.nj_batch): it gets all B + 1 matrices
    in one call.  Without it, and above 64 files, every matrix goes through neighbour_joining here: the same texts, byte for byte.  The
    distances are made here either way, slab after slab, so Saturated and NoSharedColumn rise as they do from tree_text.  keep: a dict
    that receives the main tree as "tree" and, where "tree" is wanted and there are replicates, the support of its internal edges as
    "support" -- what a caller needs to map changes onto the branches of the text without a second neighbour joining"""
    B = len(counts) - 1
    D = np.stack([distances(counts[r], K, model, names) for r in range(B + 1)])
    n = D.shape[1]
    boot = B and "boottrees" in want
    if nj is not None and n <= NJ_BATCH_MAX_FILES:
        records, splits = nj(D)
        main = Tree.of_records(records[0])
        tally = split_tally(splits[1:]) if "tree" in want else {}
        reps = [Tree.of_records(records[r]) for r in range(1, B + 1)] if boot else records[1:]
    else:
        trees = [neighbour_joining(D[r]) for r in range(B + 1)]
        main, reps = trees[0], trees[1:]
        tally = split_tally(np.array([b for t in reps for b in bipartitions(t)], dtype=object)) if "tree" in want else {}
    held = {b: tally.get(b, 0) for b in bipartitions(main)} if B and "tree" in want else None
    if keep is not None:
        keep["tree"], keep["support"] = main, held
    text = newick(main, names, held, B) if "tree" in want else None
    majority = None
    if B and "consensus" in want:
        ctree, held = consensus(reps, B)
        majority = newick(ctree, names, held, B)
    lines = "".join(newick(t, names) for t in reps) if boot else None
    return text, majority, lines
