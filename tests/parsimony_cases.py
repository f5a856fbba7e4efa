"""Crafted trees and sites for sbl_group_parsimony (include/sibelia_amd.h): the word edges of the packed sites (32 files
in a word), the two tree shapes, leaf 0 next to the first-made and the last-made internal node, permuted numbering, the ties and the
absent leaves -- each with a predicate on tests/parsimony_model.py's output that proves the case is what its name says.

A case: n, edges [(node, node)], columns (one string of n letters per site, '-' where the file is absent: the sites of a partial call),
partial, device (False: not a site any call of the library can have, the model alone is asked), hits(case) -> bool.
`groups_of(case)` lays the columns out as the groups of tests/test_gpu_group_bootstrap.py: equal-length rows, substitutions only."""
import numpy as np

import parsimony_model as PM

SPACING = 8
SITE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
LEAF_COUNTS = (3, 4, 5, 32, 33, 64)


def joined(n, pick):
    """a tree as neighbour joining numbers it: pick(live nodes, step) -> the positions of the two to join; node n + s is made by join s,
    the last three hang from node 2 n - 3"""
    live, edges = list(range(n)), []
    for s in range(n - 3):
        i, j = sorted(pick(live, s))
        edges += [(n + s, live[i]), (n + s, live[j])]
        live[i] = n + s
        del live[j]
    return edges + [(2 * n - 3, v) for v in live]


def caterpillar(n, first=True):
    """first: leaves 0 and 1 are joined first and the chain grows through 2, 3, ..: leaf 0 is next to the first-made internal node;
    else the chain grows from the last leaves down and leaf 0 hangs from the last-made node"""
    if first:
        return joined(n, lambda live, s: (0, 1))
    return joined(n, lambda live, s: (len(live) - 2, len(live) - 1))


def balanced(n):
    """neighbours are joined round after round: a tree as deep as log2 n"""
    state = {"at": 0}

    def pick(live, s):
        if state["at"] + 1 >= len(live):
            state["at"] = 0
        i = state["at"]
        state["at"] += 1
        return i, i + 1
    return joined(n, pick)


def permuted(edges, n, seed):
    """the same tree with its internal nodes renumbered, its edges in another order and some turned round"""
    rng = np.random.default_rng(seed)
    inner = [int(x) for x in rng.permutation(n - 2)]
    name = lambda v: v if v < n else n + inner[v - n]      # noqa: E731
    out = [(name(u), name(v)) if rng.integers(2) else (name(v), name(u)) for u, v in edges]
    return [out[int(k)] for k in rng.permutation(len(out))]


def variable_columns(rng, n, C, absent=0.0):
    """C columns of n letters, each with two different letters at least among the files that are there (two of them at least)"""
    out = []
    while len(out) < C:
        col = [b"ACGT"[int(x)] for x in rng.integers(0, 4, n)]
        if rng.integers(3) == 0:                       # most files agree: few steps
            col = [col[0]] * n
            for f in rng.choice(n, int(rng.integers(1, 3)), replace=False):
                col[int(f)] = b"ACGT"[int(rng.integers(0, 4))]
        gone = [absent > 0 and rng.random() < absent for _ in range(n)]
        there = [c for c, g in zip(col, gone) if not g]
        if len(set(there)) >= 2:
            out.append("".join("-" if g else chr(c) for c, g in zip(col, gone)))
    return out


def rows_of(columns, n):
    """-> (S: n rows of bytes, present: n rows of flags)"""
    return ([bytes(ord(col[f]) for col in columns) for f in range(n)], [[col[f] != "-" for col in columns] for f in range(n)])


def model(case):
    S, present = rows_of(case["columns"], case["n"])
    if not case["columns"]:
        S, present = [b""] * case["n"], [[]] * case["n"]
    return PM.fitch(S, present if case["partial"] else None, case["edges"])


def traces(case):
    for col in case["columns"]:
        yield col, PM.site_trace([ord(c) for c in col], [c != "-" for c in col], case["edges"])


def case(n, edges, columns, hits, partial=False, device=True):
    assert all(len(c) == n for c in columns) and (partial or not any("-" in c for c in columns))
    return dict(n=n, edges=list(edges), columns=list(columns), partial=partial, device=device, hits=hits)


def _bits(s):
    return bin(s).count("1")


def _steps_take_both_paths(c):
    """sites with as many steps as their bases need and homoplasic ones; the star of three files has none of the latter"""
    _, steps, least, _ = model(c)
    return any(a == b for a, b in zip(steps, least)) and (c["n"] == 3 or any(a > b for a, b in zip(steps, least)))


def _all_differ(c):
    return model(c)[2] == [3] * len(c["columns"])


def _tie_by_lowest_code(c):
    """an internal node with two or more bases to choose from, none of them its parent's"""
    return any(v >= c["n"] and _bits(S[v]) >= 2 and not S[v] >> state[parent[v]] & 1 for _, (S, state, parent, top) in traces(c) for v in parent)


def _top_excludes_file_0(c):
    return all(not S[0] & S[top] for _, (S, state, parent, top) in traces(c))


def _absent_leaf_carries_no_change(c):
    counts, _, _, changes = model(c)
    top, parent, children, pedge = PM.rooted(c["edges"], c["n"])
    gone = {(x, pedge[f]) for x, col in enumerate(c["columns"]) for f in range(1, c["n"]) if col[f] == "-"}
    return bool(gone) and not any((x, e) in gone for x, e, _, _ in changes) and len(changes) > 0


def _absent_subtree(c):
    """an internal node all of whose leaves are absent: its set is 0xF and nothing below it changes"""
    return any(v >= c["n"] and v != top and S[v] == 0xF for _, (S, state, parent, top) in traces(c) for v in parent) and _absent_leaf_carries_no_change(c)


def _top_children_absent(c):
    top, parent, children, pedge = PM.rooted(c["edges"], c["n"])
    return all(all(S[w] == 0xF for w in children[top]) for _, (S, state, parent, top) in traces(c)) and model(c)[1] == [0] * len(c["columns"])


def _leaf_0_absent(c):
    return all(col[0] == "-" and state[0] == state[top] for col, (S, state, parent, top) in traces(c)) and sum(model(c)[1]) > 0


def _unordered(edges):
    return sorted(tuple(sorted(e)) for e in edges)


_RNG = np.random.default_rng(1404)
_T4 = joined(4, lambda live, s: (0, 1))               # [(4, 0), (4, 1), (5, 4), (5, 2), (5, 3)]: top is node 4
_T5 = caterpillar(5)                                  # ((0, 1), 2), 3, 4: top is node 5

CASES = {
    # the star of three files; file 0 holds a base that neither of the others does: two steps, one on its own edge
    "star_top_excludes_file_0": case(3, [(3, 0), (3, 1), (3, 2)], ["ACG", "TCA", "GAT"], _top_excludes_file_0),
    # files 2 and 3 differ from each other and from 0 and 1: node 5 chooses between C and T without its parent's A, and takes C
    "tie_lowest_code": case(4, _T4, ["AACT", "AATC", "GGTC"], _tie_by_lowest_code),
    "all_leaves_differ": case(4, _T4, ["ACGT", "TGCA", "CATG"], _all_differ),
    "all_bases_in_64_files": case(64, balanced(64), ["ACGT" * 16, "TTGGCCAA" * 8], _all_differ),
    "one_absent_leaf": case(5, _T5, ["AC-CA", "AC-AG", "GT-TC"], _absent_leaf_carries_no_change, partial=True),
    "absent_subtree": case(5, _T5, ["ACG--", "AAC--", "CAT--"], _absent_subtree, partial=True),
    "top_children_absent": case(3, [(3, 0), (3, 1), (3, 2)], ["A--", "G--"], _top_children_absent, partial=True, device=False),
    "leaf_0_absent": case(5, _T5, ["-ACCA", "-CAGT", "-TTGG"], _leaf_0_absent, partial=True),
}
for _n in LEAF_COUNTS:
    CASES["caterpillar_%d_leaf_0_at_first_node" % _n] = case(_n, caterpillar(_n), variable_columns(_RNG, _n, 24), _steps_take_both_paths)
    CASES["caterpillar_%d_leaf_0_at_last_node" % _n] = case(_n, caterpillar(_n, first=False), variable_columns(_RNG, _n, 24), _steps_take_both_paths)
    CASES["balanced_%d" % _n] = case(_n, balanced(_n), variable_columns(_RNG, _n, 24), _steps_take_both_paths)
    CASES["permuted_%d" % _n] = case(_n, permuted(balanced(_n), _n, _n), variable_columns(_RNG, _n, 24),
                                     lambda c: c["edges"] != balanced(c["n"]) and (c["n"] == 3 or _unordered(c["edges"]) != _unordered(balanced(c["n"]))))
    CASES["partial_%d" % _n] = case(_n, permuted(caterpillar(_n), _n, 100 + _n), sorted(variable_columns(_RNG, _n, 12, 0.3), key=lambda col: [ch == "-" for ch in col]),
                                    lambda c: any("-" in col for col in c["columns"]), partial=True)
for _c in SITE_COUNTS:
    CASES["sites_%d" % _c] = case(4, _T4, variable_columns(_RNG, 4, _c), lambda c: True)


def groups_of(c, rng=None):
    """-> (groups, cls): one group per run of columns with the same files, its rows the files that are there in ascending order; a site
    stands every SPACING columns in a background all rows share, so the rows align without a gap.  No column: one group of equal rows"""
    rng = rng or np.random.default_rng(len(c["columns"]) + c["n"])
    runs = []
    for col in c["columns"]:
        there = tuple(f for f in range(c["n"]) if col[f] != "-")
        if not runs or runs[-1][0] != there:
            runs.append((there, []))
        runs[-1][1].append(col)
    if not runs:
        runs = [(tuple(range(c["n"])), [])]
    groups, cls = [], []
    for there, cols in runs:
        back = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), SPACING * (len(cols) + 2) + 4))
        rows = []
        for f in there:
            r = bytearray(back)
            for k, col in enumerate(cols):
                r[SPACING * (k + 1)] = ord(col[f])
            rows.append(bytes(r))
        groups.append(rows)
        cls += list(there)
    return groups, cls
