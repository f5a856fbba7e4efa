"""Fitch parsimony of the sites on a tree (include/sibelia_amd.h) restated in plain Python, for
tests/test_parsimony_model.py and the GPU tests of sbl_group_parsimony (never used by the product), with a small Newick reader and the
texts of --corebranches, --corebranchsites and --coresnptree rebuilt from files a run wrote.

`rooted(edges, n)`                      -> (top, parent, children, parent edge) of the tree read from leaf 0; Refused for what the library
                                           answers SBL_ERR_BAD_ARG, TooLarge for SBL_ERR_TOO_LARGE.
`fitch(S, present, edges)`              -> (counts [edge][from][to], steps, minsteps, changes [(site, edge, from, to)] by (site, edge)).
                                           S: rows of bytes, row f the class f (boot_model.site_matrix); present: rows of flags or None.
`site_steps(column, held, edges, root)` -> the steps of one site with the tree read from leaf `root` (0: the definition).
`brute_steps(column, held, edges)`      -> the fewest changes over all assignments of the internal nodes.
`read_newick(text)`                     -> (names, edges [(node, node, length text)], labels {node: text}) of a canonical --coretree text.
`branches_text`, `branch_sites_text`, `snp_tree_text` -> the three files from a SNP FASTA, a sites table and a Newick text.
"""
BASES = "ACTG"
MAX_LEAVES = 64


class Refused(ValueError):
    """what the library answers with SBL_ERR_BAD_ARG"""


class TooLarge(ValueError):
    """what the library answers with SBL_ERR_TOO_LARGE"""


def code(ch):
    return (ch >> 1) & 3


def rooted(edges, n):
    if n < 3:
        raise Refused("fewer than three leaves")
    if n > MAX_LEAVES:
        raise TooLarge("more than 64 leaves")
    if len(edges) != 2 * n - 3:
        raise Refused("not 2 n - 3 edges")
    nodes = 2 * n - 2
    adj = [[] for _ in range(nodes)]
    for e, edge in enumerate(edges):
        u, v = int(edge[0]), int(edge[1])
        if not (0 <= u < nodes and 0 <= v < nodes):
            raise Refused("a node that is not below 2 n - 2")
        adj[u].append((v, e))
        adj[v].append((u, e))
    for v in range(nodes):
        if len(adj[v]) != (1 if v < n else 3):
            raise Refused("node %d has %d edges" % (v, len(adj[v])))
    top = adj[0][0][0]
    if top < n:
        raise Refused("leaf 0 hangs on a leaf")
    parent, pedge, children = {top: 0}, {top: adj[0][0][1]}, {}
    seen, todo = {0, top}, [top]
    while todo:
        v = todo.pop()
        children[v] = []
        for w, e in adj[v]:
            if e == pedge[v]:
                continue
            if w in seen:
                raise Refused("a cycle")
            seen.add(w)
            parent[w], pedge[w] = v, e
            children[v].append(w)
            todo.append(w)
    if len(seen) != nodes:
        raise Refused("not connected")
    return top, parent, children, pedge


def _postorder(top, children, n):
    order, todo = [], [top]
    while todo:
        v = todo.pop()
        order.append(v)
        todo += [w for w in children[v] if w >= n]
    return order[::-1]                               # children before their parent, top last


def _lowest(s):
    return next(k for k in range(4) if s >> k & 1)


def _site(column, held, n, top, parent, children, pedge, post):
    """one site -> (steps, minsteps, {node: state}, {node: set})"""
    S = {f: (1 << code(column[f])) if held[f] else 0xF for f in range(n)}
    steps = 0
    for v in post:
        a, b = children[v]
        S[v] = S[a] & S[b]
        if not S[v]:
            S[v] = S[a] | S[b]
            steps += 1
    if not S[0] & S[top]:
        steps += 1
    state = {0: code(column[0]) if held[0] else _lowest(S[top])}
    for v in [top] + [w for u in post[::-1] for w in children[u]]:
        state[v] = state[parent[v]] if S[v] >> state[parent[v]] & 1 else _lowest(S[v])
    distinct = len({code(column[f]) for f in range(n) if held[f]})
    return steps, max(distinct - 1, 0), state, S


def fitch(S, present, edges):
    n = len(S)
    top, parent, children, pedge = rooted(edges, n)
    post = _postorder(top, children, n)
    C = len(S[0])
    counts = [[[0] * 4 for _ in range(4)] for _ in edges]
    steps, least, changes = [], [], []
    below = sorted((pedge[v], v) for v in parent)      # ascending edge index: the node below every edge
    for x in range(C):
        column = [S[f][x] for f in range(n)]
        held = [True] * n if present is None else [bool(present[f][x]) for f in range(n)]
        st, mn, state, _ = _site(column, held, n, top, parent, children, pedge, post)
        steps.append(st)
        least.append(mn)
        for e, v in below:
            a, b = state[parent[v]], state[v]
            if a != b:
                changes.append((x, e, a, b))
                counts[e][a][b] += 1
    return counts, steps, least, changes


def site_trace(column, held, edges):
    """one site -> ({node: set}, {node: state}, parent, top): what the predicates of tests/parsimony_cases.py look at"""
    n = len(column)
    top, parent, children, pedge = rooted(edges, n)
    _, _, state, S = _site(column, held, n, top, parent, children, pedge, _postorder(top, children, n))
    return S, state, parent, top


def reroot(edges, n, root):
    """the same tree with leaf `root` and leaf 0 exchanged, so that `rooted` reads it from `root`"""
    swap = {0: root, root: 0}
    return [(swap.get(int(e[0]), int(e[0])), swap.get(int(e[1]), int(e[1]))) for e in edges]


def site_steps(column, held, edges, root=0):
    n = len(column)
    swapped = reroot(edges, n, root)
    column, held = list(column), list(held)
    column[0], column[root] = column[root], column[0]
    held[0], held[root] = held[root], held[0]
    top, parent, children, pedge = rooted(swapped, n)
    return _site(column, held, n, top, parent, children, pedge, _postorder(top, children, n))[0]


def brute_steps(column, held, edges):
    """the fewest edges with two different states over all 4^(n - 2) assignments of the internal nodes; an absent leaf is free: it
    costs nothing on its edge"""
    n = len(column)
    best = None
    pairs = [(int(e[0]), int(e[1])) for e in edges]
    for k in range(4 ** (n - 2)):
        state = {n + i: (k >> (2 * i)) & 3 for i in range(n - 2)}
        cost = 0
        for u, v in pairs:
            a = state[u] if u >= n else (code(column[u]) if held[u] else None)
            b = state[v] if v >= n else (code(column[v]) if held[v] else None)
            cost += a is not None and b is not None and a != b
        best = cost if best is None else min(best, cost)
    return best


# ------------------------------------------------------------------------------------------ Newick and the three texts

def read_newick(text):
    """the canonical one-line text of --coretree -> (names of the leaves in the order met, edges (parent, child, length text) with the
    leaves numbered in that order and the internal nodes behind them in the order they close, labels {internal node: its label text})"""
    assert text.endswith(";\n") and text.count("\n") == 1
    names, inner, stack, edges, labels = [], [], [], [], {}
    at, last = 0, None
    body = text[:-2]

    def token(stop):
        nonlocal at
        start = at
        while at < len(body) and body[at] not in stop:
            at += 1
        return body[start:at]
    while at < len(body):
        ch = body[at]
        if ch == "(":
            stack.append([])
            at += 1
        elif ch == ",":
            at += 1
        elif ch == ")":
            at += 1
            kids = stack.pop()
            node = ("inner", len(inner))
            inner.append(kids)
            label = token(":,)")
            if label:
                labels[node] = label
            last = node
            if at < len(body) and body[at] == ":":
                at += 1
                length = token(",)")
                stack[-1].append((node, length))
        else:
            name = token(":")
            at += 1
            length = token(",)")
            node = ("leaf", len(names))
            names.append(name)
            stack[-1].append((node, length))
    assert not stack and last is not None
    n = len(names)
    number = lambda node: node[1] if node[0] == "leaf" else n + node[1]      # noqa: E731
    for k, kids in enumerate(inner):
        edges += [(n + k, number(node), length) for node, length in kids]
    return names, edges, {number(v): t for v, t in labels.items()}


def fasta_rows(text, names):
    rows, name = {}, None
    for line in text.decode("latin1").split("\n"):
        if line.startswith(">"):
            name = line[1:]
            rows[name] = []
        elif line:
            rows[name].append(line)
    return ["".join(rows[a]).encode("latin1") for a in names]


def _preorder(names, edges):
    """the edges of read_newick in the order the text visits the node below them -> [(node, edge index, leaves below, length text)]"""
    n = len(names)
    kids = {}
    for e, (u, v, length) in enumerate(edges):
        kids.setdefault(u, []).append((v, e, length))
    top = 2 * n - 3                                   # the node that closes last

    def leaves(v):
        return [v] if v < n else [f for w, _, _ in kids[v] for f in leaves(w)]
    out, todo = [], list(reversed(kids[top]))
    while todo:
        v, e, length = todo.pop()
        out.append((v, e, sorted(leaves(v)), length))
        if v >= n:
            todo += reversed(kids[v])
    return out


def _ci(M, S):
    if S == 0:
        return "nan"
    v = (M * 10 ** 6 + S // 2) // S
    return "%d.%06d" % (v // 10 ** 6, v % 10 ** 6)


def _header(comments, steps, least):
    S, M = sum(steps), sum(least)
    return list(comments) + ["# sites=%d steps=%d minsteps=%d homoplasic=%d ci=%s" % (len(steps), S, M, sum(a > b for a, b in zip(steps, least)), _ci(M, S))]


def mapped(snps, newick_text, file_names):
    """the SNP FASTA (gaps: absent) and the Newick text of one run, the files in input order -> (names and edges of read_newick with the
    leaves renumbered to the input order, the preorder of the branches, what fitch makes of them)"""
    names, edges, labels = read_newick(newick_text.decode("latin1"))
    where = [file_names.index(a) for a in names]     # leaf of the text -> file
    n = len(names)
    as_file = lambda v: where[v] if v < n else v      # noqa: E731
    rows = fasta_rows(snps, file_names)
    present = [[ch != 0x2D for ch in r] for r in rows]
    order = [(as_file(v), e, sorted(where[f] for f in below), length) for v, e, below, length in _preorder(names, edges)]
    result = fitch(rows, present, [(as_file(u), as_file(v)) for u, v, _ in edges])
    return order, labels, result


def branches_text(snps, newick_text, file_names, comments=()):
    order, labels, (counts, steps, least, _) = mapped(snps, newick_text, file_names)
    n = len(file_names)
    out = _header(comments, steps, least) + ["branch\tfiles\tlength\tsupport\tchanges\ttransitions\ttransversions"]
    for k, (v, e, below, length) in enumerate(order):
        c = counts[e]
        total = sum(sum(r) for r in c)
        ts = c[0][3] + c[3][0] + c[1][2] + c[2][1]
        out.append("\t".join([str(k + 1), ",".join(file_names[f] for f in below), length, labels.get(v, ".") if v >= n else ".", str(total), str(ts), str(total - ts)]))
    return ("\n".join(out) + "\n").encode("latin1")


def branch_sites_text(snps, newick_text, sites_table, file_names):
    order, _, (_, steps, least, changes) = mapped(snps, newick_text, file_names)
    lines = sites_table.decode("latin1").split("\n")[:-1]
    comments = [x for x in lines if x.startswith("#")]
    rows = lines[len(comments) + 1:]
    assert lines[len(comments)] == "column\tblock\trecord\tposition\tstrand" and len(rows) == len(steps)
    number = {e: k + 1 for k, (_, e, _, _) in enumerate(order)}
    out = _header(comments, steps, least) + [lines[len(comments)] + "\tbranch\tfrom\tto\tsteps\tminsteps"]
    for x, b, a, c in sorted((x, number[e], a, c) for x, e, a, c in changes):
        out.append("%s\t%d\t%s\t%s\t%d\t%d" % (rows[x], b, BASES[a], BASES[c], steps[x], least[x]))
    return ("\n".join(out) + "\n").encode("latin1"), comments


def write_newick(names, edges, labels, length_of):
    """the text read_newick read, with length_of(node, edge index, length text) as the length above every node"""
    n = len(names)
    kids = {}
    for e, (u, v, length) in enumerate(edges):
        kids.setdefault(u, []).append((v, e, length))

    def text(v):
        return names[v] if v < n else "(" + ",".join("%s:%s" % (text(w), length_of(w, e, length)) for w, e, length in kids[v]) + ")" + labels.get(v, "")
    return text(2 * n - 3) + ";\n"


def snp_tree_text(snps, newick_text, file_names):
    """the Newick text with every length replaced by the changes of its branch"""
    _, _, (counts, _, _, _) = mapped(snps, newick_text, file_names)
    names, edges, labels = read_newick(newick_text.decode("latin1"))
    return write_newick(names, edges, labels, lambda v, e, length: "%d" % sum(sum(r) for r in counts[e])).encode("latin1")
