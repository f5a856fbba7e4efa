"""The arithmetic of sbl_nj_batch (csrc/tree_nj.hip) restated in plain Python floats, one operation per line of the
rules: what the kernel computes and, bit for bit, what sibelia_amd.tree.neighbour_joining computes through numpy.  No numpy in here: a
Python float is an IEEE double and every +, -, * and / on it rounds once, so nothing is fused and no order is left to a library."""


def row_sum(a):
    """numpy's sum of one row of m <= 128 doubles: from 0.0 left to right below 8 entries; from 8 on eight partial sums over the whole
    blocks of 8, folded in pairs, the m % 8 tail entries added left to right, and that added to the 0.0 the reduction starts from"""
    m = len(a)
    if m < 8:
        s = 0.0
        for x in a:
            s = s + x
        return s
    r = [a[k] for k in range(8)]
    i = 8
    while i < m - m % 8:
        for k in range(8):
            r[k] = r[k] + a[i + k]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(m - m % 8, m):
        s = s + a[k]
    return 0.0 + s


def neighbour_joining(D):
    """D: n x n floats, symmetric with a zero diagonal, n >= 3 -> (edges in the order of Tree.edges, splits: per join s the leaves below
    node n + s as a bit mask, complemented within n bits where it holds file 0)"""
    n = len(D)
    D = [[float(x) for x in row] for row in D]
    full = (1 << n) - 1
    live = list(range(n))                               # the rows that are left, in compacted order
    ids = list(range(n))                                # the node a row stands for
    mask = [1 << f for f in range(n)]                   # the leaves below that node
    edges, splits = [], []
    for s in range(n - 3):
        m = len(live)
        r = [row_sum([D[p][q] for q in live]) for p in live]
        best, bi, bj = None, 0, 1
        for i in range(m):
            for j in range(i + 1, m):
                q = (float(m - 2) * D[live[i]][live[j]] - r[i]) - r[j]
                if best is None or q < best:            # the first of the smallest, row-major
                    best, bi, bj = q, i, j
        pi, pj = live[bi], live[bj]
        dij = D[pi][pj]
        li = dij / 2.0 + (r[bi] - r[bj]) / float(2 * (m - 2))
        lj = dij - li
        if li < 0:
            li, lj = 0.0, dij
        elif lj < 0:
            li, lj = dij, 0.0
        edges += [(n + s, ids[pi], li), (n + s, ids[pj], lj)]
        row = [((D[pi][q] + D[pj][q]) - dij) / 2.0 for q in range(n)]
        for q in live:
            D[pi][q] = row[q]
            D[q][pi] = row[q]
        D[pi][pi] = 0.0
        ids[pi] = n + s
        mask[pi] |= mask[pj]
        splits.append(full ^ mask[pi] if mask[pi] & 1 else mask[pi])
        del live[bj]
    a, b, c = live
    top = n + (n - 3)
    for p, x in ((a, ((D[a][b] + D[a][c]) - D[b][c]) / 2.0), (b, ((D[a][b] + D[b][c]) - D[a][c]) / 2.0), (c, ((D[a][c] + D[b][c]) - D[a][b]) / 2.0)):
        edges.append((top, ids[p], x if x > 0 else 0.0))
    return edges, splits
