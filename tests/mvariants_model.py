"""A plain Python restatement of the variant segments of a multiple alignment (include/sibelia_amd.h), for the tests
(never used by the product).  Everything works on the rows of ONE aligned group: r byte strings of L columns, the centre first.

`classes(rows)`           -> one class per column: 0 equal, 1 unequal, 3 unequal and gapped.
`automaton(cls)`          -> the unequal segments [(s, e)] by the automaton parse_alignment runs over the columns (reference
                             src/csibelia/C-Sibelia.py:212-226), with "the two symbols match" read as "the column is equal".
`closed_form(cls)`        -> the same segments from the kept equal runs: a run is kept if it starts at column 0, ends at column L or has
                             at least 30 columns; a segment is a maximal stretch between kept runs.
`segments(rows)`          -> [(s, e, before, lead, gapped, [slice per row])] as sbl_group_variants defines them.
`records(rows, start, end, reverse)` -> [(POS, [allele per row])] for a centre instance [start, end) read on '-' if reverse.
"""
MINIMUM_CONTEXT_SIZE = 30
GAP = 45                                           # '-'
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def classes(rows):
    if len(rows) < 2:
        return [0] * (len(rows[0]) if rows else 0)
    out = []
    for col in zip(*rows):
        if all(x == col[0] for x in col):
            assert col[0] != GAP, "a column of gaps"
            out.append(0)
        else:
            out.append(3 if GAP in col else 1)
    return out


def automaton(cls):
    """State: the kind of the current run (`last`), where the current stretch started (`at`) and the list of stretches so far.  At
    every change of kind the stretch is closed -- unless it is an equal one that is short and does not start the alignment: then it is
    dropped, and so is the stretch before it, whose start the current one takes over."""
    last, at, found = None, None, []
    for now, c in enumerate(cls):
        equal = c == 0
        if last is None:
            last, at = equal, 0
        elif last != equal:
            if not last or now - at >= MINIMUM_CONTEXT_SIZE or at == 0:
                found.append((at, now, last))
                at = now
            elif found:
                at = found.pop()[0]
            last = equal
    if last is not None:
        found.append((at, len(cls), last))
    return [(s, e) for s, e, equal in found if not equal]


def closed_form(cls):
    L = len(cls)
    kept = []                                       # the kept equal runs
    c = 0
    while c < L:
        if cls[c]:
            c += 1
            continue
        e = c
        while e < L and not cls[e]:
            e += 1
        if c == 0 or e == L or e - c >= MINIMUM_CONTEXT_SIZE:
            kept.append((c, e))
        c = e
    out, at = [], 0
    for s, e in kept + [(L, L)]:
        if s > at:
            out.append((at, s))
        at = e
    return out


def segments(rows):
    cls = classes(rows)
    out = []
    for s, e in closed_form(cls):
        lead = 0 if s == 0 or (e - s == 1 and cls[s] == 1) else 1
        before = sum(1 for x in rows[0][:s] if x != GAP)
        out.append((s, e, before, lead, int(any(c == 3 for c in cls[s:e])), [bytes(r[s - lead:e]) for r in rows]))
    return out


def records(rows, start, end, reverse):
    first, step = (end, -1) if reverse else (start + 1, 1)
    out = []
    for s, e, before, lead, _, slices in segments(rows):
        alleles = [x.replace(b"-", b"") for x in slices]
        if reverse:
            alleles = [x.translate(_COMPLEMENT)[::-1] for x in alleles]
        out.append((first + step * before - lead, alleles))
    return out
