"""The concatenation of the multiple alignments (include/sibelia_amd.h) restated in plain Python / numpy on the rows of
msa_model.msa, for tests/test_concat_model.py and the GPU tests of sbl_group_concat (never used by the product).

A call is a list of groups, each given by its ROWS (a list of r byte strings of L columns, centre first) or by an int r: a group of r
instances that was skipped.  `cls` gives every instance of every group -- the skipped ones included -- a class, flat, in group order.

`used(groups, want)`                                   -> the indices of the used groups: wanted, aligned, L > 0.
`concat(groups, cls, nclass, headers, width, mode, want)` -> (text, parts, sites) as sbl_group_concat returns them; Refused where it
                                                          returns SBL_ERR_BAD_ARG.
"""
import numpy as np

import msa_model as MM

ALL, VARIABLE = 0, 1
MAX_CLASS = 1024
_BASE = np.zeros(256, dtype=bool)
_BASE[list(b"ACGT")] = True


class Refused(ValueError):
    """what the library answers with SBL_ERR_BAD_ARG"""


def ninst(group) -> int:
    return group if isinstance(group, int) else len(group)


def used(groups, want=None):
    return [g for g, rows in enumerate(groups) if not isinstance(rows, int) and len(rows[0]) > 0 and (want is None or want[g])]


def kept_columns(rows, mode):
    """the columns of one used group that the mode keeps, ascending"""
    L = len(rows[0])
    if mode == ALL:
        return list(range(L))
    a = np.array([np.frombuffer(r, dtype=np.uint8) for r in rows]).reshape(len(rows), L)
    keep = _BASE[a].all(axis=0) & (a != a[0]).any(axis=0)
    return [int(x) for x in np.nonzero(keep)[0]]


def wrap(row: bytes, width: int) -> bytes:
    """st_text_len's rule: a line feed after every `width` bytes and one after the last; nothing for an empty row"""
    return b"".join(row[i:i + width] + b"\n" for i in range(0, len(row), width))


def concat(groups, cls, nclass, headers, width, mode, want=None):
    total = sum(ninst(g) for g in groups)
    if mode not in (ALL, VARIABLE) or not 1 <= width <= 2 ** 32 - 1 or not 1 <= nclass <= MAX_CLASS:
        raise Refused("mode, width or number of classes")
    if headers is None or len(headers) != nclass or (cls is None and total):
        raise Refused("headers or classes missing")
    if any(not 0 <= x < nclass for x in (cls or [])):
        raise Refused("a class is not below the number of classes")
    first = [0]
    for g in groups:
        first.append(first[-1] + ninst(g))
    out_rows = [bytearray() for _ in range(nclass)]
    parts, sites = [], []
    for g in used(groups, want):
        rows = groups[g]
        classes = cls[first[g]:first[g + 1]]
        if sorted(classes) != list(range(nclass)):
            raise Refused("group %d does not hold every class exactly once" % g)
        cols = kept_columns(rows, mode)
        parts.append((g, len(out_rows[0]), len(cols)))
        for i, f in enumerate(classes):
            out_rows[f] += bytes(rows[i][x] for x in cols)
        if mode == VARIABLE:
            centre = rows[0]
            sites += [(g, x, x - centre[:x].count(b"-")) for x in cols]
    text = b"".join(bytes(h) + wrap(bytes(r), width) for h, r in zip(headers, out_rows))
    return text, parts, sites


def rows_of(groups_of_strings, skipped=()):
    """the rows of groups of strings (centre first) through the model's alignment; an index in `skipped` becomes its instance count"""
    return [len(g) if k in skipped else MM.msa(g)[0] for k, g in enumerate(groups_of_strings)]


def split_fasta(text: bytes, headers):
    """the rows of a text of `concat` without their line feeds; every header is one line that starts with '>' (no row holds that byte)"""
    assert text.endswith(b"\n") or not text
    out, seen = [], []
    for line in text.split(b"\n")[:-1]:
        if line.startswith(b">"):
            seen.append(line + b"\n")
            out.append(bytearray())
        else:
            out[-1] += line
    assert seen == [bytes(h) for h in headers]
    return [bytes(r) for r in out]
