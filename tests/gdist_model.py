"""The pairwise counts of a multiple alignment and their fold into a class matrix (include/sibelia_amd.h), restated in
numpy on top of msa_model.msa for tests/test_gdist_model.py and the GPU tests of sbl_group_distances.

Counts of the ordered row pair (i, j): (match, mismatch, ambiguous, gap(i -> j)); gap(j -> i) is the fourth count of (j, i)."""
import numpy as np

import msa_model as MM

FIELDS = ("match", "mismatch", "ambiguous", "gap")
_BASE = np.zeros(256, dtype=bool)
_BASE[list(b"ACGT")] = True


def row_pair_counts(x: bytes, y: bytes):
    """(match, mismatch, ambiguous, gap(x -> y)) of two rows of one alignment"""
    a, b = np.frombuffer(x, dtype=np.uint8), np.frombuffer(y, dtype=np.uint8)
    assert len(a) == len(b)
    ga, gb = a == ord("-"), b == ord("-")
    both = _BASE[a] & _BASE[b]
    return (int((both & (a == b)).sum()), int((both & (a != b)).sum()), int((~ga & ~gb & ~both).sum()), int((~ga & gb).sum()))


def rows_counts(rows):
    """counts[i, j] of every ordered pair of the rows of one group (the diagonal stays zero)"""
    r = len(rows)
    out = np.zeros((r, r, 4), dtype=np.uint64)
    for i in range(r):
        for j in range(r):
            if i != j:
                out[i, j] = row_pair_counts(rows[i], rows[j])
    return out


def group_counts(group):
    """... of a group of strings, centre first, through the model's alignment"""
    return rows_counts(MM.msa(group)[0])


def fold(per_group, classes, nclass):
    """M[nclass][nclass]: per_group is a list of counts[r, r, 4] (None: a group that gives nothing), classes the class of every
    instance, flat, in group order -- those of a group that gives nothing included"""
    M = np.zeros((nclass, nclass, 4), dtype=np.uint64)
    at = 0
    for counts in per_group:
        r = counts if isinstance(counts, int) else len(counts)
        if not isinstance(counts, int):
            for i in range(r):
                for j in range(r):
                    if i != j:
                        M[classes[at + i], classes[at + j]] += counts[i, j]
        at += r
    return M


def skipped(r: int) -> int:
    """what fold takes for a group of r instances that gives nothing (skipped, not wanted)"""
    return int(r)
