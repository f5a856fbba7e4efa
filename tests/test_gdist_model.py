"""tests/gdist_model.py, the restatement of the pairwise counts (include/sibelia_amd.h) the GPU tests compare against:
matrices counted by hand, the row-length identity and the symmetry on crafted and random groups, and the fold into classes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gdist_cases as DC                           # noqa: E402
import gdist_model as DM                           # noqa: E402
import msa_cases as MC                             # noqa: E402
import msa_model as MM                             # noqa: E402


def test_three_tiny_groups_counted_by_hand():
    # rows ACGT / ACTT: three matches, one mismatch, both ways
    got = DM.rows_counts([b"ACGT", b"ACTT"])
    assert got.tolist() == [[[0, 0, 0, 0], [3, 1, 0, 0]], [[3, 1, 0, 0], [0, 0, 0, 0]]]
    # rows AC-GT / ACNG- / -CAGT:
    #   0/1: A=A C=C -/N G=G T/-  -> match 3, gap(0->1) 1 (T), gap(1->0) 1 (N)
    #   0/2: A/- C=C -/A G=G T=T  -> match 3, gap(0->2) 1 (A), gap(2->0) 1 (A)
    #   1/2: A/- C=C N/A G=G -/T  -> match 2, ambiguous 1, gap(1->2) 1, gap(2->1) 1
    got = DM.rows_counts([b"AC-GT", b"ACNG-", b"-CAGT"])
    assert got.tolist() == [[[0, 0, 0, 0], [3, 0, 0, 1], [3, 0, 0, 1]],
                            [[3, 0, 0, 1], [0, 0, 0, 0], [2, 0, 1, 1]],
                            [[3, 0, 0, 1], [2, 0, 1, 1], [0, 0, 0, 0]]]
    # through the alignment: the member lacks the centre's last two bases and differs in one; a is lower case
    rows, _ = MM.msa([b"ACGTACGT", b"ACGaAC"])
    assert rows == [b"ACGTACGT", b"ACGaAC--"]
    assert DM.group_counts([b"ACGTACGT", b"ACGaAC"]).tolist() == [[[0, 0, 0, 0], [5, 0, 1, 2]], [[5, 0, 1, 0], [0, 0, 0, 0]]]


def check_identity_and_symmetry(group):
    counts = DM.group_counts(group)
    for i, s in enumerate(group):
        for j in range(len(group)):
            if i != j:
                assert int(counts[i, j].sum()) == len(s), (group, i, j)
                assert counts[i, j, :3].tolist() == counts[j, i, :3].tolist(), (group, i, j)


def test_row_length_identity_and_symmetry_on_crafted_groups():
    assert len(DC.CRAFTED) == 13
    for name in sorted(DC.CRAFTED):
        check_identity_and_symmetry(DC.CRAFTED[name])


def test_row_length_identity_and_symmetry_on_random_groups():
    for g in MC.random_groups(seed=81, count=200, rmin=2, rmax=5, max_len=60, max_indel=6):
        check_identity_and_symmetry(g)


def test_crafted_groups_hold_the_cases_they_are_named_for():
    c = DM.group_counts(DC.NEW["members_differ_where_centre_agrees_with_neither"])
    assert c[1, 2].tolist() == [11, 1, 0, 0] and c[0, 1].tolist() == [11, 1, 0, 0] and c[0, 2].tolist() == [11, 1, 0, 0]
    c = DM.group_counts(DC.NEW["codes_other_than_acgt"])
    assert [c[0, k, 2] for k in (1, 2, 3)] == [1, 1, 1] and [c[a, b, 2] for a, b in ((1, 2), (1, 3), (2, 3))] == [1, 1, 1]
    assert c[1, 4].tolist() == [16, 0, 0, 1] and c[4, 1].tolist() == [16, 0, 0, 0]      # N opposite the gap: a gap column, not an ambiguous one
    c = DM.group_counts(DC.NEW["three_and_one_in_one_slot"])
    assert c[1, 2].tolist() == [13, 0, 0, 2] and c[2, 1, 3] == 0 and c[0, 1, 3] == 0 and c[1, 0, 3] == 3
    c = DM.group_counts(DC.NEW["identical_instances"])
    assert all(c[i, j].tolist() == [12, 0, 0, 0] for i in range(4) for j in range(4) if i != j)
    c = DM.group_counts(DC.NEW["centre_of_length_0"])
    assert c[0].sum() == 0 and c[1, 0].tolist() == [0, 0, 0, 6] and c[1, 3].tolist() == [5, 1, 0, 0]


def test_fold():
    groups = [DC.NEW["three_and_one_in_one_slot"], DC.NEW["codes_other_than_acgt"]]
    per = [DM.group_counts(g) for g in groups]
    # one class: the diagonal cell holds every unordered pair twice
    M = DM.fold(per, [0] * 9, 1)
    once = sum(int(c[i, j, 0]) for c in per for i in range(len(c)) for j in range(i + 1, len(c)))
    assert M[0, 0, 0] == 2 * once and all(int(v) % 2 == 0 for v in M[0, 0, :3])
    assert M[0, 0, 3] == sum(int(c[i, j, 3]) for c in per for i in range(len(c)) for j in range(len(c)))
    # classes permuted: the matrix permuted
    cls = [0, 1, 2, 3, 3, 2, 1, 0, 4]
    perm = [3, 0, 4, 1, 2]
    A, B = DM.fold(per, cls, 5), DM.fold(per, [perm[x] for x in cls], 5)
    for f in range(5):
        for g in range(5):
            assert A[f, g].tolist() == B[perm[f], perm[g]].tolist()
    assert A[:, :, :3].tolist() == A.transpose(1, 0, 2)[:, :, :3].tolist()
    # a group that gives nothing keeps its place in the classes
    C = DM.fold([DM.skipped(4), per[1]], cls, 5)
    assert C.tolist() == DM.fold([per[1]], cls[4:], 5).tolist()
