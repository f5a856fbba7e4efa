"""Groups for the tests of the pairwise counts, shared by tests/test_gdist_model.py and tests/test_gpu_group_distances.py:
the eight of msa_cases.CRAFTED and five of their own.  A group is a list of byte strings, centre first."""
import msa_cases as MC

NEW = {
    # column 4: the centre holds A, the members C and G -- a mismatch between two members where the centre agrees with neither
    "members_differ_where_centre_agrees_with_neither": [b"ACGTACGTACGT", b"ACGTCCGTACGT", b"ACGTGCGTACGT"],
    # N, R and a lower-case base opposite a base (rows 0/1, 0/2, 0/3), opposite each other (1/2, 1/3, 2/3) and opposite a gap (row 4 lacks the column)
    "codes_other_than_acgt": [b"ACGTACGTACGTACGTA", b"ACGTACGNACGTACGTA", b"ACGTACGRACGTACGTA", b"ACGTACGtACGTACGTA", b"ACGTACGACGTACGTA"],
    # slot 6: one member inserts GGG, another G -- inside the slot the second holds a gap opposite the first's bases, and both a base opposite the centre's gap
    "three_and_one_in_one_slot": [b"AAAAAACCCCCC", b"AAAAAAGGGCCCCCC", b"AAAAAAGCCCCCC", b"AAAAAACCCCCC"],
    "identical_instances": [b"ACGTTGCATGCA"] * 4,
    "centre_of_length_0": [b"", b"ACGTAC", b"ACG", b"ACTTAC"],
}

CRAFTED = {name: group for name, (group, _) in MC.CRAFTED.items()}
CRAFTED.update(NEW)


def indel_group(rng, r, n=40):
    """r instances of about n bases: copies of one record with substitutions, an N and a few one- and two-base indels"""
    c = MC.rand(rng, n)
    out = [c]
    for _ in range(r - 1):
        b = bytearray(c)
        for _ in range(int(rng.integers(0, 3))):
            b[int(rng.integers(0, len(b)))] = MC.rand(rng, 1)[0]
        if rng.random() < 0.3:
            b[int(rng.integers(0, len(b)))] = ord("N")
        u = rng.random()
        at = int(rng.integers(1, len(b) - 3))
        if u < 0.15:
            del b[at:at + int(rng.integers(1, 3))]
        elif u < 0.3:
            b[at:at] = MC.rand(rng, int(rng.integers(1, 3)))
        out.append(bytes(b))
    return out
