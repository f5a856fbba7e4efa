"""Crafted calls for the tests of the concatenated alignment, shared by tests/test_concat_model.py and
tests/test_gpu_group_concat.py.  A case: groups (lists of byte strings, centre first), cls (flat, one class per instance), nclass,
headers (one per class), width, want (None: all) and refused (the call is SBL_ERR_BAD_ARG).  What each case is for stands next to it;
tests/test_concat_model.py checks that it does what it says."""


def case(groups, cls, nclass, headers=None, width=80, want=None, refused=False):
    if headers is None:
        headers = [b">s%d\n" % f for f in range(nclass)]
    return dict(groups=[[bytes(s) for s in g] for g in groups], cls=list(cls), nclass=nclass, headers=list(headers), width=width, want=want, refused=refused)


def identity_classes(groups):
    return [i for g in groups for i in range(len(g))]


# 32 columns, three rows.  Row 1: column 0 and column 31 differ (first and last column variable), column 5 holds N, column 9 a lower-case
# base other than the centre's, column 12 a third base, column 17 another base.  Row 2: column 12 a base neither of the others holds
# (every row differs), and it lacks column 17 (a gap under a column in which the other two differ).
_C32 = b"AACCGGTTACGTTGCAAGCTTCGAAGGCCTTA"
_R1 = b"CACCGNTTAgGTAGCAATCTTCGAAGGCCTTC"
_R2 = b"AACCGGTTACGTCGCAACTTCGAAGGCCTTA"

# consecutive groups of L = 1, 2, 3, 15, 16, 17 columns, two rows, first and last column variable: group boundaries fall inside one
# 16-byte piece of the text, and the sites of several groups share one
_SHORT = [[b"A", b"C"], [b"AC", b"GT"], [b"ACG", b"TCA"],
          [b"ACGTACGTACGTACG", b"CCGTACGTACGTACT"], [b"ACGTACGTACGTACGT", b"CCGTACGTACGTACGA"], [b"ACGTACGTACGTACGTA", b"CCGTACGTACGTACGTC"]]
SHORT_L = [1, 2, 3, 15, 16, 17]

_FIVE = [b"ACGTACGTACGTACGTACGT", b"ACGTACGTAAGTACGTACGT", b"ACGTACGTACGTACGTACGT", b"ACGTTCGTACGTACGTACGT", b"ACGTACGTACGTACGTACGA"]
HEADER_LENGTHS = [2, 15, 16, 17, 300]


def _header(n: int) -> bytes:
    return b">" + (b"abcdefghij" * 30)[:n - 2] + b"\n"


def _many(r: int):
    """r rows of 20 columns: row i differs from the centre in column i % 20"""
    c = b"ACGTTGCAACGTTGCAACGT"
    out = [c]
    for i in range(1, r):
        b = bytearray(c)
        b[i % 20] = b"ACGT"[(b"ACGT".index(c[i % 20]) + 1 + i // 20) % 4]
        out.append(bytes(b))
    return out


CASES = {
    "two_rows_one_site": case([[b"ACGT", b"AGGT"]], [0, 1], 2, [b">a\n", b">b\n"]),
    "classes_in_permuted_row_order": case([[b"ACGT", b"AGGT", b"ACGA"], [b"TTTT", b"TTAT", b"TTTT"]], [2, 0, 1, 1, 2, 0], 3, [b">a\n", b">b\n", b">c\n"], width=5),
    "codes_gap_and_edges": case([[_C32, _R1, _R2]], [0, 1, 2], 3),
    "columns_a_multiple_of_width": case([[_C32, _R1]], [0, 1], 2, width=16),
    "header_lengths": case([_FIVE], range(5), 5, [_header(n) for n in HEADER_LENGTHS], width=7),
    "one_class": case([[b"ACGTACGTAC"], [b"TTGCA"]], [0, 0], 1, [b">\n"], width=4),
    "thirty_three_classes": case([_many(33), list(reversed(_many(33)))], list(range(33)) + list(range(32, -1, -1)), 33, width=16),
    "no_site": case([[b"ACGTTGCATGCA"] * 2, [b"GGCAT", b"GGCAT"]], [0, 1, 1, 0], 2),
    "centre_of_length_0": case([[b"", b"ACGTAC", b"ACG", b"ACTTAC"], [b"ACGT", b"ACTT", b"ACGT", b"CCGT"]], [0, 1, 2, 3, 3, 2, 1, 0], 4, width=3),
    "empty_headers": case([[b"ACGT", b"AGGT"]], [1, 0], 2, [b"", b""], width=3),
    # group 1 holds class 1 twice and has three instances for two classes: not wanted, so not checked
    "unwanted_group_breaks_the_class_rule": case([[b"ACGTA", b"ACCTA"], [b"ACGT", b"ACGA", b"AGGT"], [b"GGA", b"GCA"]], [0, 1, 0, 1, 1, 1, 0], 2, want=[True, False, True]),
    "wanted_group_with_too_many_instances": case([[b"ACGTA", b"ACCTA"], [b"ACGT", b"ACGA", b"AGGT"], [b"GGA", b"GCA"]], [0, 1, 0, 1, 1, 1, 0], 2, refused=True),
    "wanted_group_with_a_class_twice": case([[b"ACGTA", b"ACCTA"], [b"ACGT", b"ACGA"]], [0, 1, 1, 1], 2, refused=True),
    "wanted_group_with_too_few_instances": case([[b"ACGTA", b"ACCTA"]], [0, 1], 3, refused=True),
}
for _w in (1, 15, 16, 17, 80, 100):                    # 54 columns: lines of one byte, either side of a 16-byte piece, the pipeline's, one line
    CASES["short_groups_width_%d" % _w] = case(_SHORT, identity_classes(_SHORT), 2, [b">first\n", b">second file\n"], width=_w)
CASES["short_groups_swapped_classes"] = case(_SHORT, [1, 0] * 6, 2, width=17)

# the texts of the smallest cases, written out by hand: (mode ALL, mode VARIABLE), and the sites (group, col, before)
BY_HAND = {
    "two_rows_one_site": (b">a\nACGT\n>b\nAGGT\n", b">a\nC\n>b\nG\n", [(0, 1, 1)]),
    "classes_in_permuted_row_order": (b">a\nAGGTT\nTTT\n>b\nACGAT\nTTT\n>c\nACGTT\nTAT\n", b">a\nGTT\n>b\nCAT\n>c\nCTA\n", [(0, 1, 1), (0, 3, 3), (1, 2, 2)]),
    "one_class": (b">\nACGT\nACGT\nACTT\nGCA\n", b">\n", []),
    "empty_headers": (b"AGG\nT\nACG\nT\n", b"G\nC\n", [(0, 1, 1)]),
}
