"""The SNP-density mask of the multiple alignments (include/sibelia_amd.h) restated in plain Python on the rows of
msa_model.msa, for tests/test_gmask_model.py and the GPU tests of sbl_group_mask (never used by the product).

A call is a list of groups, each given by its ROWS (a list of r byte strings of L columns, centre first) or by an int r: a group of r
instances that was skipped (tests/concat_model.py's convention).

`differences(rows, i)`            -> [(column, centre index)] of member row i, ascending.
`row_intervals(diffs, W, T)`      -> [(first, last, before_first, before_last, ndiff)] of one row, straight from the definition: the hull
                                     of differences k .. k + T for every k with p[k + T] - p[k] < W; hulls that share a difference are one.
`used(groups, want)`              -> the indices of the groups the mask uses: wanted, aligned, L > 0, two rows at least.
`mask(groups, W, T, want)`        -> (intervals as sbl_group_mask returns them, the groups with their rows masked); Refused where it
                                     returns SBL_ERR_BAD_ARG.
"""
BASES = b"ACGT"
GAP, N = 45, 78


class Refused(ValueError):
    """what the library answers with SBL_ERR_BAD_ARG"""


def differences(rows, i):
    out, before = [], 0
    for x, (a, b) in enumerate(zip(rows[0], rows[i])):
        if a in BASES and b in BASES and a != b:
            out.append((x, before))
        before += a != GAP
    return out


def row_intervals(diffs, W, T):
    out = []                                                   # [first difference, last difference] of every interval so far
    for k in range(len(diffs) - T):
        if diffs[k + T][1] - diffs[k][1] < W:
            if out and k <= out[-1][1]:                        # shares a difference with the hull before
                out[-1][1] = k + T
            else:
                out.append([k, k + T])
    return [(diffs[a][0], diffs[b][0], diffs[a][1], diffs[b][1], b - a + 1) for a, b in out]


def used(groups, want=None):
    return [g for g, rows in enumerate(groups) if not isinstance(rows, int) and len(rows) >= 2 and len(rows[0]) > 0 and (want is None or want[g])]


def masked_row(row: bytes, intervals) -> bytes:
    out = bytearray(row)
    for first, last, _, _, _ in intervals:
        for x in range(first, last + 1):
            if out[x] != GAP:
                out[x] = N
    return bytes(out)


def mask(groups, W, T, want=None):
    if not 1 <= W <= 2 ** 32 - 1 or not 1 <= T <= 2 ** 32 - 1:
        raise Refused("window or number of differences")
    intervals = []
    masked = [rows if isinstance(rows, int) else [bytes(r) for r in rows] for rows in groups]
    for g in used(groups, want):
        rows = groups[g]
        for i in range(1, len(rows)):
            found = row_intervals(differences(rows, i), W, T)
            intervals += [(g, i) + iv for iv in found]
            masked[g][i] = masked_row(rows[i], found)
    return intervals, masked
