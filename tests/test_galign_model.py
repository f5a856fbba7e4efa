"""The definition of the block alignment (tests/galign_model.py) checked against itself -- the band certificate -- and the device-free
writers of --maf / --variants (sibelia_amd/formats.py) against hand-written cases and against the model's column-by-column restatement
of the reference's rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import galign_model as GM                          # noqa: E402

from sibelia_amd import formats as F               # noqa: E402


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def mutated(rng, a, max_indel=40):
    """a copy with substitutions and a few indels of up to max_indel bases"""
    b = bytearray()
    i = 0
    while i < len(a):
        u = rng.random()
        if u < 0.02:
            i += int(rng.integers(1, max_indel + 1))
        elif u < 0.04:
            b += rand(rng, int(rng.integers(1, max_indel + 1)))
        else:
            b += rand(rng, 1) if rng.random() < 0.05 else a[i:i + 1]
            i += 1
    return bytes(b)


def test_banded_with_doubling_equals_unbanded_on_random_pairs():
    rng = np.random.default_rng(2024)
    wide = doubled = 0
    for case in range(300):
        a = rand(rng, int(rng.integers(0, 121)))
        b = mutated(rng, a)[:120] if rng.random() < 0.9 else rand(rng, int(rng.integers(0, 121)))
        want = GM.align(a, b)
        for w0 in (1, 4):
            score, steps, w, passes = GM.align_doubling(a, b, w0)
            assert (score, steps) == want, (case, w0, a, b)
            doubled += passes > 1
        wide += abs(len(a) - len(b)) > 4
        assert GM.score_of_rows(*GM.rows(a, b, want[1])) == want[0]
        assert sum(n for _, n in GM.runs(a, b, want[1])) == len(want[1])
    assert wide >= 30 and doubled >= 100


@pytest.mark.parametrize("a, b", [
    (b"A" * 40, b"A" * 33), (b"A" * 33, b"A" * 40), (b"AC" * 30, b"AC" * 26), (b"ACG" * 20, b"ACG" * 23),
    (b"GATTACA" + b"T" * 30 + b"GATTACA", b"GATTACA" + b"T" * 24 + b"GATTACA"), (b"ACGT" + b"CA" * 20 + b"ACGT", b"ACGT" + b"CA" * 25 + b"TCGT"),
    (b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"C"), (b"A", b"A")])
def test_ties_in_indel_placement_do_not_depend_on_the_band(a, b):
    want = GM.align(a, b)
    for w0 in (1, 2, 8, 64):
        assert GM.align_doubling(a, b, w0)[:2] == want
    if a and b and len(a) != len(b) and len(set(a + b)) == 1:      # a homopolymer: diagonal steps first, the gap at the far end
        assert want[1] == "M" * min(len(a), len(b)) + ("I" if len(a) > len(b) else "D") * abs(len(a) - len(b))


def test_the_certificate_refuses_a_band_that_cuts_the_optimum():
    rng = np.random.default_rng(1)
    a = rand(rng, 100)
    b = a[:20] + rand(rng, 10) + a[20:70] + a[80:]        # equal lengths, but the middle lies 10 off the main diagonal
    want = GM.align(a, b)
    score, steps, ok = GM.align_banded(a, b, 1)
    assert score < want[0] and not ok                     # the narrow band loses the optimum, and the certificate says so
    score, steps, w, passes = GM.align_doubling(a, b, 1)
    assert (score, steps) == want and passes > 1 and w >= 10


# ---- variants: two rows -> records, expected records written out by hand

E40 = b"ACGTTGCAAGCTTAGCCATGGATCCTAGGCTAACGTTAGC"            # 40 columns
E30 = b"TTGACCGATAGCTAGGATCCAAGTCGATCA"                      # 30 columns
E10 = b"GGATCCAAGT"


def ops_of(row_a, row_b):
    steps = "".join("I" if y == 45 else "D" if x == 45 else "M" for x, y in zip(row_a, row_b))
    a, b = row_a.replace(b"-", b""), row_b.replace(b"-", b"")
    assert GM.rows(a, b, steps) == (row_a, row_b)
    return GM.runs(a, b, steps)


CASES = {
    # name: (row a, row b, records on a '+' instance starting at 0-based 100)
    "lone_snp": (E40 + b"A" + E40, E40 + b"G" + E40, [(141, b"A", b"G")]),
    "snp_at_column_0": (b"A" + E40, b"C" + E40, [(101, b"A", b"C")]),
    "deletion_after_40_equal": (E40 + b"TTT" + E40, E40 + b"---" + E40, [(140, b"CTTT", b"C")]),          # anchor base E40[-1] = C
    "two_snps_10_apart": (E40 + b"A" + E10[1:] + b"A" + E40, E40 + b"G" + E10[1:] + b"C" + E40, [(140, b"CA" + E10[1:] + b"A", b"CG" + E10[1:] + b"C")]),
    "two_snps_30_apart": (E40 + b"A" + E30 + b"A" + E40, E40 + b"G" + E30 + b"C" + E40, [(141, b"A", b"G"), (172, b"A", b"C")]),
    "insertion_at_the_last_column": (E40 + b"--", E40 + b"GG", [(140, b"C", b"CGG")]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_variants_on_a_forward_reference_instance(name):
    row_a, row_b, want = CASES[name]
    n = len(row_a.replace(b"-", b""))
    assert GM.variants(row_a, row_b, 100, 100 + n, False) == want
    assert F.variants_from_runs(ops_of(row_a, row_b), row_a, row_b, 100, 100 + n, False) == want


def rc(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


REVERSE = {
    # the same rows read on a '-' instance [100, 100 + n): column c of row a is position 100 + n - (bases before c), POS descends,
    # the anchor base is subtracted from POS as the reference does, alleles are reverse-complemented
    "lone_snp": [(100 + 81 - 40, b"T", b"C")],
    "snp_at_column_0": [(141, b"T", b"G")],
    "deletion_after_40_equal": [(100 + 83 - 40 - 1, rc(b"CTTT"), rc(b"C"))],
    "two_snps_10_apart": [(100 + 91 - 40 - 1, rc(b"CA" + E10[1:] + b"A"), rc(b"CG" + E10[1:] + b"C"))],
    "two_snps_30_apart": [(100 + 112 - 40, b"T", b"C"), (100 + 112 - 71, b"T", b"G")],
    "insertion_at_the_last_column": [(100 + 40 - 40 - 1, rc(b"C"), rc(b"CGG"))],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_variants_on_a_reverse_reference_instance(name):
    row_a, row_b, _ = CASES[name]
    n = len(row_a.replace(b"-", b""))
    assert GM.variants(row_a, row_b, 100, 100 + n, True) == REVERSE[name]
    assert F.variants_from_runs(ops_of(row_a, row_b), row_a, row_b, 100, 100 + n, True) == REVERSE[name]


def test_variants_from_runs_equal_the_column_scan_on_random_alignments():
    rng = np.random.default_rng(77)
    for case in range(150):
        a = rand(rng, int(rng.integers(1, 300)))
        b = mutated(rng, a, 8) or b"A"
        _, steps = GM.align(a, b)
        row_a, row_b = GM.rows(a, b, steps)
        for reverse in (False, True):
            assert F.variants_from_runs(GM.runs(a, b, steps), row_a, row_b, 17, 17 + len(a), reverse) == GM.variants(row_a, row_b, 17, 17 + len(a), reverse), case


def test_vcf_text():
    text = F.vcf_text("gi|1|ref|NC_000001.2|", [("chrB", 9, b"A", b""), ("chrA", 12, b"", b"CG"), ("chrA", 3, b"A", b"T")]).decode()
    lines = text.split("\n")
    assert lines[:3] == ["##fileformat=VCFv4.1", "##source=sibelia_amd", "##reference=NC_000001"]
    assert lines[3].startswith("##INFO=<ID=SVTYPE") and lines[4].startswith("##INFO=<ID=IMPRECISE") and lines[5].startswith("##INFO=<ID=CIPOS")
    assert lines[6] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    assert lines[7:] == ["chrA\t3\t.\tA\tT\t.\t.\t.", "chrA\t12\t.\t.\tCG\t.\t.\t.", "chrB\t9\t.\tA\t.\t.\t.\t.", ""]


def test_maf_coordinates_for_both_strands():
    assert GM.maf_fields(10, 25, False, 100) == (10, 15, "+", 100)
    assert GM.maf_fields(10, 25, True, 100) == (75, 15, "-", 100)
    assert F.maf_line("chr1", 10, 25, False, 100, b"ACG-T") == b"s chr1 10 15 + 100 ACG-T"
    assert F.maf_line("chr1", 10, 25, True, 100, b"ACG-T") == b"s chr1 75 15 - 100 ACG-T"
    text = F.maf_text([[b"s x 0 3 + 9 ACG", b"s y 1 3 - 8 A-G"], [b"s x 5 1 + 9 A", b"s y 0 1 + 8 A"]])
    assert text == b"##maf version=1\n\na\ns x 0 3 + 9 ACG\ns y 1 3 - 8 A-G\n\na\ns x 5 1 + 9 A\ns y 0 1 + 8 A\n\n"
    assert F.maf_text([]) == b"##maf version=1\n\n"
