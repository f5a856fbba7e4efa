"""tests/mvariants_model.py (the variant segments of a multiple alignment) against itself -- the automaton and its closed
form -- against formats.variants_from_runs for two rows, and on cases written out by hand; formats.multi_vcf_text byte for byte.
Device-free."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_cases as MC                             # noqa: E402
import msa_model as MM                             # noqa: E402
import mvariants_model as MV                       # noqa: E402

from sibelia_amd import formats                    # noqa: E402

P = b"ACGTTGCAAGCTTAGCCATGGATCCGTAAC"              # 30 columns of context
Q = b"TTGACCGATAGCTAGGCTAACGTCAGTCAG"
assert len(P) == len(Q) == MV.MINIMUM_CONTEXT_SIZE == formats.MINIMUM_CONTEXT_SIZE


def test_automaton_equals_closed_form_on_random_class_strings():
    rng = np.random.default_rng(2024)
    for k in range(2000):
        n = int(rng.integers(0, 201))
        p = (0.02, 0.1, 0.5)[k % 3]                                             # sparse edits: long equal runs; dense: short ones
        cls = [int(x) for x in rng.choice([0, 1, 3], n, p=[1 - p, p / 2, p / 2])]
        assert MV.automaton(cls) == MV.closed_form(cls), cls


@pytest.mark.parametrize("run", [29, 30, 31])
def test_equal_runs_of_the_context_size_at_the_start_in_the_middle_and_at_the_end(run):
    eq = [0] * run
    kept = run >= 30
    cases = {
        "start": (eq + [1, 0, 0, 1], [(run, run + 4)]),                          # a run at column 0 is kept whatever its length
        "middle": ([1] + eq + [3], [(0, 1), (run + 1, run + 2)] if kept else [(0, run + 2)]),
        "end": ([1, 0, 1] + eq, [(0, 3)]),                                      # ... and so is one that ends at L
        "middle_after_start": ([0, 0, 1] + eq + [1, 0], [(2, 3), (run + 3, run + 4)] if kept else [(2, run + 4)]),
        "two_middles": ([1] + eq + [1] + eq + [1], [(0, 1), (run + 1, run + 2), (2 * run + 2, 2 * run + 3)] if kept else [(0, 2 * run + 3)]),
    }
    for name, (cls, want) in cases.items():
        assert MV.closed_form(cls) == want, name
        assert MV.automaton(cls) == want, name
    for cls in ([], [0], [0] * 40, [1], [3, 3]):
        assert MV.automaton(cls) == MV.closed_form(cls) == ([(0, len(cls))] if cls and cls[0] else [])


@pytest.mark.parametrize("seed", [1, 2])
def test_two_rows_give_variants_from_runs_on_both_strands(seed):
    checked = 0
    for group in MC.random_groups(seed, 60, 2, 2, 400, 20):
        rows, _ = MM.msa(group)
        _, runs = MM.pair(group[0], group[1])
        n = len(group[0])
        for reverse in (False, True):
            want = formats.variants_from_runs(runs, rows[0], rows[1], 1000, 1000 + n, reverse)
            got = [(pos, ref, alt) for pos, (ref, alt) in MV.records(rows, 1000, 1000 + n, reverse)]
            assert got == want, group
            checked += len(want)
    assert checked > 200


def test_three_rows_with_overlapping_indels():
    rows = [P + b"AAGG--TT" + Q, P + b"A--GCCTT" + Q, P + b"AAGG-CTT" + Q]
    assert MV.classes(rows)[30:38] == [0, 3, 3, 0, 3, 3, 0, 0]
    assert MV.segments(rows) == [(31, 36, 31, 1, 1, [b"AAGG--", b"A--GCC", b"AAGG-C"])]
    assert MV.records(rows, 1000, 1066, False) == [(1031, [b"AAGG", b"AGCC", b"AAGGC"])]
    assert MV.records(rows, 1000, 1066, True) == [(1066 - 31 - 1, [b"CCTT", b"GGCT", b"GCCTT"])]


def test_one_column_substitution_shared_by_two_members():
    rows = [P + b"A" + Q, P + b"C" + Q, P + b"C" + Q, P + b"A" + Q]
    assert MV.segments(rows) == [(30, 31, 30, 0, 0, [b"A", b"C", b"C", b"A"])]
    assert MV.records(rows, 500, 561, False) == [(531, [b"A", b"C", b"C", b"A"])]


def test_one_gapped_column_quotes_the_base_before_it():
    rows = [P + b"A" + Q, P + b"-" + Q, P + b"A" + Q]
    assert MV.segments(rows) == [(30, 31, 30, 1, 1, [b"CA", b"C-", b"CA"])]
    assert MV.records(rows, 1000, 1061, False) == [(1030, [b"CA", b"C", b"CA"])]
    assert MV.records(rows, 1000, 1061, True) == [(1030, [b"TG", b"G", b"TG"])]


def test_a_segment_at_column_0_has_no_lead():
    assert MV.segments([b"A" + Q, b"C" + Q]) == [(0, 1, 0, 0, 0, [b"A", b"C"])]
    rows = [b"--A" + Q, b"GGA" + Q, b"-TA" + Q]
    assert MV.segments(rows) == [(0, 2, 0, 0, 1, [b"--", b"GG", b"-T"])]
    assert MV.records(rows, 10, 41, False) == [(11, [b"", b"GG", b"T"])]


def test_groups_without_unequal_columns_have_no_segments():
    assert MV.segments([b"ACGT"]) == MV.segments([b""]) == MV.segments([b"", b""]) == MV.segments([P, P, P]) == []


def test_group_variants_records_is_the_model():
    rows = [P + b"AAGG--TT" + Q + b"A" + P, P + b"A--GCCTT" + Q + b"C" + P, P + b"AAGG-CTT" + Q + b"A" + P]
    segs = [(5, s, e, before, lead, slices) for s, e, before, lead, _, slices in MV.segments(rows)]
    assert len(segs) == 2
    for reverse in (False, True):
        assert formats.group_variants_records(segs, 70, 70 + 97, reverse) == MV.records(rows, 70, 70 + 97, reverse)


def test_multi_vcf_text_byte_for_byte():
    records = [("gi|9|ref|NC_000009.2|", 1031, 7, b"AAGG", [b"AGCC", None, b"AAGGC"]),
               ("gi|9|ref|NC_000009.2|", 50, 3, b"", [b"GG", b"", b"GG"]),
               ("gi|9|ref|NC_000009.2|", 50, 2, b"C", [b"", b"C", None])]
    head = ("##fileformat=VCFv4.1\n##source=sibelia_amd\n%s##reference=NC_000009\n"
            '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">\n'
            '##INFO=<ID=IMPRECISE,Number=0,Type=Flag,Description="Imprecise structural variation">\n'
            '##INFO=<ID=CIPOS,Number=2,Type=Integer,Description="Confidence interval around POS for imprecise variants">\n'
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tb.fa\tc.fa\td.fa\n")
    body = ("NC_000009\t50\t.\tC\t.\t.\t.\t.\tGT\t1\t0\t.\n"
            "NC_000009\t50\t.\t.\tGG\t.\t.\t.\tGT\t1\t0\t1\n"
            "NC_000009\t1031\t.\tAAGG\tAGCC,AAGGC\t.\t.\t.\tGT\t1\t.\t2\n")
    assert formats.multi_vcf_text("gi|9|ref|NC_000009.2|", ["b.fa", "c.fa", "d.fa"], records) == (head % "" + body).encode()
    assert formats.multi_vcf_text("gi|9|ref|NC_000009.2|", ["b.fa", "c.fa", "d.fa"], records, 400) == (head % "##sibelia_amd_gapopen=400\n" + body).encode()
    assert formats.multi_vcf_text("r", ["s"], []) == formats.vcf_text("r", []).replace(
        b"#CHROM", b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n#CHROM').replace(b"INFO\n", b"INFO\tFORMAT\ts\n")
