"""The model of --uncovered (tests/uncovered_model.py) pinned on lists whose calls were worked out by hand: every rule of DESIGN.md 0.4
once.  tests/test_gpu_uncovered.py holds the library to the model on the same table.  Device-free."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncovered_model as UM                       # noqa: E402


@pytest.mark.parametrize("name", sorted(UM.CASES))
def test_the_model_gives_the_calls_worked_out_by_hand(name):
    lists, want = UM.CASES[name]
    assert UM.calls(lists, UM.SIZES, UM.NREF, UM.M) == want


def test_the_table_covers_every_kind_and_both_anchor_positions():
    kinds = {c[0] for _, want in UM.CASES.values() for c in want}
    assert kinds == {"D", "I", "U"}
    assert any(c[0] == "D" and c[2] == 0 for _, want in UM.CASES.values() for c in want)
    assert any(c[0] == "D" and c[3] == UM.SIZES[0] for _, want in UM.CASES.values() for c in want)
    assert len({c[5] for _, want in UM.CASES.values() for c in want if c[0] == "I"}) >= 3


def test_the_texts_of_the_model():
    names = ["gi|1|ref|NC_1.1|", "contig"]
    seqs = [b"aCGTACGTAC", b"ttgcaTTGCA" * 7]
    found = [("D", 0, 0, 3, 0, 0), ("D", 0, 5, 9, 0, 5), ("I", 1, 2, 6, 0, 4), ("U", 1, 0, 70, 0, 0)]
    assert UM.variant_rows(names, seqs, found) == [(names[0], 0, "ACG", "."), (names[0], 5, "ACGTA", "A"), (names[0], 4, "T", "TGCAT")]
    assert UM.record_lines(UM.variant_rows(names, seqs, found)) == ["NC_1\t0\t.\tACG\t.\t.\t.\t.", "NC_1\t4\t.\tT\tTGCAT\t.\t.\t.", "NC_1\t5\t.\tACGTA\tA\t.\t.\t."]
    assert UM.bnd_lines(names, seqs, found) == ["NC_1\t1\tbnd_0\ta\ta[contig:1[\t.\t.\tIMPRECISE;SVTYPE=BND;CIPOS=0,10",
                                                "NC_1\t1\tbnd_1\ta\t]contig:71]a\t.\t.\tIMPRECISE;SVTYPE=BND;CIPOS=0,10"]
    assert UM.unmapped_fasta(names, seqs, found) == b'>Seq="contig",Start=1",End=70\n' + b"TTGCA" * 12 + b"\n" + b"TTGCA" * 2 + b"\n"


def test_blocks_coords_are_read_back():
    text = ("Seq_id\tSize\tDescription\n1\t100\ta\n2\t100\tb\n" + "-" * 80 + "\nBlock #1\nSeq_id\tStrand\tStart\tEnd\tLength\n"
            "1\t+\t11\t50\t40\n2\t-\t40\t1\t40\n" + "-" * 80 + "\n")
    assert UM.parse_blocks_coords(text) == [(1, 0, 10, 50), (-1, 1, 0, 40)]
