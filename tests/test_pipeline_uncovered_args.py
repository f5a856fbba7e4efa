"""The command line of --uncovered / --unmapped (sibelia_amd/pipeline.py), the piece lists of their files (sibelia_amd/formats.py) and
the new entry points in the header and the export list: device-free."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncovered_model as UM                       # noqa: E402

from sibelia_amd import formats as F               # noqa: E402
from sibelia_amd import pipeline as P              # noqa: E402

BASE = ["-s", "fine", "-o", "out"]
FULL = ["--allstages", "--variants", "v.vcf", "--uncovered"]


@pytest.mark.parametrize("argv, named", [
    (["--allstages", "--uncovered"], "--variants"),
    (["--variants", "v.vcf", "--uncovered"], "--allstages"),
    (["--allstages", "--variants", "v.vcf", "--unmapped", "u.fa"], "--uncovered"),
])
def test_each_missing_companion_is_an_error_that_names_it(argv, named):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + argv + ["x.fa", "y.fa"])
    assert "needs " + named in str(e.value)


def test_the_options_parse_and_need_two_files():
    o = P.parse_args(BASE + FULL + ["--unmapped", "u.fa", "x.fa", "y.fa"])
    assert o.uncovered and o.unmapped == "u.fa"
    o = P.parse_args(BASE + ["--variants", "v.vcf", "x.fa", "y.fa"])
    assert not o.uncovered and o.unmapped is None
    with pytest.raises(P.PipelineError, match="only two FASTA files"):
        P.parse_args(BASE + FULL + ["x.fa"])


@pytest.mark.parametrize("argv, message", [
    (["--unmapped", "v.vcf"], "--variants and --unmapped name the same file: v.vcf"),
    (["--maf", "sub/../a", "--unmapped", "./a"], "--maf and --unmapped name the same file: sub/../a"),
    (["--unmapped", "u", "--multimaf", "u"], "--unmapped and --multimaf name the same file: u"),
    (["--unmapped", "blocks_coords2.txt"], "--unmapped names a file the program writes itself: blocks_coords2.txt"),
    (["--unmapped", "genomes_permutations.txt"], "--unmapped names a file the program writes itself: genomes_permutations.txt"),
    (["--unmapped", "sub/"], "--unmapped needs a file name, not 'sub/'"),
])
def test_unmapped_joins_the_name_clash_check(argv, message):
    with pytest.raises(P.PipelineError) as e:
        P.parse_args(BASE + FULL + argv + ["x.fa", "y.fa"])
    assert str(e.value) == message


def test_planned_files_with_and_without_unmapped():
    base = ["blocks_coords%d.txt" % i for i in range(4)] + ["genomes_permutations.txt", "coverage_report.txt"]
    plan = lambda argv: P.planned_files(P.parse_args(BASE + argv + ["x.fa", "y.fa"]), 3)      # noqa: E731
    assert plan(FULL) == base + ["v.vcf"]
    assert plan(FULL + ["--unmapped", "sub/u.fa"]) == base + ["v.vcf", "sub/u.fa"]
    assert plan(FULL + ["--maf", "a.maf", "--unmapped", "u.fa", "--multimaf", "m.maf"]) == base + ["a.maf", "v.vcf", "u.fa", "m.maf"]


def test_duplicate_record_ids():
    P.check_duplicate_ids(["b", "a", "c"])
    with pytest.raises(P.PipelineError) as e:
        P.check_duplicate_ids(["z", "contig7", "a", "z", "contig7"])
    assert str(e.value) == 'Found duplicated sequence id "contig7"'


def test_first_base_keeps_the_case_of_the_file(tmp_path):
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"\n>one two\n\n  \ngATC\nAA\n>next\nTT\n")
    assert P.first_base(str(fa)) == b"g"


def render(pieces: F.TextPieces, seqs):
    """A piece list as sbl_spell_text defines it, joined on the host"""
    out = []
    for kind, c, s, e, width, _ in pieces.pieces().tolist():
        if kind == F.PIECE_LITERAL:
            out.append(bytes(pieces.literals[s:e]))
        elif not width:
            out.append(seqs[c][s:e].upper())
        else:
            out += [seqs[c][o:min(o + width, e)].upper() + b"\n" for o in range(s, e, width)]
    return b"".join(out)


def calls_array(found):
    kinds = {"D": F.CALL_DELETION, "I": F.CALL_INSERTION, "U": F.CALL_UNMAPPED}
    dt = np.dtype([("kind", "<u4"), ("chr", "<u4"), ("start", "<u8"), ("end", "<u8"), ("ref_chr", "<u4"), ("pad_", "<u4"), ("pos", "<u8")])
    return np.array([(kinds[k], c, s, e, r, 0, p) for k, c, s, e, r, p in found], dtype=dt)


def test_the_piece_lists_spell_the_files_of_the_model():
    rng = np.random.default_rng(11)
    names = ["gi|1|ref|NC_1.1|", "ctg_b", "ctg_a"]
    seqs = [bytes(rng.choice(np.frombuffer(b"acgtACGT", dtype=np.uint8), n)) for n in (300, 200, 150)]
    found = [("D", 0, 0, 20, 0, 0), ("D", 0, 100, 230, 0, 100), ("U", 1, 0, 61, 0, 0), ("I", 1, 90, 200, 0, 100), ("I", 2, 5, 30, 0, 7), ("U", 2, 30, 150, 0, 0)]
    aligned = [(names[0], 100, b"A", b"C"), (names[0], 7, b"AT", b""), (names[0], 250, b"", b"G")]
    for breakends in (True, False):
        t = F.vcf_pieces(names, len(seqs[0]), seqs[0][:1], aligned, calls_array(found), breakends)
        lines = F.vcf_header_lines(names[0]) + (UM.bnd_lines(names, seqs, found) if breakends else [])
        rows = [(n, p, r.decode() or ".", a.decode() or ".") for n, p, r, a in aligned] + UM.variant_rows(names, seqs, found)
        lines += UM.record_lines(rows)
        assert render(t, seqs) == ("\n".join(lines) + "\n").encode()
        # stable: at (NC_1, 7) and (NC_1, 100) the alignment record stands before the calls, and those in the order they were found
        body = [ln.split("\t") for ln in lines if ln.startswith("NC_1\t100\t") or ln.startswith("NC_1\t7\t")]
        assert [len(x[3]) for x in body] == [2, 1, 1, 131, 1]
    fa = F.unmapped_fasta_pieces(names, calls_array(found))
    assert render(fa, seqs) == UM.unmapped_fasta(names, seqs, found)
    # literals that follow each other are one piece: a file is a few pieces per call, not one per field
    assert len(t.pieces()) <= 4 * len(found) + 2
    assert len(F.unmapped_fasta_pieces(names, calls_array([])).pieces()) == 0


def test_without_the_option_the_vcf_text_is_what_it_was():
    recs = [("gi|1|ref|NC_1.1|", 5, b"A", b""), ("gi|1|ref|NC_1.1|", 2, b"", b"GG")]
    assert F.vcf_text("gi|1|ref|NC_1.1|", recs) == ("\n".join(F.vcf_header_lines("gi|1|ref|NC_1.1|") + ["NC_1\t2\t.\t.\tGG\t.\t.\t.", "NC_1\t5\t.\tA\t.\t.\t.\t."]) + "\n").encode()
    assert F.vcf_header_lines("x")[1] == "##source=sibelia_amd" and len(F.vcf_header_lines("x")) == 7


def test_the_new_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    from sibelia_amd.build import LIB, SOURCES
    lib = ctypes.CDLL(LIB)
    hdr = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    for name in ("sbl_uncovered_calls", "sbl_spell_text", "sbl_spell_text_times"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(lib, name), name
    assert "uncovered.hip" in SOURCES
    # the Python mirrors of the two structs have the C layout: 40 and 32 bytes, 64-bit fields on 8-byte offsets
    assert api.CALL_DTYPE.itemsize == 40 and api.CALL_DTYPE.fields["pos"][1] == 32
    assert api.PIECE_DTYPE.itemsize == 32 and api.PIECE_DTYPE.fields["width"][1] == 24
