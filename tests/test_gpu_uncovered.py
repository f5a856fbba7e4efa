"""sbl_uncovered_calls and sbl_spell_text (csrc/uncovered.hip) on one context: the calls against the per-base model
(tests/uncovered_model.py) on the hand-written case table, the spelled text against a Python join, and the argument checks.

Records: the two 100-base records of the case table -- the first, the reference set, in lower case -- and a third of 9000 bases in
mixed case for the ranges that are longer than a workgroup's span; the model is given all three."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncovered_model as UM                       # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["gi|1|ref|NC_1.1|", "contig_1", "long"]
KIND = "DIU"
BIG = 2


def _records():
    rng = np.random.default_rng(2024)
    pick = lambda alphabet, n: bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))      # noqa: E731
    return [pick(b"acgt", UM.SIZES[0]), pick(b"ACGT", UM.SIZES[1]), pick(b"ACGTacgtNnRy", 9000)]


SEQS = _records()
SIZES = [len(s) for s in SEQS]


@pytest.fixture(scope="module")
def bf():
    from sibelia_amd import BlockFinder
    b = BlockFinder(SEQS, device=0)
    yield b
    b.close()


def as_blocks(lst):
    from sibelia_amd import formats as F
    return np.array(lst, dtype=F.BLOCK_DTYPE) if lst else np.zeros(0, dtype=F.BLOCK_DTYPE)


def as_tuples(calls):
    return [(KIND[int(u["kind"])], int(u["chr"]), int(u["start"]), int(u["end"]), int(u["ref_chr"]), int(u["pos"])) for u in calls]


# ------------------------------------------------------------------------------------------ the calls

@pytest.mark.parametrize("name", sorted(UM.CASES))
def test_the_calls_equal_the_model(bf, name):
    lists, by_hand = UM.CASES[name]
    got = as_tuples(bf.uncovered_calls([as_blocks(x) for x in lists], UM.M, UM.NREF))
    assert got == UM.calls(lists, SIZES, UM.NREF, UM.M)
    assert [c for c in got if c[1] != BIG] == by_hand and [c for c in got if c[1] == BIG] == [("U", BIG, 0, SIZES[BIG], 0, 0)]


def test_random_lists_equal_the_model(bf):
    """Overlapping instances, blocks that are mixed in one stage and not in another, several instances per block."""
    rng = np.random.default_rng(7)
    seen = set()
    for case in range(60):
        lists = []
        for _ in range(int(rng.integers(1, 4))):
            lst = []
            for b in range(1, int(rng.integers(1, 7))):
                for _ in range(int(rng.integers(1, 4))):
                    c = int(rng.integers(0, 2))
                    s = int(rng.integers(0, 95))
                    lst.append((b * (1 if rng.integers(0, 2) else -1), c, s, s + int(rng.integers(1, min(40, 100 - s) + 1))))
            lists.append(lst)
        got = as_tuples(bf.uncovered_calls([as_blocks(x) for x in lists], UM.M, UM.NREF))
        assert got == UM.calls(lists, SIZES, UM.NREF, UM.M), lists
        seen |= {c[0] for c in got}
    assert seen == {"D", "I", "U"}


def test_the_files_of_a_lower_case_reference(bf):
    """The alleles come out upper-cased whatever the record holds; the breakend records quote the first base as it is given."""
    from sibelia_amd import formats as F
    lists = [[(1, 0, 10, 50), (1, 1, 0, 40), (2, 0, 50, 90), (2, 1, 80, 100)]]
    calls = bf.uncovered_calls([as_blocks(x) for x in lists], UM.M, UM.NREF)
    found = as_tuples(calls)
    assert found == [("D", 0, 0, 10, 0, 0), ("D", 0, 90, 100, 0, 90), ("I", 1, 40, 80, 0, 50), ("U", BIG, 0, SIZES[BIG], 0, 0)]
    aligned = [(NAMES[0], 50, b"A", b"G")]
    for breakends in (True, False):
        t = F.vcf_pieces(NAMES, SIZES[0], SEQS[0][:1], aligned, calls, breakends)
        lines = F.vcf_header_lines(NAMES[0]) + (UM.bnd_lines(NAMES, SEQS, found) if breakends else [])
        lines += UM.record_lines([(NAMES[0], 50, "A", "G")] + UM.variant_rows(NAMES, SEQS, found))
        text = bf.spell_text(t.pieces(), t.literals)
        assert text == ("\n".join(lines) + "\n").encode()
        assert (b"\tbnd_0\t" + SEQS[0][:1] + b"\t" in text) == breakends and SEQS[0][:1].islower()
    fa = F.unmapped_fasta_pieces(NAMES, calls)
    assert bf.spell_text(fa.pieces(), fa.literals) == UM.unmapped_fasta(NAMES, SEQS, found)


# ------------------------------------------------------------------------------------------ the text

def join(pieces, literals):
    out = []
    for kind, c, s, e, width in pieces:
        if kind == 0:
            out.append(literals[s:e])
        elif not width:
            out.append(SEQS[c][s:e].upper())
        else:
            out += [SEQS[c][o:min(o + width, e)].upper() + b"\n" for o in range(s, e, width)]
    return b"".join(out)


def spell(bf, pieces, literals):
    from sibelia_amd import formats as F
    arr = np.array([p + (0,) for p in pieces], dtype=F.PIECE_DTYPE) if pieces else np.zeros(0, dtype=F.PIECE_DTYPE)
    return bf.spell_text(arr, literals)


LITERALS = bytes(range(1, 256)) * 2


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 4095, 4096, 4097])
def test_a_range_at_every_source_and_output_alignment(bf, length):
    pieces, at = [], 0
    for src in range(16):
        for dst in range(16):
            pad = (dst - at) % 16                   # literal bytes that bring the range to output alignment dst
            pieces.append((0, 0, 7 * src, 7 * src + pad, 0))
            pieces.append((1, BIG, 100 + src, 100 + src + length, 0))
            at += pad + length
    want = join(pieces, LITERALS)
    assert len(want) == at and (length < 4097 or at > 2 * 4096)      # the long ones: more than two workgroup spans
    assert spell(bf, pieces, LITERALS) == want


@pytest.mark.parametrize("width", [1, 15, 16, 17, 60, 80, 4000])
def test_wrapped_ranges(bf, width):
    pieces = []
    for i, length in enumerate([0, 1, 59, 60, 61, 120, 121, width - 1, width, width + 1, 2 * width, 2 * width + 1, 3 * width + 14, 3 * width + 15, 3 * width + 16]):
        length = min(length, SIZES[BIG] - 3 * i)      # 3 * 4000 + 14 and more: to the record's end
        pieces.append((0, 0, i, i + (i * 5) % 16, 0))                 # shifts the output alignment from range to range
        pieces.append((1, BIG, 3 * i, 3 * i + length, width))
    assert spell(bf, pieces, LITERALS) == join(pieces, LITERALS)


def test_lengths_59_60_61_120_in_lines_of_60_at_every_output_alignment(bf):
    pieces = []
    for dst in range(16):
        for length in (59, 60, 61, 120):
            pieces.append((0, 0, 0, (dst - sum(p[3] - p[2] + ((p[3] - p[2] + 59) // 60 if p[4] else 0) for p in pieces)) % 16, 0))
            pieces.append((1, BIG, 11 + dst, 11 + dst + length, 60))
    assert spell(bf, pieces, LITERALS) == join(pieces, LITERALS)


def test_literals_of_no_and_one_byte_between_ranges_and_whole_records(bf):
    pieces = [(1, 0, 0, 100, 0), (0, 0, 5, 5, 0), (1, 1, 0, 100, 0), (0, 0, 9, 10, 0), (1, BIG, 0, SIZES[BIG], 0), (0, 0, 0, 0, 0), (1, 0, 99, 100, 0),
              (0, 0, 0, len(LITERALS), 0), (1, 1, 50, 50, 60), (1, BIG, SIZES[BIG] - 1, SIZES[BIG], 60), (0, 0, 509, 510, 0)]
    got = spell(bf, pieces, LITERALS)
    assert got == join(pieces, LITERALS) and got[:100] == SEQS[0].upper() and SEQS[0].islower()


def test_more_pieces_in_one_span_than_the_kernel_keeps_on_chip(bf):
    pieces = []
    for i in range(1500):                           # 3 bytes per pair: some 1360 pieces in a span of 4096 bytes
        pieces += [(0, 0, i % 500, i % 500 + 1, 0), (1, i % 3, i % 90, i % 90 + 2, 0)]
    assert spell(bf, pieces, LITERALS) == join(pieces, LITERALS)


def test_an_empty_piece_list_and_pieces_that_are_all_empty(bf):
    assert spell(bf, [], b"") == b""
    assert spell(bf, [(0, 0, 3, 3, 0), (1, 0, 7, 7, 0), (1, 1, 100, 100, 60)], LITERALS) == b""


# ------------------------------------------------------------------------------------------ arguments

def test_bad_pieces_are_refused_before_any_launch(bf):
    from sibelia_amd import SibeliaError
    spell(bf, [(1, 0, 0, 50, 0)], b"")
    before = bf.spell_text_times()
    bad = [(1, 3, 0, 1, 0),                        # no such record
           (1, 0, 5, 4, 0),                        # ends before it starts
           (1, 0, 0, 101, 0),                      # beyond its record
           (1, 0, 101, 101, 0),
           (0, 0, 0, len(LITERALS) + 1, 0),        # beyond the literal text
           (0, 0, 9, 8, 0),
           (0, 0, 0, 4, 60),                       # a wrapped literal
           (2, 0, 0, 1, 0)]                        # no such kind
    for p in bad:
        with pytest.raises(SibeliaError, match="bad argument"):
            spell(bf, [(1, 0, 0, 10, 0), p], LITERALS)
    assert bf.L.sbl_spell_text(bf.h, 1, None, LITERALS, len(LITERALS), None, None) == 1      # SBL_ERR_BAD_ARG
    from sibelia_amd import formats as F
    hold = np.array([(0, 0, 0, 4, 0, 0)], dtype=F.PIECE_DTYPE)      # literal [0, 4) of a literal text that is not there
    assert bf.L.sbl_spell_text(bf.h, 1, hold.ctypes.data, None, 4, None, None) == 1
    assert bf.spell_text_times() == before         # the times are those of the last launch: none happened


def test_bad_lists_are_refused(bf):
    from sibelia_amd import SibeliaError
    ok = as_blocks([(1, 0, 10, 50), (1, 1, 0, 40)])
    assert len(bf.uncovered_calls([ok], UM.M, 1)) == 4
    for nref in (0, 3, 4):
        with pytest.raises(SibeliaError, match="bad argument"):
            bf.uncovered_calls([ok], UM.M, nref)
    for block in ((1, 3, 0, 1), (1, 0, 5, 4), (1, 0, 0, 101), (0, 0, 0, 1)):
        with pytest.raises(SibeliaError, match="bad argument"):
            bf.uncovered_calls([ok, as_blocks([block])], UM.M, 1)
    raw = lambda nlists, first: bf.L.sbl_uncovered_calls(bf.h, nlists, (C.c_uint64 * len(first))(*first), ok.ctypes.data, UM.M, 1, None, None)      # noqa: E731
    assert raw(1, [0, 2]) == 0
    assert raw(0, [0]) == 1                        # SBL_ERR_BAD_ARG: no list
    assert raw(1, [1, 2]) == 1                     # the first list does not start at 0
    assert raw(2, [0, 2, 1]) == 1                  # offsets descend
    assert bf.L.sbl_uncovered_calls(bf.h, 1, None, ok.ctypes.data, UM.M, 1, None, None) == 1
