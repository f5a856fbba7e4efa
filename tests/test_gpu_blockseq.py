"""blocks_sequences.fasta (spelled on the device by k_spell_text, csrc/spell_text.hip, from the pieces csrc/blockseq.hip lists) and
blocks_coords.gff on synthetic block lists.

The expected text is restated here from the format's description (include/sibelia_amd.h): per instance a header
`>Seq="<description>",Strand='<+|->',Block_id=<|id|>,Start=<from>,End=<to>`, the bases in lines of 80 without a line feed after the
last one, then one line feed; reverse instances read downwards with ACGT / acgt complemented and every other byte unchanged.
The reference orders instances by ONE unstable sort by |id|, whose ties cannot be restated: ids must ascend exactly, the records of
one id are compared as a sorted collection; the byte order is pinned by the fixtures of tests/test_gpu_pipeline.py."""
import os
import re

import numpy as np
import pytest

from sibelia_amd import formats as F
from sibelia_amd import workloads as W

pytestmark = pytest.mark.gpu

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
GFF_HEAD = b"##gff-version 2\n##source-version Sibelia 3.0.7\n##Type DNA\n"


def blocks_of(rows):
    return np.array(rows, dtype=F.BLOCK_DTYPE)


def conventional(b):
    return (int(b["start"]) + 1, int(b["end"])) if b["id"] > 0 else (int(b["end"]), int(b["start"]) + 1)


def expected_records(blocks, seqs, names):
    out = []
    for b in blocks:
        s = seqs[int(b["chr"])][int(b["start"]):int(b["end"])]
        if b["id"] < 0:
            s = s[::-1].translate(COMPLEMENT)
        frm, to = conventional(b)
        head = b'>Seq="%s",Strand=\'%s\',Block_id=%d,Start=%d,End=%d\n' % (names[int(b["chr"])].encode(), b"+" if b["id"] > 0 else b"-", abs(int(b["id"])), frm, to)
        out.append((abs(int(b["id"])), head + b"\n".join(s[i:i + 80] for i in range(0, len(s), 80)) + b"\n"))
    return out


def striped(name):
    tok = name.replace("|", " ").replace(".", " ").split()
    return tok[3] if len(tok) == 5 else name


def expected_gff_rows(blocks, names):
    out = []
    for b in blocks:
        frm, to = conventional(b)
        out.append((abs(int(b["id"])), b"%s\tSibelia\tsynteny_block_copy\t%d\t%d\t.\t%s\t.\t%d\n" % (
            striped(names[int(b["chr"])]).encode(), min(frm, to), max(frm, to), b"+" if b["id"] > 0 else b"-", abs(int(b["id"])))))
    return out


def check_grouped(got_records, id_of, want):
    ids = [id_of(r) for r in got_records]
    assert ids == sorted(w[0] for w in want), "ids must ascend, one record per instance"
    assert sorted(zip(ids, got_records)) == sorted(want)


def check_sequences(text, blocks, seqs, names):
    records = [r for r in re.split(rb"(?m)^(?=>)", text) if r]
    assert b"".join(records) == text
    check_grouped(records, lambda r: int(re.match(rb'>Seq="[^"]*",Strand=\'.\',Block_id=(\d+),', r).group(1)), expected_records(blocks, seqs, names))


def check_gff(text, blocks, names):
    assert text.startswith(GFF_HEAD)
    rows = text[len(GFF_HEAD):].splitlines(keepends=True)
    check_grouped(rows, lambda r: int(r.rstrip(b"\n").split(b"\t")[8]), expected_gff_rows(blocks, names))


def random_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


@pytest.fixture(scope="module")
def small():
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(11)
    seqs = [bytearray(random_seq(rng, n)) for n in (1000, 161, 3000)]
    for s in seqs:                                             # ambiguity codes, densely: reverse instances run over them
        for p in rng.choice(len(s), len(s) // 7, replace=False):
            s[int(p)] = b"NRYKMSWBDHX-U"[int(rng.integers(0, 13))]
    seqs[1][:6] = b"NRYACG"
    seqs[1][-6:] = b"TTYRNA"
    seqs = [bytes(s) for s in seqs]
    names = ["gi|15644634|ref|NC_000915.1|", "plain_name", "a.b.c"]
    bf = BlockFinder(seqs, device=0)
    yield bf, seqs, names
    bf.close()


def test_line_lengths_record_ends_overlaps_and_ambiguity_codes(small):
    bf, seqs, names = small
    rng = np.random.default_rng(5)
    rows, bid = [], 1
    for ln in (1, 79, 80, 81, 160, 161):
        for c, s in enumerate(seqs):
            for start in {0, len(s) - ln, int(rng.integers(0, len(s) - ln + 1))}:          # touching both ends of the record
                for sign in (1, -1):
                    rows.append((sign * bid, c, start, start + ln))
            bid += 1
    rows += [(bid, 0, 10, 400), (-bid, 0, 200, 700), (bid, 0, 10, 400), (bid, 0, 10, 400), (-bid, 0, 10, 400)]      # overlapping and identical
    rows += [(-(bid + 1), 1, 0, 161), (bid + 1, 1, 0, 161), (-(bid + 2), 1, 0, 6), (-(bid + 2), 1, 155, 161)]       # whole record; N R Y at both ends
    rows += [(bid + 3, 2, 17, 17), (-(bid + 3), 2, 3000, 3000)]                                                      # empty instances
    rows = [rows[i] for i in rng.permutation(len(rows))]
    blocks = blocks_of(rows)
    text = bf.blocks_sequences(blocks, names)
    check_sequences(text, blocks, seqs, names)
    assert b">Seq=\"plain_name\",Strand='-',Block_id=%d,Start=6,End=1\nCGTYRN\n" % (bid + 2) in text      # N, R, Y pass through unchanged
    check_gff(bf.blocks_gff(blocks, names), blocks, names)
    assert b"NC_000915\tSibelia\tsynteny_block_copy\t" in bf.blocks_gff(blocks, names)      # five tokens: the fourth
    assert b"a.b.c\tSibelia" in bf.blocks_gff(blocks, names)
    # without names: empty descriptions (sbl_load has none)
    check_sequences(bf.blocks_sequences(blocks), blocks, seqs, [""] * 3)


def test_random_lists_many_lengths(small):
    bf, seqs, names = small
    rng = np.random.default_rng(6)
    rows = []
    for _ in range(3000):
        c = int(rng.integers(0, 3))
        a, b = sorted(int(x) for x in rng.integers(0, len(seqs[c]) + 1, 2))
        if rng.random() < 0.5:
            b = min(b, a + int(rng.integers(0, 200)))
        rows.append((int(rng.integers(1, 40)) * int(rng.choice([-1, 1])), c, a, b))
    blocks = blocks_of(rows)
    check_sequences(bf.blocks_sequences(blocks, names), blocks, seqs, names)
    check_gff(bf.blocks_gff(blocks, names), blocks, names)


def test_empty_list(small):
    bf, seqs, names = small
    assert bf.blocks_sequences(blocks_of([]), names) == b""
    assert bf.blocks_gff(blocks_of([]), names) == GFF_HEAD


def test_hundred_thousand_tiny_instances(small):
    """Many pieces per workgroup span.  More pieces in a span than the kernel keeps on chip (ST_LDS = 256) cannot come from a block list:
    the shortest instance -- empty description, one base, one-digit id and positions -- is 44 bytes of header, the base and a line feed,
    46 bytes in two pieces, so a span of 4096 bytes holds at most 2 * 91 = 182.  The kernel's path through global memory is covered by
    tests/test_gpu_uncovered.py::test_more_pieces_in_one_span_than_the_kernel_keeps_on_chip."""
    bf, seqs, names = small
    rng = np.random.default_rng(7)
    n = 100_000
    chr_ = rng.integers(0, 3, n)
    ln = rng.integers(1, 4, n)
    start = np.array([rng.integers(0, len(seqs[c]) - l + 1) for c, l in zip(chr_, ln)])
    blocks = np.zeros(n, dtype=F.BLOCK_DTYPE)
    blocks["id"] = rng.integers(1, 5000, n) * rng.choice([-1, 1], n)
    blocks["chr"], blocks["start"], blocks["end"] = chr_, start, start + ln
    check_sequences(bf.blocks_sequences(blocks, names), blocks, seqs, names)


# ------------------------------------------------------------------------------------------ one mixed-case record

def head_len(bid, frm, to):
    return len(b'>Seq="m",Strand=\'+\',Block_id=%d,Start=%d,End=%d\n' % (bid, frm, to))


@pytest.fixture(scope="module")
def mixed():
    """One record of 256 bases, as record 0: base s is element 1 + s on the device.  Mixed case, ambiguity codes sprinkled in."""
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(12)
    seq = bytearray(np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, 256)].tobytes())
    for p in rng.choice(256, 40, replace=False):
        seq[int(p)] = b"NnRrYykMsW"[int(rng.integers(0, 10))]
    seq[:7] = b"aacgNry"
    seq = bytes(seq)
    bf = BlockFinder([seq], device=0)
    yield bf, [seq], ["m"]
    bf.close()


def record_len(bid, start, end, fwd):
    frm, to = (start + 1, end) if fwd else (end, start + 1)
    ln = end - start
    return head_len(bid, frm, to), head_len(bid, frm, to) + ln + ((ln - 1) // 80 if ln else 0) + 1


def with_fillers(wanted, rows=()):
    """wanted: (sign, start, end, residue) per tested instance; rows: instances that come first.  -> rows with ids ascending in list order
    (the unstable sort has nothing to reorder), every tested instance after one filler instance [0, f) whose length f in 1 .. 40 brings
    the first byte after the tested instance's header to `residue` mod 16 in the text."""
    rows = list(rows)
    at = sum(record_len(abs(bid), a, b, bid > 0)[1] for bid, _, a, b in rows)
    for sign, start, end, residue in wanted:
        bid = len(rows) + 1
        head, whole = record_len(bid + 1, start, end, sign > 0)
        f = next(f for f in range(1, 41) if (at + record_len(bid, 0, f, True)[1] + head) % 16 == residue)
        rows += [(bid, 0, 0, f), (sign * (bid + 1), 0, start, end)]
        at += record_len(bid, 0, f, True)[1] + whole
    return rows


def expected_text(rows, seqs, names):
    """-> the text, and per instance the offsets of the first byte after its header and of its last byte"""
    records = [r for _, r in expected_records(blocks_of(rows), seqs, names)]
    ends = np.cumsum([len(r) for r in records])
    return b"".join(records), [int(e) - len(r) + r.index(b"\n") + 1 for e, r in zip(ends, records)], [int(e) - 1 for e in ends]


LENGTHS = (1, 15, 16, 17, 79, 80, 81, 96, 97, 161)


def test_an_instance_at_every_source_and_output_alignment_on_both_strands(mixed):
    """What tests/test_gpu_uncovered.py::test_a_range_at_every_source_and_output_alignment asserts on forward pieces: the 16-byte windows
    at an instance's first and last bases, read upwards and downwards, cut from every source alignment and stored at every output
    alignment; lengths around the piece and the line, and 15 bases before the final line feed."""
    bf, seqs, names = mixed
    wanted = [(sign, start, start + ln, dst) for sign in (1, -1) for ln in LENGTHS for start in range(16) for dst in range(16)]
    rows = with_fillers(wanted)
    text, body, _ = expected_text(rows, seqs, names)
    seen = {}
    for (sign, start, end, _), at in zip(wanted, body[1::2]):
        seen.setdefault((sign, end - start), set()).add((start % 16, at % 16))
    assert len(seen) == 2 * len(LENGTHS) and all(len(v) == 256 for v in seen.values())      # on the inputs: every pair occurs
    assert len(rows) == 2 * 2 * len(LENGTHS) * 256
    assert bf.blocks_sequences(blocks_of(rows), names) == text


def test_the_case_is_kept_and_spell_text_still_upper_cases_on_the_same_finder(mixed):
    bf, seqs, names = mixed
    ranges = [(0, 7), (0, 256), (3, 200), (17, 33), (40, 41), (100, 256)]
    rows = [(sign * (2 * i + (sign < 0) + 1), 0, a, b) for i, (a, b) in enumerate(ranges) for sign in (1, -1)]
    text, _, _ = expected_text(rows, seqs, names)
    assert b"End=7\naacgNry\n" in text and b"End=1\nyrNcgtt\n" in text          # a <-> t, c <-> g in their case; N, r, y as they are
    first = bf.blocks_sequences(blocks_of(rows), names)
    assert first == text
    pieces = np.array([(1, 0, a, b, 80, 0) for a, b in ranges], dtype=F.PIECE_DTYPE)
    kept = b"".join(seqs[0][o:min(o + 80, b)] + b"\n" for a, b in ranges for o in range(a, b, 80))
    assert bf.spell_text(pieces) == kept.upper() and kept != kept.upper()
    assert bf.blocks_sequences(blocks_of(rows), names) == first      # the two share their device buffers and the staging buffer


def test_empty_instances_at_the_ends_of_the_text_and_of_a_16_byte_piece(mixed):
    """An instance without bases is its header and one line feed: first in the text, last in the text, and with the line feed as the
    last (15) and as the first (0) byte of a lane's 16 bytes."""
    bf, seqs, names = mixed
    rows = with_fillers([(1, 5, 5, 15), (-1, 256, 256, 0), (1, 0, 0, 15), (-1, 9, 9, 0)], [(1, 0, 0, 0)])
    rows.append((-(len(rows) + 1), 0, 256, 256))
    text, body, last = expected_text(rows, seqs, names)
    empty = [i for i, r in enumerate(rows) if r[2] == r[3]]
    assert empty == [0, 2, 4, 6, 8, 9] and all(body[i] == last[i] and text[last[i] - 1:last[i] + 1] == b"\n\n" for i in empty)
    assert text.startswith(b">Seq=\"m\",Strand='+',Block_id=1,Start=1,End=0\n\n>") and text.endswith(b",Start=256,End=257\n\n")
    assert [last[i] % 16 for i in empty[1:5]] == [15, 0, 15, 0]
    assert bf.blocks_sequences(blocks_of(rows), names) == text


def test_whole_records_of_4_6_mbp():
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(8)
    seqs = [random_seq(rng, 4_600_000), random_seq(rng, 4_600_001)]
    names = ["first", "second"]
    bf = BlockFinder(seqs, device=0)
    blocks = blocks_of([(1, 0, 0, len(seqs[0])), (-1, 1, 0, len(seqs[1])), (-2, 0, 0, len(seqs[0])), (2, 1, 0, len(seqs[1])), (3, 1, 1, len(seqs[1]) - 1)])
    text = bf.blocks_sequences(blocks, names)
    check_sequences(text, blocks, seqs, names)
    bf.close()


@pytest.mark.parametrize("row", [(0, 0, 1, 5), (1, 3, 1, 5), (1, 0, 5, 4), (1, 1, 100, 162), (-1, 0, 0, 1001)])
def test_bad_block_lists_are_bad_arguments(small, row):
    from sibelia_amd import SibeliaError
    bf, seqs, names = small
    for fn in (bf.blocks_sequences, bf.blocks_gff):
        with pytest.raises(SibeliaError, match="bad argument"):
            fn(blocks_of([(1, 0, 0, 10), row]), names)


def test_no_records_loaded_is_a_bad_argument():
    import ctypes as C
    from sibelia_amd import load_library
    L = load_library()
    h = C.c_void_p()
    assert L.sbl_create(C.byref(h), 0) == 0
    b = blocks_of([(1, 0, 0, 0)])
    t, n = C.c_void_p(), C.c_uint64()
    for fn in (L.sbl_blocks_sequences, L.sbl_blocks_gff):
        assert fn(h, b.ctypes.data, 1, None, C.byref(t), C.byref(n)) == 1          # SBL_ERR_BAD_ARG
        assert b"no records loaded" in L.sbl_last_error(h)
    L.sbl_destroy(h)


@pytest.fixture(scope="module")
def strains():
    return W.gen_strains(L0=60_000, n=3, seed=3, inv_min=2000, inv_max=6000)


def test_explicit_list_equals_the_context_list_after_generate_blocks(strains):
    from sibelia_amd import BlockFinder
    names = ["s0", "s1", "s2"]
    bf = BlockFinder(strains, device=0)
    bf.PerformGraphSimplifications(25, 150, 4)
    blocks = bf.GenerateSyntenyBlocks(25, 25, 500)
    assert len(blocks) > 10
    assert bf.blocks_sequences(None, names) == bf.blocks_sequences(blocks, names)
    assert bf.blocks_gff(None, names) == bf.blocks_gff(blocks, names)
    check_sequences(bf.blocks_sequences(None, names), blocks, strains, names)
    glued, _ = bf.postprocess(names)
    check_sequences(bf.blocks_sequences(None, names), glued, strains, names)
    check_gff(bf.blocks_gff(None, names), glued, names)
    bf.close()


def test_sharded_finder_gives_the_same_reports(strains):
    from sibelia_amd import BlockFinder
    from sibelia_amd.dist import LocalShardedFinder
    names = ["s0", "s1", "s2"]
    one, two = BlockFinder(strains, device=0), LocalShardedFinder(strains, [0, 0])
    assert one.PerformGraphSimplifications(25, 150, 4) == two.PerformGraphSimplifications(25, 150, 4)
    a, b = one.GenerateSyntenyBlocks(25, 25, 500), two.generate_blocks(25, 25, 500)
    assert np.array_equal(a, b) and len(a) > 10
    assert two.blocks_sequences(None, names) == one.blocks_sequences(None, names)
    assert two.blocks_sequences(a[::-1], names) == one.blocks_sequences(a[::-1], names)
    assert two.blocks_gff(None, names) == one.blocks_gff(None, names)
    one.close()
    two.close()


def test_two_input_files_equal_the_same_records_in_one_file(strains, tmp_path):
    from sibelia_amd import pipeline as P
    names = ["strainA", "strainB", "strainC"]
    W.write_fasta(str(tmp_path / "all.fa"), strains, names)
    W.write_fasta(str(tmp_path / "first.fa"), strains[:1], names[:1])
    W.write_fasta(str(tmp_path / "rest.fa"), strains[1:], names[1:])
    args = ["-s", "fine", "-r", "-q", "--gff", "-m", "500", "-o", str(tmp_path / "out")]
    rc1, files1, text1 = P.run(args + [str(tmp_path / "all.fa")])
    rc2, files2, text2 = P.run(args + [str(tmp_path / "first.fa"), str(tmp_path / "rest.fa")])
    assert rc1 == rc2 == 0 and text1 == text2
    assert files1 == files2
    assert files1["blocks_sequences.fasta"].count(b">") > 10 and files1["blocks_coords.gff"].count(b"\n") > 13
    assert not os.path.exists(str(tmp_path / "out"))             # run() returns the files; only the command line writes them
