"""The device FASTA loader (csrc/fasta_load.hip, sbl_load_fasta) at its tile edges, against the reference's FASTAReader.

tests/fasta_cases.py builds the texts: newlines, CRLF, blanks and headers on the 16-byte, 1024-byte and 4096-byte boundaries of the
line splitter, more than 256 lines per block of the line kernels, errors in different chunks, a column and a line index beyond 2^24.
tests/golden/fasta_limits.json holds what the UNMODIFIED reference reader made of each (tests/golden/gen/make_fasta_limits_golden.py);
for the 64 random texts the expected result comes from tests/fasta_model.py, which tests/test_fasta_model.py holds to the reference.
Then the ambiguity list (k_amb_flags / k_amb_write) across chunk and block boundaries, checked through the rand() stream of one stage
against the oracle, and a context that is loaded again and again."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import fasta_cases as F
from tests import fasta_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "fasta_limits.json")))["cases"]


def first_difference(got, model):
    """for the message of a failed comparison by digest: where the loaded records first differ from the model's reading of the text"""
    if isinstance(model, bytes) or len(got) != len(model):
        return "%d records loaded; the model reads %s" % (len(got), model if isinstance(model, bytes) else "%d records" % len(model))
    for r, ((n, s), (mn, ms)) in enumerate(zip(got, model)):
        if n != mn:
            return "record %d: name %r, the model reads %r" % (r, n[:80], mn[:80])
        if s != ms:
            at = next((i for i, (x, y) in enumerate(zip(s, ms)) if x != y), min(len(s), len(ms)))
            return "record %d (%r): lengths %d / %d, first difference at base %d: %r, the model reads %r" % (r, n[:80], len(s), len(ms), at, s[at:at + 20], ms[at:at + 20])
    return "the loaded records equal the model's: the model differs from the fixture"


def check_load(text, want, small, tmp_path):
    """want: the reader's message as bytes with <file> for the path, or its result as tests/fasta_cases.fixture_result puts it: the records
    whole (small) or by length and sha256"""
    from sibelia_amd import BlockFinder, SibeliaError
    fa = str(tmp_path / "in.fa")
    with open(fa, "wb") as f:
        f.write(text)
    if isinstance(want, bytes):
        with pytest.raises(SibeliaError) as ei:
            BlockFinder.from_fasta(fa, device=0)
        got = str(ei.value).encode("utf-8", "surrogateescape")
        assert want.replace(b"<file>", os.fsencode(fa)) + b")" in got, got[-200:]      # the WHOLE message: nothing follows it but the bracket of SibeliaError
        return
    bf = BlockFinder.from_fasta(fa, device=0)
    try:
        seqs, pos = bf.state()
        got = list(zip([n.encode() for n in bf.record_names()], seqs))
        assert F.fixture_result(got, small) == want, first_difference(got, M.parse(text))
        assert [len(s) for s in seqs] == bf.record_sizes()
        assert all(np.array_equal(p, np.arange(len(s), dtype=np.uint32)) for s, p in zip(seqs, pos))      # originalPos_ = identity
    finally:
        bf.close()


@pytest.mark.parametrize("name", list(F.CASES))
def test_crafted_text_loads_as_the_reference_reads_it(name, tmp_path):
    case = GOLD[name]
    want = case["error"].encode("latin1") if "error" in case else F.result_keys(case)
    check_load(F.text(name), want, "text_b64" in case, tmp_path)


@pytest.mark.parametrize("i", range(F.RANDOM_COUNT))
def test_random_text_loads_as_the_model_reads_it(i, tmp_path):
    text = F.random_text(i)
    want = M.parse(text)
    check_load(text, want if isinstance(want, bytes) else F.fixture_result(want, True), True, tmp_path)      # every byte of every record


# ---- the ambiguity list
@pytest.fixture(scope="module")
def amb_oracle():
    from oracle.oracle import Oracle
    recs = F.amb_records()
    orc = Oracle(recs)
    bulges = orc.simplify_stage(25, 150, 1)
    seqs, pos = orc.state()
    orc.close()
    return recs, bulges, seqs, pos


@pytest.mark.parametrize("way", ["from_fasta", "in_memory"])
def test_ambiguity_list_across_chunks_and_blocks_feeds_rand_in_the_reference_order(way, amb_oracle, tmp_path):
    # the codes of fasta_cases.amb_plan() are replaced by rand() letters in element order at the head of the stage: one position out of
    # order, lost or doubled shifts the stream and shows in every letter replaced after it
    from sibelia_amd import BlockFinder, workloads as W
    recs, bulges, want_seqs, want_pos = amb_oracle
    if way == "from_fasta":
        fa = str(tmp_path / "amb.fa")
        W.write_fasta(fa, recs, width=97)                      # lines that are no multiple of anything
        bf = BlockFinder.from_fasta(fa, device=0)
    else:
        bf = BlockFinder(recs, device=0)
    try:
        assert bf.state()[0] == recs
        assert bf.simplify_stage(25, 150, 1) == bulges
        seqs, pos = bf.state()
        planted = [e for e, _ in F.amb_plan()]
        assert bulges == 0                                      # random sequence has no bulges (the oracle is the witness): the records keep their lengths
        got = b"$" + b"$".join(seqs) + b"$"
        assert all(got[e] in b"ACGT" for e in planted) and [i for i, c in enumerate(got) if c == 36] == F.amb_seps()
        assert seqs == want_seqs and all(np.array_equal(x, y) for x, y in zip(pos, want_pos))
    finally:
        bf.close()


# ---- one context, loaded again and again: everything it reports belongs to the last load
def test_reloading_a_context_leaves_nothing_of_the_load_before(tmp_path):
    from sibelia_amd import api
    L = api.load_library()
    texts = {"bad": b">x\nACGT\n>y\nAC?T\n>z\nGG\n",
             "three": b">one a\nACGT\nNN\n>two\nGGCC\n>three\nT\n",
             "one": b">single\n" + F.dna(5000, 90) + b"\nAC\n"}
    assert len(texts["one"]) > len(texts["three"]) and texts["one"].count(b"\n") < texts["three"].count(b"\n")
    paths = {}
    for k, t in texts.items():
        paths[k] = str(tmp_path / (k + ".fa"))
        with open(paths[k], "wb") as f:
            f.write(t)
    h = C.c_void_p()
    assert L.sbl_create(C.byref(h), 0) == 0
    bf = api.BlockFinder.__new__(api.BlockFinder)              # the Python surface over THIS context (state(), record_names())
    bf.L, bf.h = L, h
    try:
        for step in ("bad", "three", "one", "bad", "three"):
            rc = L.sbl_load_fasta(h, os.fsencode(paths[step]))
            want = M.parse(texts[step])
            if isinstance(want, bytes):
                assert rc == 1                                  # SBL_ERR_BAD_ARG
                assert L.sbl_last_error(h) == want.replace(b"<file>", os.fsencode(paths[step]))
                # a text that does not parse leaves no records behind, and certainly not those of the load before
                assert L.sbl_nchr(h) == 0 and L.sbl_record_name(h, 0) == b"" and L.sbl_record_size(h, 0) == 0
                assert L.sbl_get_state(h, 0, None, None, None) != 0
                continue
            assert rc == 0
            assert L.sbl_last_error(h) == b""                   # ... nor the message of the failed load, or of the failed call, before it
            assert L.sbl_nchr(h) == len(want)
            assert [L.sbl_record_name(h, i) for i in range(len(want) + 2)] == [n for n, _ in want] + [b"", b""]
            assert [L.sbl_record_size(h, i) for i in range(len(want) + 2)] == [len(s) for _, s in want] + [0, 0]
            seqs, pos = bf.state()
            assert seqs == [s for _, s in want] and all(np.array_equal(p, np.arange(len(s), dtype=np.uint32)) for s, p in zip(seqs, pos))
            assert L.sbl_get_state(h, len(want), None, None, None) != 0
    finally:
        bf.close()
