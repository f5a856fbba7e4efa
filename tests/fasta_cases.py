"""Crafted inputs for the device FASTA loader (csrc/fasta_load.hip), in the manner of tests/tiny_index_cases.py: every text is built
in pure Python from a short recipe and carries the precondition that makes it a test of the edge it is named after (the byte offset
its newline lands on, the line index of its header, ...).  tests/test_fasta_model.py runs the preconditions without a GPU;
tests/golden/gen/make_fasta_limits_golden.py runs the unmodified reference reader on every text (tests/golden/fasta_limits.json);
tests/test_gpu_fasta_limits.py loads every text on the device.

Geometry of the loader: the line splitter (k_fa_count_nl / k_fa_line_starts) reads 16 bytes per thread, 1024 per wave and
FA_CHUNK = 4096 per block; k_fa_lines / k_fa_place take 256 lines per block; k_fa_scatter 256 bytes per block; the ambiguity list
(k_amb_flags / k_amb_write) 1024 elements per chunk and 256 chunks per block."""
import hashlib
import random
from collections import namedtuple

THREAD, WAVE, CHUNK, LINES, SCATTER = 16, 1024, 4096, 256, 256
AMB_CHUNK, AMB_BLOCK = 1024, 256
SMALL_MAX = 1024                            # texts up to this size are stored whole in the fixture, with their full result; longer ones by digest
RECORDS_MAX = 8                             # a digested result lists its records up to this many; beyond, one digest over all of them
BLANKS = b" \t\n\r\x0b\x0c"

_ACGT = bytes(b"ACGT"[i & 3] for i in range(256))
_MIXED = bytes(b"ACGTacgt"[i & 7] for i in range(256))

Case = namedtuple("Case", "build pre")
CASES = {}


def dna(n, seed=0, mixed=False):
    """n pseudo-random bases (a hash stream: the same bytes on every Python), upper case or mixed case"""
    return hashlib.shake_256(b"fasta_cases %d" % seed).digest(n).translate(_MIXED if mixed else _ACGT)


def records_digest(records):
    """one sha256 over the names and the sequences of [(name, sequence)], in order"""
    h = hashlib.sha256()
    for name, seq in records:
        h.update(b"%d %d\n" % (len(name), len(seq)))
        h.update(name)
        h.update(seq)
    return h.hexdigest()


def fixture_result(got, small):
    """what the fixture keeps of a reader's result: got is the message (bytes) or [(name, sequence)].  Names and messages are kept as
    latin-1 text, one code point per byte"""
    if isinstance(got, bytes):
        return {"error": got.decode("latin1")}
    if small:
        return {"records": [{"name": n.decode("latin1"), "seq": s.decode("latin1")} for n, s in got]}
    if len(got) <= RECORDS_MAX:
        return {"records": [{"name": n.decode("latin1"), "len": len(s), "sha256": hashlib.sha256(s).hexdigest()} for n, s in got]}
    return {"nrecords": len(got), "bases": sum(len(s) for _, s in got), "records_sha256": records_digest(got)}


def result_keys(entry):
    return {k: v for k, v in entry.items() if not k.startswith("text_")}


def case(fn):
    """registers a case: fn returns (text, pre) or just the text; pre(text) asserts what the case relies on"""
    CASES[fn.__name__] = Case(lambda: _made(fn)[0], lambda: _made(fn)[1](_made(fn)[0]))
    return fn


_cache = {}


def _made(fn):
    """(text, pre) of a case, built once per process (the largest texts are 17 MB and 34 MB)"""
    if fn.__name__ not in _cache:
        r = fn()
        _cache[fn.__name__] = r if isinstance(r, tuple) else (r, lambda t: None)
    return _cache[fn.__name__]


def text(name):
    return CASES[name].build()


def newlines(t):
    return [i for i, c in enumerate(t) if c == 10]


def chunk_of(off):
    return off // CHUNK


def line_index(t, off):
    return t.count(b"\n", 0, off)


def with_newlines_at(total, offsets, seed, first=b""):
    """`total` bytes of sequence that start with `first` and have a newline at exactly the given offsets"""
    t = bytearray(first + dna(total - len(first), seed, mixed=True))
    for o in offsets:
        t[o] = 10
    return bytes(t)


# ---- newlines on every boundary
NL_OFFSETS = (15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)


@case
def newline_on_every_boundary():
    t = with_newlines_at(8192 + 40, NL_OFFSETS, 1, first=b">boundaries_001")      # the header is the 15 bytes ahead of the first newline

    def pre(t):
        assert tuple(newlines(t)) == NL_OFFSETS and t[:1] == b">" and not t.endswith(b"\n")
        assert {o % THREAD for o in NL_OFFSETS} == {15, 0, 1} and {o % WAVE for o in NL_OFFSETS[3:]} == {1023, 0, 1}
        assert {o % CHUNK for o in NL_OFFSETS[6:]} == {4095, 0, 1}
    return t, pre


@case
def crlf_across_chunks():
    t = bytearray(with_newlines_at(4096 + 300, (2, 2000, 4096, 4200), 2, first=b">r"))
    t[4095] = 13

    def pre(t):
        assert t[4095:4097] == b"\r\n" and chunk_of(4095) == 0 and chunk_of(4096) == 1
    return bytes(t), pre


# ---- end of file at a boundary
def _eof(total, final_newline):
    def build():
        offs = list(range(3 + 100, total - 1, 101))
        t = bytearray(with_newlines_at(total, [2] + offs, 3 + total, first=b">r"))
        if final_newline:
            t[total - 1] = 10
        if t[total - 2] == 10:                 # keep the last line non-empty
            t[total - 2] = ord("A")

        def pre(t):
            assert len(t) == total and (t[-1:] == b"\n") == final_newline and t[-2:-1] != b"\n"
        return bytes(t), pre
    build.__name__ = "eof_at_%d_%s" % (total, "newline" if final_newline else "bare")
    return case(build)


for _n in (4096, 4097, 8192):
    for _f in (True, False):
        _eof(_n, _f)


@case
def eof_last_line_blank_no_newline():
    t = b">r\n" + dna(4085, 4) + b"\n" + b" \t \x0b\x0c \r  \t  "

    def pre(t):
        last = t[t.rindex(b"\n") + 1:]
        assert last and not last.strip(BLANKS) and chunk_of(t.rindex(b"\n")) == 0 and chunk_of(len(t) - 1) == 1
    return t, pre


# ---- blanks that span chunks
@case
def blank_line_of_9000():
    t = b">r\nACGT\n" + b" \t" * 4500 + b"\nGGCC\n>s\nTT\n"

    def pre(t):
        a = t.index(b"\n", 3) + 1
        b = t.index(b"\n", a)
        assert b - a == 9000 and not t[a:b].strip(b" \t") and chunk_of(b) - chunk_of(a) == 2
    return t, pre


@case
def blanks_around_acgt():
    t = b">r\n" + b" \t \t " * 1000 + b"ACGT" + b"\t  \t " * 1000 + b"\nTTGA\n"

    def pre(t):
        at = t.index(b"ACGT")
        assert at == 5003 and chunk_of(3) == 0 and chunk_of(at) == 1 and chunk_of(t.index(b"\n", at)) == 2
    return t, pre


@case
def err_inner_vertical_tab():
    return b"\x0b>r\x0c x\n\x0b\x0cACGT\x0c\x0b\n\x0b\n\x0c\n\x0cGG\x0b\r\n \x0b>s\nT\x0bT\n"      # ... and an inner \v is an illegal character


@case
def vertical_tab_and_form_feed_ok():
    return b"\x0b>r\x0c x\n\x0b\x0cACGT\x0c\x0b\n\x0b\n\x0c\n\x0cGG\x0b\r\n \x0b>s\nTT\x0b\n"


# ---- a chunk that is all newlines
@case
def chunk_of_newlines():
    t = b">r\n" + dna(4000, 5) + b"\n" * 4200 + dna(8300, 6) + b"\nACGT\n\n\nAC!T\nGG\n"

    def pre(t):
        assert t[CHUNK:2 * CHUNK] == b"\n" * CHUNK and b"\n" * 4200 in t and b"\n" * 4201 not in t
        assert b"\n" not in t[3 * CHUNK:4 * CHUNK]
        assert line_index(t, t.index(b"!")) > 4200      # raw line index; the message counts 5 non-empty lines
    return t, pre


# ---- many lines
def _one_base_lines(n, seed):
    return b"\n".join(bytes([c]) for c in dna(n, seed)) + b"\n"


def _many(h):
    def build():
        # 70 000 one-base lines in three records; the second header on line index h, the third 199 line blocks further on
        h2 = h + 199 * LINES
        body = _one_base_lines(70_000, 7)
        t = b">a\n" + body[:2 * (h - 1)] + b">b\n" + body[2 * (h - 1):2 * (h2 - 2)] + b">c\n" + body[2 * (h2 - 2):]

        def pre(t):
            lines = t.split(b"\n")
            assert len(lines) == 70_004 and [i for i, x in enumerate(lines) if x[:1] == b">"] == [0, h, h2]
            assert all(len(x) == 1 for i, x in enumerate(lines[:-1]) if i not in (0, h, h2))
        return t, pre
    build.__name__ = "many_lines_header_at_%d" % h
    return case(build)


for _h in (255, 256, 257):
    _many(_h)


@case
def many_lines_three_headers_in_a_row():
    # headers on line indices 255, 256 and 257 -- the last thread of one line block and the first two of the next.  The 255 lines ahead
    # of the first header join its record, so the second header is fine and the THIRD meets an empty sequence.
    body = _one_base_lines(70_000, 8)
    t = body[:2 * 255] + b">a\n>b\n>c\n" + body[2 * 255:]

    def pre(t):
        lines = t.split(b"\n")
        assert [i for i, x in enumerate(lines) if x[:1] == b">"] == [255, 256, 257] and len(lines) == 70_004
    return t, pre


@case
def five_thousand_records():
    rng = random.Random(11)
    out = [b"ACG\n", b"\n", b"tt\n"]                       # two sequence lines ahead of the first header
    for i in range(5000):
        out.append(b">rec%d%s\n" % (i, b" d" if rng.random() < 0.3 else b""))
        if rng.random() < 0.4:
            out.append(b"\n" if rng.random() < 0.5 else b" \t\r\n")
        n = 1 + int(rng.random() * 9)
        s = dna(n, 100 + i, mixed=True)
        cut = int(rng.random() * n)
        if 0 < cut and rng.random() < 0.5:
            out += [s[:cut] + b"\n", b"\n" if rng.random() < 0.3 else b"", s[cut:] + b"\n"]
        else:
            out.append(s + b"\n")
    t = b"".join(out)

    def pre(t):
        assert t.count(b">") == 5000 and t.count(b"\n\n") > 300 and t.count(b"\n") > 20 * LINES
    return t, pre


# ---- long headers
@case
def header_name_of_5000():
    name = dna(5000, 12).replace(b"A", b"n").replace(b"C", b"|")
    t = b">a\nAC\n>" + name + b"\nACGT\n>c\nG\n"

    def pre(t):
        a = t.index(name)
        assert chunk_of(a) == 0 and chunk_of(a + 4999) == 1 and b" " not in name
    return t, pre


@case
def header_description_of_6000():
    desc = b" ".join(dna(11, 200 + i) for i in range(501))
    t = b">name" + b"  " + desc + b" \nACGT\n>b x\nGG\n"

    def pre(t):
        assert len(desc) >= 6000 and chunk_of(t.index(b"\n")) == 1
    return t, pre


@case
def header_starts_on_last_byte_of_chunk():
    t = b">a\n" + dna(4091, 13) + b"\n>b desc\nGG\n"

    def pre(t):
        assert t[4095:4098] == b">b " and t[4094:4095] == b"\n"
    return t, pre


@case
def tab_is_not_the_name_delimiter():
    return b">a\tb\nACGT\n>c\td e\nGG\n"


# ---- error order across tiles
def _rows(*rows):
    return b"".join(r + b"\n" for r in rows)


def _dna_rows(n, seed):
    return [dna(1000, seed + i) for i in range(n)]


@case
def err_empty_header_then_illegal():
    bad = bytearray(dna(1000, 30))
    bad[500] = ord("Z")
    t = _rows(b">r", *_dna_rows(5, 14), b">", *_dna_rows(7, 20), bytes(bad))

    def pre(t):
        assert chunk_of(t.index(b"\n>\n") + 1) == 1 and chunk_of(t.index(b"Z")) == 3
    return t, pre


@case
def err_illegal_then_empty_header():
    bad = bytearray(dna(1000, 31))
    bad[500] = ord("Z")
    t = _rows(b">r", *_dna_rows(5, 14), bytes(bad), *_dna_rows(7, 20), b">")

    def pre(t):
        assert chunk_of(t.index(b"Z")) == 1 and chunk_of(t.index(b"\n>\n") + 1) == 3
    return t, pre


@case
def err_two_illegal_on_one_line():
    t = b">r\nACGT\n" + dna(100, 32) + b"Z" + dna(5999, 33) + b"!" + dna(100, 34) + b"\n"

    def pre(t):
        z, e = t.index(b"Z"), t.index(b"!")
        assert e - z == 6000 and line_index(t, z) == line_index(t, e) == 2 and b"!" < b"Z" and chunk_of(z) < chunk_of(e)
    return t, pre


def _empty_sequence_in_chunk_2(bad_row):
    rows = [b">r"] + _dna_rows(9, 40) + [b">e", b">f"] + _dna_rows(5, 50)
    bad = bytearray(rows[bad_row])
    bad[700] = ord("J")
    rows[bad_row] = bytes(bad)
    return _rows(*rows)


@case
def err_illegal_before_empty_sequence():
    t = _empty_sequence_in_chunk_2(2)

    def pre(t):
        assert chunk_of(t.index(b">f")) == 2 and chunk_of(t.index(b"J")) == 0
    return t, pre


@case
def err_empty_sequence_before_illegal():
    t = _empty_sequence_in_chunk_2(16)

    def pre(t):
        assert chunk_of(t.index(b">f")) == 2 and chunk_of(t.index(b"J")) == 3
    return t, pre


@case
def err_empty_sequence_after_300_blank_lines():
    t = b">a\nACGT\n>b\n" + b"\n \n\t\r\n" * 100

    def pre(t):
        assert t.count(b"\n", t.index(b">b")) == 301 and not t[t.index(b">b") + 2:].strip(BLANKS)
    return t, pre


@case
def err_illegal_high_byte():
    return b">r\nACGT\nAC\xe9GT\xff\n"


@case
def err_illegal_high_byte_0x80():
    return b">r\n" + dna(4093, 60) + b"\x80" + b"ACGT\n"


# ---- large cases: the error record beyond 24 bits of column and of line index
WIDE = 1 << 24


@case
def wide_column():
    line = bytearray(b"ACGT" * ((WIDE + 4096) // 4))
    line[WIDE + 10] = ord("Z")
    line[WIDE + 2000] = ord("!")
    t = b">r\n" + bytes(line) + b"\n"

    def pre(t):
        assert t.index(b"Z") - 3 == WIDE + 10 and t.index(b"!") - 3 == WIDE + 2000 and t.count(b"\n") == 2 and len(t) == WIDE + 4096 + 4
    return t, pre


def _late(q, bang, header):
    def build():
        # line index 0 is the header; line index i >= 1 starts at byte 3 + 2 * (i - 1)
        t = bytearray(b">r\n" + b"A\n" * (WIDE + 8))
        if q:
            t[3 + 2 * (WIDE - 5 - 1)] = ord("Q")
        if bang:
            t[3 + 2 * (WIDE + 3 - 1)] = ord("!")
        if header:
            at = 3 + 2 * (WIDE + 2 - 1)
            t[at:at] = b">s\n"
        t = bytes(t)

        def pre(t):
            assert t.count(b"\n") == WIDE + 9 + (1 if header else 0)
            assert (line_index(t, t.index(b"Q")) == WIDE - 5) if q else b"Q" not in t
            assert (line_index(t, t.index(b"!")) == WIDE + 3) if bang else b"!" not in t
            assert (line_index(t, t.index(b">s")) == WIDE + 2) if header else t.count(b">") == 1
        return t, pre
    return build


for _name, _args in (("late_line", (True, True, False)), ("late_line_only", (False, True, False)), ("late_line_ok", (False, False, True))):
    _b = _late(*_args)
    _b.__name__ = _name
    case(_b)

LARGE = ("wide_column", "late_line", "late_line_only", "late_line_ok")


# ---- random texts: the expected result of these comes from tests/fasta_model.py
RANDOM_SEED, RANDOM_COUNT, RANDOM_MAX = 20330, 64, 12 * 1024
_CODES = b"ACGTURYKMSWBDHNX-"


def random_text(i):
    rng = random.Random(RANDOM_SEED * 1000 + i)
    ri = lambda a, b: a + int(rng.random() * (b - a + 1))      # noqa: E731  (random() only: the same stream on every Python)
    pick = lambda s: s[int(rng.random() * len(s))]             # noqa: E731
    eol = lambda: b"\r\n" if rng.random() < 0.25 else b"\n"    # noqa: E731
    pad = lambda: bytes(pick(b" \t\x0b\x0c ") for _ in range(ri(0, 3) if rng.random() < 0.3 else 0))      # noqa: E731

    def seqline():
        n = pick((0, 1, 2, 15, 16, 17, 59, 60, 61, 255, 256, 257, 1023, 1024, ri(0, 5000), ri(0, 300), ri(0, 300)))
        s = bytearray(dna(n, ri(0, 1 << 30), mixed=True))
        for _ in range(ri(0, 4) if n else 0):
            c = pick(_CODES)
            s[ri(0, n - 1)] = c if rng.random() < 0.5 else bytes([c]).lower()[0]
        return bytes(s)

    out, size = [], 0
    faults = ri(1, 2) if rng.random() < 0.3 else 0
    nparts = ri(3, 40)
    fault_at = sorted(ri(0, nparts - 1) for _ in range(faults))
    for p in range(nparts):
        r = rng.random()
        if p in fault_at:
            kind = rng.random()
            if kind < 0.3:
                part = pad() + pick((b">", b"> x", b">  y z")) + pad() + eol()
            elif kind < 0.5:
                part = pad() + b">bare" + eol()             # a header without its sequence: an empty sequence if a header or the end follows
            else:
                s = bytearray(seqline() or b"A")
                s[ri(0, len(s) - 1)] = pick(b"ZJ!*.>0 \x01\x7f\x80\xff@[`{eEfFiIlLoOpPqQzZ")
                part = pad() + bytes(s) + pad() + eol()
        elif r < 0.25 or (p == 0 and r < 0.8):
            name = bytes(pick(b"abcXYZ019|_.-\t>") for _ in range(ri(1, 12)))
            desc = b"".join(b" " + bytes(pick(b"de f=1\t") for _ in range(ri(0, 9))) for _ in range(ri(0, 3))) if rng.random() < 0.5 else b""
            part = pad() + b">" + name + desc + pad() + eol() + pad() + (seqline() or b"N") + pad() + eol()      # never an empty record by accident
        elif r < 0.4:
            part = pad() + eol()
        else:
            part = pad() + seqline() + pad() + eol()
        if size + len(part) > RANDOM_MAX:
            break
        out.append(part)
        size += len(part)
    t = b"".join(out)
    if rng.random() < 0.3:
        t = t.rstrip(b"\r\n")
    return t or b"ACGT"


def random_texts():
    return [random_text(i) for i in range(RANDOM_COUNT)]


# ---- the ambiguity list: three records of random ACGT with codes planted by ELEMENT position ('$' c0 '$' c1 '$' c2 '$')
AMB_LENGTHS = (100_003, 99_991, 100_010)


def amb_seps():
    seps, e = [0], 0
    for n in AMB_LENGTHS:
        e += n + 1
        seps.append(e)
    return seps


def amb_plan():
    """[(element position, code)] ascending: what is planted, and hence the order in which rand() replaces"""
    seps = amb_seps()
    nelem = seps[-1] + 1
    last = (nelem - 1) // AMB_CHUNK
    plan = {1023: "N", 1024: "R", 1025: "Y"}
    for s, before, after in zip(seps, "KMSW", "BDHX"):
        if s > 0:
            plan[s - 1] = before
        if s < nelem - 1:
            plan[s + 1] = after
    for e in range(50 * AMB_CHUNK - 200, 50 * AMB_CHUNK + 1300):      # crosses the chunk boundaries at 51 200 and 52 224
        plan[e] = "N"
    plan[200 * AMB_CHUNK + 517] = "D"                                 # alone in its chunk, with empty chunks either side
    plan[256 * AMB_CHUNK] = "H"                                       # first element of the second block of k_amb_write
    plan[256 * AMB_CHUNK + 1023] = "X"
    plan[257 * AMB_CHUNK + 5] = "-"
    plan[last * AMB_CHUNK + 1] = "U"                                  # the last, partial chunk
    return sorted(plan.items())


def amb_records():
    seps = amb_seps()
    elems = bytearray(dna(seps[-1] + 1, 70))
    for e, code in amb_plan():
        assert e not in seps
        elems[e] = ord(code)
    return [bytes(elems[a + 1:b]) for a, b in zip(seps, seps[1:])]
