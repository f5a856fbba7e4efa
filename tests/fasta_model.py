"""The reference's FASTA reader restated in plain Python: FASTAReader::GetSequences, ValidateHeader and ValidateSequence
(reference src/fasta.cpp:23-104).  Test infrastructure: tests/test_fasta_model.py holds it to what the unmodified reader wrote
(tests/golden/fasta_cases.json, tests/golden/fasta_limits.json); the random texts of tests/fasta_cases.py take their expected result
from it.

parse(text) returns the records [(name, sequence)] as bytes, or the reader's message as bytes with <file> standing for the path."""

BLANKS = b" \t\n\r\x0b\x0c"                       # std::isspace in the "C" locale: what boost::trim removes
VALID = frozenset(b"ACGTURYKMSWBDHWNX-")


def message(lineno, what):
    return b"parse error in <file> on line %d: %s" % (lineno, what)


def first_illegal(line):
    """index of the first byte of an (already trimmed) sequence line that is not a valid character once upper-cased, or -1"""
    rest = line.upper().translate(None, bytes(VALID))          # bytes.upper touches a-z only, as toupper does in the "C" locale
    return line.upper().index(rest[:1]) if rest else -1


def parse(text):
    records, name, seq, line = [], None, [], 1                 # line = 1 + the non-empty lines read so far
    for raw in text.split(b"\n"):                               # getline until eof: a final newline leaves one more, empty, line
        buf = raw.strip(BLANKS)
        if not buf:
            continue                                            # skipped and not counted
        if buf[:1] == b">":
            if name is not None:
                if not any(seq):
                    return message(line, b"empty sequence")     # noticed at the NEXT header, ahead of that header's own validation
                records.append((name, b"".join(seq)))
                name, seq = None, []
            sp = buf.find(b" ")
            new = buf[1:sp] if sp >= 0 else buf[1:]
            if not new:
                return message(line, b"empty header")
            name = new                                          # sequence lines ahead of the first header stay in seq: they join this record
        else:
            at = first_illegal(buf)
            if at >= 0:
                return message(line, b"illegal character: " + buf[at:at + 1])      # as written, not upper-cased
            seq.append(buf.upper())
        line += 1
    if not any(seq):
        return message(line, b"empty sequence")
    records.append((name or b"", b"".join(seq)))               # no header at all: one record with an empty name
    return records
