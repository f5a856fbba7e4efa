#!/usr/bin/env python3
"""Regenerate tests/golden/fasta_limits.json from the UNMODIFIED reference reader (build container only).

Test infrastructure, in the manner of make_fasta_golden.py: needs oracle/_ref/ref_dump (oracle/build_ref.sh).  Every text of
tests/fasta_cases.py is written to a file and read by the reference's FASTAReader through `ref_dump <file> <prefix> state`.
  small cases (text up to 1 kB): the text (base64) and the full result, in the format of fasta_cases.json -- records (name,
    sequence) or the error message with the file name replaced by <file>;
  larger cases: sha256 and length of the text (tests/fasta_cases.py rebuilds it), and the error message or per record the name, the
    length and the sha256 of the sequence -- for more than 8 records their number, the total length and ONE sha256 over all names and
    sequences (fasta_cases.records_digest).  This keeps the fixture small enough to read; nothing is checked less exactly.
Names and messages are stored as latin-1 text (one code point per byte): an illegal byte of 0x80 or above is part of a message.
The random texts of tests/fasta_cases.py are stored by sha256 only -- their expected result comes from tests/fasta_model.py -- but
the model is held to the reference on each of them here.

usage: make_fasta_limits_golden.py
"""
import base64, hashlib, json, os, struct, subprocess, sys, tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, ROOT)
from tests import fasta_cases as F  # noqa: E402
from tests import fasta_model as M  # noqa: E402

REF_DUMP = os.path.join(ROOT, "oracle", "_ref", "ref_dump")


def reference(text):
    """the error message (bytes, <file> for the path) or [(name, sequence)] as the reference reads the text"""
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "in.fa")
        with open(fa, "wb") as f:
            f.write(text)
        r = subprocess.run([REF_DUMP, fa, os.path.join(d, "o"), "state"], capture_output=True)
        if r.returncode == 4:
            return open(os.path.join(d, "o.err"), "rb").read().replace(fa.encode(), b"<file>")
        if r.returncode != 0:
            raise SystemExit("ref_dump rc %d: %s" % (r.returncode, r.stderr.decode()))
        b = open(os.path.join(d, "o.0.out"), "rb").read()
        names = open(os.path.join(d, "o.0.out.names"), "rb").read().split(b"\n")[:-1]
        nchr = struct.unpack_from("<I", b, 8)[0]
        assert nchr == len(names)
        off, recs = 12, []
        for c in range(nchr):
            n = struct.unpack_from("<Q", b, off)[0]
            off += 8
            seq = b[off:off + n]
            off += n
            assert np.array_equal(np.frombuffer(b, "<u4", n, off), np.arange(n, dtype=np.uint32))      # originalPos_ = identity
            off += 4 * n
            recs.append((names[c], seq))
        assert off == len(b)
        return recs


def main():
    out = {}
    for name in F.CASES:
        text = F.text(name)
        F.CASES[name].pre()
        got = reference(text)
        small = len(text) <= F.SMALL_MAX
        e = {"text_b64": base64.b64encode(text).decode()} if small else {"text_sha256": hashlib.sha256(text).hexdigest(), "text_len": len(text)}
        e.update(F.fixture_result(got, small))
        out[name] = e
        print(name, len(text), {k: (v if k != "records" else len(v)) for k, v in F.result_keys(e).items()}, flush=True)
    rnd = []
    for i, text in enumerate(F.random_texts()):
        assert M.parse(text) == reference(text), "the model differs from the reference on random text %d" % i
        rnd.append(hashlib.sha256(text).hexdigest())
    path = os.path.join(ROOT, "tests", "golden", "fasta_limits.json")
    with open(path, "w") as f:
        json.dump({"reference": "bioinf/Sibelia 3.0.7 FASTAReader (oracle/_ref/ref_dump state)", "random_seed": F.RANDOM_SEED,
                   "random_sha256": rnd, "cases": out}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
