#!/usr/bin/env python3
"""Regenerate tests/golden/tiny_index.json from the UNMODIFIED reference (build container only).

Test infrastructure, in the manner of make_synteny_limits_golden.py: needs oracle/_ref/ref_dump (oracle/build_ref.sh).  The inputs
are the cases of tests/tiny_index_cases.py: the sequences of every block that must be indexed are written as one FASTA file and
ref_dump's enum:K (format in make_golden.py) run on it.  Per distinct (sequences, k) -- keyed by the input digest and k, so a block
that occurs in several cases is run once -- the bifurcation count, the two list lengths and the sha256 of each list's bytes are
committed, and the lists themselves ((id, chr, pos) flattened) where each holds at most LIST_MAX instances.

usage: make_tiny_index_golden.py
"""
import base64, hashlib, json, os, struct, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tests import tiny_index_cases as T  # noqa: E402
import make_golden as G  # noqa: E402

LIST_MAX = 24


def main():
    out = os.path.join(ROOT, "tests", "golden", "tiny_index.json")
    index, cases = {}, {}
    for name, case in T.CASES.items():
        records, jobs = T.made(name)
        n = 0
        for k, blocks in jobs:
            for block in blocks:
                if T.expected_status(records, block, k) != T.INDEXED:
                    continue
                n += 1
                seqs = T.sequences(records, block)
                key = T.fixture_key(seqs, k)
                if key in index:
                    continue
                b = base64.b64decode(G.run_case(seqs, ["enum:%d" % k], keep_bytes=True, timeout=60)[0]["b64"])
                bif, npos = struct.unpack_from("<IQ", b, 0)
                pos = b[12:12 + 12 * npos]
                nneg = struct.unpack_from("<Q", b, 12 + 12 * npos)[0]
                neg = b[20 + 12 * npos:]
                assert len(neg) == 12 * nneg
                e = {"bif": bif, "n": [npos, nneg], "sha256": [hashlib.sha256(pos).hexdigest(), hashlib.sha256(neg).hexdigest()]}
                if max(npos, nneg) <= LIST_MAX:
                    e["pos"] = list(struct.unpack("<%dI" % (3 * npos), pos))
                    e["neg"] = list(struct.unpack("<%dI" % (3 * nneg), neg))
                index[key] = e
        cases[name] = n
        print(name, n, len(index), flush=True)
    with open(out, "w") as f:
        json.dump({"reference": "bioinf/Sibelia 3.0.7 (unmodified, sources compiled in place by oracle/build_ref.sh, -O3 -DNDEBUG)",
                   "list_max": LIST_MAX, "cases": cases, "index": index}, f, indent=0, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", out, len(index), "entries", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
