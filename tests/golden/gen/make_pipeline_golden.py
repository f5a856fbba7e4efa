#!/usr/bin/env python3
"""Fixtures for tests/test_gpu_pipeline.py: the UNMODIFIED reference program (oracle/_ref/sibelia_ref, built by
oracle/build_dropin.sh) is run on the CPU with command lines that make blocks_coords.gff and blocks_sequences.fasta non-trivial
(several input records, reverse-strand instances over ambiguity codes, with and without -r); sizes and sha256 of every file it
writes and of its standard output go to tests/golden/pipeline_cases.json, in the format of dropin_cases.json."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_dropin_golden import REF, run_case      # noqa: E402

CASES = [
    ("hpylori_loose_inram_sequences_gff", "Helicobacter_pylori", ["-s", "loose", "-r", "-q", "--gff"]),
    ("ambig_fine_inram_sequences_gff", "ambig:60000:4:77:9", ["-s", "fine", "-r", "-q", "--gff", "-m", "500"]),
    ("ambig_fine_tempfiles_allstages_sequences_gff", "ambig:60000:4:77:9", ["-s", "fine", "-q", "--allstages", "--gff", "-m", "500"]),
    ("saureus_loose_inram_sequences_gff", "Staphylococcus_aureus_pair", ["-s", "loose", "-r", "-q", "--gff"]),
]

if __name__ == "__main__":
    if not os.path.exists(REF):
        sys.exit("build oracle/_ref/sibelia_ref first: bash oracle/build_dropin.sh")
    out = {"generator": "tests/golden/gen/make_pipeline_golden.py", "program": "oracle/_ref/sibelia_ref (unmodified reference, oracle/build_dropin.sh)", "cases": []}
    for name, inp, args in CASES:
        with tempfile.TemporaryDirectory() as wd:
            rc, so, files, stdout, stderr = run_case(REF, inp, args, wd)
            ext = ".gff"
            rows = sum(open(os.path.join(wd, "out", f), "rb").read().count(b"\n") - 3 for f in files if f.startswith("blocks_coords") and f.endswith(ext))
            nseq = open(os.path.join(wd, "out", "blocks_sequences.fasta"), "rb").read().count(b">") if "blocks_sequences.fasta" in files else 0
        print(name, "rc", rc, len(files), "files,", rows, "gff rows,", nseq, "block sequences", file=sys.stderr)
        if rows <= 0 or nseq <= 0:
            sys.exit("case %s has no blocks: replace it" % name)
        out["cases"].append({"name": name, "input": inp, "args": args, "returncode": rc, "stdout_sha256": so, "stdout_bytes": len(stdout), "files": files})
    with open(os.path.join(ROOT, "tests", "golden", "pipeline_cases.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
