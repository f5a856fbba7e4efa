#!/usr/bin/env python3
"""Regenerate tests/golden/synteny_limits.json from the UNMODIFIED reference (build container only).

Test infrastructure, in the manner of make_golden.py: needs oracle/_ref/ref_dump (oracle/build_ref.sh).  The inputs are the crafted
cases of tests/synteny_cases.py; every op of a case is one command of ref_dump (stage:K:D:ITER / blocks:K:T:M:S, formats in
make_golden.py), all on one BlockFinder in order.  Only the case name, the input digest and per command the size and sha256 of what
the reference wrote are committed.

usage: make_synteny_limits_golden.py [--only NAME ...]
"""
import json, os, subprocess, sys, time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from sibelia_amd import workloads as W  # noqa: E402
from tests import synteny_cases as S  # noqa: E402
import make_golden as G  # noqa: E402

TIMEOUT = int(os.environ.get("GOLDEN_LIMITS_TIMEOUT", "600"))


def main():
    out = os.path.join(ROOT, "tests", "golden", "synteny_limits.json")
    old = json.load(open(out)) if os.path.exists(out) else {"cases": [], "skipped": []}
    only = [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--only"]
    byname = {c["name"]: c for c in old["cases"]}
    skipped = set(old.get("skipped", []))
    for name, case in S.CASES.items():
        if only and name not in only:
            continue
        seqs, ops = case.make()
        cmds = [S.cmd_of(op) for op in ops]
        t = time.time()
        try:
            outs = G.run_case(seqs, cmds, timeout=TIMEOUT)
        except subprocess.TimeoutExpired:
            print(name, "skipped (reference > %d s)" % TIMEOUT, flush=True)
            skipped.add(name)
            byname.pop(name, None)
            continue
        skipped.discard(name)
        byname[name] = {"name": name, "input_sha256": W.input_digest(seqs),
                        "outputs": [{"cmd": o["cmd"], "size": o["size"], "sha256": o["sha256"]} for o in outs]}
        print(name, "%.1f s" % (time.time() - t), [(o["cmd"], o["size"]) for o in outs], flush=True)
    with open(out, "w") as f:
        json.dump({"reference": "bioinf/Sibelia 3.0.7 (unmodified, sources compiled in place by oracle/build_ref.sh, -O3 -DNDEBUG)",
                   "skipped": sorted(skipped), "cases": [byname[n] for n in S.CASES if n in byname]}, f, indent=1)
        f.write("\n")
    print("wrote", out, len(byname), "cases")


if __name__ == "__main__":
    main()
