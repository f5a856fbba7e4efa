#!/usr/bin/env python3
"""Times the boundary correction (--correctboundaries; csrc/boundary_align.hip) on the Staphylococcus aureus example: the finished genome
as the reference set, the 179 contigs as the assembly, `-s loose` (R = 1024).  The pipeline runs up to the post-processing once per
run (the correction replaces the list it works on); kernel time, launches, levels and cells are the library's own counters
(sbl_correct_stats: event pairs around every launch), the whole call is timed on the host.  One warm-up, then RUNS runs; medians.
The reference's CPU time for the same step, as recorded by tests/golden/gen/make_correct_golden.py on the host that generated the
fixtures, is copied beside it.  Writes one JSON document (default: profiles/correct_boundaries_timing.json)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from correct_fixtures import records_of                                # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P                     # noqa: E402

RUNS = 5


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "correct_boundaries_timing.json")
    torch.cuda.init()
    files = records_of("split:Staphylococcus_aureus_pair")[0]
    names = [n for f in files for n, _ in f]
    seqs = [s for f in files for _, s in f]
    stages = P.PARAMETER_SETS["loose"]
    last_k, trim_k = P.final_k(stages, 5000)
    kernel, call, st = [], [], {}
    for i in range(RUNS + 1):
        bf = BlockFinder(seqs, device=0)
        for k, d in stages:
            bf.PerformGraphSimplifications(k, d, 4)
        bf.GenerateSyntenyBlocks(last_k, trim_k, 5000)
        bf.postprocess(names)
        t0 = time.perf_counter()
        bf.correct_boundaries(5000, len(files[0]), names)
        t1 = time.perf_counter()
        st = bf.correct_stats()
        bf.close()
        if i:
            kernel.append(st["kernel_ms"])
            call.append((t1 - t0) * 1e3)
    km = statistics.median(kernel)
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/correct_timing.py", "input": "Staphylococcus_aureus_pair: record 0 against records 1..179, -s loose",
           "runs": RUNS, "groups": st["groups"], "alignments": st["alignments"], "levels": st["levels"], "launches": st["launches"], "cells": st["cells"],
           "kernel_ms": km, "kernel_ms_all": kernel, "call_ms": statistics.median(call), "call_ms_all": call, "cells_per_s": st["cells"] / km * 1e3}
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "correct_cases.json")))
    if "reference_cpu_time" in golden:
        res["reference_cpu"] = golden["reference_cpu_time"]
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
