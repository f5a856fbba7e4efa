#!/usr/bin/env python3
"""Times the alignment of the unique blocks with and without a gap opening cost (--gapopen; the affine against the linear model of
k_block_align in csrc/block_align.hip) on the Staphylococcus aureus case of tools/block_align_timing.py: the pipeline
runs up to the corrected block list once; then sbl_align_unique_blocks runs RUNS + 1 times on that list (the first is a warm-up) at
o = 0 and again at o = 300, in one process.  Kernel times are the library's own counters (sbl_align_stats: event pairs), medians; the bytes of trace codes
are computed from the band every pair ended at and the passes it took.  Writes one JSON document (default:
profiles/gapopen_timing.json)."""
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

RUNS = 3
MIN_BLOCK_SIZE, LAST_K = 500, 30
W0 = 64


def code_bytes(descs, aligned, affine):
    """bytes of trace codes written over all passes: per pass of a pair (n + m + 1) diagonals of B bytes, B = ceil(ceil(W / 2) / 4)
    lanes of one byte (two with an opening cost), W = |m - n| + 2 w + 1 at w = 64, 128, ... up to the band the pair ended at"""
    total = 0
    for d, a in zip(descs, aligned):
        n, m = d[2] - d[1], d[6] - d[5]
        if not n or not m:
            continue
        w = W0
        for _ in range(a.passes):
            wp = min(w, n, m)
            W = abs(m - n) + 2 * wp + 1
            total += (n + m + 1) * (((W + 1) // 2 + 3) // 4) * (2 if affine else 1)
            w *= 2
    return total


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gapopen_timing.json")
    torch.cuda.init()
    files = records_of("split:Staphylococcus_aureus_pair")[0]
    names = [n for f in files for n, _ in f]
    seqs = [s for f in files for _, s in f]
    stages = P.PARAMETER_SETS["fine"]
    last_k, trim_k = P.final_k(stages, MIN_BLOCK_SIZE, LAST_K)
    bf = BlockFinder(seqs, device=0)
    for k, d in stages:
        bf.PerformGraphSimplifications(k, d, 4)
    bf.GenerateSyntenyBlocks(last_k, trim_k, MIN_BLOCK_SIZE)
    bf.postprocess(names, glue=False)
    bf.correct_boundaries(MIN_BLOCK_SIZE, len(files[0]), names)
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/gapopen_timing.py", "runs": RUNS,
           "input": "Staphylococcus_aureus_pair: record 0 against records 1..179, -s fine -m 500 --lastk 30 --nopostprocess --correctboundaries"}
    for o in (0, 300):
        bf.set_gap_open(o)
        kernel, call, st = [], [], {}
        for i in range(RUNS + 1):
            t0 = time.perf_counter()
            ids, descs, aligned = bf.align_unique_blocks(MIN_BLOCK_SIZE, len(files[0]))
            t1 = time.perf_counter()
            st = bf.align_stats()
            if i:
                kernel.append(st["kernel_ms"])
                call.append((t1 - t0) * 1e3)
        km = statistics.median(kernel)
        res["open_%d" % o] = {"gap_open": o, "pairs": st["pairs"], "skipped": st["skipped"], "passes": st["passes"], "launches": st["launches"],
                              "cells": st["cells"], "kernel_ms": km, "kernel_ms_all": kernel, "call_ms": statistics.median(call),
                              "code_bytes": code_bytes(descs, aligned, o > 0), "widest_band_w": max((a.band_w for a in aligned), default=0),
                              "gap_runs": sum(1 for a in aligned for op, _ in a.runs if op in "ID"),
                              "cells_per_s": st["cells"] / km * 1e3 if km else None}
    bf.close()
    a, b = res["open_0"], res["open_300"]
    res["kernel_ms_ratio"] = b["kernel_ms"] / a["kernel_ms"] if a["kernel_ms"] else None
    res["ns_per_cell_ratio"] = (b["kernel_ms"] / b["cells"]) / (a["kernel_ms"] / a["cells"]) if a["kernel_ms"] and a["cells"] and b["cells"] else None
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
