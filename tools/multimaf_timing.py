#!/usr/bin/env python3
"""Times the multiple alignment of every block (--multimaf; sbl_align_block_groups in csrc/block_align.hip) on the 8-strain workload of
sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp), `-s loose`, minimum block size 5000.  The pipeline runs up to the final block list
once; then the call runs RUNS + 1 times on that list (the first is a warm-up).  Pair and spelling times are the library's own counters
(sbl_align_stats: event pairs), medians.  Beside the spelling kernel stand a device-to-device copy of as many bytes as the text it
writes and the device-to-host copy of that many bytes into pinned memory, both timed by event pairs in the same process: the only
comparison drawn is the spelling kernel against that copy.  Writes one JSON document (first argument; default:
profiles/multimaf_timing.json).  An optional second argument is the gap opening cost (--gapopen; default 0): it is there
to reach the LDS classes of the affine model of k_block_align, which tools/gapopen_timing.py (every pair at w = 64) does not."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from blockseq_timing import d2d_copy_ms                                # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P, workloads as W    # noqa: E402

RUNS = 5
MIN_BLOCK_SIZE = 5000


def d2h_copy_ms(nbytes):
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    times = []
    for i in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        if i:
            times.append(a.elapsed_time(b))
    return times


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "multimaf_timing.json")
    gap_open = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    torch.cuda.init()
    seqs = W.gen_strains()
    names = ["strain%d" % i for i in range(len(seqs))]
    stages = P.PARAMETER_SETS["loose"]
    last_k, trim_k = P.final_k(stages, MIN_BLOCK_SIZE)
    bf = BlockFinder(seqs, device=0)
    for k, d in stages:
        bf.PerformGraphSimplifications(k, d, 4)
    bf.GenerateSyntenyBlocks(last_k, trim_k, MIN_BLOCK_SIZE)
    bf.postprocess(names)
    bf.set_gap_open(gap_open)
    kernel, spell, call, st, aligned = [], [], [], {}, []
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        ids, insts, aligned = bf.align_block_groups(MIN_BLOCK_SIZE)
        t1 = time.perf_counter()
        st = bf.align_stats()
        if i:
            kernel.append(st["kernel_ms"])
            spell.append(st["spell_ms"])
            call.append((t1 - t0) * 1e3)
    bf.close()
    text = sum(len(a.rows) * a.L for a in aligned)
    by_w = {}                                       # pairs by the band they ended at: 2 w + 1 offsets at least, so w >= 256 is an LDS class
    for a in aligned:
        for _, w, _ in a.members:
            by_w[w] = by_w.get(w, 0) + 1
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/multimaf_timing.py",
           "input": "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d" % MIN_BLOCK_SIZE, "runs": RUNS, "gap_open": gap_open,
           "groups": len(aligned), "groups_skipped": sum(a.status != 0 for a in aligned), "instances": sum(len(i) for i in insts),
           "pairs": st["pairs"], "pairs_skipped": st["skipped"], "passes": st["passes"], "launches": st["launches"], "cells": st["cells"],
           "pairs_by_band_w": {str(w): by_w[w] for w in sorted(by_w)}, "text_bytes": text, "kernel_ms": statistics.median(kernel), "kernel_ms_all": kernel,
           "spell_ms": statistics.median(spell), "spell_ms_all": spell, "call_ms": statistics.median(call), "call_ms_all": call}
    if text:
        d2d, d2h = d2d_copy_ms(text), d2h_copy_ms(text)
        res.update({"d2d_copy_ms": statistics.median(d2d), "d2d_copy_ms_all": d2d, "device_to_host_ms": statistics.median(d2h),
                    "device_to_host_ms_all": d2h, "spell_over_copy": res["spell_ms"] / statistics.median(d2d)})
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
