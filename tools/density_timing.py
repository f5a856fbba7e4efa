#!/usr/bin/env python3
"""Times the SNP-density mask (--corefiltered / --coredense; sbl_group_mask in csrc/group_mask.hip) on two workloads:
  strains   the 8-strain workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp), `-s loose`, minimum block size 5000: the
            pipeline runs up to the final block list and aligns its groups once (sbl_align_block_groups); the core blocks
            (pipeline.core_blocks, one record per strain) are masked with W = 1000, T = 3
  wide      one synthetic group of 64 rows x 1 Mbp: copies of one random record with sparse substitutions and, per row, 100 planted
            clusters of 5 substitutions 19 bases apart, no indels (sbl_align_groups); W = 1000, T = 3
On the rows each groups call left on the device sbl_group_mask runs RUNS + 1 times (the first is a warm-up).  Kernel and copy-back times
are the library's own counters (sbl_group_mask_times: event pairs around the kernels -- the flags, the compactions, the scan, the
intervals and the masked rows -- and around the device-to-host copy of the intervals), medians.  Beside them stands a device-to-device
copy of as many bytes as the rows, timed by event pairs in the same process: the floor of a pass that reads the rows once and writes
them once.  Writes one JSON document (default: profiles/density_timing.json), after every workload."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from blockseq_timing import d2d_copy_ms                                # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P, workloads as W    # noqa: E402

RUNS = 5
MIN_BLOCK_SIZE = 5000
WINDOW, MAX_DIFF = P.DENSITYWINDOW_DEFAULT, P.DENSITYMAX_DEFAULT
WIDE_ROWS, WIDE_LEN, WIDE_SUBSTITUTIONS, WIDE_CLUSTERS = 64, 1 << 20, 200, 100
WIDE_OFFSETS = (0, 19, 38, 57, 76)                     # the 5 substitutions of a cluster


def measure(bf, aligned, want):
    used = [a for w, a in zip(want, aligned) if w and a.status == 0 and a.L > 0 and len(a.rows) >= 2]
    row_bytes = sum(len(a.rows) * a.L for a in aligned if a.status == 0)
    res = {"groups": len(aligned), "groups_used": len(used), "window": WINDOW, "max_diff": MAX_DIFF, "row_bytes": row_bytes,
           "row_bytes_used": sum(len(a.rows) * a.L for a in used)}
    kernel, copy, call = [], [], []
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        intervals = bf.group_mask(WINDOW, MAX_DIFF, want)
        t1 = time.perf_counter()
        k, c = bf.group_mask_times()
        if i:
            kernel.append(k)
            copy.append(c)
            call.append((t1 - t0) * 1e3)
    base = np.zeros(256, dtype=bool)
    base[list(b"ACGT")] = True
    differences = 0
    for a in used:
        rows = np.array([np.frombuffer(r, dtype=np.uint8) for r in a.rows])
        differences += int((base[rows[0]] & base[rows[1:]] & (rows[1:] != rows[0])).sum())
    masked = sum(last - first + 1 - aligned[g].rows[row][first:last + 1].count(b"-") for g, row, first, last, _, _, _ in intervals)
    res.update({"differences": differences, "intervals": len(intervals), "differences_masked": sum(iv[6] for iv in intervals), "masked_bases": masked,
                "kernel_ms": statistics.median(kernel), "kernel_ms_all": kernel, "copyback_ms": statistics.median(copy), "copyback_ms_all": copy,
                "call_ms": statistics.median(call), "call_ms_all": call})
    if row_bytes:
        d2d = d2d_copy_ms(row_bytes)
        res.update({"d2d_copy_ms": statistics.median(d2d), "d2d_copy_ms_all": d2d, "kernel_over_copy": res["kernel_ms"] / statistics.median(d2d)})
    return res


def strains():
    seqs = W.gen_strains()
    names = ["strain%d" % i for i in range(len(seqs))]
    stages = P.PARAMETER_SETS["loose"]
    last_k, trim_k = P.final_k(stages, MIN_BLOCK_SIZE)
    bf = BlockFinder(seqs, device=0)
    try:
        for k, d in stages:
            bf.PerformGraphSimplifications(k, d, 4)
        bf.GenerateSyntenyBlocks(last_k, trim_k, MIN_BLOCK_SIZE)
        blocks, _ = bf.postprocess(names)
        core = set(P.core_blocks(blocks, [1] * len(seqs), MIN_BLOCK_SIZE))
        ids, insts, aligned = bf.align_block_groups(MIN_BLOCK_SIZE)
        res = measure(bf, aligned, [b in core and a.status == 0 for b, a in zip(ids, aligned)])
        res["core_blocks"] = len(core)
    finally:
        bf.close()
    res["input"] = "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d, the core blocks, W = %d, T = %d" % (MIN_BLOCK_SIZE, WINDOW, MAX_DIFF)
    return res


def wide_records():
    rng = np.random.default_rng(8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = rng.choice(acgt, WIDE_LEN)
    seqs = [base.tobytes()]
    for _ in range(WIDE_ROWS - 1):
        s = base.copy()
        at = rng.choice(np.arange(50, WIDE_LEN - 50, 100), WIDE_SUBSTITUTIONS + WIDE_CLUSTERS, replace=False)      # at least 100 bases apart: no indel pays
        at = np.concatenate([at[:WIDE_SUBSTITUTIONS]] + [at[WIDE_SUBSTITUTIONS:] + d for d in WIDE_OFFSETS])
        for y in acgt:                                  # a base the record holds neither there nor next to it: a shift by one gains nothing
            s[at] = np.where((base[at - 1] != y) & (base[at] != y) & (base[at + 1] != y), y, s[at])
        assert (s[at] != base[at]).all()
        seqs.append(s.tobytes())
    return seqs


def wide():
    seqs = wide_records()
    bf = BlockFinder(seqs, device=0)
    try:
        aligned = bf.align_groups([[(i, 0, WIDE_LEN, False) for i in range(WIDE_ROWS)]])
        assert aligned[0].status == 0 and aligned[0].L == WIDE_LEN, (aligned[0].status, aligned[0].L)
        res = measure(bf, aligned, [True])
    finally:
        bf.close()
    res["input"] = ("one group of %d rows x %d columns: copies of one random record with %d lone substitutions and %d clusters of 5 each, no indels, W = %d, T = %d"
                    % (WIDE_ROWS, WIDE_LEN, WIDE_SUBSTITUTIONS, WIDE_CLUSTERS, WINDOW, MAX_DIFF))
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "density_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/density_timing.py", "runs": RUNS}
    for name, fn in (("wide", wide), ("strains", strains)):
        res[name] = fn()
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res[name], sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
