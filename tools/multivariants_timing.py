#!/usr/bin/env python3
"""Times the variant segments of the multiple alignments (--multivariants; sbl_group_variants in csrc/group_variants.hip) on the 8-strain
workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp), `-s loose`, minimum block size 5000.  The pipeline runs up to the final
block list and aligns its groups once (sbl_align_block_groups); then sbl_group_variants runs RUNS + 1 times on the rows that call left
on the device (the first is a warm-up), over all groups.  Kernel and copy-back times are the library's own counters
(sbl_group_variants_times: event pairs around k_column_classes .. k_segment_bounds and the segment tables, and around k_gather_slices;
around the device-to-host copy of the slices), medians.  Beside them stand a device-to-device copy of as many bytes as the rows hold
(instances x columns: what k_column_classes reads once) and the device-to-host copy of as many bytes as the slices into pinned memory, both
timed by event pairs in the same process.  Writes one JSON document (default: profiles/multivariants_timing.json)."""
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
from multimaf_timing import d2h_copy_ms                                # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P, workloads as W    # noqa: E402

RUNS = 5
MIN_BLOCK_SIZE = 5000


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "multivariants_timing.json")
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
    ids, insts, aligned = bf.align_block_groups(MIN_BLOCK_SIZE)
    rows = sum(len(a.rows) * a.L for a in aligned)
    kernel, copy, call, segs = [], [], [], []
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        segs = bf.group_variants()
        t1 = time.perf_counter()
        k, c = bf.group_variants_times()
        if i:
            kernel.append(k)
            copy.append(c)
            call.append((t1 - t0) * 1e3)
    raw = bf.last_group_segments
    bf.close()
    slices = sum(len(s[5]) * (s[2] - s[1] + s[4]) for s in segs)
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/multivariants_timing.py",
           "input": "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d" % MIN_BLOCK_SIZE, "runs": RUNS,
           "groups": len(aligned), "groups_skipped": sum(a.status != 0 for a in aligned), "instances": sum(len(i) for i in insts),
           "row_bytes": rows, "columns": sum(a.L for a in aligned if len(a.rows) >= 2), "segments": len(segs),
           "segments_gapped": int(raw["gapped"].sum()) if len(raw) else 0, "slice_bytes": slices,
           "row_loads": "two aligned 16-byte words per lane and row, shifted in registers (window16)",
           "kernel_ms": statistics.median(kernel), "kernel_ms_all": kernel, "copyback_ms": statistics.median(copy), "copyback_ms_all": copy,
           "call_ms": statistics.median(call), "call_ms_all": call}
    if rows:
        d2d = d2d_copy_ms(rows)
        res.update({"d2d_copy_ms": statistics.median(d2d), "d2d_copy_ms_all": d2d, "kernels_over_copy": res["kernel_ms"] / statistics.median(d2d)})
    if slices:
        d2h = d2h_copy_ms(slices)
        res.update({"device_to_host_pinned_ms": statistics.median(d2h), "device_to_host_pinned_ms_all": d2h})
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
