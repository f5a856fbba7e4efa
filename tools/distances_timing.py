#!/usr/bin/env python3
"""Times the pairwise counts of the multiple alignments (--distances / --distancecounts; sbl_group_distances in
csrc/group_distances.hip) on two workloads:
  strains   the 8-strain workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp), `-s loose`, minimum block size 5000: the
            pipeline runs up to the final block list and aligns its groups once (sbl_align_block_groups); all groups are counted, the
            class of an instance is its record (one record per strain)
  wide      one synthetic group of 64 rows x 1 Mbp: copies of one random record with sparse substitutions only, so that the first band
            width certifies every pair (sbl_align_groups); every row a class of its own
On the rows each groups call left on the device sbl_group_distances runs RUNS + 1 times (the first is a warm-up).  Kernel and copy-back
times are the library's own counters (sbl_group_distances_times: event pairs around clearing the matrix and k_group_distances; around
the device-to-host copy of the matrix), medians.  Beside them stands a device-to-device copy of as many bytes as the rows hold
(instances x columns), timed by event pairs in the same process.  Writes one JSON document (default: profiles/distances_timing.json)."""
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
WIDE_ROWS, WIDE_LEN, WIDE_SUBSTITUTIONS = 64, 1 << 20, 200


def measure(bf, aligned, cls, nclass):
    rows = sum(len(a.rows) * a.L for a in aligned)
    kernel, copy, call, M = [], [], [], None
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        M = bf.group_distances(cls, nclass)
        t1 = time.perf_counter()
        k, c = bf.group_distances_times()
        if i:
            kernel.append(k)
            copy.append(c)
            call.append((t1 - t0) * 1e3)
    res = {"groups": len(aligned), "groups_skipped": sum(a.status != 0 for a in aligned), "groups_counted": sum(a.status == 0 and a.L > 0 and len(a.rows) >= 2 for a in aligned),
           "instances": len(cls), "classes": nclass, "row_bytes": rows, "row_pairs": sum(len(a.rows) * (len(a.rows) - 1) // 2 for a in aligned),
           "pair_columns": sum(len(a.rows) * (len(a.rows) - 1) // 2 * a.L for a in aligned), "matrix_bytes": int(M.nbytes),
           "match": int(M[:, :, 0].sum()) // 2, "mismatch": int(M[:, :, 1].sum()) // 2, "ambiguous": int(M[:, :, 2].sum()) // 2, "gap": int(M[:, :, 3].sum()),
           "kernel_ms": statistics.median(kernel), "kernel_ms_all": kernel, "copyback_ms": statistics.median(copy), "copyback_ms_all": copy,
           "call_ms": statistics.median(call), "call_ms_all": call}
    if rows:
        d2d = d2d_copy_ms(rows)
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
        bf.postprocess(names)
        _, insts, aligned = bf.align_block_groups(MIN_BLOCK_SIZE)
        res = measure(bf, aligned, [c for inst in insts for c, _, _, _ in inst], len(seqs))
    finally:
        bf.close()
    res["input"] = "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d, all groups, class = record" % MIN_BLOCK_SIZE
    return res


def wide():
    rng = np.random.default_rng(8)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), WIDE_LEN)
    seqs = []
    for _ in range(WIDE_ROWS):
        s = base.copy()
        at = rng.choice(np.arange(50, WIDE_LEN - 50, 100), WIDE_SUBSTITUTIONS, replace=False)      # at least 100 bases apart: no indel pays
        s[at] = np.frombuffer(b"CGTA", dtype=np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), s[at])]
        seqs.append(s.tobytes())
    bf = BlockFinder(seqs, device=0)
    try:
        aligned = bf.align_groups([[(i, 0, WIDE_LEN, False) for i in range(WIDE_ROWS)]])
        assert aligned[0].status == 0 and aligned[0].L == WIDE_LEN, (aligned[0].status, aligned[0].L)
        res = measure(bf, aligned, list(range(WIDE_ROWS)), WIDE_ROWS)
        res["align_passes"] = bf.align_stats()["passes"]
    finally:
        bf.close()
    res["input"] = "one group of %d rows x %d columns: copies of one random record with %d substitutions each, no indels" % (WIDE_ROWS, WIDE_LEN, WIDE_SUBSTITUTIONS)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "distances_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/distances_timing.py", "runs": RUNS,
           "row_loads": "two aligned 16-byte words per lane and 16 bytes of a row, shifted in registers (window16), staged into LDS once per tile and row block"}
    res["wide"] = wide()
    print(json.dumps(res["wide"], sort_keys=True), flush=True)
    res["strains"] = strains()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
