#!/usr/bin/env python3
"""Times the concatenated alignment (--corealignment / --coresnps; sbl_group_concat in csrc/group_concat.hip) in both modes on two
workloads:
  strains   the 8-strain workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp), `-s loose`, minimum block size 5000: the
            pipeline runs up to the final block list and aligns its groups once (sbl_align_block_groups); the core blocks
            (pipeline.core_blocks, one record per strain) are concatenated, the class of an instance is its record, lines of 80
  wide      one synthetic group of 64 rows x 1 Mbp: copies of one random record with sparse substitutions only, so that the first band
            width certifies every pair (sbl_align_groups); every row a class of its own
On the rows each groups call left on the device sbl_group_concat runs RUNS + 1 times per mode (the first is a warm-up).  Kernel and
copy-back times are the library's own counters (sbl_group_concat_times: event pairs around the kernels -- in mode VARIABLE the flags, the
compaction, the sites and the text -- and around the device-to-host copy of the text), medians.  Beside them stands a device-to-device
copy of as many bytes as the text, timed by event pairs in the same process.  Writes one JSON document (default:
profiles/core_timing.json)."""
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
from sibelia_amd.api import CONCAT_ALL, CONCAT_VARIABLE               # noqa: E402

RUNS = 5
MIN_BLOCK_SIZE = 5000
WIDTH = 80
WIDE_ROWS, WIDE_LEN, WIDE_SUBSTITUTIONS = 64, 1 << 20, 200


def measure(bf, aligned, cls, nclass, want):
    headers = [b">strain%d\n" % f for f in range(nclass)]
    res = {"groups": len(aligned), "groups_used": sum(bool(w) and a.status == 0 and a.L > 0 for w, a in zip(want, aligned)), "classes": nclass, "width": WIDTH,
           "row_bytes_used": sum(len(a.rows) * a.L for w, a in zip(want, aligned) if w and a.status == 0)}
    for name, mode in (("all", CONCAT_ALL), ("variable", CONCAT_VARIABLE)):
        kernel, copy, call = [], [], []
        for i in range(RUNS + 1):
            t0 = time.perf_counter()
            text, parts, sites = bf.group_concat(cls, nclass, headers, mode, WIDTH, want)
            t1 = time.perf_counter()
            k, c = bf.group_concat_times()
            if i:
                kernel.append(k)
                copy.append(c)
                call.append((t1 - t0) * 1e3)
        m = {"text_bytes": len(text), "columns": sum(n for _, _, n in parts), "sites": len(sites),
             "kernel_ms": statistics.median(kernel), "kernel_ms_all": kernel, "copyback_ms": statistics.median(copy), "copyback_ms_all": copy,
             "call_ms": statistics.median(call), "call_ms_all": call}
        if len(text):
            d2d = d2d_copy_ms(len(text))
            m.update({"d2d_copy_ms": statistics.median(d2d), "d2d_copy_ms_all": d2d, "kernel_over_copy": m["kernel_ms"] / statistics.median(d2d)})
        res[name] = m
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
        res = measure(bf, aligned, [c for inst in insts for c, _, _, _ in inst], len(seqs), [b in core and a.status == 0 for b, a in zip(ids, aligned)])
        res["core_blocks"] = len(core)
    finally:
        bf.close()
    res["input"] = "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d, the core blocks, class = record" % MIN_BLOCK_SIZE
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
        res = measure(bf, aligned, list(range(WIDE_ROWS)), WIDE_ROWS, [True])
    finally:
        bf.close()
    res["input"] = "one group of %d rows x %d columns: copies of one random record with %d substitutions each, no indels" % (WIDE_ROWS, WIDE_LEN, WIDE_SUBSTITUTIONS)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "core_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/core_timing.py", "runs": RUNS}
    res["wide"] = wide()
    print(json.dumps(res["wide"], sort_keys=True), flush=True)
    res["strains"] = strains()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
