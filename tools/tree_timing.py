#!/usr/bin/env python3
"""Times the bootstrap pair counts and the trees made from them (--coretree --bootstrap B; sbl_group_bootstrap in csrc/group_boot.hip,
sibelia_amd/tree.py) on two workloads:
  strains   the 8-strain workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp), `-s loose`, minimum block size 5000: the
            pipeline runs up to the final block list and aligns its groups once (sbl_align_block_groups); the core blocks
            (pipeline.core_blocks, one record per strain), B = 1000
  wide      the synthetic group of tools/density_timing.py: 64 rows x 1 Mbp with 44 100 differences, B = 1000
On the rows each groups call left on the device sbl_group_bootstrap runs RUNS + 1 times (the first is a warm-up) with 0 replicates and
with B.  Kernel and copy-back times are the library's own counters (sbl_group_bootstrap_times: event pairs), medians: the call without
replicates is the site / pack phase (flags, compaction, packing, slab 0), the difference to the call with B is the replicate phase
-- a difference of two medians, never measured on its own, since the library keeps one counter for all phases.
Beside them: the kernel time of one sbl_group_concat call in mode VARIABLE on the same rows -- what finding the sites costs already --,
the host time of the B + 1 neighbour joinings with their supports, and the time tests/boot_model.py takes on the host for 10 of the
replicates, scaled to B.  Writes one JSON document (default: profiles/tree_timing.json), after every workload."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_model as BM                                                 # noqa: E402
from density_timing import MIN_BLOCK_SIZE, WIDE_LEN, WIDE_ROWS, wide_records      # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P, tree, workloads as W           # noqa: E402
from sibelia_amd.api import CONCAT_VARIABLE                             # noqa: E402

RUNS = 5
B = 1000
SEED = 1
MODEL_REPLICATES = 10


def measure(bf, aligned, cls, n, want):
    names = ["f%d" % i for i in range(n)]
    res = {"files": n, "replicates": B, "groups": len(aligned), "groups_used": sum(bool(w) for w in want)}
    times = {}
    for label, reps in (("sites", 0), ("all", B)):
        kernel, copy, call = [], [], []
        for i in range(RUNS + 1):
            t0 = time.perf_counter()
            counts, C, K = bf.group_bootstrap(cls, n, reps, SEED, 0, want)
            t1 = time.perf_counter()
            k, c = bf.group_bootstrap_times()
            if i:
                kernel.append(k)
                copy.append(c)
                call.append((t1 - t0) * 1e3)
        times[label] = (kernel, copy, call)
    draws, pairs = B * C, n * (n - 1) // 2
    site_ms, all_ms = statistics.median(times["sites"][0]), statistics.median(times["all"][0])
    rep_ms = all_ms - site_ms
    res.update({"sites": C, "clean_columns": K, "draws": draws, "pairs": pairs,
                "site_pack_kernel_ms": site_ms, "site_pack_kernel_ms_all": times["sites"][0],
                "kernel_ms": all_ms, "kernel_ms_all": times["all"][0], "replicate_kernel_ms": rep_ms,
                "replicate_kernel_ms_is": "kernel_ms - site_pack_kernel_ms: a difference of two medians, the library keeps one counter for all phases",
                "copyback_ms": statistics.median(times["all"][1]), "copyback_ms_all": times["all"][1],
                "call_ms": statistics.median(times["all"][2]), "call_ms_all": times["all"][2],
                "draws_per_s": draws / (rep_ms * 1e-3) if rep_ms > 0 else None,
                "pair_comparisons_per_s": draws * pairs / (rep_ms * 1e-3) if rep_ms > 0 else None})
    headers = [b">" + a.encode() + b"\n" for a in names]
    concat = []
    for i in range(RUNS + 1):
        text, _, _ = bf.group_concat(cls, n, headers, CONCAT_VARIABLE, 80, want)
        if i:
            concat.append(bf.group_concat_times()[0])
    res.update({"concat_variable_kernel_ms": statistics.median(concat), "concat_variable_kernel_ms_all": concat})
    t0 = time.perf_counter()
    newick = tree.tree_text(counts, K, "p", names)
    res["host_tree_ms"] = (time.perf_counter() - t0) * 1e3
    res["newick_bytes"] = len(newick)
    # the host restatement on the SNP matrix the concatenation spelled: 10 replicates, scaled to B; its counts are the device's
    S = np.array([np.frombuffer("".join(rec.split("\n")[1:]).encode(), dtype=np.uint8) for rec in text.decode().split(">")[1:]]).reshape(n, -1)
    t0 = time.perf_counter()
    model = BM.counts_of_sites(S, MODEL_REPLICATES, SEED)
    res["host_model_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * B / MODEL_REPLICATES
    assert (model == counts[:MODEL_REPLICATES + 1]).all()
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
        cls = [c for inst in insts for c, _, _, _ in inst]                       # one record per strain: the record is the file
        res = measure(bf, aligned, cls, len(seqs), [b in core and a.status == 0 for b, a in zip(ids, aligned)])
        res["core_blocks"] = len(core)
    finally:
        bf.close()
    res["input"] = "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d, the core blocks, B = %d" % (MIN_BLOCK_SIZE, B)
    return res


def wide():
    seqs = wide_records()
    bf = BlockFinder(seqs, device=0)
    try:
        aligned = bf.align_groups([[(i, 0, WIDE_LEN, False) for i in range(WIDE_ROWS)]])
        assert aligned[0].status == 0 and aligned[0].L == WIDE_LEN, (aligned[0].status, aligned[0].L)
        res = measure(bf, aligned, list(range(WIDE_ROWS)), WIDE_ROWS, [True])
    finally:
        bf.close()
    res["input"] = "one group of %d rows x %d columns, the records of tools/density_timing.py, B = %d" % (WIDE_ROWS, WIDE_LEN, B)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tree_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/tree_timing.py", "runs": RUNS, "seed": SEED}
    for name, fn in (("wide", wide), ("strains", strains)):
        res[name] = fn()
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res[name], sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
