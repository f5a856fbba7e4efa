#!/usr/bin/env python3
"""Times the neighbour joining of the B + 1 trees of a bootstrap (--coretree / --coreconsensus / --coreboottrees --bootstrap B;
sbl_nj_batch in csrc/tree_nj.hip against sibelia_amd/tree.py's neighbour_joining) on the two workloads of tools/tree_timing.py:
  strains   the 8-strain workload of sibelia_amd/workloads.py, `-s loose`, minimum block size 5000, the core blocks, B = 1000
  wide      the synthetic group of tools/density_timing.py: 64 rows x 1 Mbp, B = 1000
The counts come from one sbl_group_bootstrap call on the rows the groups call left on the device, the distances (model p) from
tree.distances on the host, as in the pipeline.  On those B + 1 matrices BlockFinder.nj_batch runs RUNS + 1 times (the first is a
warm-up): the wall time of the call (validation, upload, kernel, copy-back, the copies into numpy arrays) and the library's own kernel
and copy times (sbl_nj_batch_times: event pairs), as median, lowest and highest.  Beside them, in the same process, the host loop over the
same matrices -- tree.neighbour_joining B + 1 times, the code every tree went through before -- HOST_RUNS times.  Every edge of the last
device call is compared with the host's, bit for bit.  Writes one JSON document (default: profiles/nj_timing.json), after every workload."""
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
from density_timing import MIN_BLOCK_SIZE, WIDE_LEN, WIDE_ROWS, wide_records      # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P, tree, workloads as W           # noqa: E402

RUNS = 5
HOST_RUNS = 3
B = 1000
SEED = 1


def spread(values):
    return {"median": statistics.median(values), "lowest": min(values), "highest": max(values), "all": values}


def measure(bf, cls, n, want):
    counts, C, K = bf.group_bootstrap(cls, n, B, SEED, 0, want)
    D = np.stack([tree.distances(counts[r], K, "p") for r in range(B + 1)])
    call, kernel, copy = [], [], []
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        edges, splits = bf.nj_batch(D)
        t1 = time.perf_counter()
        k, c = bf.nj_batch_times()
        if i:
            call.append((t1 - t0) * 1e3)
            kernel.append(k)
            copy.append(c)
    host = []
    for _ in range(HOST_RUNS):
        t0 = time.perf_counter()
        trees = [tree.neighbour_joining(D[r]) for r in range(B + 1)]
        host.append((time.perf_counter() - t0) * 1e3)
    want_edges = np.array([t.edges for t in trees], dtype=tree.EDGE_RECORD)
    assert np.array_equal(edges.view(np.uint8), want_edges.view(np.uint8)), "the device's edges are not the host's"
    assert all(sorted(splits[r].tolist()) == sorted(tree.bipartitions(trees[r])) for r in range(0, B + 1, 97))
    return {"files": n, "trees": B + 1, "sites": C, "clean_columns": K, "matrix_bytes": int(D.nbytes),
            "device_call_ms": spread(call), "device_kernel_ms": spread(kernel), "device_copy_ms": spread(copy),
            "host_loop_ms": spread(host), "host_over_device_call": statistics.median(host) / statistics.median(call),
            "distinct_trees": len({e.tobytes() for e in edges["child"]})}


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
        res = measure(bf, cls, len(seqs), [b in core and a.status == 0 for b, a in zip(ids, aligned)])
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
        res = measure(bf, list(range(WIDE_ROWS)), WIDE_ROWS, [True])
    finally:
        bf.close()
    res["input"] = "one group of %d rows x %d columns, the records of tools/density_timing.py, B = %d" % (WIDE_ROWS, WIDE_LEN, B)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nj_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/nj_timing.py", "runs": RUNS, "host_runs": HOST_RUNS, "seed": SEED, "model": "p"}
    for name, fn in (("wide", wide), ("strains", strains)):
        res[name] = fn()
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res[name], sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
