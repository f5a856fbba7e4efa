#!/usr/bin/env python3
"""Times the parsimony mapping of the sites onto the tree (--corebranches / --corebranchsites / --coresnptree; sbl_group_parsimony in
csrc/group_parsimony.hip) on the two workloads of tools/tree_timing.py:
  strains   the 8-strain workload of sibelia_amd/workloads.py, `-s loose`, minimum block size 5000, the core blocks
  wide      the synthetic group of tools/density_timing.py: 64 rows x 1 Mbp
One sbl_group_bootstrap call (no replicates) leaves the packed sites on the device; the tree is the neighbour-joining tree of its
counts (model p), as in the pipeline.  BlockFinder.group_parsimony then runs RUNS + 1 times (the first is a warm-up): the wall time of
the call (validation, schedule, two passes, scan, copy-back, the copies into numpy arrays) and the library's own kernel and copy times
(sbl_group_parsimony_times: event pairs), as median, lowest and highest.  Beside them a device-to-device copy of as many bytes as the
packed sites take, timed by events the same number of times -- the least any pass over the sites can cost -- and tests/parsimony_model.py,
the plain-Python statement of the same rules, on the first SAMPLE sites, whose result is compared with the device's, change for change.
Writes one JSON document (default: profiles/parsimony_timing.json), after every workload."""
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
import parsimony_model as PM                                                       # noqa: E402
from density_timing import MIN_BLOCK_SIZE, WIDE_LEN, WIDE_ROWS, wide_records      # noqa: E402
from sibelia_amd import BlockFinder, pipeline as P, tree, workloads as W           # noqa: E402
from sibelia_amd.api import CONCAT_VARIABLE                                        # noqa: E402

RUNS = 5
SAMPLE = 10000
SEED = 1


def spread(values):
    return {"median": statistics.median(values), "lowest": min(values), "highest": max(values), "all": values}


def copy_ms(nbytes):
    """a device-to-device copy of nbytes, RUNS times after a warm-up, by events"""
    src = torch.randint(0, 255, (max(1, nbytes),), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    out = []
    for i in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return out


def measure(bf, cls, n, want):
    counts, C, K = bf.group_bootstrap(cls, n, 0, SEED, 0, want)
    main = tree.neighbour_joining(tree.distances(counts[0], K, "p"))
    edges = [(u, v) for u, v, _ in main.edges]
    call, kernel, copy = [], [], []
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        ecounts, steps, least, changes = bf.group_parsimony(edges)
        t1 = time.perf_counter()
        k, c = bf.group_parsimony_times()
        if i:
            call.append((t1 - t0) * 1e3)
            kernel.append(k)
            copy.append(c)
    packed_bytes = C * ((n + 31) // 32) * 8
    # the host's statement of the rules on the first SAMPLE sites
    text = bf.group_concat(cls, n, [b">%d\n" % f for f in range(n)], CONCAT_VARIABLE, 2 ** 31, want)[0]
    rows = [line[:SAMPLE] for line in text.split(b"\n")[1::2]]
    assert len(rows) == n and len(rows[0]) == min(C, SAMPLE)
    t0 = time.perf_counter()
    hcounts, hsteps, hleast, hchanges = PM.fitch(rows, None, edges)
    host = (time.perf_counter() - t0) * 1e3
    m = len(hsteps)
    head = changes[changes["site"] < m]
    assert steps[:m].tolist() == hsteps and least[:m].tolist() == hleast, "the device's steps are not the model's"
    assert list(zip(head["site"].tolist(), head["edge"].tolist(), head["from"].tolist(), head["to"].tolist())) == hchanges, "the device's changes are not the model's"
    assert int(ecounts.sum()) == int(steps.sum()) == len(changes)
    return {"files": n, "sites": C, "clean_columns": K, "changes": int(len(changes)), "steps": int(steps.sum()), "minsteps": int(least.sum()),
            "homoplasic_sites": int((steps > least).sum()), "packed_bytes": packed_bytes, "change_list_bytes": int(changes.nbytes),
            "device_call_ms": spread(call), "device_kernel_ms": spread(kernel), "device_copy_ms": spread(copy),
            "d2d_copy_of_packed_sites_ms": spread(copy_ms(packed_bytes)),
            "host_model_sites": m, "host_model_ms": host, "host_model_us_per_site": host * 1e3 / max(1, m),
            "device_kernel_us_per_site": statistics.median(kernel) * 1e3 / max(1, C)}


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
    res["input"] = "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d, the core blocks" % MIN_BLOCK_SIZE
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
    res["input"] = "one group of %d rows x %d columns, the records of tools/density_timing.py" % (WIDE_ROWS, WIDE_LEN)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parsimony_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/parsimony_timing.py", "runs": RUNS, "sample": SAMPLE, "model": "p"}
    for name, fn in (("wide", wide), ("strains", strains)):
        res[name] = fn()
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res[name], sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
