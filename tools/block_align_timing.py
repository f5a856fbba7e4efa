#!/usr/bin/env python3
"""Times the alignment of the unique blocks (--maf / --variants; csrc/block_align.hip) on the Staphylococcus aureus example: the
finished genome as the reference set, the 179 contigs as the assembly, `-s fine -m 500 --lastk 30 --nopostprocess --correctboundaries`,
the command line C-Sibelia.py gives the reference program.  The pipeline runs up to the corrected block list once; then
sbl_align_unique_blocks runs RUNS + 1 times on that list (the first is a warm-up).  Kernel and spelling times are the library's own
counters (sbl_align_stats: event pairs), the whole call is timed on the host; medians.  There is nothing to compare with: the parent has
no such step and LAGAN cannot be run.  Writes one JSON document (default: profiles/block_align_timing.json)."""
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
MIN_BLOCK_SIZE, LAST_K = 500, 30


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "block_align_timing.json")
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
    kernel, spell, call, st = [], [], [], {}
    for i in range(RUNS + 1):
        t0 = time.perf_counter()
        ids, descs, aligned = bf.align_unique_blocks(MIN_BLOCK_SIZE, len(files[0]))
        t1 = time.perf_counter()
        st = bf.align_stats()
        if i:
            kernel.append(st["kernel_ms"])
            spell.append(st["spell_ms"])
            call.append((t1 - t0) * 1e3)
    bf.close()
    km = statistics.median(kernel)
    longest = max((max(d[2] - d[1], d[6] - d[5]) for d in descs), default=0)
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/block_align_timing.py",
           "input": "Staphylococcus_aureus_pair: record 0 against records 1..179, -s fine -m 500 --lastk 30 --nopostprocess --correctboundaries",
           "runs": RUNS, "pairs": st["pairs"], "skipped": st["skipped"], "passes": st["passes"], "launches": st["launches"], "cells": st["cells"],
           "longest_instance": int(longest), "widest_band_w": max((a.band_w for a in aligned), default=0),
           "aligned_columns": sum(len(a.row_a) for a in aligned),
           "kernel_ms": km, "kernel_ms_all": kernel, "spell_ms": statistics.median(spell), "spell_ms_all": spell,
           "call_ms": statistics.median(call), "call_ms_all": call, "cells_per_s": st["cells"] / km * 1e3 if km else None}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
