#!/usr/bin/env python3
"""Times the multiple alignment of every block (sbl_align_block_groups in csrc/block_align.hip) with and without the global band class
(sbl_align_set_wide, --wideband) on the 8-strain workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6 Mbp),
`-s loose`, minimum block size 5000, as tools/multimaf_timing.py runs it.  The pipeline runs up to the final block list once; then, per
gap opening cost (default 0 and 300) and per setting (off, on), the call runs RUNS + 1 times on that list (the first is a warm-up).
Kernel times are the library's own counters (sbl_align_stats / sbl_align_wide_stats: event pairs), medians.

Per cost and setting one document `open_<cost>_<off|on>`: pairs, skipped pairs and groups, passes, launches, cells, pairs_by_band_w,
kernel_ms, the counters of the global class, the most band offsets a pair reached, and the pairs still skipped with the limit that
skipped each (found by one more, untimed, sbl_align_pairs call on the members of the skipped groups).  Per cost also `class_rate_<cost>`:
the pairs that ended in the widest LDS class run once more at the w they ended at (SBL_TEST_GALIGN_W0), alone, first through that class
and then -- the same pairs, the same cells -- through the global class (SBL_TEST_GALIGN_WIDE_FROM=0): cells per second of either, which
is what the score arrays in device memory cost.

usage: tools/wideband_timing.py [OUT.json [COST | off | on ...]]      (default OUT: profiles/wideband_timing.json, costs 0 and 300,
both settings; the documents that a call does not write are kept as the file has them -- a call with the setting on takes minutes per
cost, so the parts can be run one at a time)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sibelia_amd import BlockFinder, pipeline as P, workloads as W    # noqa: E402

RUNS = 5
MIN_BLOCK_SIZE = 5000
W0 = 64
MAX_DIAG, PAIR_CAP = 1 << 23, 8 << 30                                   # GA_MAX_DIAG, GA_PAIR_CAP (csrc/block_align.hip)
LIMITS = {False: (4096, 12288, 1), True: (2048, 4992, 2)}               # per model: MID_W, MAX_W, code bytes of a lane's 4 cells


def offsets(n, m, w):
    return abs(m - n) + 2 * min(w, n, m) + 1


def limit_of(n, m, al, affine, wide):
    """the limit that skipped the pair `al` (a PairAlignment): it was about to run at twice the w it ran at last"""
    if n + m >= MAX_DIAG:
        return "length"
    w = min(2 * al.band_w if al.passes else W0, n, m)
    width = offsets(n, m, w)
    _, max_w, code = LIMITS[affine]
    if ((width + 1) // 2 + 3) // 4 * code * (n + m + 1) > PAIR_CAP:
        return "trace memory"
    return "band width" if not wide and width > max_w else "unknown"


def pairs_of(insts, groups):
    """(group, descriptor) of centre against member for the groups given"""
    out = []
    for g in groups:
        c, s, e, rev = insts[g][0]
        out += [(g, (c, s, e, rev, mc, ms, me, mrev)) for mc, ms, me, mrev in insts[g][1:]]
    return out


def document(bf, cost, wide):
    bf.set_gap_open(cost)
    bf.set_wide(wide)
    kernel, wide_ms, st, ws = [], [], {}, {}
    for i in range(RUNS + 1):
        ids, insts, aligned = bf.align_block_groups(MIN_BLOCK_SIZE)
        st, ws = bf.align_stats(), bf.align_wide_stats()
        if i:
            kernel.append(st["kernel_ms"])
            wide_ms.append(ws["kernel_ms"])
        print("cost %d wide %d run %d: kernel %.1f ms, global class %.1f ms" % (cost, wide, i, st["kernel_ms"], ws["kernel_ms"]), flush=True)
    by_w, widest = {}, 0
    for inst, a in zip(insts, aligned):
        n = inst[0][2] - inst[0][1]
        for (_, s, e, _), (_, w, passes) in zip(inst[1:], a.members):
            by_w[w] = by_w.get(w, 0) + 1
            if passes:
                widest = max(widest, offsets(n, e - s, w))
    skipped_groups = [g for g, a in enumerate(aligned) if a.status != 0]
    todo = pairs_of(insts, skipped_groups)
    still = []
    if todo:
        for (g, d), al in zip(todo, bf.align_pairs([d for _, d in todo])):
            if al.status != 0:
                n, m = d[2] - d[1], d[6] - d[5]
                still.append({"block": int(ids[g]), "n": n, "m": m, "last_band_w": al.band_w, "passes": al.passes, "limit": limit_of(n, m, al, cost > 0, wide)})
    doc = {"gap_open": cost, "wide": int(wide), "runs": RUNS, "groups": len(aligned), "groups_skipped": len(skipped_groups),
           "pairs": st["pairs"], "pairs_skipped": st["skipped"], "passes": st["passes"], "launches": st["launches"], "cells": st["cells"],
           "pairs_by_band_w": {str(w): by_w[w] for w in sorted(by_w)}, "most_band_offsets": widest,
           "kernel_ms": statistics.median(kernel), "kernel_ms_all": kernel,
           "wide_stats": {"pairs": ws["pairs"], "passes": ws["passes"], "launches": ws["launches"], "cells": ws["cells"],
                          "kernel_ms": statistics.median(wide_ms), "kernel_ms_all": wide_ms},
           "still_skipped": still}
    return doc, insts, aligned


def class_rate(bf, cost, insts, aligned):
    """the pairs that ended in the widest LDS class, alone, one pass at the w they ended at: through that class, then through the global one"""
    mid_w, max_w, _ = LIMITS[cost > 0]
    by_w = {}
    for inst, a in zip(insts, aligned):
        if a.status != 0:
            continue
        c, s, e, rev = inst[0]
        for (mc, ms, me, mrev), (_, w, _) in zip(inst[1:], a.members):
            if mid_w < offsets(e - s, me - ms, w) <= max_w:
                by_w.setdefault(w, []).append((c, s, e, rev, mc, ms, me, mrev))
    out = {"gap_open": cost, "pairs": sum(len(v) for v in by_w.values()), "runs": RUNS}
    bf.set_gap_open(cost)
    try:
        for name, wide in (("lds_widest", False), ("global", True)):
            bf.set_wide(wide)
            if wide:
                os.environ["SBL_TEST_GALIGN_WIDE_FROM"] = "0"
            cells, ms = 0, []
            for i in range(RUNS + 1):
                cells, total = 0, 0.0
                for w, descs in sorted(by_w.items()):
                    os.environ["SBL_TEST_GALIGN_W0"] = str(w)
                    got = bf.align_pairs(descs)
                    st = bf.align_stats()
                    assert all(g.passes == 1 and g.status == 0 for g in got) and st["passes"] == len(descs)
                    cells += st["cells"]
                    total += st["kernel_ms"]
                if i:
                    ms.append(total)
            med = statistics.median(ms) if ms else 0.0
            out[name] = {"cells": cells, "kernel_ms": med, "kernel_ms_all": ms, "cells_per_s": cells / (med * 1e-3) if med else None}
    finally:
        os.environ.pop("SBL_TEST_GALIGN_W0", None)
        os.environ.pop("SBL_TEST_GALIGN_WIDE_FROM", None)
        bf.set_wide(False)
    if out["pairs"]:
        out["global_over_lds_time"] = out["global"]["kernel_ms"] / out["lds_widest"]["kernel_ms"]
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wideband_timing.json")
    costs = [int(x) for x in sys.argv[2:] if x not in ("off", "on")] or [0, 300]
    settings = [x == "on" for x in ("off", "on") if x in sys.argv[2:]] or [False, True]
    res = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            res = json.load(f)
    torch.cuda.init()
    res.update({"device": torch.cuda.get_device_name(0), "tool": "tools/wideband_timing.py",
                "input": "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d" % MIN_BLOCK_SIZE})
    seqs = W.gen_strains()
    names = ["strain%d" % i for i in range(len(seqs))]
    stages = P.PARAMETER_SETS["loose"]
    last_k, trim_k = P.final_k(stages, MIN_BLOCK_SIZE)
    bf = BlockFinder(seqs, device=0)
    for k, d in stages:
        bf.PerformGraphSimplifications(k, d, 4)
    bf.GenerateSyntenyBlocks(last_k, trim_k, MIN_BLOCK_SIZE)
    bf.postprocess(names)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)

    for cost in costs:
        for wide in settings:
            doc, insts, aligned = document(bf, cost, wide)
            res["open_%d_%s" % (cost, "on" if wide else "off")] = doc
            save()
            if not wide:
                res["class_rate_%d" % cost] = class_rate(bf, cost, insts, aligned)
                save()
    bf.close()
    print(json.dumps({k: ({x: v[x] for x in ("pairs_skipped", "groups_skipped", "kernel_ms", "most_band_offsets")} if k.startswith("open_") else v)
                      for k, v in res.items() if k.startswith(("open_", "class_rate_"))}, sort_keys=True))


if __name__ == "__main__":
    main()
