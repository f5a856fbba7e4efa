#!/usr/bin/env python3
"""Times the soft core (sbl_group_set_partial) on the 8-strain workload of sibelia_amd/workloads.py (gen_strains: 8 x 4.6
Mbp, `-s loose`, minimum block size 5000, B = 1000): the pipeline runs up to the final block list and aligns its groups once
(sbl_align_block_groups); on the rows that call left on the device, in ONE process,
  strict_off   sbl_group_concat ALL, sbl_group_concat VARIABLE and sbl_group_bootstrap over the strict core blocks, the setting off
  strict_on    the same calls over the same blocks with the setting on: the results are the same, only the instantiations differ
  soft_on      the same calls with the setting on over the soft core at --coremin 6 (pipeline.soft_core_blocks); the number of soft-core
               blocks at every --coremin is recorded, and where --coremin 2 gives another set than 6 it is measured too (soft_on_coremin_2)
each RUNS + 1 times (the first is a warm-up).  Kernel times are the library's own counters (event pairs), medians with all values beside
them.  The bootstrap call runs with 0 replicates and with B: the difference of the two medians is the replicate phase, which is
k_boot_count alone.
--trace runs the same calls once more in a child process under rocprofv3's kernel trace and reads the time of every launch of
k_boot_count<false>, k_boot_count<true>, k_boot_clean and k_boot_clean_groups from it: per call the sum over its launches, the warm-up
call dropped -- k_boot_count on equal input in both instantiations, measured directly, and the kernel time of the per-group clean count.
Writes one JSON document (default: profiles/softcore_timing.json).  With SOFTCORE_TIMING_STRICT_ONLY=1 only strict_off is measured and
nothing of the setting is called: what a build of the parent commit can run, for an A/B of the strict path in one session;
--parent=FILE takes the document such a run wrote, keeps its numbers as strict_parent and adds the ratios of strict_off to them."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = 5
B = 1000
SEED = 1
COREMIN = 6
MIN_BLOCK_SIZE = 5000
STRICT_ONLY = os.environ.get("SOFTCORE_TIMING_STRICT_ONLY") == "1"
KERNELS = ("k_boot_count<false>", "k_boot_count<true>", "k_boot_clean_groups", "k_boot_clean")


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "all": values}


def measure(bf, cls, n, want, partial):
    from sibelia_amd.api import CONCAT_ALL, CONCAT_VARIABLE
    if not STRICT_ONLY:
        bf.set_partial(partial)
    headers = [b">strain%d\n" % i for i in range(n)]
    res, sizes = {}, {}
    try:
        for label, mode in (("concat_all_kernel_ms", CONCAT_ALL), ("concat_variable_kernel_ms", CONCAT_VARIABLE)):
            ms = []
            for i in range(RUNS + 1):
                text, parts, sites = bf.group_concat(cls, n, headers, mode, 80, want)
                if i:
                    ms.append(bf.group_concat_times()[0])
            res[label] = spread(ms)
            sizes["columns" if mode == CONCAT_ALL else "sites"] = sum(k for _, _, k in parts)
            sizes["blocks"] = len(parts)
        for label, reps in (("bootstrap_sites_kernel_ms", 0), ("bootstrap_kernel_ms", B)):
            ms = []
            for i in range(RUNS + 1):
                counts, C, K = bf.group_bootstrap(cls, n, reps, SEED, 0, want)
                if i:
                    ms.append(bf.group_bootstrap_times()[0])
            res[label] = spread(ms)
        assert C == sizes["sites"]
        sizes["clean_columns"] = K
        res["replicate_kernel_ms"] = res["bootstrap_kernel_ms"]["median"] - res["bootstrap_sites_kernel_ms"]["median"]
        res["replicate_kernel_ms_is"] = "bootstrap_kernel_ms - bootstrap_sites_kernel_ms, a difference of two medians: the launches of k_boot_count for the replicates"
        res.update(sizes)
        res["checksum"] = int(counts.sum())
    finally:
        if not STRICT_ONLY:
            bf.set_partial(False)
    return res


def workload():
    from sibelia_amd import BlockFinder, pipeline as P, workloads as W
    seqs = W.gen_strains()
    names = ["strain%d" % i for i in range(len(seqs))]
    stages = P.PARAMETER_SETS["loose"]
    last_k, trim_k = P.final_k(stages, MIN_BLOCK_SIZE)
    bf = BlockFinder(seqs, device=0)
    for k, d in stages:
        bf.PerformGraphSimplifications(k, d, 4)
    bf.GenerateSyntenyBlocks(last_k, trim_k, MIN_BLOCK_SIZE)
    blocks, _ = bf.postprocess(names)
    n = len(seqs)
    ids, insts, aligned = bf.align_block_groups(MIN_BLOCK_SIZE)
    cls = [c for inst in insts for c, _, _, _ in inst]                           # one record per strain: the record is the file
    ok = lambda chosen: [b in chosen and a.status == 0 for b, a in zip(ids, aligned)]      # noqa: E731
    strict = ok(set(P.core_blocks(blocks, [1] * n, MIN_BLOCK_SIZE)))
    soft = {} if STRICT_ONLY else {m: ok(set(P.soft_core_blocks(blocks, [1] * n, MIN_BLOCK_SIZE, m))) for m in range(2, n + 1)}
    return bf, cls, n, strict, soft


def run_all():
    bf, cls, n, strict, soft = workload()
    try:
        res = {"strict_off": measure(bf, cls, n, strict, False)}
        if not STRICT_ONLY:
            res["strict_on"] = measure(bf, cls, n, strict, True)
            res["soft_on"] = measure(bf, cls, n, soft[COREMIN], True)
            res["soft_core_blocks_by_coremin"] = {str(m): sum(w) for m, w in sorted(soft.items())}
            if soft[2] != soft[COREMIN]:                # the widest soft core, where it is another one
                res["soft_on_coremin_2"] = measure(bf, cls, n, soft[2], True)
            same = ("blocks", "columns", "sites", "clean_columns", "checksum")
            assert [res["strict_on"][k] for k in same] == [res["strict_off"][k] for k in same]
            a, b = res["strict_off"], res["strict_on"]
            res["partial_over_strict"] = {k: b[k]["median"] / a[k]["median"] for k in ("concat_all_kernel_ms", "concat_variable_kernel_ms", "bootstrap_kernel_ms")}
            res["partial_over_strict"]["replicate_kernel_ms"] = b["replicate_kernel_ms"] / a["replicate_kernel_ms"]
    finally:
        bf.close()
    return res


def traced():
    """the per-call kernel times of the bootstrap kernels from a kernel trace of a child process that runs the same calls"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"],
                       check=True, stdout=subprocess.DEVNULL, timeout=900)
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    launches = {k: [(e - s) / 1e6 for name, s, e in rows if k in name and (k != "k_boot_clean" or "k_boot_clean_groups" not in name)] for k in KERNELS}
    per = 3 * (RUNS + 1)               # k_boot_count launches of one measure(): RUNS + 1 calls without replicates (slab 0) and RUNS + 1 with B
    out = {"launches": {k: len(v) for k, v in launches.items()}}     # (slab 0, then the one batch of B replicates)

    def replicates(ms):                # the launch over the B replicates of every call but the warm-up
        assert len(ms) == per, len(ms)
        return spread(ms[RUNS + 1:][1::2][1:])

    def clean(ms):                     # one launch per bootstrap call; the first call of both kinds dropped
        assert len(ms) == 2 * (RUNS + 1), len(ms)
        return spread(ms[1:RUNS + 1] + ms[RUNS + 2:])
    strict, partial = launches["k_boot_count<false>"], launches["k_boot_count<true>"]
    if len(strict) == per and len(partial) in (2 * per, 3 * per):
        out["k_boot_count_replicates_ms"] = {"strict_off": replicates(strict), "strict_on": replicates(partial[:per]), "soft_on": replicates(partial[per:2 * per])}
        if len(partial) == 3 * per:
            out["k_boot_count_replicates_ms"]["soft_on_coremin_2"] = replicates(partial[2 * per:])
        r = out["k_boot_count_replicates_ms"]
        out["k_boot_count_partial_over_strict"] = {"median": r["strict_on"]["median"] / r["strict_off"]["median"],
                                                   "lowest": r["strict_on"]["min"] / r["strict_off"]["max"], "highest": r["strict_on"]["max"] / r["strict_off"]["min"]}
    g = launches["k_boot_clean_groups"]
    if len(launches["k_boot_clean"]) == 2 * (RUNS + 1) and len(g) in (4 * (RUNS + 1), 6 * (RUNS + 1)):
        out["clean_count_kernel_ms"] = {"k_boot_clean strict_off": clean(launches["k_boot_clean"]), "k_boot_clean_groups strict_on": clean(g[:2 * (RUNS + 1)]),
                                        "k_boot_clean_groups soft_on": clean(g[2 * (RUNS + 1):4 * (RUNS + 1)])}
        if len(g) == 6 * (RUNS + 1):
            out["clean_count_kernel_ms"]["k_boot_clean_groups soft_on_coremin_2"] = clean(g[4 * (RUNS + 1):])
    return out


def main():
    if "--child" in sys.argv:
        run_all()
        return
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "softcore_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/softcore_timing.py", "runs": RUNS, "replicates": B, "seed": SEED, "coremin": COREMIN,
           "strict_only": STRICT_ONLY,
           "input": "workloads.gen_strains() (8 x 4.6 Mbp), -s loose -m %d; the strict core and the soft core at --coremin %d" % (MIN_BLOCK_SIZE, COREMIN)}
    res.update(run_all())
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for a in sys.argv[1:]:
        if a.startswith("--parent="):
            with open(a[len("--parent="):]) as f:
                parent = json.load(f)["strict_off"]
            res["strict_parent"] = parent
            res["strict_over_parent"] = {k: res["strict_off"][k]["median"] / parent[k]["median"]
                                         for k in ("concat_all_kernel_ms", "concat_variable_kernel_ms", "bootstrap_sites_kernel_ms", "bootstrap_kernel_ms")}
            assert all(res["strict_off"][k] == parent[k] for k in ("blocks", "columns", "sites", "clean_columns", "checksum"))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    if "--trace" in sys.argv and not STRICT_ONLY:
        res["kernel_trace"] = traced()
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_trace"}, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
