#!/usr/bin/env python3
"""A/B timing of the headline workload against the parent commit (written for the one-launch commit, used again for the listed
walking probe): `python bench.py --no-cpu-baseline` RUNS times in a built checkout of the parent commit and RUNS times in this tree,
alternating (parent first), each run a process of its own; then one `--full --no-cpu-full --no-cpu-baseline` run per tree for the state
hash and the check against the reference's fixture.  Every run is kept (ms_per_step, rounds, bulges, phase_ms);
the summary holds the medians, the parent's own spread (max - min) and whether the head's median is below the parent's by more than
three times that spread -- the acceptance bound of both changes.

usage: tools/one_launch_timing.py PARENT_TREE [OUT.json]      (default OUT: profiles/one_launch_timing.json;
                                                               the listed probe: profiles/listed_probe_timing.json)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5


def bench(tree, extra=()):
    """one bench.py process in `tree`; its JSON result line"""
    p = subprocess.run([sys.executable, "bench.py", "--no-cpu-baseline", *extra], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("bench.py failed in %s (exit %d):\n%s" % (tree, p.returncode, p.stderr[-4000:]))
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    return json.loads(lines[-1])


def brief(r):
    return {"ms_per_step": r["ms_per_step"], "rounds": r["config"]["rounds"], "bulges": r["config"]["bulges"], "iterations": r["config"]["iterations"],
            "replays": r["config"]["replays"], "phase_ms": r["phase_ms"]}


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "one_launch_timing.json")
    trees = {"parent": parent, "head": ROOT}
    runs = {"parent": [], "head": []}
    for i in range(RUNS):
        for name in ("parent", "head"):
            r = brief(bench(trees[name]))
            runs[name].append(r)
            print("run %d %-6s %.3f ms/step, %d rounds" % (i, name, r["ms_per_step"], r["rounds"]), flush=True)
    full = {}
    for name in ("parent", "head"):
        r = bench(trees[name], ("--full", "--no-cpu-full"))
        full[name] = {"ms_per_step": r["ms_per_step"], "rounds": r["config"]["rounds"], "bulges": r["config"]["bulges"],
                      "state_sha256": r["state_sha256"], "matches_reference_fixture": r["matches_reference_fixture"],
                      "roofline": r.get("roofline")}
        print("full  %-6s sha %s fixture %s" % (name, r["state_sha256"][:16], r["matches_reference_fixture"]), flush=True)
    ms = {n: [x["ms_per_step"] for x in runs[n]] for n in runs}
    spread = max(ms["parent"]) - min(ms["parent"])
    med = {n: statistics.median(ms[n]) for n in ms}
    res = {"tool": "tools/one_launch_timing.py", "command": "python bench.py --no-cpu-baseline", "runs_per_tree": RUNS, "order": "alternating, parent first",
           "runs": runs, "full": full,
           "summary": {"parent_median_ms": med["parent"], "head_median_ms": med["head"], "gain_ms": med["parent"] - med["head"],
                       "parent_spread_ms": spread, "head_spread_ms": max(ms["head"]) - min(ms["head"]),
                       "gain_exceeds_3x_parent_spread": med["parent"] - med["head"] > 3 * spread,
                       "same_rounds": len({x["rounds"] for n in runs for x in runs[n]}) == 1,
                       "same_bulges": len({x["bulges"] for n in runs for x in runs[n]}) == 1,
                       "same_state_sha256": full["parent"]["state_sha256"] == full["head"]["state_sha256"],
                       "head_matches_reference_fixture": full["head"]["matches_reference_fixture"]}}
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:      # noqa: BLE001 -- the name is a label only
        res["device"] = None
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res["summary"], sort_keys=True))


if __name__ == "__main__":
    main()
