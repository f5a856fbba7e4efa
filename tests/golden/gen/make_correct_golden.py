#!/usr/bin/env python3
"""Fixtures for --correctboundaries (tests/test_boundary_model.py, tests/test_gpu_correct_boundaries.py): the UNMODIFIED reference
program (oracle/_ref/sibelia_ref, built by oracle/build_dropin.sh) is run on the CPU on two-file inputs with the flag; return code,
sha256 of the standard output and size + sha256 of every file go to tests/golden/correct_cases.json in the format of
dropin_cases.json.  For the small cases and for the `fine` run the texts of blocks_coords.txt with and without the flag are kept
too, so that a failure can be read and the numpy model (tests/boundary_model.py) can be pinned to the reference without a GPU.

Inputs (tests/correct_fixtures.py reads them): "split:<name>" = an example of tests/golden/data split into two files; "craft:<name>" =
a few kbp built here from a seed (crafted) and written to tests/golden/data/correct_crafted.json FIRST, so that the tests read the very
bytes the reference program was run on and do not depend on the random number generator.

Every case is run twice and kept only if both runs agree; a case whose pre-correction list reaches a place where the reference is
undefined (tests/boundary_model.py: hits_undefined_case) is refused.  The wall-clock time of the reference with and without the flag
is recorded for the `loose` case, which runs before all the others with nothing beside it: their difference is the reference's CPU
time for the step on the host that ran this script."""
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
REF = os.path.join(ROOT, "oracle", "_ref", "sibelia_ref")
OUT = os.path.join(ROOT, "tests", "golden", "correct_cases.json")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from correct_fixtures import CRAFTED, records_of, run_case      # noqa: E402

FLAG = "--correctboundaries"


def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def _mutate(rng, s, rate, indel=0.0):
    out = bytearray()
    for ch in s:
        u = rng.random()
        if u < indel / 2:
            continue                                     # deletion
        if u < indel:
            out += _rand(rng, 1)                         # insertion before the base
        out.append(rng.choice([c for c in b"ACGT" if c != ch]) if rng.random() < rate else ch)
    return bytes(out)


def _ambiguous(rng, s, count):
    g = bytearray(s)
    for pos in rng.choice(len(g), count, replace=False):
        g[int(pos)] = b"NRYKMSWN"[int(rng.integers(0, 8))]
    return bytes(g)


def _rc(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def crafted(name):
    """-> ([[(record name, sequence)] per file], stage file text, minimum block size, files named once more).  A shared core is exact in both genomes; its
    flanks are shared with substitutions and a few indels, so the blocks the reference finds end somewhere inside the flanks and
    the local alignments move them."""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + len(name))

    def locus(core, flank, rate=0.08, indel=0.01):
        l, c, r = _rand(rng, flank), _rand(rng, core), _rand(rng, flank)
        return l + c + r, _mutate(rng, l, rate, indel) + c + _mutate(rng, r, rate, indel)

    stage, m, again = "1\n15 60\n", 300, []
    if name == "near_start":            # no predecessor and start < R
        a, b = locus(1400, 350)
        ref, asm = [a[280:] + _rand(rng, 900)], [_rand(rng, 700) + b + _rand(rng, 800)]
    elif name == "near_end":            # no successor, the right window is cut by the end of the record
        a, b = locus(1400, 350)
        ref, asm = [_rand(rng, 900) + a[:-260]], [_rand(rng, 600) + b + _rand(rng, 50)]
    elif name == "reverse_reference":   # the assembly carries the locus reversed
        a, b = locus(1500, 400)
        a2, b2 = locus(1300, 300)
        ref, asm = [_rand(rng, 800) + a + _rand(rng, 700) + a2 + _rand(rng, 600)], [_rand(rng, 500) + b2 + _rand(rng, 900) + _rc(b) + _rand(rng, 700)]
    elif name == "ambiguity_codes":
        a, b = locus(1500, 400)
        a = _ambiguous(rng, a[:400], 12) + a[400:1900] + _ambiguous(rng, a[1900:], 12)
        b = b[:200] + _ambiguous(rng, b[200:-200], 10) + b[-200:]
        ref, asm = [_rand(rng, 900) + a + _rand(rng, 900)], [_rand(rng, 700) + b + _rand(rng, 800)]
    elif name == "adjacent_blocks":     # two loci 90 bp apart in the reference, far apart and in the other order in the assembly
        a, b = locus(1200, 200)
        a2, b2 = locus(1000, 200)
        ref, asm = [_rand(rng, 800) + a + _rand(rng, 90) + a2 + _rand(rng, 800)], [_rand(rng, 600) + b2 + _rand(rng, 1500) + b + _rand(rng, 600)]
    elif name == "two_contigs":         # the assembly in two records, one locus on each, odd R
        a, b = locus(1300, 300)
        a2, b2 = locus(1100, 300)
        ref, asm = [_rand(rng, 700) + a + _rand(rng, 1100) + a2 + _rand(rng, 700)], [_rand(rng, 400) + _rc(b2) + _rand(rng, 400), _rand(rng, 300) + b + _rand(rng, 500)]
        m = 257
    elif name == "no_shared_block":     # unrelated sequences: the list is empty, the correction a no-op
        ref, asm = [_rand(rng, 3000)], [_rand(rng, 2500), _rand(rng, 700)]
    elif name == "three_files":
        ref, asm, again = [_rand(rng, 500)], [_rand(rng, 500)], [0]
    else:
        raise KeyError(name)
    return [[("ref%d" % i, s) for i, s in enumerate(ref)], [("ctg%d" % i, s) for i, s in enumerate(asm)]], stage, m, again


CRAFTED_NAMES = ("near_start", "near_end", "reverse_reference", "ambiguity_codes", "adjacent_blocks", "two_contigs", "no_shared_block", "three_files")
MIN_BLOCK_SIZE = {n: crafted(n)[2] for n in CRAFTED_NAMES}

# name, input, arguments before "-o out <files>", keep the texts of blocks_coords.txt
CASES = [
    ("saureus_loose_inram_correct_gff_sequences", "split:Staphylococcus_aureus_pair", ["-s", "loose", "-r", FLAG, "--gff", "-q"], False),
    ("saureus_fine_inram_m500_correct", "split:Staphylococcus_aureus_pair", ["-s", "fine", "-r", "-m", "500", FLAG], True),
] + [("craft_" + n, "craft:" + n, ["-k", "stages.txt", "-r", "-m", str(MIN_BLOCK_SIZE[n]), FLAG], n not in ("no_shared_block", "three_files")) for n in CRAFTED_NAMES]


def write_crafted():
    out = {}
    for n in CRAFTED_NAMES:
        files, stage, m, again = crafted(n)
        out[n] = {"files": [[[r, s.decode()] for r, s in f] for f in files], "stage": stage, "min_block_size": m, "again": again}
    with open(CRAFTED, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)


def min_block_size(args):
    return int(args[args.index("-m") + 1]) if "-m" in args else 5000


def _coords(workdir):
    p = os.path.join(workdir, "out", "blocks_coords.txt")
    return open(p).read() if os.path.exists(p) else None


def one(case):
    import boundary_model as BM
    name, inp, args, keep = case
    runs = []
    for _ in range(2):                                   # twice with the flag: a kept case is deterministic
        with tempfile.TemporaryDirectory() as wd:
            t0 = time.time()
            r = run_case(REF, inp, args, wd)
            runs.append((r[:3], r[3], r[4], _coords(wd), time.time() - t0))
    if runs[0][0] != runs[1][0] or runs[0][3] != runs[1][3]:
        sys.exit("case %s is not deterministic over two reference runs: replace it" % name)
    (rc, so, files), stdout, stderr, with_flag, t_with = runs[0]
    entry = {"name": name, "input": inp, "args": args, "returncode": rc, "stdout_sha256": so, "stdout_bytes": len(stdout), "files": files}
    if rc:
        entry["stderr"] = stderr.decode()
        return entry, None
    with tempfile.TemporaryDirectory() as wd:
        plain = [a for a in args if a not in (FLAG, "--gff")]
        t0 = time.time()
        r = run_case(REF, inp, plain, wd)
        t_without = time.time() - t0
        without = _coords(wd)
    if r[0] != 0 or without is None:
        sys.exit("case %s fails without the flag" % name)
    nref = len(records_of(inp)[0][0])
    m = min_block_size(args)
    if BM.hits_undefined_case([list(b) for b in BM.parse_blocks_coords(without)], nref, m):
        sys.exit("case %s reaches a place where the reference is undefined: replace it" % name)
    entry.update({"min_block_size": m, "n_reference_records": nref})
    if keep:
        if with_flag is None:
            sys.exit("case %s wrote no blocks_coords.txt" % name)
        entry.update({"coords_without_flag": without, "coords_with_flag": with_flag, "moved": with_flag != without})
    timing = {"with_flag_s": round(min(t_with, runs[1][4]), 2), "without_flag_s": round(t_without, 2)}
    print(name, "rc", rc, len(files), "files", "moved" if keep and with_flag != without else "", timing, file=sys.stderr)
    return entry, timing


if __name__ == "__main__":
    if not os.path.exists(REF):
        sys.exit("build oracle/_ref/sibelia_ref first: bash oracle/build_dropin.sh")
    from concurrent.futures import ThreadPoolExecutor
    write_crafted()
    only = [a for a in sys.argv[1:] if not a.startswith("-")]
    cases = [c for c in CASES if not only or c[0] in only]
    timed = [c for c in cases if c[0] == CASES[0][0]]
    done = [one(c) for c in timed]                       # alone: its wall clock is recorded
    with ThreadPoolExecutor(max_workers=3) as ex:
        done += list(ex.map(one, [c for c in cases if c not in timed]))
    cases = timed + [c for c in cases if c not in timed]
    out = {"generator": "tests/golden/gen/make_correct_golden.py", "program": "oracle/_ref/sibelia_ref (unmodified reference, oracle/build_dropin.sh)",
           "cases": sorted((e for e, _ in done), key=lambda e: [c[0] for c in CASES].index(e["name"]))}
    t = dict(zip((c[0] for c in cases), (t for _, t in done))).get(CASES[0][0])
    if t:
        out["reference_cpu_time"] = dict(t, case=CASES[0][0], correction_s=round(t["with_flag_s"] - t["without_flag_s"], 2),
                                         what="wall clock of the reference program on one core of the host that ran the generator, nothing running beside it; with_flag_s = the smaller of two runs, correction_s = with - without")
    if only:
        print(json.dumps(out, indent=1)[:3000])
    else:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
