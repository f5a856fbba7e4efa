"""The inputs of the --correctboundaries fixtures (tests/golden/correct_cases.json) and how a program is run on them; shared by the
tests and by the generator of the fixtures (tests/golden/gen/make_correct_golden.py).

Inputs: "split:<name>" = tests/golden/data/<name>.fa.gz with its FIRST record written to file 0 and all the others to file 1 (the
Staphylococcus aureus example is a finished genome followed by the 179 contigs of an assembly of another strain: reference and
assembly, the use the option was made for); "craft:<name>" = a few kbp, committed in tests/golden/data/correct_crafted.json as the
generator made them."""
import gzip
import hashlib
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
CRAFTED = os.path.join(DATA, "correct_crafted.json")

_crafted = None


def crafted_inputs():
    """{name: {"files": [[[record name, sequence]] per file], "stage": stage file text, "min_block_size": m, "again": [indices of files
    named once more on the command line]}}"""
    global _crafted
    if _crafted is None:
        with open(CRAFTED) as f:
            _crafted = json.load(f)
    return _crafted


def records_of(inp):
    """-> [[(name, sequence)] per file], stage file text or None, minimum block size or None"""
    kind, name = inp.split(":")
    if kind == "craft":
        c = crafted_inputs()[name]
        return [[(n, s.encode()) for n, s in f] for f in c["files"]], c["stage"], c["min_block_size"]
    recs = []
    with gzip.open(os.path.join(DATA, name + ".fa.gz"), "rb") as f:
        for line in f:
            line = line.strip()
            if line[:1] == b">":
                recs.append([line[1:].split()[0].decode(), bytearray()])
            elif line:
                recs[-1][1] += line.upper()
    recs = [(n, bytes(s)) for n, s in recs]
    return [recs[:1], recs[1:]], None, None


def write_inputs(inp, workdir):
    """-> file names"""
    files, stage, _ = records_of(inp)
    names = []
    for i, recs in enumerate(files):
        names.append("in%d.fa" % i)
        with open(os.path.join(workdir, names[-1]), "wb") as g:
            for n, s in recs:
                g.write(b">" + n.encode() + b"\n")
                for o in range(0, len(s), 80):
                    g.write(s[o:o + 80] + b"\n")
    kind, name = inp.split(":")
    if kind == "craft":
        names += [names[i] for i in crafted_inputs()[name].get("again", [])]
    if stage is not None:
        with open(os.path.join(workdir, "stages.txt"), "w") as g:
            g.write(stage)
    return names


def run_case(program, inp, args, workdir, env=None):
    """-> (returncode, sha256 of stdout, {relative path: [size, sha256]}, stdout, stderr); files are left under workdir/out"""
    names = write_inputs(inp, workdir)
    p = subprocess.run([program] + args + ["-o", "out"] + names, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=3600)
    files = {}
    for d, _, found in os.walk(os.path.join(workdir, "out")):
        for n in found:
            path = os.path.join(d, n)
            b = open(path, "rb").read()
            files[os.path.relpath(path, os.path.join(workdir, "out"))] = [len(b), hashlib.sha256(b).hexdigest()]
    return p.returncode, hashlib.sha256(p.stdout).hexdigest(), files, p.stdout, p.stderr
