#!/usr/bin/env python3
"""Times the text kernel (k_spell_text, csrc/spell_text.hip) on the pieces of blocks_sequences.fasta (csrc/blockseq.hip) next to a
device-to-device copy of as many bytes as the text it writes.

Three inputs: the final block list of `-s loose -r -q` on tests/golden/data/Helicobacter_pylori.fa.gz, one forward plus one reverse
whole-record instance for each of 8 records of 4.6 Mbp, and the 100 000 instances of one to three bases of
tests/test_gpu_blockseq.py::test_hundred_thousand_tiny_instances (same records, same seed): the shape with the most pieces per
workgroup span.  Kernel and device-to-host times are the library's own event pairs
(sbl_blocks_sequences_times); the copy is a hipMemcpyAsync between two device buffers timed by an event pair in the same process.
One warm-up, then RUNS runs; medians are reported.  Writes one JSON document (default: profiles/blockseq_timing.json)."""
import ctypes as C
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sibelia_amd import BlockFinder, formats as F, pipeline as P      # noqa: E402

RUNS = 7


def d2d_copy_ms(nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    times = []
    for i in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None)      # hipMemcpyDeviceToDevice, null stream (torch's default)
        b.record()
        torch.cuda.synchronize()
        assert rc == 0
        if i:
            times.append(a.elapsed_time(b))
    return times


def measure(bf, blocks, names):
    kernel, d2h, text = [], [], b""
    for i in range(RUNS + 1):
        text = bf.blocks_sequences(blocks, names)
        k, d = bf.blocks_sequences_times()
        if i:
            kernel.append(k)
            d2h.append(d)
    copy = d2d_copy_ms(len(text))
    km, cm, dm = statistics.median(kernel), statistics.median(copy), statistics.median(d2h)
    return {"instances": int(len(blocks)) if blocks is not None else None, "text_bytes": len(text), "runs": RUNS,
            "kernel_ms": km, "kernel_ms_all": kernel, "d2d_copy_ms": cm, "d2d_copy_ms_all": copy, "kernel_over_copy": km / cm,
            "kernel_gb_per_s": len(text) / km / 1e6, "d2d_copy_gb_per_s": len(text) / cm / 1e6, "device_to_host_ms": dm}


def tiny_instances():
    """the records of the test module's `small` finder and the list of its test -> (finder, blocks, names)"""
    rng = np.random.default_rng(11)
    seqs = [bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()) for n in (1000, 161, 3000)]
    for s in seqs:
        for p in rng.choice(len(s), len(s) // 7, replace=False):
            s[int(p)] = b"NRYKMSWBDHX-U"[int(rng.integers(0, 13))]
    seqs[1][:6], seqs[1][-6:] = b"NRYACG", b"TTYRNA"
    bf = BlockFinder([bytes(s) for s in seqs], device=0)
    rng, n = np.random.default_rng(7), 100_000
    chr_ = rng.integers(0, 3, n)
    ln = rng.integers(1, 4, n)
    start = np.array([rng.integers(0, len(seqs[c]) - l + 1) for c, l in zip(chr_, ln)])
    blocks = np.zeros(n, dtype=F.BLOCK_DTYPE)
    blocks["id"] = rng.integers(1, 5000, n) * rng.choice([-1, 1], n)
    blocks["chr"], blocks["start"], blocks["end"] = chr_, start, start + ln
    return bf, blocks, ["gi|15644634|ref|NC_000915.1|", "plain_name", "a.b.c"]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "blockseq_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/blockseq_timing.py"}
    with tempfile.TemporaryDirectory() as wd:
        fa = os.path.join(wd, "Helicobacter_pylori.fa")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "data", "Helicobacter_pylori.fa.gz"), "rb") as f, open(fa, "wb") as g:
            shutil.copyfileobj(f, g)
        bf = BlockFinder.from_fasta(fa, device=0)
        stages = P.PARAMETER_SETS["loose"]
        for k, d in stages:
            bf.PerformGraphSimplifications(k, d, 4)
        last_k, trim_k = P.final_k(stages, 5000)
        bf.GenerateSyntenyBlocks(last_k, trim_k, 5000)
        blocks, _ = bf.postprocess()
        res["hpylori_loose_q"] = measure(bf, blocks, None)
        bf.close()
    rng = np.random.default_rng(1)
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4_600_000)].tobytes() for _ in range(8)]
    bf = BlockFinder(seqs, device=0)
    blocks = np.array([(s * (c + 1), c, 0, len(seqs[c])) for c in range(8) for s in (1, -1)], dtype=F.BLOCK_DTYPE)
    res["whole_records_8x4600k_both_strands"] = measure(bf, blocks, ["strain%d" % c for c in range(8)])
    bf.close()
    res["tiny_instances_100k"] = measure(*tiny_instances())
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
