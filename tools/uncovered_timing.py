#!/usr/bin/env python3
"""Times the text kernel of --uncovered (k_spell_text, csrc/spell_text.hip) next to a device-to-device copy of as many bytes as the text
it writes.

Two inputs: the VCF of the Staphylococcus aureus pair (tests/golden/data) under C-Sibelia's command line with --uncovered -- the piece
list the pipeline itself builds -- and a piece list of 16 whole records over 8 records of 4.6 Mbp, half of them wrapped into lines of
60.  Kernel and device-to-host times are the library's own event pairs (sbl_spell_text_times); the copy is a hipMemcpyAsync between two
device buffers timed by an event pair in the same process.  One warm-up, then RUNS runs; medians are reported.  Writes one JSON
document (default: profiles/uncovered_timing.json)."""
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from blockseq_timing import RUNS, d2d_copy_ms      # noqa: E402
from correct_fixtures import write_inputs          # noqa: E402
from sibelia_amd import BlockFinder, formats as F, pipeline as P      # noqa: E402


def measure(bf, pieces):
    kernel, d2h, text = [], [], b""
    arr = pieces.pieces()
    for i in range(RUNS + 1):
        text = bf.spell_text(arr, pieces.literals)
        k, d = bf.spell_text_times()
        if i:
            kernel.append(k)
            d2h.append(d)
    copy = d2d_copy_ms(len(text))
    km, cm, dm = statistics.median(kernel), statistics.median(copy), statistics.median(d2h)
    return {"pieces": int(len(arr)), "record_bytes": int(sum(int(p["end"] - p["start"]) for p in arr if p["kind"] == F.PIECE_RECORD)),
            "text_bytes": len(text), "runs": RUNS, "kernel_ms": km, "kernel_ms_all": kernel, "d2d_copy_ms": cm, "d2d_copy_ms_all": copy,
            "kernel_over_copy": km / cm, "kernel_gb_per_s": len(text) / km / 1e6, "d2d_copy_gb_per_s": len(text) / cm / 1e6, "device_to_host_ms": dm}


def saureus_vcf_pieces(wd):
    """the stages of `-s fine -m 500 --lastk 30 --correctboundaries --nopostprocess --allstages -r --variants --uncovered` through the
    API, up to the piece list of the VCF -> (finder, pieces)"""
    inputs = [os.path.join(wd, n) for n in write_inputs("split:Staphylococcus_aureus_pair", wd)]
    bf, names, nfirst = P.load_input(inputs, 0)
    stages, history = P.PARAMETER_SETS["fine"], []
    for i, (k, d) in enumerate(stages):
        history.append(bf.GenerateSyntenyBlocks(k, P.stage_trim_k(stages, i), k, False))
        bf.PerformGraphSimplifications(k, d, 4)
    _, trim_k = P.final_k(stages, 500, 30)
    bf.GenerateSyntenyBlocks(30, trim_k, 500, False)
    bf.postprocess(names, glue=False)
    blocks, _ = bf.correct_boundaries(500, nfirst, names)
    history.append(blocks)
    ids, descs, aligned = bf.align_unique_blocks(500, nfirst)
    records = []
    for (ca, sa, ea, ra, *_), al in zip(descs, aligned):
        if al.status == 0:
            records += [(names[ca],) + v for v in F.variants_from_runs(al.runs, al.row_a, al.row_b, sa, ea, ra)]
    calls = bf.uncovered_calls(history, 500, nfirst)
    return bf, F.vcf_pieces(names, bf.record_sizes()[0], P.first_base(inputs[0]), records, calls, True), calls


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "uncovered_timing.json")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "tool": "tools/uncovered_timing.py"}
    with tempfile.TemporaryDirectory() as wd:
        bf, pieces, calls = saureus_vcf_pieces(wd)
        res["saureus_vcf"] = dict(measure(bf, pieces), calls={k: int((calls["kind"] == v).sum()) for k, v in
                                                               (("deletions", F.CALL_DELETION), ("insertions", F.CALL_INSERTION), ("unmapped", F.CALL_UNMAPPED))})
        bf.close()
    rng = np.random.default_rng(1)
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4_600_000)].tobytes() for _ in range(8)]
    bf = BlockFinder(seqs, device=0)
    pieces = F.TextPieces()
    for c in range(8):
        for width in (0, F.LINE_LENGTH):
            pieces.lit(b">strain%d\n" % c)
            pieces.rec(c, 0, len(seqs[c]), width)
    res["whole_records_8x4600k_twice"] = measure(bf, pieces)
    bf.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
