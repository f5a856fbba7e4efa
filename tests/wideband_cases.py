"""Cases for the tests of the global band class (sbl_align_set_wide, --wideband), shared by tests/test_wideband_cases.py,
tests/test_gpu_wideband.py and tests/test_gpu_wideband_pipeline.py: batches of pairs whose band is beyond the LDS classes, a run with
the setting, and a crafted pair of FASTA records whose one block carries an insertion longer than those classes hold."""
import numpy as np

from galign_cases import Batch, mutated, rand, rc

LIMIT = {0: 12288, 1: 4992}                        # the most band offsets of the LDS classes: GaLinear::MAX_W, GaAffine::MAX_W
W0 = 64


def offsets(n, m, w=W0):
    w = min(w, n, m)
    return abs(m - n) + 2 * w + 1


def run(bt, o, wide):
    """Batch.run with the wide setting -> (alignments, align_stats, align_wide_stats)"""
    from sibelia_amd import BlockFinder
    bf = BlockFinder(bt.records, device=0)
    try:
        bf.set_gap_open(o)
        bf.set_wide(wide)
        assert bf.wide == int(wide)
        return bf.align_pairs(bt.desc), bf.align_stats(), bf.align_wide_stats()
    finally:
        bf.close()


def key(got):
    return [(g.status, g.score, g.runs, g.row_a, g.row_b, g.band_w, g.passes) for g in got]


def far_of(rng, a, total):
    """a with random bases in its middle, `total` bases in all"""
    h = len(a) // 2
    return a[:h] + rand(rng, total - len(a)) + a[h:]


def limit_batch(o):
    """Pairs just beyond the limit of the model at the first w, at small n -> (Batch, the indices of the far pairs).  Without an opening
    cost 100 against 12400 bases (12429 offsets, 1554 quads of cells a diagonal: more than any workgroup has lanes), both ways round and
    with both strands reversed; with one 100 against 5000 (5029 offsets) and 60 against 9000 (9061 offsets, 1133 quads)."""
    rng = np.random.default_rng(61 + o)
    s = rand(rng, 300)
    if o == 0:
        a = rand(rng, 100)
        far = far_of(rng, a, 12400)
        pairs, revs = [(a, far), (far, a), (a, far)], [(False, False), (False, False), (True, True)]
    else:
        a, b = rand(rng, 100), rand(rng, 60)
        far, farther = far_of(rng, a, 5000), far_of(rng, b, 9000)
        pairs, revs = [(a, far), (far, a), (a, far), (b, farther)], [(False, False), (False, False), (True, True), (False, False)]
    nfar = len(pairs)
    pairs.append((s, mutated(rng, s)))
    revs.append((False, False))
    for a, b in pairs[:nfar]:
        assert offsets(len(a), len(b)) > LIMIT[min(o, 1)]
    return Batch(pairs, revs), set(range(nfar))


def shape_pairs(seed=62):
    """About 200 pairs of 1 .. 400 bases: the lengths 1, 2, 7, 8, 9 against each other and against 300, an empty string against a
    non-empty one, mutated pairs at 3 % (certified at the first w) and at 30 % (doubling, up to the band that covers the matrix),
    unrelated pairs, all four strand combinations"""
    rng = np.random.default_rng(seed)
    x = rand(rng, 300)
    small = (1, 2, 7, 8, 9)
    pairs = [(x[:n], x[3:3 + m]) for n in small for m in small]
    pairs += [(x[:n], x) for n in small] + [(x, x[:n]) for n in small]
    pairs += [(b"", x[:9]), (x[:9], b"")]
    # nothing matches: the certificate needs w + 1 > 100 min(n, m) / 175 -- 120 bases fail at 64 and end at the band that covers the matrix,
    # 400 bases double twice
    pairs += [(b"A" * 120, b"C" * 120), (b"A" * 120, b"C" * 400), (b"A" * 400, b"C" * 400)]
    while len(pairs) < 200:
        a = rand(rng, int(rng.integers(1, 401)))
        u = rng.random()
        b = rand(rng, int(rng.integers(1, 401))) if u < 0.15 else (mutated(rng, a, 0.03 if u < 0.6 else 0.3, 30) or b"A")[:400]
        pairs.append((a, b))
    revs = [(bool(k & 1), bool(k & 2)) for k in range(len(pairs))]
    return pairs, revs


# ---- the crafted pipeline input: one block whose second instance carries an insertion of INS random bases

STAGES = {5200: [(30, 150), (100, 6000)], 12400: [(30, 150), (100, 13000)]}      # -k: the last stage's D collapses the insertion's bulge
OPEN = {5200: 1, 12400: 0}                         # the gap opening cost at which the block is beyond the limit
MIN_BLOCK_SIZE, LAST_K, MAX_ITER = 500, 100, 4
ARGS = ["-m", str(MIN_BLOCK_SIZE), "--lastk", str(LAST_K)]
# the one block the CPU oracle finds (tests/test_wideband_cases.py): (start, end) of its instance in the first / the second file
INSTANCES = {5200: ((500, 1701), (300, 6701)), 12400: ((500, 1700), (300, 13900))}


def substituted(s, every):
    out = bytearray(s)
    for at in range(every // 2, len(s), every):
        out[at] = b"ACGT".replace(s[at:at + 1], b"")[at % 3]
    return bytes(out)


def crafted(ins):
    """first = rand(500) + X + Y + rand(500), second = rand(300) + X' + rand(ins) + Y' + rand(700); X, Y: 600 random bases, X' / Y'
    with a substitution every 211 / 197 bases -> (first, second)"""
    rng = np.random.default_rng(7000 + ins)
    x, y = rand(rng, 600), rand(rng, 600)
    first = rand(rng, 500) + x + y + rand(rng, 500)
    second = rand(rng, 300) + substituted(x, 211) + rand(rng, ins) + substituted(y, 197) + rand(rng, 700)
    return first, second


def stage_text(ins):
    """the stage file: the number of stages, then k and D of each"""
    return "%d\n" % len(STAGES[ins]) + "".join("%d %d\n" % s for s in STAGES[ins])


def write_crafted(tmp_path, ins):
    """the two FASTA files and the stage file -> (argument list up to the output options, [first, second])"""
    seqs = crafted(ins)
    paths = []
    for name, s in zip(("refgenome", "assembly"), seqs):
        paths.append(str(tmp_path / (name + ".fa")))
        with open(paths[-1], "wb") as f:
            f.write(b">" + name.encode() + b"\n" + s + b"\n")
    stages = str(tmp_path / "stages.txt")
    with open(stages, "w") as f:
        f.write(stage_text(ins))
    return ["-k", stages] + ARGS, paths, seqs


def oracle_blocks(ins):
    """what the CPU oracle makes of the crafted pair through the stages and the final block generation of the pipeline (trimK: the
    smallest k of the stages) -> [(id, chr, start, end)]"""
    from oracle.oracle import Oracle
    orc = Oracle(list(crafted(ins)))
    try:
        for k, d in STAGES[ins]:
            orc.simplify_stage(k, d, MAX_ITER)
        blocks = orc.generate_blocks(LAST_K, min(k for k, _ in STAGES[ins]), MIN_BLOCK_SIZE)
        blocks, _ = orc.postprocess(blocks, ["refgenome", "assembly"])
        return [(int(b["id"]), int(b["chr"]), int(b["start"]), int(b["end"])) for b in blocks]
    finally:
        orc.close()


# ---- the synthetic pair of tests/test_gpu_gapopen.py, built again here: no block of it comes near any limit

PLAIN_ARGS = ["-s", "fine", "-m", "500", "--lastk", "30", "-r", "--correctboundaries"]


def plain_pair():
    """One 40 kbp random record; a copy with ten planted deletions of 8 .. 12 bases, each with a substitution next to it, 39 lone
    substitutions and one 4 kbp segment reverse-complemented -> (ref, copy)"""
    rng = np.random.default_rng(505)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 40000))
    copy = bytearray(ref)

    def substitute(at):
        copy[at] = b"ACGT".replace(ref[at:at + 1], b"")[int(rng.integers(0, 3))]
    for p in range(1000, 40000, 1000):
        substitute(p + 300 + int(rng.integers(0, 400)))
    cuts = []
    for k, at in enumerate((3000, 6000, 9000, 12000, 15000, 18000, 27000, 30000, 33000, 36000)):
        n = 8 + k % 5
        substitute(at - 2 - k % 2 if k % 4 < 2 else at + n + 1 + k % 2)
        cuts.append((at, n))
    copy[21000:25000] = rc(bytes(copy[21000:25000]))
    for at, n in reversed(cuts):
        del copy[at:at + n]
    return ref, bytes(copy)
