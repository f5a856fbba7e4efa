"""Cases that pin k_block_align (csrc/block_align.hip) at the limits of its band classes and of its trace walk,
shared by tests/test_bandedge_cases.py (their preconditions, on the numpy models alone) and tests/test_gpu_band_edges.py (the device).

Edge pairs   `W = |m - n| + 2 w + 1` offsets at the first band w = 64, for every W next to a class limit, with an optimal path that runs
             along the band's first offset (k = 0) or its last (k = W - 1): 64 bases of one string that nothing matches, 400 shared
             bases, and a filler of W - 129 + 64 'T' -- a letter the other string lacks -- on the other side.
Walk pairs   one X / I / D run of 63 .. 129 steps, in the middle, from (0, 0) and up to the end of the strings.
Group        a centre with a `high` partner one offset beyond the register class, a `low` partner at its limit and a mutated copy.

The model results are computed once per process and kept."""
import functools

import numpy as np

import galign_model as GM
import gapopen_model as AM
from galign_cases import Batch, mutated, rand
from wideband_cases import W0, offsets

MODELS = ("linear", "affine")
# an edge-hugging pair has two gap runs and clears U(w) by exactly 175 (the certificate ignores the opening cost), so the
# affine cases need 2 o < 175
OPEN = {"linear": 0, "affine": 80}
LIMITS = {"linear": (512, 4096, 12288), "affine": (512, 2048, 4992)}      # REG_W, MID_W, MAX_W of GaLinear / GaAffine
KINDS = ("low", "high", "low_swapped", "high_swapped")
CORE, EDGE = 400, 64


def align(model, a, b):
    """the UNBANDED model -> (score, steps)"""
    return GM.align(a, b) if model == "linear" else AM.align(a, b, OPEN[model])


def align_banded(model, a, b, w):
    return GM.align_banded(a, b, w) if model == "linear" else AM.align_banded(a, b, OPEN[model], w)


def want_of(a, b, result):
    """(score, runs, rows): what Batch.check compares"""
    score, steps = result
    return score, GM.runs(a, b, steps), GM.rows(a, b, steps)


def reach(steps):
    """the least and the greatest j - i along a path"""
    off = np.cumsum([0] + [{"M": 0, "I": -1, "D": 1}[s] for s in steps])
    return int(off.min()), int(off.max())


def cells(pairs, w=W0):
    """align_stats()["cells"] of one pass over the pairs"""
    return sum((len(a) + len(b) + 1) * ((offsets(len(a), len(b), w) + 1) // 2) for a, b in pairs)


# ---- pairs whose optimal path runs along an edge of the band

def filler(W):
    return b"T" * (W - (2 * W0 + 1) + EDGE)


@functools.lru_cache(maxsize=None)
def edge_pairs(model, W):
    """the four pairs of KINDS with W offsets at w = 64, one of them with both strands reversed -> (pairs, revs)"""
    rng = np.random.default_rng(7100 + 100000 * MODELS.index(model) + W)
    core, U, V = rand(rng, CORE, b"ACG"), rand(rng, EDGE, b"ACG"), filler(W)
    pairs = [(U + core, core + V),          # low: 64 I, 400 =, |V| D -- j - i falls to lo - 64
             (core + U, V + core),          # high: |V| D, 400 =, 64 I -- j - i rises to hi + 64
             (V + core, core + U),          # low, n > m: |V| I, 400 =, 64 D
             (core + V, U + core)]          # high, n > m: 64 D, 400 =, |V| I
    down = (W + MODELS.index(model)) % 4    # over the three W of a limit three different kinds are staged downwards
    return pairs, [(k == down, k == down) for k in range(4)]


@functools.lru_cache(maxsize=None)
def edge_model(model, W):
    return tuple(align(model, a, b) for a, b in edge_pairs(model, W)[0])


def edge_batch(model, Ws):
    """the pairs of every W in Ws, in that order -> (Batch, what the model gives)"""
    pairs, revs, want = [], [], []
    for W in Ws:
        p, r = edge_pairs(model, W)
        pairs += p
        revs += r
        want += [want_of(a, b, res) for (a, b), res in zip(p, edge_model(model, W))]
    return Batch(pairs, revs), want


# ---- pairs with one long run for the trace walk

WALK_L = (63, 64, 65, 127, 128, 129)


def walk_first_w(op, L):
    """The first band at which a walk pair certifies.  An X run of L costs 100 L (a lost match and a mismatch per column) and the
    certificate needs 175 (w + 1) + 75 |m - n| to exceed the cost: with equal lengths no pair with 114 or more
    mismatches certifies at w = 64, whatever surrounds them.  Those run at a first band of 128 -- one pass, as all the others."""
    return 2 * W0 if op == "X" and 100 * L >= 175 * (W0 + 1) else W0


@functools.lru_cache(maxsize=None)
def walk_cases(model):
    """[(op, L, where, a, b)]: where 'mid' (300 shared bases either side), 'start' (the run begins at (0, 0)) or 'end' (it ends at n / m)"""
    rng = np.random.default_rng(7200 + MODELS.index(model))
    P, S = rand(rng, 300, b"ACG"), rand(rng, 300, b"ACG")
    out = []
    for L in WALK_L:
        T, N = b"T" * L, b"N" * L
        for where, p, s in (("mid", P, S), ("start", b"", S), ("end", P, b"")):
            out.append(("X", L, where, p + T + s, p + N + s))
            out.append(("I", L, where, p + T + s, p + s))
            out.append(("D", L, where, p + s, p + T + s))
    return out


def walk_runs(op, L, where):
    """the run list the construction is meant to give"""
    return ([("=", 300)] if where != "start" else []) + [(op, L)] + ([("=", 300)] if where != "end" else [])


@functools.lru_cache(maxsize=None)
def walk_model(model):
    return tuple(align(model, a, b) for _, _, _, a, b in walk_cases(model))


def walk_batch(model, first_w):
    """the walk pairs that certify at first_w -> (Batch, what the model gives)"""
    pairs, want = [], []
    for (op, L, _, a, b), res in zip(walk_cases(model), walk_model(model)):
        if walk_first_w(op, L) == first_w:
            pairs.append((a, b))
            want.append(want_of(a, b, res))
    return Batch(pairs), want


# ---- one group across the limit of the register class

def group_case(model):
    """The centre c is `core + U` of the high pair and, read as its first 64 bases and the other 400, `U + core` of the low pair ->
    [c, the high partner with REG_W + 1 offsets, the low partner with REG_W offsets, a mutated copy]"""
    rng = np.random.default_rng(7300 + MODELS.index(model))
    c = rand(rng, CORE + EDGE, b"ACG")
    reg_w = LIMITS[model][0]
    return [c, filler(reg_w + 1) + c[:CORE], c[EDGE:] + filler(reg_w), mutated(rng, c)]
