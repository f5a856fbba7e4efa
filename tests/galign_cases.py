"""Pairs for the tests of the pair alignment on the device, shared by tests/test_gpu_block_align.py and
tests/test_gpu_gapopen.py: seeded strings and a batch of pairs with the results the numpy models (tests/galign_model.py,
tests/gapopen_model.py) give for them."""
import numpy as np

import galign_model as GM
import gapopen_model as AM

_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(s):
    return s.translate(_COMPLEMENT)[::-1]


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def mutated(rng, a, rate=0.03, max_indel=12):
    b = bytearray()
    i = 0
    while i < len(a):
        u = rng.random()
        if u < rate / 3:
            i += int(rng.integers(1, max_indel + 1))
        elif u < 2 * rate / 3:
            b += rand(rng, int(rng.integers(1, max_indel + 1)))
        else:
            b += rand(rng, 1) if rng.random() < rate else a[i:i + 1]
            i += 1
    return bytes(b)


class Batch:
    """pairs of strings laid out as ranges of two records (all a's, all b's); a reverse range holds the reverse complement, so that the
    strings the kernel reads are the ones given.  The model's results are computed once per opening cost and kept."""

    def __init__(self, pairs, revs=None):
        self.pairs = [(bytes(a), bytes(b)) for a, b in pairs]
        self.revs = revs or [(False, False)] * len(pairs)
        ra, rb, self.desc = bytearray(b"G"), bytearray(b"T"), []
        for (a, b), (va, vb) in zip(self.pairs, self.revs):
            self.desc.append((0, len(ra), len(ra) + len(a), va, 1, len(rb), len(rb) + len(b), vb))
            ra += rc(a) if va else a
            rb += rc(b) if vb else b
        self.records = [bytes(ra) + b"C", bytes(rb) + b"A"]
        self._want = {}

    def want(self, o, linear=False):
        key = "linear" if linear else o
        if key not in self._want:
            out = []
            for a, b in self.pairs:
                score, steps = GM.align(a, b) if linear else AM.align(a, b, o)
                out.append((score, GM.runs(a, b, steps), GM.rows(a, b, steps)))
            self._want[key] = out
        return self._want[key]

    def run(self, o):
        from sibelia_amd import BlockFinder
        bf = BlockFinder(self.records, device=0)
        try:
            bf.set_gap_open(o)
            assert bf.gap_open == o
            return bf.align_pairs(self.desc), bf.align_stats()
        finally:
            bf.close()

    def check(self, got, want, skipped=()):
        assert len(got) == len(self.pairs)
        for k, (g, (score, runs, rows)) in enumerate(zip(got, want)):
            a, b = self.pairs[k]
            if k in skipped:
                assert (g.status, g.score, g.runs, g.row_a, g.row_b) == (1, None, [], b"", b""), k
                continue
            assert g.status == 0, (k, len(a), len(b))
            assert g.score == score, (k, len(a), len(b), a[:60], b[:60])
            assert g.runs == runs, (k, len(a), len(b), a[:60], b[:60])
            assert (g.row_a, g.row_b) == rows, (k, len(a), len(b))
