"""Groups for the tests of the multiple alignment, shared by tests/test_msa_model.py and tests/test_gpu_multi_align.py.

CRAFTED: name -> (group, rows written out by hand or None).  A group is a list of byte strings, centre first.  The hand-written rows
follow from the scores (+25 / -75 / -75) alone: every inserted stretch below consists of bases that differ from both neighbours, so the
optimal alignment is unique and the tie rules never decide."""
import numpy as np

CRAFTED = {
    # the member has two more bases at either end: D runs in slot 0 and in slot n = 8
    "slots_0_and_n": ([b"ACGTACGT", b"TTACGTACGTGG"],
                      [b"--ACGTACGT--", b"TTACGTACGTGG"]),
    # slot 4 holds GG, TTT and nothing: G[4] = 3, the shorter run is left-justified and padded
    "same_slot_different_lengths": ([b"AAAACCCC", b"AAAAGGCCCC", b"AAAATTTCCCC", b"AAAACCCC"],
                                    [b"AAAA---CCCC", b"AAAAGG-CCCC", b"AAAATTTCCCC", b"AAAA---CCCC"]),
    # member 1 lacks centre bases 4 .. 7 (an I run); member 2 has one base more in slot 6, inside that stretch
    "i_run_spans_a_slot": ([b"AAAACCGGTTTT", b"AAAATTTT", b"AAAACCAGGTTTT"],
                           [b"AAAACC-GGTTTT", b"AAAA-----TTTT", b"AAAACCAGGTTTT"]),
    "empty_centre": ([b"", b"", b"ACG", b"ACGTACG"],
                     [b"-------", b"-------", b"ACG----", b"ACGTACG"]),
    "empty_member": ([b"ACGT", b"", b"ACGT"],
                     [b"ACGT", b"----", b"ACGT"]),
    "one_instance": ([b"ACGTA"], [b"ACGTA"]),
    "nothing_at_all": ([b""], [b""]),
    "short_group": ([b"ACGTC", b"ACTC"], None),                                  # L < 16
}


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def mutated(rng, a, rate=0.05, max_indel=20):
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


def random_groups(seed, count, rmin, rmax, max_len, max_indel):
    """Seeded groups of rmin .. rmax instances of 0 .. max_len bases: members are mutated copies of the centre (substitutions, indels of
    up to max_indel bases), now and then an unrelated or an empty string."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        c = rand(rng, int(rng.integers(0, max_len + 1)))
        g = [c]
        for _ in range(int(rng.integers(rmin, rmax + 1)) - 1):
            u = rng.random()
            g.append(mutated(rng, c, 0.05, max_indel)[:max_len] if u < 0.85 else rand(rng, int(rng.integers(0, max_len + 1))) if u < 0.95 else b"")
        out.append(g)
    return out
