"""The set-up of a simplification stage (csrc/graphbuild.hip, StageAttempt::setup_graph): compact marks of both strands from one pass
over the mark arrays, the block index records that pass writes on the way, the instance lists from ONE stable sort over
(strand, id) -- every mark placed at its rank in list order beforehand --, the per-mark aux words and the positional order of the ids.

Everything is compared with a numpy model built from sbl_enumerate's instances (which the parity tests pin to the oracle) and the
input sequences.  The list order is the reference's initial slist order, as documented at k_instance_input: + list = elements
descending; - list = chromosomes descending, elements ascending within a chromosome.

Element slots: slot 0 is the '$' before record 0, record c occupies sep[c] + 1 .. sep[c + 1] - 1, sep[c + 1] = sep[c] + len(c) + 1,
E = sep[nchr] + 1.  A + instance at position p of record c sits at sep[c] + 1 + p; a - instance, reported in reverse-complement
coordinates, at sep[c + 1] - 1 - p."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(s):
    return s.translate(_COMP)[::-1]


def _rand(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _with_repeats(rng, n, copies=12, span=45):
    """n random bases with `copies` stretches of `span` bases copied to another place (forward or reverse-complemented): every copy
    makes bifurcations at both of its ends"""
    g = bytearray(_rand(rng, n))
    for _ in range(copies):
        a, b = (int(x) for x in rng.integers(0, n - span, 2))
        piece = bytes(g[a:a + span])
        g[b:b + span] = _rc(piece) if rng.integers(0, 2) else piece
    return bytes(g)


def _cut(g, lengths):
    out, p = [], 0
    for n in lengths:
        out.append(g[p:p + n])
        p += n
    assert p == len(g)
    return out


def _records_for(rng, E, lengths_head):
    """records whose element count is exactly E: the given lengths first, one last record takes the rest"""
    rest = E - 1 - sum(n + 1 for n in lengths_head) - 1
    assert rest >= 1
    lengths = list(lengths_head) + [rest]
    return _cut(_with_repeats(rng, sum(lengths)), lengths)


def _model(seqs, k, nid, pos, neg):
    """what the stage set-up must leave, from the instances of the enumeration"""
    nchr = len(seqs)
    sep = np.zeros(nchr + 1, dtype=np.int64)
    for c, s in enumerate(seqs):
        sep[c + 1] = sep[c] + len(s) + 1
    E = int(sep[nchr]) + 1
    ch = np.full(E, ord("$"), dtype=np.uint8)
    for c, s in enumerate(seqs):
        ch[sep[c] + 1:sep[c + 1]] = np.frombuffer(s, dtype=np.uint8)
    code = np.full(256, 3, dtype=np.int64)
    code[ord("A")], code[ord("C")], code[ord("G")] = 0, 1, 2
    m = {"E": E, "melem": [], "mid": [], "maux": [], "lists": [], "lsize": []}
    for t, inst in enumerate((pos, neg)):
        c, p = inst["chr"].astype(np.int64), inst["pos"].astype(np.int64)
        e = sep[c] + 1 + p if t == 0 else sep[c + 1] - 1 - p
        order = np.argsort(e, kind="stable")
        e, c, ids = e[order], c[order], inst["id"].astype(np.int64)[order]
        assert len(np.unique(e)) == len(e)
        dist = sep[c + 1] - e if t == 0 else e - sep[c]
        bit = np.zeros(len(e), dtype=np.int64)
        ok = dist >= k + 1
        x = code[ch[(e + k if t == 0 else e - k)[ok]]]
        bit[ok] = 1 << (x if t == 0 else 3 - x)
        m["melem"].append(e.astype(np.uint32)); m["mid"].append(ids.astype(np.uint32))
        m["maux"].append(((bit << 24) | np.minimum(dist, 0xFFFFFF)).astype(np.uint32))
        # list order: + elements descending; - chromosomes descending, elements ascending
        rank = np.lexsort((-e,)) if t == 0 else np.lexsort((e, -c))
        lists = [[] for _ in range(nid)]
        for j in rank:
            lists[ids[j]].append(int(e[j]))
        m["lists"].append(lists)
        m["lsize"].append(np.array([len(x) for x in lists], dtype=np.uint32))
    nblk = (E + 63) // 64
    bidx = np.zeros((nblk, 4), dtype=np.uint64)
    for w, slots in enumerate((m["melem"][0], m["melem"][1], sep)):
        for s in slots:
            bidx[int(s) >> 6, w] |= np.uint64(1) << np.uint64(int(s) & 63)
    m["bidx"] = bidx
    key = np.array([(m["lists"][0][i] or m["lists"][1][i] or [NONE])[0] for i in range(nid)], dtype=np.int64)
    m["perm"] = np.argsort(key, kind="stable").astype(np.uint32)
    return m


def _check(seqs, k, D=40, expect=None):
    from sibelia_amd import BlockFinder
    bf = BlockFinder(seqs, device=0)
    try:
        nid, pos, neg = bf.enumerate(k)
        m = _model(seqs, k, nid, np.array(pos), np.array(neg))
        before = bf.state()
        g = bf.test_graph_build(k, D)
        after = bf.state()
        assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1], after[1])), "the set-up changed the state"
        assert g["nid"] == nid and g["E"] == m["E"]
        assert g["nblk"] == (m["E"] + 63) // 64 and g["index_from_marks"], "the block index of a stage start comes from the marks pass"
        for t in (0, 1):
            for f in ("melem", "mid", "maux", "lsize"):
                assert np.array_equal(g[f][t], m[f][t]), "%s of strand %d differs" % (f, t)
            base = 0 if t == 0 else len(m["melem"][0])
            nodeof = np.full(m["E"], NONE, dtype=np.uint32)
            for i in range(nid):
                assert list(g["lists"][t][i]) == m["lists"][t][i], "list of id %d, strand %d: %s, model %s" % (i, t, list(g["lists"][t][i]), m["lists"][t][i])
                nodes = g["nodes"][t][i]
                # node number = sorted position: strand 0 first, then strand 1, each by (id, list order)
                assert np.array_equal(nodes, base + np.arange(len(nodes))), "nodes of id %d, strand %d are not the run %d .." % (i, t, base)
                base += len(nodes)
                if len(nodes):
                    assert (g["nidst"][nodes] == ((i << 1) | t)).all()
                    assert np.array_equal(g["melem"][t][g["nmark"][nodes]], g["nslot"][nodes]), "nmark of id %d, strand %d" % (i, t)
                    nodeof[g["nslot"][nodes]] = nodes
            assert np.array_equal(g["nodeof"][t], nodeof), "nodeof of strand %d differs" % t
        assert np.array_equal(g["bidx"], m["bidx"]), "block index records differ in blocks %s" % np.nonzero((g["bidx"] != m["bidx"]).any(1))[0][:8]
        assert np.array_equal(g["perm"], m["perm"]), "positional order of the ids differs"
        if expect:
            expect(m, nid)
        if nid == 0:
            assert bf.simplify_stage(k, D, 4) == 0
            end = bf.state()
            assert before[0] == end[0] and all(np.array_equal(a, b) for a, b in zip(before[1], end[1])), "a stage without bifurcations changed the state"
        return m, nid
    finally:
        bf.close()


def _some_single_stranded(m, nid):
    only1 = [i for i in range(nid) if not m["lists"][0][i] and m["lists"][1][i]]
    only0 = [i for i in range(nid) if m["lists"][0][i] and not m["lists"][1][i]]
    assert only0 and only1, "no id with all of its instances on one strand (k_id_position_keys takes head1 for those without a + instance)"


@pytest.mark.parametrize("E", [2048, 2049, 3071, 4096 + 64, 1024 + 63], ids=lambda e: "E=%d" % e)
def test_one_record_at_the_chunk_edges(E):
    """E mod 64 in {0, 1, 63}, E mod 256 (a wave's chunk of the marks pass) and E mod 1024 in {0, 1, last}"""
    rng = np.random.default_rng(E)
    _check(_records_for(rng, E, []), 15, expect=_some_single_stranded)


def test_three_records():
    rng = np.random.default_rng(3)
    seqs = _records_for(rng, 2049, [700, 650])
    m, nid = _check(seqs, 15, expect=_some_single_stranded)
    assert nid > 0 and len({c for t in (0, 1) for c in np.searchsorted(np.cumsum([len(s) + 1 for s in seqs]), m["melem"][t], side="right")}) == 3, "marks in all three records"


def test_seventy_records_some_shorter_than_k():
    """70 records, among them records of k - 1, k and k + 1 bases and of a single base; E mod 64 = 63"""
    k = 15
    rng = np.random.default_rng(70)
    head = [k - 1, k, k + 1, 1] + [int(x) for x in rng.integers(20, 70, 65)]
    seqs = _records_for(rng, 3071 + 1024, head)
    assert len(seqs) == 70
    m, nid = _check(seqs, k, expect=_some_single_stranded)
    assert nid > 0
    # more than one chromosome in some - list: the order "chromosomes descending" is exercised
    assert any(len({int(np.searchsorted(np.cumsum([len(s) + 1 for s in seqs]), e, side="right")) for e in l}) > 1 for l in m["lists"][1]), "no - list spans two records"


def test_even_k_with_a_palindromic_bifurcation():
    """k = 8: AACGCGTT is its own reverse complement; two occurrences with different neighbours make it a bifurcation whose id has
    instances on both strands at the same slots"""
    rng = np.random.default_rng(8)
    pal = b"AACGCGTT"
    assert _rc(pal) == pal
    seqs = [_rand(rng, 300) + b"A" + pal + b"C" + _rand(rng, 300) + b"G" + pal + b"T" + _rand(rng, 300)]

    def expect(m, nid):
        both = [i for i in range(nid) if m["lists"][0][i] and sorted(m["lists"][0][i]) == sorted(e - 7 for e in m["lists"][1][i])]
        assert both, "no id whose + and - instances are the same k-mer occurrences"
    _check(seqs, 8, expect=expect)


def test_repeat_family_of_more_than_256_instances():
    rng = np.random.default_rng(256)
    unit = _rand(rng, 15)
    parts = []
    for i in range(300):
        parts += [unit, _rand(rng, int(rng.integers(3, 9)))]
    seqs = [b"".join(parts), _rand(rng, 100) + _rc(unit) + _rand(rng, 100)]

    def expect(m, nid):
        assert max(int(a) + int(b) for a, b in zip(m["lsize"][0], m["lsize"][1])) > 256
    _check(seqs, 15, expect=expect)


def test_single_random_record():
    """a single random record: no k-mer occurs twice, the only bifurcations are the k-mers at the record's two ends"""
    rng = np.random.default_rng(0)
    m, nid = _check([_rand(rng, 1500)], 15)
    assert nid == 4 and len(m["melem"][0]) == 2 and len(m["melem"][1]) == 2


def test_no_bifurcation_at_all():
    """a single record shorter than k has no k-mer: nid = 0, every array empty, the stage returns 0 and leaves the state as it is"""
    rng = np.random.default_rng(0)
    m, nid = _check([_rand(rng, 11)], 15)
    assert nid == 0 and len(m["melem"][0]) == 0 and len(m["melem"][1]) == 0
