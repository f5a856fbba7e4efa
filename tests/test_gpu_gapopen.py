"""The alignment with a gap opening cost (sbl_align_set_gap_open, the affine model of k_block_align in csrc/block_align.hip, --gapopen;
DESIGN.md 0.5) against the numpy model tests/gapopen_model.py: status, score, runs and the device-spelled rows must equal the UNBANDED
model."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import galign_model as GM                          # noqa: E402
import gapopen_model as AM                         # noqa: E402
from galign_cases import Batch, mutated, rand, rc  # noqa: E402

pytestmark = pytest.mark.gpu

PAIR_A = b"CACTGGAGACACACCGAGTGGATAGTCCTATCCCATGAGC"
PAIR_B = b"CACTGGAGACACATCGTCCTATCCCATGAGC"
PAIR_RUNS = [("=", 13), ("X", 1), ("=", 2), ("I", 9), ("=", 15)]


def edge_pairs():
    rng = np.random.default_rng(41)
    x = rand(rng, 1000)
    pairs = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C"), (b"A", b"ACGT")]
    pairs += [(x[:n], x[:n]) for n in (1, 63, 64, 65, 1000)]
    for at in (0, 500, 999):                                   # one substitution: first, middle, last position
        pairs.append((x, x[:at] + (b"A" if x[at:at + 1] != b"A" else b"C") + x[at + 1:]))
    pairs += [(x, x[3:]), (x[3:], x), (x, x[:-5]), (x[:-5], x)]      # an indel of 3 / 5 bases at either end
    pairs += [(b"A" * 33, b"A" * 90), (b"A" * 90, b"A" * 33), (PAIR_A, PAIR_B)]
    a = rand(rng, 500)
    pairs += [(a, mutated(rng, a))] * 4                        # one mutated pair on all four strand combinations
    revs = [(False, False)] * (len(pairs) - 4) + [(False, False), (True, False), (False, True), (True, True)]
    return pairs, revs


@pytest.fixture(scope="module")
def edges():
    return Batch(*edge_pairs())


def random_pairs(seed=44, count=200):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(count):
        a = rand(rng, int(rng.integers(1, 401)))
        u = rng.random()
        b = (mutated(rng, a, 0.06, 30) or b"A")[:400] if u < 0.85 else rand(rng, int(rng.integers(1, 401)))
        pairs.append((a, b))
    return pairs


@pytest.fixture(scope="module")
def random_batch():
    return Batch(random_pairs())


@pytest.mark.parametrize("o", [1, 300])
def test_edge_shapes(edges, o):
    got, st = edges.run(o)
    edges.check(got, edges.want(o))
    n = len(edges.pairs)
    assert st["pairs"] == n and st["skipped"] == 0 and st["kernel_ms"] > 0
    assert got[1].score == got[2].score == -(o + 300) and got[0].score == 0 and got[0].runs == []
    if o == 300:
        assert got[n - 5].runs == PAIR_RUNS and got[n - 5].score == -300                    # the printed pair, literally
    assert got[n - 4].runs == got[n - 3].runs == got[n - 2].runs == got[n - 1].runs         # the four strand combinations
    assert got[n - 7].runs == [("=", 33), ("D", 57)] and got[n - 6].runs == [("=", 33), ("I", 57)]


def launch_class_pairs():
    """one wave in registers (129 offsets), 256 lanes over LDS (629), the widest class (4097: 640 lanes, 1024 without an opening cost)"""
    rng = np.random.default_rng(45)
    s = rand(rng, 400)
    a = rand(rng, 3000)
    b = a[:1400] + rand(rng, 500) + a[1400:]
    u, v = b"A" * 2200, b"C" * 2200              # nothing matches: -165000 clears U(w) = 55000 - 175 (w + 1) only at w = 2048
    return [(s, mutated(rng, s)), (a, b), (u, v)]


@pytest.fixture(scope="module")
def launch_classes():
    return Batch(launch_class_pairs())


def test_every_launch_class(launch_classes):
    bt = launch_classes
    got, st = bt.run(300)
    bt.check(got, bt.want(300))
    assert got[0].band_w == 64 and got[0].passes == 1
    assert sum(n for op, n in got[1].runs if op == "D") == 500 and got[1].score == 3000 * 25 - 500 * 75 - 300 and got[1].band_w == 64
    assert got[2].band_w == 2048 and got[2].passes == 6 and got[2].runs == [("X", 2200)], (got[2].passes, got[2].band_w)
    assert st["launches"] >= 3


def test_a_batch_of_random_pairs_at_any_first_band(random_batch, monkeypatch):
    passes, first = {}, None
    for w0 in (1, 8, 64):
        monkeypatch.setenv("SBL_TEST_GALIGN_W0", str(w0))
        got, st = random_batch.run(300)
        random_batch.check(got, random_batch.want(300))
        passes[w0] = st["passes"]
        key = [(g.status, g.score, g.runs, g.row_a, g.row_b) for g in got]
        first = first or key
        assert key == first
    assert passes[1] > passes[8] > passes[64] >= 200, passes      # doubling ran
    lin = random_batch.want(0, linear=True)
    assert sum(x[1] != y[1] for x, y in zip(lin, random_batch.want(300))) >= 20      # the cost matters on this batch


def test_no_opening_cost_through_the_new_kernel_is_the_linear_alignment(edges, random_batch, monkeypatch):
    monkeypatch.setenv("SBL_TEST_GALIGN_AFFINE", "1")
    for bt in (edges, random_batch):
        got, st = bt.run(0)
        bt.check(got, bt.want(0, linear=True))
    monkeypatch.delenv("SBL_TEST_GALIGN_AFFINE")
    got_old, st_old = random_batch.run(0)
    random_batch.check(got_old, random_batch.want(0, linear=True))
    assert [(g.score, g.runs, g.band_w, g.passes) for g in got] == [(g.score, g.runs, g.band_w, g.passes) for g in got_old]
    assert (st["passes"], st["cells"]) == (st_old["passes"], st_old["cells"])


def test_no_opening_cost_is_the_linear_alignment_in_every_launch_class(launch_classes, monkeypatch):
    """o = 0 through the affine model against the linear one beyond the register class: both over LDS with 256 lanes (629 offsets) and
    in the widest class of either (4097 offsets: 640 lanes against 1024)"""
    bt = launch_classes
    want = bt.want(0, linear=True)
    monkeypatch.setenv("SBL_TEST_GALIGN_AFFINE", "1")
    affine, _ = bt.run(0)
    monkeypatch.delenv("SBL_TEST_GALIGN_AFFINE")
    linear, _ = bt.run(0)
    for got in (affine, linear):
        bt.check(got, want)
        assert got[2].band_w == 2048 and got[2].passes == 6, (got[2].passes, got[2].band_w)
    assert [(g.score, g.runs, g.band_w, g.passes) for g in affine] == [(g.score, g.runs, g.band_w, g.passes) for g in linear]
    assert [(g.row_a, g.row_b) for g in affine] == [(g.row_a, g.row_b) for g in linear]


def test_the_band_limit_with_an_opening_cost():
    rng = np.random.default_rng(46)
    a = rand(rng, 100)
    far = a[:50] + rand(rng, 4900) + a[50:]                     # 100 against 5000 bases: 4900 + 2 * 64 + 1 = 5029 offsets at the first w
    s = rand(rng, 300)
    bt = Batch([(s, mutated(rng, s)), (a, far), (far[:200], far[:200]), (PAIR_A, PAIR_B)])
    got, st = bt.run(0)
    bt.check(got, bt.want(0, linear=True))
    assert st["skipped"] == 0 and got[1].band_w == 64
    got, st = bt.run(1)
    bt.check(got, bt.want(1), skipped={1})
    assert st["skipped"] == 1


def test_the_per_alignment_cap_binds_at_half_the_length(monkeypatch):
    """4 KiB of codes: 17 bytes per diagonal at w = 64 without an opening cost, 34 with one"""
    rng = np.random.default_rng(47)
    pairs = []
    for n in (30, 55, 65, 110, 130, 200):
        a = rand(rng, n)
        pairs.append((a, a[:n // 2] + (b"A" if a[n // 2:n // 2 + 1] != b"A" else b"C") + a[n // 2 + 1:]))
    bt = Batch(pairs)
    # n = m, w = min(64, n), W = 2 w + 1: bytes per diagonal B = ceil(ceil(W / 2) / 4), doubled with an opening cost; skipped when (2 n + 1) B > 4096
    def beyond(n, factor):
        w = min(64, n)
        return (2 * n + 1) * (((2 * w + 2) // 2 + 3) // 4) * factor > 4096
    lens = [len(a) for a, _ in pairs]
    skip0 = {k for k, n in enumerate(lens) if beyond(n, 1)}
    skip1 = {k for k, n in enumerate(lens) if beyond(n, 2)}
    assert skip0 == {4, 5} and skip1 == {2, 3, 4, 5}           # 130 and 200 bases without, from 65 bases on with an opening cost
    monkeypatch.setenv("SBL_TEST_GALIGN_CAP_KB", "4")
    got, st = bt.run(0)
    bt.check(got, bt.want(0, linear=True), skipped=skip0)
    got, st = bt.run(300)
    bt.check(got, bt.want(300), skipped=skip1)
    assert st["skipped"] == len(skip1)


def test_bad_arguments_leave_the_context_usable_and_the_value_stays():
    from sibelia_amd import BlockFinder
    from sibelia_amd.api import SibeliaError
    bt = Batch([(PAIR_A, PAIR_B)])
    bf = BlockFinder(bt.records, device=0)
    try:
        assert bf.gap_open == 0
        bf.set_gap_open(300)
        for bad in (100001, 2 ** 32 - 1):
            with pytest.raises(SibeliaError, match="bad argument"):
                bf.set_gap_open(bad)
            assert bf.gap_open == 300
        for _ in range(2):                                      # the value holds from one call to the next
            got = bf.align_pairs(bt.desc)
            assert got[0].status == 0 and got[0].runs == PAIR_RUNS and got[0].score == -300
        bf.set_gap_open(100000)
        assert bf.gap_open == 100000 and bf.align_pairs(bt.desc)[0].status == 0
        bf.set_gap_open(0)
        got = bf.align_pairs(bt.desc)
        assert got[0].score == 0 and got[0].runs == [("=", 13), ("X", 1), ("=", 2), ("I", 2), ("=", 1), ("I", 7), ("=", 14)]
    finally:
        bf.close()


def test_groups_against_the_model():
    from sibelia_amd import BlockFinder
    rng = np.random.default_rng(48)
    record, groups, texts = bytearray(b"N"), [], []
    for r in (1, 3, 5, 3):
        c = rand(rng, int(rng.integers(100, 301)))
        insts, strings = [], []
        for k in range(r):
            s = c if k == 0 else (mutated(rng, c, 0.06, 12) or b"A")[:300]
            rev = bool((k + r) % 2) and k > 0 or (r == 3 and k == 0 and len(groups) == 3)      # reverse members; one reverse centre
            insts.append((0, len(record), len(record) + len(s), rev))
            record += rc(s) if rev else s
            record += b"N"
            strings.append(s)
        groups.append(insts)
        texts.append(strings)
    assert any(i[3] for g in groups for i in g[1:]) and groups[3][0][3]
    bf = BlockFinder([bytes(record)], device=0)
    try:
        bf.set_gap_open(300)
        got = bf.align_groups(groups)
    finally:
        bf.close()
    for g, strings in zip(got, texts):
        rows, scores = AM.msa(strings, 300)
        assert g.status == 0 and g.rows == rows and [m[0] for m in g.members] == scores


# ---- end to end: --gapopen on a seeded synthetic pair

ARGS = ["-s", "fine", "-m", "500", "--lastk", "30", "-r", "--correctboundaries"]
SEGMENT = (21000, 25000)
PLANTED = (3000, 6000, 9000, 12000, 15000, 18000, 27000, 30000, 33000, 36000)


def synthetic():
    """One 40 kbp random record; a copy with ten planted deletions of 8 .. 12 bases, each with a substitution two or three bases before
    or behind it, 39 lone substitutions well away from them and one 4 kbp segment reverse-complemented -> (ref, copy, [(position,
    length)] of the deletions)."""
    rng = np.random.default_rng(505)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 40000))
    copy = bytearray(ref)

    def substitute(at):
        copy[at] = b"ACGT".replace(ref[at:at + 1], b"")[int(rng.integers(0, 3))]
    for p in range(1000, 40000, 1000):
        substitute(p + 300 + int(rng.integers(0, 400)))         # 300 .. 700 past a multiple of 1000: clear of the planted sites
    cuts = []
    for k, at in enumerate(PLANTED):
        n = 8 + k % 5
        substitute(at - 2 - k % 2 if k % 4 < 2 else at + n + 1 + k % 2)
        cuts.append((at, n))
    s, e = SEGMENT
    copy[s:e] = rc(bytes(copy[s:e]))
    for at, n in reversed(cuts):
        del copy[at:at + n]
    return ref, bytes(copy), cuts


def run_pipeline(tmp_path, extra):
    from sibelia_amd import pipeline as P
    ref, copy, _ = synthetic()
    os.makedirs(str(tmp_path), exist_ok=True)
    fa = []
    for name, s in (("refgenome", ref), ("assembly", copy)):
        fa.append(str(tmp_path / (name + ".fa")))
        with open(fa[-1], "wb") as f:
            f.write(b">" + name.encode() + b"\n" + s + b"\n")
    code, files, out = P.run(ARGS + extra + ["-o", str(tmp_path / "out")] + fa)
    assert code == 0
    return files, out


def parse_maf(text, comment=None):
    lines = text.decode().split("\n")
    head = ["##maf version=1"] + ([comment] if comment else []) + [""]
    assert lines[:len(head)] == head and lines[-1] == ""
    blocks, at = [], len(head)
    while at < len(lines) - 1:
        assert lines[at] == "a" and lines[at + 3] == "", lines[at:at + 4]
        rows = []
        for ln in lines[at + 1:at + 3]:
            tag, name, start, size, strand, total, row = ln.split(" ")
            assert tag == "s"
            rows.append((name, int(start), int(size), strand == "-", int(total), row.encode()))
        blocks.append(rows)
        at += 4
    return blocks


def instance(seq, start, size, rev):
    """the bases of an `s` line: its start counts from the record's end for '-'"""
    return rc(seq[len(seq) - start - size:len(seq) - start]) if rev else seq[start:start + size]


def gap_runs_near(row_a, row_b, centre, reach=15):
    """the maximal runs of '-' in row b that start within `reach` bases of base `centre` of a -> their lengths"""
    out, ai, run = [], 0, 0
    for x, y in zip(row_a, row_b):
        if y == 45 and x != 45:
            if run == 0:
                first = ai
            run += 1
        else:
            if run and abs(first - centre) <= reach:
                out.append(run)
            run = 0
        ai += x != 45
    return out


def test_gapopen_end_to_end(tmp_path, capsys):
    from sibelia_amd import formats
    ref, copy, cuts = synthetic()
    files, out = run_pipeline(tmp_path / "on", ["--gapopen", "300", "--maf", "a.maf", "--variants", "v.vcf"])
    plain, out_plain = run_pipeline(tmp_path / "off", ["--maf", "a.maf", "--variants", "v.vcf"])
    zero, out_zero = run_pipeline(tmp_path / "zero", ["--gapopen", "0", "--maf", "a.maf", "--variants", "v.vcf"])
    assert capsys.readouterr().err == ""                        # no block is skipped
    assert zero == plain and out_zero == out_plain == out       # --gapopen 0 is the run without the option, byte for byte
    assert list(files) == list(plain) and {k for k in files if files[k] != plain[k]} == {"a.maf", "v.vcf"}
    maf, maf_plain = parse_maf(files["a.maf"], "# gapopen=300"), parse_maf(plain["a.maf"])
    assert len(maf) == len(maf_plain) >= 3
    vcf = files["v.vcf"].decode().split("\n")
    assert vcf[1:3] == ["##source=sibelia_amd", "##sibelia_amd_gapopen=300"] and "gapopen" not in plain["v.vcf"].decode()
    records, whole, split = [], set(), set()
    for (ra, rb), (pa, pb) in zip(maf, maf_plain):
        assert ra[:5] == pa[:5] and rb[:5] == pb[:5] and not ra[3]      # the same blocks; the correction turns the reference instance to '+'
        a, b = instance(ref, *ra[1:4]), instance(copy, *rb[1:4])
        score, steps = AM.pair_banded(a, b, 300)
        assert (ra[5], rb[5]) == GM.rows(a, b, steps), ra[:5]
        start, end = ra[1], ra[1] + ra[2]
        records += [("refgenome",) + v for v in formats.variants_from_runs(GM.runs(a, b, steps), ra[5], rb[5], start, end, False)]
        for at, n in cuts:
            if start + 50 <= at and at + n + 50 <= end and not rb[3]:
                assert gap_runs_near(ra[5], rb[5], at - start) == [n], (at, n)      # a planted deletion is ONE run with the opening cost
                whole.add(at)
                if len(gap_runs_near(pa[5], pb[5], at - start)) == 2:
                    split.add(at)                               # ... and two without it
    assert len(whole) >= 3 and len(split) >= 1, (whole, split)
    assert files["v.vcf"] == formats.vcf_text("refgenome", records, 300)
