"""The synteny stage's small-block index at its limits (needs an MI355X: -m gpu).

The inputs are the crafted cases of tests/synteny_cases.py (their preconditions are verified on the oracle by
tests/test_synteny_cases.py).  Every op of a case runs in order on one context; block lists must equal the oracle's and the
reference's (tests/golden/synteny_limits.json), and the library's path counters (sbl_synteny_stats) must show that the block the case
is about took the path it is about.  A second context under SBL_NO_TINY_INDEX=1 must give the same blocks through the general child
index alone.

These tests compare block lists only, and by the way TrimBlocks reads an index a block list cannot show the order of the instances
within one id's list nor a uniform shift of all ids.  The small-block index itself -- every (id, chr, pos) of both instance lists -- is
compared with the oracle, the reference and the general index by tests/test_gpu_tiny_index.py (cases: tests/tiny_index_cases.py)."""
import json
import os

import pytest

from sibelia_amd import formats as F
from tests import synteny_cases as S
from tests import vectors as V

pytestmark = pytest.mark.gpu

GOLD = {c["name"]: c for c in json.load(open(os.path.join(V.GOLDEN, "synteny_limits.json")))["cases"]}
FIELDS = ("id", "chr", "start", "end")
TINY_COUNTERS = ("batch_launches", "batch_indices", "speculated_used", "single_launches", "batch_declines", "single_declines",
                 "tiny_max_elements", "tiny_max_records", "tiny_max_keys")
_oracle, _reports = {}, {}


def names_of(seqs):
    return ["seq%d" % i for i in range(len(seqs))]


def oracle_run(name):
    """(records, ops, per op: the oracle's output bytes and its block list), computed once per case"""
    if name not in _oracle:
        from oracle.oracle import Oracle
        seqs, ops = S.CASES[name].make()
        o, res = Oracle(seqs), []
        for op in ops:
            if op[0] == "stage":
                res.append((V.run_cmd(o, S.cmd_of(op)), None))
            else:
                b = o.generate_blocks(*op[1:])
                res.append((F.blocks_bytes(b), b))
        o.close()
        _oracle[name] = (seqs, ops, res)
    return _oracle[name]


def oracle_reports(name, i):
    """GlueStripes + the three report texts of the oracle on its block list of op i (its procedure rescans per merge: seconds on the
    chunk case, so it is computed where it is compared and nowhere else)"""
    if (name, i) not in _reports:
        from oracle.oracle import Oracle
        seqs, _, res = oracle_run(name)
        o = Oracle(seqs)
        _reports[(name, i)] = o.postprocess(res[i][1], names_of(seqs), True)
        o.close()
    return _reports[(name, i)]


def same_blocks(a, b):
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in FIELDS)


def hip_run(name, compare_reports=False):
    """ops on one context: every result against the oracle and the reference fixture (compare_reports: after every blocks op the glued
    list and the three texts against the oracle's instead); -> the path counters per op (None for a stage)"""
    from sibelia_amd import BlockFinder
    seqs, ops, want = oracle_run(name)
    bf, stats = BlockFinder(seqs, device=0), []
    try:
        for i, op in enumerate(ops):
            gold = GOLD[name]["outputs"][i]
            assert gold["cmd"] == S.cmd_of(op)
            if op[0] == "stage":
                got = V.run_cmd(bf, gold["cmd"])
                stats.append(None)
            else:
                b = bf.generate_blocks(*op[1:])
                stats.append(bf.synteny_stats())
                print(name, gold["cmd"], stats[-1])
                assert same_blocks(b, want[i][1]), "%s: %s differs from the oracle" % (name, gold["cmd"])
                got = F.blocks_bytes(b)
                if compare_reports:
                    g, t = bf.postprocess(names_of(seqs), True)
                    wg, wt = oracle_reports(name, i)
                    assert same_blocks(g, wg) and list(t) == list(wt), "%s: reports after %s differ from the oracle" % (name, gold["cmd"])
            assert got == want[i][0] and len(got) == gold["size"] and F.sha256(got) == gold["sha256"], "%s: %s differs from the reference" % (name, gold["cmd"])
    finally:
        bf.close()
    return seqs, ops, stats


@pytest.mark.parametrize("name", list(S.CASES))
def test_blocks_at_the_limit_equal_oracle_and_reference_and_took_the_intended_path(name, monkeypatch):
    monkeypatch.delenv("SBL_NO_TINY_INDEX", raising=False)
    case = S.CASES[name]
    seqs, ops, stats = hip_run(name)
    if not case.ambiguous:                               # (with non-ACGT bytes the edge list depends on where the rand() stream stands)
        groups = S.oracle_groups(seqs, ops)
        for st, g in zip(stats, groups):
            assert st is None or st["groups_resolved"] == len(g[0]), (st, len(g[0]))
    for st in stats:
        if st is not None:
            assert st["speculated_used"] <= st["batch_indices"] and st["single_declines"] <= st["single_launches"]
            assert st["tiny_max_elements"] <= S.MAX_ELEM and st["tiny_max_records"] <= S.MAX_REC and st["tiny_max_keys"] < 2 * S.MAX_ELEM
    case.expect(stats)


@pytest.mark.parametrize("name", list(S.CASES))
def test_glued_blocks_and_reports_at_the_limit_equal_the_oracle(name, monkeypatch):
    # GlueStripes and the three writers after every blocks op, as the parity test of the small-block index does
    monkeypatch.delenv("SBL_NO_TINY_INDEX", raising=False)
    hip_run(name, True)


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c.no_tiny_twin])
def test_general_child_index_alone_gives_the_same_blocks(name, monkeypatch):
    monkeypatch.setenv("SBL_NO_TINY_INDEX", "1")
    _, _, stats = hip_run(name)
    for st in stats:
        if st is not None:
            assert all(st[f] == 0 for f in TINY_COUNTERS), st
            assert st["general_indices"] > 0 or st["groups_resolved"] == 0, st
