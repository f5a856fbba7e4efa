"""tests/fasta_model.py and the inputs of tests/fasta_cases.py, checked where no GPU is needed: the model reads every text of
tests/golden/fasta_cases.json and every text of tests/golden/fasta_limits.json but the three of 34 MB exactly as the unmodified
reference reader did (both fixtures are written by tests/golden/gen/, from oracle/_ref/ref_dump); every crafted text still has the digest the reference
was run on and really reaches the edge it is named after; the random texts split into enough that parse and enough that fail; the
codes planted for the ambiguity-list test sit where the chunk geometry of k_amb_flags / k_amb_write says they must."""
import base64
import hashlib
import json
import os

import pytest

from tests import fasta_cases as F
from tests import fasta_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OLD = json.load(open(os.path.join(GOLDEN, "fasta_cases.json")))["cases"]
GOLD = json.load(open(os.path.join(GOLDEN, "fasta_limits.json")))
NEW = GOLD["cases"]


def expected(case):
    """a fixture entry in the model's terms: the message as bytes, or [(name, sequence)]"""
    if "error" in case:
        return case["error"].encode("latin1")
    return [(r["name"].encode("latin1"), r["seq"].encode("latin1")) for r in case["records"]]


@pytest.mark.parametrize("name", sorted(OLD))
def test_model_reads_the_first_fixture_as_the_reference_did(name):
    assert M.parse(base64.b64decode(OLD[name]["text_b64"])) == expected(OLD[name])


def test_every_case_has_a_reference_fixture():
    assert list(NEW) == list(F.CASES) and GOLD["random_seed"] == F.RANDOM_SEED
    assert all(("text_b64" in NEW[n]) == (len(F.text(n)) <= F.SMALL_MAX) for n in F.CASES)
    assert set(F.LARGE) <= {n for n in NEW if "text_sha256" in NEW[n]}
    assert any("records_sha256" in NEW[n] for n in NEW) and sum("text_b64" in NEW[n] for n in NEW) >= 5


@pytest.mark.parametrize("name", list(F.CASES))
def test_recipe_builds_the_recorded_text_and_its_precondition_holds(name):
    text, case = F.text(name), NEW[name]
    if "text_b64" in case:
        assert text == base64.b64decode(case["text_b64"])
    else:
        assert len(text) == case["text_len"] and hashlib.sha256(text).hexdigest() == case["text_sha256"]
    F.CASES[name].pre()


@pytest.mark.parametrize("name", [n for n in F.CASES if n not in F.LARGE] + ["wide_column"])
def test_model_reads_the_crafted_cases_as_the_reference_did(name):
    # the fixture keeps the whole result of a text up to 1 kB and digests of a longer one: the model's result, put the same way, is equal
    # (the three 34 MB texts are left to the reference alone: 17 M lines are slow in Python)
    assert F.fixture_result(M.parse(F.text(name)), "text_b64" in NEW[name]) == F.result_keys(NEW[name])


def test_the_large_cases_are_the_ones_the_old_error_record_could_not_hold():
    # line << 40 | min(column, 0xFFFFFF) << 16 | byte << 8 | code, reduced with a minimum: what the record was before it carried 32 bits
    # of line index and 32 bits of column
    pack = lambda line, col, byte: ((line << 40) & (2 ** 64 - 1)) | min(col, 0xFFFFFF) << 16 | byte << 8 | 2      # noqa: E731
    assert pack(1, F.WIDE + 10, ord("Z")) > pack(1, F.WIDE + 2000, ord("!"))                 # wide_column: the later, smaller byte won
    assert pack(F.WIDE + 3, 0, ord("!")) >> 40 == 3 < F.WIDE - 5                             # late_line: the later error, on "line index 3", won
    assert NEW["wide_column"]["error"].endswith("on line 2: illegal character: Z")
    assert NEW["late_line"]["error"].endswith("on line %d: illegal character: Q" % (F.WIDE - 5 + 1))
    assert NEW["late_line_only"]["error"].endswith("on line %d: illegal character: !" % (F.WIDE + 3 + 1))
    assert [(r["name"], r["len"]) for r in NEW["late_line_ok"]["records"]] == [("r", F.WIDE + 1), ("s", 7)]


def test_random_texts_are_the_recorded_ones_and_split_both_ways():
    texts = F.random_texts()
    assert len(texts) == F.RANDOM_COUNT == 64 and max(map(len, texts)) <= F.RANDOM_MAX
    assert [hashlib.sha256(t).hexdigest() for t in texts] == GOLD["random_sha256"]
    results = [M.parse(t) for t in texts]
    ok = sum(isinstance(r, list) for r in results)
    assert ok >= 20 and len(texts) - ok >= 20
    kinds = {r.split(b": ", 1)[1][:13] for r in results if isinstance(r, bytes)}
    assert kinds == {b"empty header", b"empty sequenc", b"illegal chara"}
    assert sum(b"\r\n" in t for t in texts) >= 20 and sum(len(t) > F.CHUNK for t in texts) >= 20
    assert sum(len(r) > 1 for r in results if isinstance(r, list)) >= 10


def test_planted_ambiguity_codes_sit_on_the_chunk_geometry():
    plan, seps, recs = F.amb_plan(), F.amb_seps(), F.amb_records()
    nelem = seps[-1] + 1
    assert [len(r) for r in recs] == list(F.AMB_LENGTHS) and nelem == sum(F.AMB_LENGTHS) + 4
    nchunks = -(-nelem // F.AMB_CHUNK)
    assert nchunks > F.AMB_BLOCK and nelem % F.AMB_CHUNK != 0                   # a second block of k_amb_write; a partial last chunk
    at = dict(plan)
    elems = b"$" + b"$".join(recs) + b"$"
    assert len(elems) == nelem and [i for i, c in enumerate(elems) if c == ord("$")] == seps
    assert [(i, chr(c)) for i, c in enumerate(elems) if c not in b"ACGT$"] == plan      # exactly what is planted, nothing else
    assert {1023, 1024, 1025} <= set(at)
    for s in seps:
        assert (s == 0 or s - 1 in at) and (s == nelem - 1 or s + 1 in at)
    run = [e for e, c in plan if c == "N" and e > 2000]
    assert len(run) == 1500 and run == list(range(run[0], run[0] + 1500)) and run[-1] // F.AMB_CHUNK - run[0] // F.AMB_CHUNK == 2
    used = sorted({e // F.AMB_CHUNK for e in at})
    assert 200 in used and 199 not in used and 201 not in used and sum(e // F.AMB_CHUNK == 200 for e in at) == 1
    assert {256, 257, nchunks - 1} <= set(used) and 256 * F.AMB_CHUNK in at
    gaps = [b - a for a, b in zip(used, used[1:])]
    assert max(gaps) >= 90 and len(used) <= 16                                     # long stretches of chunks with none
