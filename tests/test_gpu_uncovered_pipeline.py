"""--uncovered / --unmapped end to end on the Staphylococcus aureus pair (tests/golden/data), run with the command line C-Sibelia.py gives
the reference program: the whole VCF against the per-base model (tests/uncovered_model.py) applied to the run's own blocks_coords*.txt,
and the long deletions against the ones the reference's example records (tests/golden/uncovered_saureus.json)."""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncovered_model as UM                       # noqa: E402
from correct_fixtures import records_of, write_inputs      # noqa: E402

pytestmark = pytest.mark.gpu

INPUT = "split:Staphylococcus_aureus_pair"
M = 500
ARGS = ["-s", "fine", "-m", str(M), "--lastk", "30", "--correctboundaries", "--nopostprocess", "--allstages", "-r", "--variants", "v.vcf"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the three runs -- without the option, with it, with --unmapped -- and what the model makes of the second one's block lists"""
    from sibelia_amd import pipeline as P
    wd = tmp_path_factory.mktemp("saureus")
    inputs = [str(wd / n) for n in write_inputs(INPUT, str(wd))]
    out = {}
    for key, extra in (("plain", []), ("uncovered", ["--uncovered"]), ("unmapped", ["--uncovered", "--unmapped", "u.fa"])):
        rc, files, text = P.run(ARGS + extra + ["-o", str(wd / key)] + inputs)
        assert rc == 0
        out[key] = (files, text)
    files = out["uncovered"][0]
    (reference,), assembly = records_of(INPUT)[0]
    names, seqs = [reference[0]] + [n for n, _ in assembly], [reference[1]] + [s for _, s in assembly]
    stages = sorted((n for n in files if n.startswith("blocks_coords")), key=lambda n: int(n[13:-4]))
    lists = [UM.parse_blocks_coords(files[n].decode()) for n in stages]
    out["names"], out["seqs"] = names, seqs
    out["found"] = UM.calls(lists, [len(s) for s in seqs], 1, M)
    return out


def body(vcf):
    lines = vcf.decode().split("\n")
    assert lines[-1] == "" and lines[6].startswith("#CHROM\t")
    return lines[:7], lines[7:-1]


def test_the_option_adds_records_and_changes_nothing_else(runs):
    (plain, text_plain), (unc, text_unc), (unm, text_unm) = runs["plain"], runs["uncovered"], runs["unmapped"]
    assert text_plain == text_unc == text_unm
    assert list(unc) == list(plain) and list(unm) == list(plain) + ["u.fa"]
    for files in (unc, unm):
        assert {k: v for k, v in files.items() if k not in ("v.vcf", "u.fa")} == {k: v for k, v in plain.items() if k != "v.vcf"}
    head, aligned = body(plain["v.vcf"])
    assert aligned and not any("bnd_" in ln for ln in aligned)
    for files in (unc, unm):
        h, lines = body(files["v.vcf"])
        assert h == head
        kept = iter(lines)
        assert all(ln in kept for ln in aligned)    # every alignment record, unchanged and in its order


def test_the_vcf_is_the_model_applied_to_the_blocks_the_run_wrote(runs):
    names, seqs, found = runs["names"], runs["seqs"], runs["found"]
    kinds = [c[0] for c in found]
    print("deletions %d, anchored insertions %d, unmapped insertions %d" % (kinds.count("D"), kinds.count("I"), kinds.count("U")))
    assert kinds.count("D") >= 5
    head, aligned = body(runs["plain"][0]["v.vcf"])
    rows = [(names[0], int(f[1]), f[3], f[4]) for f in (ln.split("\t") for ln in aligned)]
    want = UM.bnd_lines(names, seqs, found) + UM.record_lines(rows + UM.variant_rows(names, seqs, found))
    h, lines = body(runs["uncovered"][0]["v.vcf"])
    assert lines == want
    # sorted as DESIGN.md 0.4 says: the breakend records first, in pairs; then every record by (description, POS)
    nbnd = 2 * kinds.count("U")
    assert [ln.split("\t")[2] for ln in lines[:nbnd]] == ["bnd_%d" % i for i in range(nbnd)]
    keys = [(ln.split("\t")[0], int(ln.split("\t")[1])) for ln in lines[nbnd:]]
    assert keys == sorted(keys) and not any("bnd_" in ln for ln in lines[nbnd:])


def test_with_unmapped_the_insertions_go_to_the_fasta(runs):
    names, seqs, found = runs["names"], runs["seqs"], runs["found"]
    files = runs["unmapped"][0]
    h, lines = body(files["v.vcf"])
    nbnd = 2 * sum(c[0] == "U" for c in found)
    assert not any("bnd_" in ln for ln in lines) and lines == body(runs["uncovered"][0]["v.vcf"])[1][nbnd:]
    assert files["u.fa"] == UM.unmapped_fasta(names, seqs, found)
    assert files["u.fa"].count(b">") == nbnd // 2


def test_the_long_deletions_of_the_reference_example(runs):
    """The reference's example was written by C-Sibelia 3.0.2; the records of the fixture marked `asserted` are in this run's VCF with
    the same POS and the same REF, the others are left out for the reason the fixture gives."""
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "uncovered_saureus.json")))["records"]
    assert len(fixture) == 5
    _, lines = body(runs["uncovered"][0]["v.vcf"])
    ours = {}
    refs = {}
    for f in (ln.split("\t") for ln in lines):
        if len(f[3]) > 1000:
            ours[int(f[1])] = (len(f[3]), hashlib.sha256(f[3].encode()).hexdigest(), f[4])
            refs[int(f[1])] = f[3]
    for r in fixture:
        got = ours.get(r["pos"])
        print("reference example: POS %d, REF of %d: %s" % (r["pos"], r["ref_length"], "the same here" if got == (r["ref_length"], r["ref_sha256"], r["alt"]) else "here %r" % (got and got[::2],)))
        if r["asserted"]:
            assert got == (r["ref_length"], r["ref_sha256"], r["alt"]), r["pos"]
        else:
            assert r["reason"]
            if r["ref_is_prefix"]:                  # a neighbouring block starts later here: the example's REF and more
                assert got is not None and got[0] > r["ref_length"] and got[2] == r["alt"]
                assert hashlib.sha256(refs[r["pos"]][:r["ref_length"]].encode()).hexdigest() == r["ref_sha256"]
    assert sum(r["asserted"] for r in fixture) >= 4
