"""--wideband end to end (sibelia_amd/pipeline.py over the global band class of csrc/block_align.hip) on the crafted pair
of tests/wideband_cases.py: one block whose second instance carries an insertion of 5200 (12400) bases, beyond the band of the LDS
classes with (without) a gap opening cost.  Without the option the block is named on standard error and left out; with it the files
hold what the numpy models give for its two instances.  tests/test_wideband_cases.py pins the block itself to the CPU oracle.
Costs 1 and 0 are the ones at which the two cases cross their model's limit; cost 300 is there as well because only there is the
insertion ONE run and one VCF record of its own (see expected_files)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import galign_model as GM                          # noqa: E402
import gapopen_model as AM                         # noqa: E402
import mvariants_model as MV                       # noqa: E402
import wideband_cases as WC                        # noqa: E402

pytestmark = pytest.mark.gpu

INSTANCES = WC.INSTANCES

_model = {}


CASES = [(5200, 1), (12400, 0), (5200, 300)]      # (inserted bases, gap opening cost): each beyond the limit of its model


def model(ins, o):
    """the alignment of the block's two instances at the gap opening cost o, from band storage -> (row_a, row_b), once"""
    if (ins, o) not in _model:
        first, second = WC.crafted(ins)
        (sa, ea), (sb, eb) = INSTANCES[ins]
        a, b = first[sa:ea], second[sb:eb]
        score, steps = AM.pair_banded(a, b, o)                  # no opening cost: the linear alignment exactly, ties included
        _model[ins, o] = GM.rows(a, b, steps)
    return _model[ins, o]


def expected_files(ins, o, multi=False):
    """The files the models give.  At o = 0 and o = 1 a stray match (+25) inside the inserted bases is worth more than the gap run it
    splits, so the optimal alignment scatters the block's own bases over the insertion and parse_alignment's rules merge everything from
    the first substitution to the last into one record; at o = 300 the insertion is one run and one record of its own."""
    from sibelia_amd import formats
    first, second = WC.crafted(ins)
    (sa, ea), (sb, eb) = INSTANCES[ins]
    row_a, row_b = model(ins, o)
    maf = formats.maf_text([[formats.maf_line("refgenome", sa, ea, False, len(first), row_a),
                             formats.maf_line("assembly", sb, eb, False, len(second), row_b)]], o)
    if multi:
        records = [("refgenome", pos, 1, alleles[0], alleles[1:]) for pos, alleles in MV.records([row_a, row_b], sa, ea, False)]
        return maf, formats.multi_vcf_text("refgenome", ["assembly.fa"], records, o)
    variants = GM.variants(row_a, row_b, sa, ea, False)
    longest = max(variants, key=lambda v: len(v[2]) - len(v[1]))
    assert len(longest[2]) - len(longest[1]) == (eb - sb) - (ea - sa) >= ins - 1      # ONE record holds all the inserted bases
    if o == 300:                                                # ... the insertion alone, next to the six substitutions of X' and Y'
        assert len(longest[1]) == 1 and [(len(r), len(a)) for _, r, a in variants if (r, a) != longest[1:]] == [(1, 1)] * 6
    return maf, formats.vcf_text("refgenome", [("refgenome",) + v for v in variants], o)


def run(tmp_path, ins, o, extra):
    from sibelia_amd import pipeline as P
    os.makedirs(str(tmp_path), exist_ok=True)
    args, paths, _ = WC.write_crafted(tmp_path, ins)
    gap = ["--gapopen", str(o)] if o else []
    code, files, out = P.run(args + gap + extra + ["-o", str(tmp_path / "out")] + paths)
    assert code == 0
    return files


@pytest.mark.parametrize("ins,o", CASES)
def test_the_block_is_left_out_without_the_option_and_aligned_with_it(tmp_path, capsys, ins, o):
    from sibelia_amd import formats
    (sa, ea), (sb, eb) = INSTANCES[ins]
    assert WC.offsets(ea - sa, eb - sb) > WC.LIMIT[min(o, 1)]
    plain = run(tmp_path / "off", ins, o, ["--maf", "a.maf", "--variants", "v.vcf"])
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("block 1 not aligned: refgenome:%d-%d against assembly:%d-%d " % (sa + 1, ea, sb + 1, eb))
    assert "trace memory, band width or length" in err
    assert plain["a.maf"] == formats.maf_text([], o) and plain["v.vcf"] == formats.vcf_text("refgenome", [], o)
    files = run(tmp_path / "on", ins, o, ["--wideband", "--maf", "a.maf", "--variants", "v.vcf"])
    assert capsys.readouterr().err == ""
    assert list(files) == list(plain) and {k for k in files if files[k] != plain[k]} == {"a.maf", "v.vcf"}
    maf, vcf = expected_files(ins, o)
    assert files["a.maf"] == maf and files["a.maf"].count(b"\na\n") == 1
    assert files["v.vcf"] == vcf


def test_multimaf_and_multivariants_with_the_option(tmp_path, capsys):
    ins, o = 5200, 300
    files = run(tmp_path / "off", ins, o, ["--multimaf", "m.maf", "--multivariants", "m.vcf"])
    assert capsys.readouterr().err.count("block 1 not aligned") == 1 and b"\na\n" not in files["m.maf"]
    files = run(tmp_path / "on", ins, o, ["--wideband", "--multimaf", "m.maf", "--multivariants", "m.vcf"])
    assert capsys.readouterr().err == ""
    maf, vcf = expected_files(ins, o, multi=True)
    assert files["m.maf"] == maf and files["m.vcf"] == vcf
    assert any(len(ln.split(b"\t")[4]) >= ins for ln in files["m.vcf"].split(b"\n") if ln and not ln.startswith(b"#"))      # the insertion's record


def test_the_option_alone_is_an_argument_error():
    from sibelia_amd import pipeline as P
    with pytest.raises(P.PipelineError, match="--wideband widens the bands of the alignments: it needs at least one of --maf, --variants, --multimaf and --multivariants"):
        P.parse_args(["-s", "fine", "--wideband", "a.fa", "b.fa"])
    assert P.parse_args(["-s", "fine", "--wideband", "--maf", "a.maf", "a.fa", "b.fa"]).wideband is True
    assert P.parse_args(["-s", "fine", "--maf", "a.maf", "a.fa", "b.fa"]).wideband is False


def test_the_option_changes_no_file_where_no_block_is_beyond_the_limit(tmp_path, capsys):
    from sibelia_amd import pipeline as P
    ref, copy = WC.plain_pair()
    out = []
    for extra in ([], ["--wideband"]):
        d = tmp_path / ("on" if extra else "off")
        os.makedirs(str(d))
        fa = []
        for name, s in (("refgenome", ref), ("assembly", copy)):
            fa.append(str(d / (name + ".fa")))
            with open(fa[-1], "wb") as f:
                f.write(b">" + name.encode() + b"\n" + s + b"\n")
        code, files, text = P.run(WC.PLAIN_ARGS + ["--gapopen", "300", "--maf", "a.maf", "--variants", "v.vcf"] + extra + ["-o", str(d / "out")] + fa)
        assert code == 0
        out.append((files, text))
    assert capsys.readouterr().err == ""
    assert out[0] == out[1] and out[0][0]["a.maf"].count(b"\na\n") >= 3
