"""CPU-side checks of sbl_group_parsimony's boundary (include/sibelia_amd.h): the exports, the ctypes mirror of the arguments and of
sbl_parsimony_change, the translation unit in the build, and a missing context refused without a write."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    """the header without its comments, blanks folded"""
    text = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split())


def test_the_two_entry_points_are_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api, build
    lib = ctypes.CDLL(api.LIB)
    hdr = header()
    for name in ("sbl_group_parsimony", "sbl_group_parsimony_times"):
        assert name in api.EXPORTS and hasattr(lib, name)
        assert re.search(r"sbl_status %s\(" % name, hdr)
    for name in ("group_parsimony", "group_parsimony_times"):
        assert hasattr(api.BlockFinder, name)
    assert "group_parsimony.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "group_parsimony.hip"))
    text = open(os.path.join(build.CSRC, "group_parsimony.hip")).read()
    assert "k_fitch_steps" in text and "k_fitch_changes" in text and "prim::exclusive_scan" in text
    assert len(re.findall(r"rocprim::\w*scan", open(os.path.join(build.CSRC, "sbl_prim.h")).read())) == 3      # one helper, no second wrapper


def test_the_argument_types_and_the_change_mirror_the_header():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    hdr = header()
    decl = re.search(r"sbl_status sbl_group_parsimony\(([^)]*)\);", hdr).group(1)
    types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*").replace("* ", "*") for a in decl.split(",")]
    assert types == ["sbl_ctx*", "const sbl_nj_edge*", "uint32_t", "const uint64_t**", "const uint8_t**", "const uint8_t**", "const sbl_parsimony_change**", "uint64_t*"]
    C = ctypes
    assert list(lib.sbl_group_parsimony.argtypes) == [C.c_void_p, C.POINTER(api.NjEdge), C.c_uint32, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8)),
                                                      C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(api.ParsimonyChange)), C.POINTER(C.c_uint64)]
    assert list(lib.sbl_group_parsimony_times.argtypes) == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert re.search(r"typedef struct \{ uint64_t site; uint32_t edge; uint8_t from, to, pad_\[2\]; \} sbl_parsimony_change;", hdr)
    P = api.ParsimonyChange
    assert C.sizeof(P) == 16 and (P.site.offset, P.edge.offset, P.from_.offset, P.to.offset, P.pad_.offset) == (0, 8, 12, 13, 14)
    D = api.PARSIMONY_CHANGE_DTYPE
    assert D.itemsize == 16 and [D.fields[f][1] for f in ("site", "edge", "from", "to", "pad_")] == [0, 8, 12, 13, 14]


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    C = ctypes
    counts, steps, least, changes = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.POINTER(api.ParsimonyChange)()
    mark = C.c_void_p(0x5A5A5A5A)
    for out in (counts, steps, least, changes):
        C.memmove(C.byref(out), C.byref(mark), C.sizeof(out))
    n = C.c_uint64(77)
    edges = (api.NjEdge * 3)((3, 0, 0.0), (3, 1, 0.0), (3, 2, 0.0))
    assert lib.sbl_group_parsimony(None, edges, 3, C.byref(counts), C.byref(steps), C.byref(least), C.byref(changes), C.byref(n)) == 1      # SBL_ERR_BAD_ARG
    assert [C.cast(out, C.c_void_p).value for out in (counts, steps, least, changes)] == [0x5A5A5A5A] * 4 and n.value == 77
    k, c = C.c_double(-1.0), C.c_double(-2.0)
    assert lib.sbl_group_parsimony_times(None, C.byref(k), C.byref(c)) == 1
    assert (k.value, c.value) == (-1.0, -2.0)
