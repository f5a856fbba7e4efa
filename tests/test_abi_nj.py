"""CPU-side checks of sbl_nj_batch's boundary (include/sibelia_amd.h): the exports, the ctypes mirror of the arguments and of sbl_nj_edge,
the translation unit in the build, and a missing context refused without a write."""
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
    from sibelia_amd import api
    lib = ctypes.CDLL(api.LIB)
    hdr = header()
    for name in ("sbl_nj_batch", "sbl_nj_batch_times"):
        assert name in api.EXPORTS and hasattr(lib, name)
        assert re.search(r"sbl_status %s\(" % name, hdr)
    for name in ("nj_batch", "nj_batch_times"):
        assert hasattr(api.BlockFinder, name)
    from sibelia_amd import build
    assert "tree_nj.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "tree_nj.hip"))
    assert build.FLAGS == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]      # contraction is switched off in the unit, not here
    assert "#pragma clang fp contract(off)" in open(os.path.join(build.CSRC, "tree_nj.hip")).read()


def test_the_argument_types_and_the_edge_mirror_the_header():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api, tree
    lib = api.load_library()
    hdr = header()
    decl = re.search(r"sbl_status sbl_nj_batch\(([^)]*)\);", hdr).group(1)
    types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*").replace("* ", "*") for a in decl.split(",")]
    assert types == ["sbl_ctx*", "const double*", "uint32_t", "uint32_t", "const sbl_nj_edge**", "const uint64_t**"]
    C = ctypes
    assert list(lib.sbl_nj_batch.argtypes) == [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(api.NjEdge)), C.POINTER(C.POINTER(C.c_uint64))]
    assert list(lib.sbl_nj_batch_times.argtypes) == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert re.search(r"typedef struct \{ uint32_t parent, child; double length; \} sbl_nj_edge;", hdr)
    assert C.sizeof(api.NjEdge) == 16 and [(f, t) for f, t in api.NjEdge._fields_] == [("parent", C.c_uint32), ("child", C.c_uint32), ("length", C.c_double)]
    assert (api.NjEdge.parent.offset, api.NjEdge.child.offset, api.NjEdge.length.offset) == (0, 4, 8)
    assert api.NJ_EDGE_DTYPE.itemsize == 16 and api.NJ_EDGE_DTYPE == tree.EDGE_RECORD and tree.NJ_BATCH_MAX_FILES == 64
    assert [api.NJ_EDGE_DTYPE.fields[f][1] for f in ("parent", "child", "length")] == [0, 4, 8]


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    edges, splits = ctypes.POINTER(api.NjEdge)(), ctypes.POINTER(ctypes.c_uint64)()
    mark = ctypes.c_void_p(0x5A5A5A5A)
    for out in (edges, splits):
        ctypes.memmove(ctypes.byref(out), ctypes.byref(mark), ctypes.sizeof(out))
    D = (ctypes.c_double * 9)(0, 1, 2, 1, 0, 3, 2, 3, 0)
    assert lib.sbl_nj_batch(None, D, 3, 1, ctypes.byref(edges), ctypes.byref(splits)) == 1      # SBL_ERR_BAD_ARG
    assert ctypes.cast(edges, ctypes.c_void_p).value == 0x5A5A5A5A and ctypes.cast(splits, ctypes.c_void_p).value == 0x5A5A5A5A
    k, c = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    assert lib.sbl_nj_batch_times(None, ctypes.byref(k), ctypes.byref(c)) == 1
    assert (k.value, c.value) == (-1.0, -2.0)
