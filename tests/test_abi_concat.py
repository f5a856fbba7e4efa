"""CPU-side checks of sbl_group_concat's boundary (include/sibelia_amd.h): the two structs against their ctypes mirrors, the exports, and
a missing context refused without a write."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("struct, mirror, names", [("sbl_concat_part", "ConcatPart", ["group", "first", "ncols"]),
                                                   ("sbl_concat_site", "ConcatSite", ["group", "col", "before"])])
def test_struct_layouts_match_the_header(struct, mirror, names):
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    hdr = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
    fields = [(f.strip(), ctypes.c_uint64) for found in re.findall(r"uint64_t\s+([^;]+);", body) for f in found.split(",")]
    assert [f for f, _ in fields] == names
    assert fields == list(getattr(api, mirror)._fields_) and ctypes.sizeof(getattr(api, mirror)) == 24


def test_the_modes_match_the_header():
    from sibelia_amd import api
    hdr = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    assert int(re.search(r"#define SBL_CONCAT_ALL (\d+)", hdr).group(1)) == api.CONCAT_ALL == 0
    assert int(re.search(r"#define SBL_CONCAT_VARIABLE (\d+)", hdr).group(1)) == api.CONCAT_VARIABLE == 1


def test_both_entry_points_are_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = ctypes.CDLL(api.LIB)
    for name in ("sbl_group_concat", "sbl_group_concat_times"):
        assert name in api.EXPORTS and hasattr(lib, name)
    assert hasattr(api.BlockFinder, "group_concat") and hasattr(api.BlockFinder, "group_concat_times")


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    cls = (ctypes.c_uint32 * 2)(0, 1)
    first = (ctypes.c_uint64 * 3)(0, 3, 6)
    parts, sites = ctypes.POINTER(api.ConcatPart)(), ctypes.POINTER(api.ConcatSite)()
    for p, t in ((parts, api.ConcatPart), (sites, api.ConcatSite)):
        mark = ctypes.cast(0x5A5A5A5A, ctypes.POINTER(t))
        ctypes.memmove(ctypes.byref(p), ctypes.byref(mark), ctypes.sizeof(p))
    text = ctypes.c_void_p(0x5A5A5A5A)
    nparts, nsites, ln = ctypes.c_uint64(7), ctypes.c_uint64(8), ctypes.c_uint64(9)
    assert lib.sbl_group_concat(None, None, cls, 2, 0, 80, b">a\n>b\n", first, ctypes.byref(parts), ctypes.byref(nparts), ctypes.byref(sites), ctypes.byref(nsites),
                                ctypes.byref(text), ctypes.byref(ln)) == 1      # SBL_ERR_BAD_ARG
    assert ctypes.cast(parts, ctypes.c_void_p).value == ctypes.cast(sites, ctypes.c_void_p).value == text.value == 0x5A5A5A5A
    assert (nparts.value, nsites.value, ln.value) == (7, 8, 9)
    k, c = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    assert lib.sbl_group_concat_times(None, ctypes.byref(k), ctypes.byref(c)) == 1
    assert (k.value, c.value) == (-1.0, -2.0)
