"""CPU-side checks of sbl_group_distances' boundary (include/sibelia_amd.h): the struct against its ctypes mirror, the exports, and a
missing context refused without a write."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_counts_layout_matches_the_header():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    hdr = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sbl_pair_counts;", hdr).group(1)
    fields = [(f.strip(), ctypes.c_uint64) for names in re.findall(r"uint64_t\s+([^;]+);", body) for f in names.split(",")]
    assert [f for f, _ in fields] == ["match", "mismatch", "ambiguous", "gap"]
    assert fields == list(api.PairCounts._fields_) and ctypes.sizeof(api.PairCounts) == 32


def test_both_entry_points_are_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = ctypes.CDLL(api.LIB)
    for name in ("sbl_group_distances", "sbl_group_distances_times"):
        assert name in api.EXPORTS and hasattr(lib, name)
    assert hasattr(api.BlockFinder, "group_distances") and hasattr(api.BlockFinder, "group_distances_times")


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    cls = (ctypes.c_uint32 * 2)(0, 1)
    mark = ctypes.cast(0x5A5A5A5A, ctypes.POINTER(api.PairCounts))
    out = ctypes.POINTER(api.PairCounts)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(mark), ctypes.sizeof(out))
    assert lib.sbl_group_distances(None, None, cls, 2, ctypes.byref(out)) == 1      # SBL_ERR_BAD_ARG
    assert ctypes.cast(out, ctypes.c_void_p).value == 0x5A5A5A5A
    k, c = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    assert lib.sbl_group_distances_times(None, ctypes.byref(k), ctypes.byref(c)) == 1
    assert (k.value, c.value) == (-1.0, -2.0)
