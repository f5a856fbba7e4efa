"""CPU-side checks of sbl_group_mask's boundary (include/sibelia_amd.h): the struct against its ctypes mirror, the exports, and a missing
context refused without a write."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["group", "row", "first", "last", "before_first", "before_last", "ndiff"]


def test_the_struct_layout_matches_the_header():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    hdr = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sbl_mask_interval;", hdr).group(1)
    fields = [(f.strip(), ctypes.c_uint64) for found in re.findall(r"uint64_t\s+([^;]+);", body) for f in found.split(",")]
    assert [f for f, _ in fields] == NAMES
    assert fields == list(api.MaskInterval._fields_) and ctypes.sizeof(api.MaskInterval) == 56
    assert [getattr(api.MaskInterval, f).offset for f in NAMES] == list(range(0, 56, 8))


def test_the_four_entry_points_are_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = ctypes.CDLL(api.LIB)
    for name in ("sbl_group_mask", "sbl_group_mask_times", "sbl_group_set_masked", "sbl_group_get_masked"):
        assert name in api.EXPORTS and hasattr(lib, name)
        assert re.search(r"sbl_status %s\(" % name, open(os.path.join(ROOT, "include", "sibelia_amd.h")).read())
    for name in ("group_mask", "group_mask_times", "set_masked", "masked"):
        assert hasattr(api.BlockFinder, name)
    assert isinstance(api.BlockFinder.masked, property)


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    iv = ctypes.POINTER(api.MaskInterval)()
    mark = ctypes.cast(0x5A5A5A5A, ctypes.POINTER(api.MaskInterval))
    ctypes.memmove(ctypes.byref(iv), ctypes.byref(mark), ctypes.sizeof(iv))
    n = ctypes.c_uint64(7)
    assert lib.sbl_group_mask(None, None, 1000, 3, ctypes.byref(iv), ctypes.byref(n)) == 1      # SBL_ERR_BAD_ARG
    assert ctypes.cast(iv, ctypes.c_void_p).value == 0x5A5A5A5A and n.value == 7
    k, c = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    assert lib.sbl_group_mask_times(None, ctypes.byref(k), ctypes.byref(c)) == 1
    assert (k.value, c.value) == (-1.0, -2.0)
    on = ctypes.c_uint32(9)
    assert lib.sbl_group_set_masked(None, 1) == 1 and lib.sbl_group_get_masked(None, ctypes.byref(on)) == 1 and on.value == 9
