"""CPU-side checks of sbl_group_bootstrap's boundary (include/sibelia_amd.h): the exports, the ctypes mirror of the arguments, and a missing
context refused without a write."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_entry_points_are_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = ctypes.CDLL(api.LIB)
    hdr = open(os.path.join(ROOT, "include", "sibelia_amd.h")).read()
    for name in ("sbl_group_bootstrap", "sbl_group_bootstrap_times"):
        assert name in api.EXPORTS and hasattr(lib, name)
        assert re.search(r"sbl_status %s\(" % name, hdr)
    for name in ("group_bootstrap", "group_bootstrap_times"):
        assert hasattr(api.BlockFinder, name)
    from sibelia_amd import build
    assert "group_boot.hip" in build.SOURCES


def test_the_argument_types_mirror_the_header():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    hdr = " ".join(open(os.path.join(ROOT, "include", "sibelia_amd.h")).read().split())
    decl = re.search(r"sbl_status sbl_group_bootstrap\(([^)]*)\);", hdr).group(1)
    types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*").replace("* ", "*") for a in decl.split(",")]
    assert types == ["sbl_ctx*", "const uint8_t*", "const uint32_t*", "uint32_t", "uint32_t", "uint64_t", "uint32_t", "const uint64_t**", "uint64_t*", "uint64_t*"]
    C = ctypes
    assert list(lib.sbl_group_bootstrap.argtypes) == [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                                       C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    assert list(lib.sbl_group_bootstrap_times.argtypes) == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    out = ctypes.POINTER(ctypes.c_uint64)()
    mark = ctypes.cast(0x5A5A5A5A, ctypes.POINTER(ctypes.c_uint64))
    ctypes.memmove(ctypes.byref(out), ctypes.byref(mark), ctypes.sizeof(out))
    cls = (ctypes.c_uint32 * 2)(0, 1)
    nsites, nclean = ctypes.c_uint64(7), ctypes.c_uint64(8)
    assert lib.sbl_group_bootstrap(None, None, cls, 2, 10, 1, 0, ctypes.byref(out), ctypes.byref(nsites), ctypes.byref(nclean)) == 1      # SBL_ERR_BAD_ARG
    assert ctypes.cast(out, ctypes.c_void_p).value == 0x5A5A5A5A and (nsites.value, nclean.value) == (7, 8)
    k, c = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    assert lib.sbl_group_bootstrap_times(None, ctypes.byref(k), ctypes.byref(c)) == 1
    assert (k.value, c.value) == (-1.0, -2.0)
