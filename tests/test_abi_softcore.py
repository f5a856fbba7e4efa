"""CPU-side checks of the boundary of the partial setting (include/sibelia_amd.h): sbl_group_set_partial,
sbl_group_get_partial and sbl_group_bootstrap_pairs are exported, declared and mirrored, and refuse a missing context without a write."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sbl_group_set_partial", "sbl_group_get_partial", "sbl_group_bootstrap_pairs")


def header():
    return " ".join(open(os.path.join(ROOT, "include", "sibelia_amd.h")).read().split())


def test_the_three_entry_points_are_exported_declared_and_listed():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = ctypes.CDLL(api.LIB)
    hdr = header()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(lib, name)
        assert re.search(r"sbl_status %s\(" % name, hdr)
    for name in ("set_partial", "partial", "group_bootstrap_pairs"):
        assert hasattr(api.BlockFinder, name)
    assert isinstance(api.BlockFinder.partial, property)


def test_the_argument_types_mirror_the_header():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", header())
    C = ctypes
    want = {"sbl_group_set_partial": (["sbl_ctx*", "uint32_t"], [C.c_void_p, C.c_uint32]),
            "sbl_group_get_partial": (["const sbl_ctx*", "uint32_t*"], [C.c_void_p, C.POINTER(C.c_uint32)]),
            "sbl_group_bootstrap_pairs": (["sbl_ctx*", "const uint64_t**"], [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))])}
    for name, (types, mirror) in want.items():
        decl = re.search(r"sbl_status %s\(([^)]*)\);" % name, hdr).group(1)
        assert [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*").replace("* ", "*") for a in decl.split(",")] == types
        assert list(getattr(lib, name).argtypes) == mirror
    # no existing export changed its signature for this: the bootstrap call as tests/test_abi_bootstrap.py pins it
    decl = re.search(r"sbl_status sbl_group_bootstrap\(([^)]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 10


def test_a_null_context_is_refused_without_a_write():
    import __graft_entry__ as g
    g.build()
    from sibelia_amd import api
    lib = api.load_library()
    assert lib.sbl_group_set_partial(None, 1) == 1                                 # SBL_ERR_BAD_ARG
    on = ctypes.c_uint32(7)
    assert lib.sbl_group_get_partial(None, ctypes.byref(on)) == 1 and on.value == 7
    out = ctypes.POINTER(ctypes.c_uint64)()
    mark = ctypes.cast(0x5A5A5A5A, ctypes.POINTER(ctypes.c_uint64))
    ctypes.memmove(ctypes.byref(out), ctypes.byref(mark), ctypes.sizeof(out))
    assert lib.sbl_group_bootstrap_pairs(None, ctypes.byref(out)) == 1
    assert ctypes.cast(out, ctypes.c_void_p).value == 0x5A5A5A5A
