"""CPU: the public surface of retiring keyframes on the keyframe store -- the header declares and liblorb.so exports
lorb_kf_store_retire_dev, the ctypes mirror agrees with the header's struct (the compiled probe of
tests/test_kf_store_abi.py), the constants match, null and out-of-range arguments are rejected without a device, the
launch count is stated where the other units state theirs, and the ABI version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_kf_store_retire_dev",)
INVALID = -1


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    for s in SYMBOLS:
        getattr(L, s).restype = ctypes.c_int
    return L


def test_library_exports_the_entry_point():
    L = library()
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_header_declares_the_entry_point():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in h, s
    assert "} lorb_kf_retire_result;" in h
    # the citations the contract rests on, the launch count, and what stays out of scope
    for c in ("#define LORB_KF_RETIRE_MAX_LIST 1024", "#define LORB_KF_RETIRE_MAX_PROTECT 4", "src/frame.cpp:684-714", ":791-798",
              ":754-774", "src/map_point.cpp:141-153", ":184-199", "src/frame.cpp:686-687", "src/local_mapping.cpp:110-113",
              "lorb_kf_store_life_write", "NOT A BYTE", "6 kernel launches, no stream synchronise", "Out of scope", "KeyFramesCulling",
              "Order independence", "lorb_map_step_dev", "_refresh_dev -> _retire_dev -> _compact_dev"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_the_launch_count_is_stated():
    """retire is 6 launches: the header, the unit and DESIGN say so, and the unit has as many launch sites."""
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    u = open(os.path.join(ROOT, "lorb_slam_amd", "csrc", "lorb_kfretire.hip")).read()
    assert "6 kernel launches, no stream synchronise" in h
    assert "`lorb_kf_store_retire_dev`: 6 launches" in d
    assert "retire is SIX launches" in u
    assert u.count("hipLaunchKernelGGL(") == 6


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirror_and_constants_match_the_header():
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_kf_retire_result", A.KfRetireResult),
             # additive: the records of the calls around it keep their layout
             ("lorb_kf_cull_result", A.KfCullResult), ("lorb_kf_compact_result", A.KfCompactResult),
             ("lorb_kf_insert_result", A.KfInsertResult))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    lines.append(f'_Static_assert(LORB_KF_RETIRE_MAX_LIST == {A.LORB_KF_RETIRE_MAX_LIST}, "the list limit");')
    lines.append(f'_Static_assert(LORB_KF_RETIRE_MAX_PROTECT == {A.LORB_KF_RETIRE_MAX_PROTECT}, "the protect limit");')
    src = "\n".join(lines) + "\nint main(void) { return 0; }\n"
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    import kf_retire_ref as T
    assert tuple(f for f, _ in A.KfRetireResult._fields_) == T.FIELDS
    assert (A.LORB_KF_RETIRE_MAX_LIST, A.LORB_KF_RETIRE_MAX_PROTECT) == (T.MAX_LIST, T.MAX_PROTECT) == (1024, 4)


def test_invalid_arguments_are_rejected_without_a_device():
    """With a null context the entry point returns LORB_E_INVALID whatever else it is given -- full dummy arguments,
    each argument nulled in turn, and every bound out of range."""
    L = library()
    keep = []

    def buf(n=1024):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.c_void_p(ctypes.addressof(b))

    def args(**kw):
        a = dict(ctx=None, store=buf(), d_list=buf(), d_n_list=buf(), n_max_list=ctypes.c_int32(8), d_protect=buf(),
                 n_protect=ctypes.c_int32(2), d_src_status=buf(), d_result=buf())
        a.update(kw)
        return list(a.values())

    assert L.lorb_kf_store_retire_dev(*args()) == INVALID
    for drop in ("store", "d_list", "d_n_list", "d_protect", "d_src_status", "d_result"):
        assert L.lorb_kf_store_retire_dev(*args(**{drop: None})) == INVALID, drop
    for n in (0, -1, 1025):
        assert L.lorb_kf_store_retire_dev(*args(n_max_list=ctypes.c_int32(n))) == INVALID, n
    for n in (-1, 5):
        assert L.lorb_kf_store_retire_dev(*args(n_protect=ctypes.c_int32(n))) == INVALID, n
