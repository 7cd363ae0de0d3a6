"""CPU: the public surface of the store's appearance and of the refresh -- the header declares and liblorb.so exports
lorb_kf_store_appear_write / _appear_read / _appear_view and lorb_kf_store_refresh_dev, the ctypes mirrors agree with
the header's structs (the compiled probe of tests/test_kf_store_abi.py), null arguments are rejected without a
device, and the ABI version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_kf_store_appear_write", "lorb_kf_store_appear_read", "lorb_kf_store_appear_view", "lorb_kf_store_refresh_dev")
INVALID = -1


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    for s in SYMBOLS:
        getattr(L, s).restype = ctypes.c_int
    return L


def test_library_exports_the_entry_points():
    L = library()
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in h, s
    for t in ("lorb_kf_store_appear_host", "lorb_kf_refresh_result"):
        assert f"}} {t};" in h, t
    # the citations the contract rests on, the divergences, and what is out of scope
    for c in ("src/map_point.cpp:69-129", ":224-264", "src/visual_odometry.cpp:94-95,392-393", "src/frame.cpp:577-594", ":230",
              ":238", ":77-78", ":115-118", ":119", ":147-148", ":26-49", "mpRefKF is the FIRST entry", "no CURRENT window",
              "the descriptor STAYS", "#define LORB_KF_REFRESH_CENTERS      1", "#define LORB_KF_REFRESH_NORMAL_DEPTH 2",
              "#define LORB_KF_REFRESH_DESCRIPTOR   4", "the tracker's slot copies of a descriptor", "KeyFramesCulling"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_kf_store_appear_host", A.KfStoreAppearHost), ("lorb_kf_refresh_result", A.KfRefreshResult),
             ("lorb_kf_ba_result", A.KfBaResult))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    for k in ("CENTERS", "NORMAL_DEPTH", "DESCRIPTOR", "ALL"):
        lines.append(f'_Static_assert(LORB_KF_REFRESH_{k} == {getattr(A, "LORB_KF_REFRESH_" + k)}, "{k}");')
    lines.append(f'_Static_assert(LORB_MAX_LEVELS == {A.LORB_MAX_LEVELS}, "levels");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_invalid_arguments_are_rejected_without_a_device():
    """With a null context the refresh returns LORB_E_INVALID whatever else it is given -- full dummy arguments, and
    each argument nulled in turn; the read-outs and the view reject a null store and a null struct."""
    from lorb_slam_amd import _abi as A
    L = library()
    keep = []

    def buf(n=1024):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.c_void_p(ctypes.addressof(b))

    fp = A.FrameParams()
    full = dict(ctx=None, store=buf(), frame=ctypes.byref(fp), d_ba_result=buf(), what=ctypes.c_int32(A.LORB_KF_REFRESH_ALL),
                d_result=buf())
    assert L.lorb_kf_store_refresh_dev(*full.values()) == INVALID
    for drop in ("store", "frame", "d_ba_result", "d_result"):
        assert L.lorb_kf_store_refresh_dev(*dict(full, **{drop: None}).values()) == INVALID, drop
    assert L.lorb_kf_store_refresh_dev(*dict(full, what=ctypes.c_int32(0)).values()) == INVALID
    a = A.KfStoreAppearHost()
    for f in (L.lorb_kf_store_appear_write, L.lorb_kf_store_appear_read, L.lorb_kf_store_appear_view):
        assert f(None, ctypes.byref(a)) == INVALID
        assert f(buf(), None) == INVALID


def test_the_launch_count_is_stated():
    """A refresh is at most 3 launches with no wait and no copy: the header and DESIGN say so, the unit has three
    launch sites, and the body of the call names no synchronise and no copy."""
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    u = open(os.path.join(ROOT, "lorb_slam_amd", "csrc", "lorb_kfrefresh.hip")).read()
    assert "3 kernel launches, the centres in front of the points, no stream synchronise" in h
    assert "(still six launches, no wait, no copy): K's descriptor" in h
    assert "`lorb_kf_store_refresh_dev(frame, d_ba_result, what)`: 3 launches" in d
    assert u.count("hipLaunchKernelGGL(") == 3
    body = u[u.index("int lorb_kf_store_refresh_dev("):]
    assert body.count("hipLaunchKernelGGL(") == 3 and body.index("k_kfr_head") < body.index("k_kfr_points") < body.index("k_kfr_record")
    for word in ("hipStreamSynchronize", "hipMemcpy", "hipDeviceSynchronize", "spin_sync", "atomic"):
        assert word not in body, word
    kernels = u[:u.index('extern "C"')]
    assert "atomic" not in kernels.replace("No atomics", "")      # every point writes its own row
