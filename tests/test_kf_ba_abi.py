"""CPU: the public surface of the store's geometry and of the local bundle adjustment on the store -- the header
declares and liblorb.so exports lorb_kf_store_create_geom / _geom_read, lorb_kf_store_ba_gather_dev,
lorb_kf_store_local_ba_dev and lorb_kf_ba_window_read, the ctypes mirrors agree with the header's structs (the
compiled probe of tests/test_kf_store_abi.py), null arguments are rejected without a device, and the ABI version
is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_kf_store_create_geom", "lorb_kf_store_geom_read", "lorb_kf_store_ba_gather_dev", "lorb_kf_store_local_ba_dev",
           "lorb_kf_ba_window_read")
INVALID = -1


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    for s in SYMBOLS + ("lorb_kf_store_geom_view",):
        getattr(L, s).restype = ctypes.c_int
    return L


def test_library_exports_the_entry_points():
    L = library()
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS + ("lorb_kf_store_geom_view",):
        assert f"int {s}(" in h, s
    for t in ("lorb_kf_store_geom_host", "lorb_kf_ba_result", "lorb_kf_ba_window_host"):
        assert f"}} {t};" in h, t
    # the invariant, the citations the contract rests on, and what is out of scope
    for c in ("kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p", "src/bundle_adjust.cpp:207-330", "src/local_mapping.cpp:32",
              ":210-220", ":224-241", ":270-303", ":317-329", "src/map_point.cpp:52-55", "src/frame.cpp:729-732", "Out of scope",
              "MapPointsCulling", "lorb_map_step_dev", "#define LORB_KF_BA_MAX_LOCAL 128"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_kf_store_geom_host", A.KfStoreGeomHost), ("lorb_kf_ba_result", A.KfBaResult),
             ("lorb_kf_ba_window_host", A.KfBaWindowHost), ("lorb_kf_store_host", A.KfStoreHost),
             ("lorb_kf_store_caps", A.KfStoreCaps))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    lines.append(f'_Static_assert(LORB_KF_BA_MAX_LOCAL == {A.LORB_KF_BA_MAX_LOCAL}, "local frames");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_invalid_arguments_are_rejected_without_a_device():
    """With a null context every entry point that takes one returns LORB_E_INVALID whatever else it is given -- full
    dummy arguments, and each argument nulled in turn; the two read-outs reject a null store and a null output."""
    from lorb_slam_amd import _abi as A
    L = library()
    keep = []

    def buf(n=1024):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.c_void_p(ctypes.addressof(b))

    fp, opt, summ = A.FrameParams(), A.LMOptions.default(), A.BASummary()

    def ba_args(drop=None, solve=False):
        a = dict(ctx=None, store=buf(), frame=ctypes.byref(fp), d_kf=buf(), d_src_status=buf())
        if solve:
            a["opt"] = ctypes.byref(opt)
        a["d_result"] = buf()
        if solve:
            a["summary"] = ctypes.byref(summ)
        if drop:
            a[drop] = None
        return list(a.values())

    assert L.lorb_kf_store_ba_gather_dev(*ba_args()) == INVALID
    for drop in ("store", "frame", "d_kf", "d_src_status", "d_result"):
        assert L.lorb_kf_store_ba_gather_dev(*ba_args(drop)) == INVALID, drop
    assert L.lorb_kf_store_local_ba_dev(*ba_args(solve=True)) == INVALID
    for drop in ("store", "frame", "d_kf", "d_src_status", "opt", "d_result", "summary"):
        assert L.lorb_kf_store_local_ba_dev(*ba_args(drop, solve=True)) == INVALID, drop
    # create_geom
    out = ctypes.c_void_p()
    caps, init, geom = A.KfStoreCaps(4, 16, 16, 16), A.KfStoreHost(), A.KfStoreGeomHost()
    full = dict(ctx=None, caps=ctypes.byref(caps), init=ctypes.byref(init), geom=ctypes.byref(geom), out=ctypes.byref(out))
    assert L.lorb_kf_store_create_geom(*full.values()) == INVALID and not out.value
    for drop in ("caps", "init", "geom", "out"):
        assert L.lorb_kf_store_create_geom(*dict(full, **{drop: None}).values()) == INVALID, drop
    # the read-outs and the view
    g, w = A.KfStoreGeomHost(), A.KfBaWindowHost()
    assert L.lorb_kf_store_geom_read(None, ctypes.byref(g)) == INVALID
    assert L.lorb_kf_store_geom_read(buf(), None) == INVALID
    assert L.lorb_kf_store_geom_view(None, ctypes.byref(g)) == INVALID
    assert L.lorb_kf_store_geom_view(buf(), None) == INVALID
    assert L.lorb_kf_ba_window_read(None, ctypes.byref(w)) == INVALID
    assert L.lorb_kf_ba_window_read(buf(), None) == INVALID
