"""CPU: the public surface of the device-built local map -- the header declares and liblorb.so exports
lorb_local_map_create / _destroy / _view, lorb_local_map_update_dev and lorb_local_map_ids_back_dev, the
ctypes mirrors of the store, the view and the record agree with the header's structs (a compiled probe),
null arguments and bad bounds are rejected without a device, and the ABI version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_local_map_create", "lorb_local_map_view", "lorb_local_map_update_dev", "lorb_local_map_ids_back_dev")
INVALID = -1


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    for s in (*SYMBOLS, "lorb_local_map_destroy"):
        getattr(L, s).restype = ctypes.c_int
    return L


def test_library_exports_the_entry_points():
    L = library()
    for s in (*SYMBOLS, "lorb_local_map_destroy"):
        assert hasattr(L, s), s


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in (*SYMBOLS, "lorb_local_map_destroy"):
        assert f"int {s}(" in h, s
    for t in ("lorb_map_store", "lorb_local_map_arrays", "lorb_local_map_result"):
        assert f"}} {t};" in h, t
    # the citations the contract rests on, the ordering convention and the restated expansion loop
    for c in ("src/visual_odometry.cpp:234-340", "src/frame.cpp:735-741", "std::map<Frame*, ...>", "std::set<MapPoint*>",
              "INDEX loop over the growing list"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_map_store", A.MapStore), ("lorb_local_map_arrays", A.LocalMapArrays),
             ("lorb_local_map_result", A.LocalMapResult), ("lorb_map_points_dev", A.MapPointsDev))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def update_args(A, n_max_cur=100, n_points=100, n_kf=10, drop=None, ids=True, **counts):
    """A full argument list of lorb_local_map_update_dev over dummy host storage; `drop` nulls one."""
    keep = []

    def buf(n=64):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.addressof(b)

    cur = A.FrameOut()
    for side in (cur.left, cur.right):
        for f, _ in A.FrameSide._fields_:
            setattr(side, f, buf())
    cur.u_right, cur.depth, cur.counts = buf(), buf(), buf()
    slots = A.FrameSlots(buf(), buf(), buf())
    pts = A.MapPointsDev(n_points, buf(), buf(), buf(), buf(), buf(), buf(), buf(), None)
    store = A.MapStore(pts, buf(), buf(), buf(), buf(), buf(), buf(), buf(), n_kf, counts.get("n_obs", 5),
                       counts.get("n_kf_slots", 5), counts.get("n_cov", 5))
    src = A.TrackLocalIdSource(buf(), buf(256), buf(), 100, 0)
    keep += [cur, slots, store, src]
    a = dict(ctx=None, map=ctypes.c_void_p(buf(256)), store=ctypes.byref(store), d_cur=ctypes.byref(cur),
             n_max_cur=ctypes.c_int32(n_max_cur), d_cur_slots=ctypes.byref(slots), d_cur_slot_gid=ctypes.c_void_p(buf()),
             d_cur_slot_id=ctypes.c_void_p(buf()), d_src_status=ctypes.c_void_p(buf()),
             ids=ctypes.byref(src) if ids else None, d_result=ctypes.c_void_p(buf()))
    if drop:
        a[drop] = None
    return list(a.values()), keep


def test_invalid_arguments_are_rejected_without_a_device():
    """No entry point touches a device, or its map argument, before it has a context to work on: with a
    null context every call returns LORB_E_INVALID whatever else it is given -- full dummy arguments, each
    argument nulled in turn, the bounds 0 and -1, negative counts, counts above any capacity.  (The same
    with a live context, where the message names the cause, is tests/test_gpu_local_map.py::test_errors.)"""
    from lorb_slam_amd import _abi as A
    L = library()
    f = L.lorb_local_map_update_dev
    args, keep = update_args(A)
    assert f(*args) == INVALID
    for drop in ("map", "store", "d_cur", "d_cur_slots", "d_cur_slot_gid", "d_cur_slot_id", "d_src_status", "ids", "d_result"):
        args, keep = update_args(A, drop=drop)
        assert f(*args) == INVALID, drop
    for kw in (dict(n_max_cur=0), dict(n_max_cur=-1), dict(n_max_cur=(8 << 20) + 1), dict(n_points=-1), dict(n_kf=-1),
               dict(n_points=1 << 30), dict(n_kf=1 << 30), dict(n_obs=-1), dict(n_kf_slots=-1), dict(n_cov=-1), dict(ids=False)):
        args, keep = update_args(A, **kw)
        assert f(*args) == INVALID, kw
    # create / view / destroy / ids_back
    out = ctypes.c_void_p()
    for caps in ((16, 4, 16), (0, 4, 16), (16, 0, 16), (16, 4, 0), (-1, -1, -1)):
        assert L.lorb_local_map_create(None, *map(ctypes.c_int32, caps), ctypes.byref(out)) == INVALID and not out.value
    assert L.lorb_local_map_create(None, ctypes.c_int32(16), ctypes.c_int32(4), ctypes.c_int32(16), None) == INVALID
    view = A.LocalMapArrays()
    assert L.lorb_local_map_view(None, ctypes.byref(view)) == INVALID
    assert L.lorb_local_map_destroy(None) == INVALID
    args, keep = update_args(A)
    _, m, _, cur, nmax, slots, gid, sid, status, _, _ = args
    g = L.lorb_local_map_ids_back_dev
    assert g(None, m, cur, nmax, slots, sid, status, gid) == INVALID
    for i in range(1, 8):
        if i == 3:
            continue
        a = [None, m, cur, nmax, slots, sid, status, gid]
        a[i] = None
        assert g(*a) == INVALID, i
    for n in (0, -1):
        assert g(None, m, cur, ctypes.c_int32(n), slots, sid, status, gid) == INVALID
