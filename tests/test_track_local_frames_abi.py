"""CPU: the public surface of local-map tracking from a built frame -- the header declares and
liblorb.so exports lorb_track_local_frames_dev, the ctypes mirrors of its record and of the id source
agree with the header's structs (a compiled probe), null arguments, bad bounds and a non-NULL in_frame
are rejected without a device, and the ABI version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lorb_track_local_frames_dev"
INVALID = -1


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    getattr(L, SYMBOL).restype = ctypes.c_int
    return L


def test_library_exports_the_entry_point():
    assert hasattr(library(), SYMBOL)


def test_header_declares_the_entry_point():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    assert f"int {SYMBOL}(" in h
    for t in ("lorb_track_local_frames_result", "lorb_track_local_id_source"):
        assert f"}} {t};" in h, t
    # the citations of the reference the contract rests on, and what the device pose is equal to
    for c in ("src/visual_odometry.cpp:153-171", "src/visual_odometry.cpp:173-209", "src/bundle_adjust.cpp:198-201",
              "Tcw_in is DEFINED as what the record"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_track_local_frames_result", A.TrackLocalFramesResult),
             ("lorb_track_local_id_source", A.TrackLocalIdSource))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    lines.append(f'_Static_assert(sizeof(lorb_track_local_result) == {ctypes.sizeof(A.TrackLocalResult)}, "local size");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def local_args(A, n_max_cur=100, n_points=100, drop=None, in_frame=False, ids=True, n_levels=8, min_matches=20):
    """A full argument list of lorb_track_local_frames_dev over dummy host storage; `drop` nulls one."""
    keep = []

    def buf(n):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.addressof(b)

    cur = A.FrameOut()
    for side in (cur.left, cur.right):
        for f, _ in A.FrameSide._fields_:
            setattr(side, f, buf(64))
    cur.u_right, cur.depth, cur.counts = buf(64), buf(64), buf(64)
    slots = A.FrameSlots(buf(64), buf(64), buf(64))
    fps = A.FrameParams()
    fps.n_levels = n_levels
    pts = A.MapPointsDev(n_points, buf(64), buf(64), buf(64), buf(64), buf(64), buf(64), buf(64),
                         buf(64) if in_frame else None)
    src = A.TrackLocalIdSource(buf(64), buf(256), buf(64), 100, 0)
    par, opt = A.TrackLocalParams(0.5, 1.0, min_matches, 1.0), A.LMOptions.default()
    keep += [cur, slots, fps, pts, src, par, opt]
    a = dict(ctx=None, frame=ctypes.byref(fps), d_cur=ctypes.byref(cur), n_max_cur=ctypes.c_int32(n_max_cur),
             d_cur_slots=ctypes.byref(slots), d_cur_slot_id=ctypes.c_void_p(buf(64)), d_pose=ctypes.c_void_p(buf(64)),
             d_src_status=ctypes.c_void_p(buf(64)), ids=ctypes.byref(src) if ids else None, d_pts=ctypes.byref(pts),
             par=ctypes.byref(par), opt=ctypes.byref(opt), d_in_view=ctypes.c_void_p(buf(64)),
             d_track=ctypes.c_void_p(buf(64)), d_level=ctypes.c_void_p(buf(64)), d_assign=ctypes.c_void_p(buf(64)),
             d_result=ctypes.c_void_p(buf(512)))
    if drop:
        a[drop] = None
    return list(a.values()), keep


def test_invalid_arguments_are_rejected_without_a_device():
    """The entry point touches no device before it has a context to work on: with a null context every
    call returns LORB_E_INVALID, whatever else it is given -- full dummy arguments, each argument nulled
    in turn, the bounds 0 and -1, 4097 x 2048 > 8M against d_pts->n, a negative point count, n_levels out
    of range, a negative min_matches and a non-NULL in_frame.  (The same with a live context, where the
    message names the cause, is tests/test_gpu_track_local_frames.py::test_errors.)"""
    from lorb_slam_amd import _abi as A
    f = getattr(library(), SYMBOL)
    args, keep = local_args(A)
    assert f(*args) == INVALID
    for drop in ("frame", "d_cur", "d_cur_slots", "d_cur_slot_id", "d_pose", "d_src_status", "ids", "d_pts", "par", "opt",
                 "d_in_view", "d_track", "d_level", "d_assign", "d_result"):
        args, keep = local_args(A, drop=drop)
        assert f(*args) == INVALID, drop
    for nc, npt in ((0, 100), (-1, 100), (4097, 2048), (2048, 4097), (100, -1)):
        args, keep = local_args(A, n_max_cur=nc, n_points=npt)
        assert f(*args) == INVALID, (nc, npt)
    for kw in (dict(in_frame=True), dict(n_levels=0), dict(n_levels=17), dict(min_matches=-1), dict(ids=False)):
        args, keep = local_args(A, **kw)
        assert f(*args) == INVALID, kw
