"""CPU: the public surface of the device slots and of motion tracking from two device-built frames --
the header declares and liblorb.so exports lorb_frame_slots_fill_dev and lorb_track_motion_frames_dev,
the ctypes mirrors agree with the header's structs (a compiled probe), null arguments and a bound pair
past the asynchronous limit are rejected without a device, and the ABI version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_frame_slots_fill_dev", "lorb_track_motion_frames_dev")
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
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in h, s
    for t in ("lorb_frame_slots", "lorb_track_frames_result"):
        assert f"}} {t};" in h, t
    for d in ("#define LORB_SLOTS_UPDATE_FRAME 0", "#define LORB_SLOTS_INITIALIZE   1"):
        assert d in h, d
    # the citations of the reference the contract rests on, and what is deliberately not produced
    for c in ("src/visual_odometry.cpp:215-230", "src/visual_odometry.cpp:86-99", "src/visual_odometry.cpp:121-137",
              "src/map_point.cpp:26-35", "src/visual_odometry.cpp:80", "mNormalVector"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_frame_slots", A.FrameSlots), ("lorb_track_frames_result", A.TrackFramesResult))
    rename = {"pass_": "pass"}
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {rename.get(f, f)}) == {getattr(S, f).offset}, "{name}.{f}");')
    M = A.TrackMotionResult
    lines.append(f'_Static_assert(sizeof(lorb_track_motion_result) == {ctypes.sizeof(M)}, "motion size");')
    lines.append(f'_Static_assert(LORB_SLOTS_UPDATE_FRAME == {A.LORB_SLOTS_UPDATE_FRAME} && '
                 f'LORB_SLOTS_INITIALIZE == {A.LORB_SLOTS_INITIALIZE}, "fill modes");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def frames_args(A, n_max_cur=100, n_max_last=100, drop=None):
    """A full argument list of lorb_track_motion_frames_dev over dummy host storage; `drop` nulls one."""
    keep = []

    def buf(n):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.addressof(b)

    def frame():
        o = A.FrameOut()
        for side in (o.left, o.right):
            for f, _ in A.FrameSide._fields_:
                setattr(side, f, buf(64))
        o.u_right, o.depth, o.counts = buf(64), buf(64), buf(64)
        return o

    def slots():
        return A.FrameSlots(buf(64), buf(64), buf(64))

    fps = A.FrameParams()
    fps.n_levels = 8
    T = (ctypes.c_float * 16)()
    pi = (ctypes.c_float * 6)()
    par, opt = A.TrackMotionParams(15.0, 30.0, 20, 1.0), A.LMOptions.default()
    cur, last, cs, ls = frame(), frame(), slots(), slots()
    keep += [fps, T, pi, par, opt, cur, last, cs, ls]
    a = dict(ctx=None, cur=ctypes.byref(fps), cur_Tcw=T, pose_init=pi, d_cur=ctypes.byref(cur),
             n_max_cur=ctypes.c_int32(n_max_cur), d_cur_slots=ctypes.byref(cs), given=ctypes.c_int32(0), last_Tcw=T,
             d_last=ctypes.byref(last), n_max_last=ctypes.c_int32(n_max_last), d_last_slots=ctypes.byref(ls),
             outlier=None, par=ctypes.byref(par), opt=ctypes.byref(opt), d_assign=ctypes.c_void_p(buf(64)),
             d_result=ctypes.c_void_p(buf(256)))
    if drop:
        a[drop] = None
    return list(a.values()), keep


def test_null_arguments_are_rejected_without_a_device():
    """Neither entry point touches a device before it has a context to work on: with a null context
    every call returns LORB_E_INVALID, whatever else it is given -- full dummy arguments, any one of
    them null, and a bound pair past the asynchronous limit (2048 x 4097 > 8M).  (The same bounds with a
    live context are tests/test_gpu_track_frames.py::test_errors.)"""
    from lorb_slam_amd import _abi as A
    L = library()
    fps, out, sl = A.FrameParams(), A.FrameOut(), A.FrameSlots()
    T = (ctypes.c_float * 16)()
    fill = L.lorb_frame_slots_fill_dev
    made = ctypes.c_int32(7)
    for mode in (0, 1, 2):
        assert fill(None, ctypes.byref(fps), T, ctypes.byref(out), ctypes.c_int32(8), ctypes.c_int32(mode),
                    ctypes.byref(sl), ctypes.byref(made)) == INVALID
    assert fill(None, None, None, None, ctypes.c_int32(8), ctypes.c_int32(0), None, None) == INVALID
    assert made.value == 7
    args, keep = frames_args(A)
    assert L.lorb_track_motion_frames_dev(*args) == INVALID
    for drop in ("cur", "cur_Tcw", "pose_init", "d_cur", "d_cur_slots", "last_Tcw", "d_last", "d_last_slots", "par", "opt",
                 "d_assign", "d_result"):
        args, keep = frames_args(A, drop=drop)
        assert L.lorb_track_motion_frames_dev(*args) == INVALID, drop
    for nc, nl in ((4097, 2048), (2048, 4097), (2900, 2900), (0, 100), (100, 0), (-1, 100)):
        args, keep = frames_args(A, n_max_cur=nc, n_max_last=nl)
        assert L.lorb_track_motion_frames_dev(*args) == INVALID, (nc, nl)
