"""CPU: the public surface of the device-resident pose hand-over -- the header declares and liblorb.so
exports lorb_Tcw_to_pose, lorb_frame_pose_from_Tcw, lorb_track_motion_frames_pose_dev and
lorb_frame_pose_finish_dev; the ctypes mirrors of lorb_frame_pose and lorb_motion_model agree with the
header's structs (a compiled probe); the two host functions agree with the restatement
(tests/motion_model_ref.py) -- the vector within its derived tolerance, Twc and the translation bit for bit;
null arguments are rejected without a device; the ABI version is still 1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import motion_model_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_Tcw_to_pose", "lorb_frame_pose_from_Tcw", "lorb_track_motion_frames_pose_dev", "lorb_frame_pose_finish_dev")
INVALID = -1
F32P = ctypes.POINTER(ctypes.c_float)


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    for s in SYMBOLS:
        getattr(L, s).restype = ctypes.c_int
    return L


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_library_exports_the_entry_points():
    L = library()
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in h, s
    for t in ("lorb_frame_pose", "lorb_motion_model"):
        assert f"}} {t};" in h, t
    for c in ("src/visual_odometry.cpp:65-66", "src/frame.cpp:570-575", "cvRodrigues2", "double accumulation in k order"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_frame_pose", A.FramePose), ("lorb_motion_model", A.MotionModel))
    assert ctypes.sizeof(A.FramePose) == 4 * (16 + 16 + 6 + 1) and ctypes.sizeof(A.MotionModel) == 4 * 17
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def host_pose(L, T):
    """(lorb_Tcw_to_pose's vector and translation, lorb_frame_pose_from_Tcw's block) of a 4 x 4 float32."""
    from lorb_slam_amd import _abi as A
    T = np.ascontiguousarray(T, np.float32).reshape(16)
    r, t, blk = np.zeros(3, np.float32), np.zeros(3, np.float32), A.FramePose()
    assert L.lorb_Tcw_to_pose(T.ctypes.data_as(F32P), r.ctypes.data_as(F32P), t.ctypes.data_as(F32P)) == 0
    assert L.lorb_frame_pose_from_Tcw(T.ctypes.data_as(F32P), ctypes.byref(blk)) == 0
    return r, t, blk


def check_pose(L, name, T):
    ref = M.set_pose(T)
    r, t, blk = host_pose(L, T)
    s = ref["s"]
    assert s is None or abs(s - 1e-5) > 1e-9, (name, s)  # both sides take the same branch
    err = np.abs(r.astype(np.float64) - ref["pose"][:3].astype(np.float64))
    print(name, "s", s, "vector", r, "|dev - ref|", err, "tolerance", M.vec_tol(ref["pose"][:3], s))
    assert M.vec_close(r, ref["pose"][:3], s), name
    assert same(t, ref["pose"][3:]), name
    assert same(np.array(blk.Tcw[:], np.float32).reshape(4, 4), ref["Tcw"]), name
    assert same(np.array(blk.Twc[:], np.float32).reshape(4, 4), ref["Twc"]), name
    assert same(np.array(blk.pose[:3], np.float32), r) and same(np.array(blk.pose[3:], np.float32), t), name
    assert blk.status == 0


@pytest.mark.parametrize("name,T", M.hand_poses(), ids=[n for n, _ in M.hand_poses()])
def test_host_functions_on_the_hand_poses(name, T):
    check_pose(library(), name, T)


def test_host_functions_on_seeded_products():
    L = library()
    for i, T in enumerate(M.seeded_poses(50, 20261020)):
        check_pose(L, f"seeded_{i}", T)


def test_out_of_range_and_singular_matrices():
    """Not finite / outside [-100, 100): the zero vector.  A singular rotation block is no pose; the call
    still returns (a finite or NaN vector, never a fault) and Twc is LU32f's all-zero answer."""
    L = library()
    for bad in (np.nan, np.inf, -np.inf, 100.0, -100.5):
        T = np.eye(4, dtype=np.float32)
        T[2, 1] = bad
        r, t, _ = host_pose(L, T)
        assert same(r, np.zeros(3, np.float32))
    T = np.zeros((4, 4), np.float32)
    _, _, blk = host_pose(L, T)
    assert not np.array(blk.Twc[:]).any()


def test_null_arguments_are_rejected():
    from lorb_slam_amd import _abi as A
    L = library()
    T, r, t = (np.zeros(n, np.float32) for n in (16, 3, 3))
    p = lambda a: a.ctypes.data_as(F32P)  # noqa: E731
    assert L.lorb_Tcw_to_pose(None, p(r), p(t)) == INVALID
    assert L.lorb_Tcw_to_pose(p(T), None, p(t)) == INVALID
    assert L.lorb_Tcw_to_pose(p(T), p(r), None) == INVALID
    blk = A.FramePose()
    assert L.lorb_frame_pose_from_Tcw(None, ctypes.byref(blk)) == INVALID
    assert L.lorb_frame_pose_from_Tcw(p(T), None) == INVALID
    # the two device calls: nothing is touched before there is a context
    buf = (ctypes.c_uint8 * 512)()
    q = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.lorb_frame_pose_finish_dev(None, q, q, q, q) == INVALID
    cur = A.FrameOut()
    slots = A.FrameSlots(q, q, q)
    fps, par, opt = A.FrameParams(), A.TrackMotionParams(15.0, 30.0, 20, 1.0), A.LMOptions.default()
    f = L.lorb_track_motion_frames_pose_dev
    assert f(None, ctypes.byref(fps), q, ctypes.byref(cur), ctypes.c_int32(10), ctypes.byref(slots), ctypes.c_int32(0), q, q,
             ctypes.byref(cur), ctypes.c_int32(10), ctypes.byref(slots), None, ctypes.byref(par), ctypes.byref(opt), q, q) == INVALID
