"""CPU: the public surface of the second motion attempt on the reference keyframe -- the header declares
and liblorb.so exports lorb_track_motion_refer_pose_dev with its citations; the ctypes mirror of
lorb_track_refer_result agrees with the header's struct (a compiled probe); null arguments, a partially
given gid group and a partially given guard pair are rejected without a device; the ABI version is still 1."""
import ctypes
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lorb_track_motion_refer_pose_dev"
INVALID = -1
I32 = ctypes.c_int32


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
    assert "} lorb_track_refer_result;" in h
    decl = h[:h.index(f"int {SYMBOL}(")]
    comment = decl[decl.rindex("/* The second motion attempt"):]
    for c in ("src/visual_odometry.cpp:50-54,117-138", ":311-312", ":128-131", "lorb_track_local_id_source",
              "reported, not followed"):
        assert c in comment, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirror_matches_the_header():
    """The ctypes mirror and the C struct agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    S, name = A.TrackReferResult, "lorb_track_refer_result"
    assert ctypes.sizeof(S) == 4 * 5
    assert [f for f, _ in S._fields_] == ["due", "ran", "stale", "first_nmatches_first", "first_nmatches_retry"]
    lines = ['#include <stddef.h>', '#include "lorb_c.h"',
             f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");']
    for f, _ in S._fields_:
        lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


class Args:
    """A full argument list over host dummies.  No call made from it gets as far as reading one: each is
    rejected by the argument checks, which run before the context is touched."""

    NAMES = ("ctx", "cur", "d_cur_pose", "d_cur", "n_max_cur", "d_cur_slots", "first_slots_given", "d_refer_pose", "d_model",
             "d_refer", "n_max_refer", "d_refer_slots", "d_refer_outlier", "d_last_slot_gid", "n_max_last", "d_refer_slot_gid",
             "d_cur_slot_gid", "refer_kf", "d_refer_kf", "d_prev_update", "par", "opt", "d_assign", "d_result",
             "d_refer_result")
    REQUIRED = ("ctx", "cur", "d_cur_pose", "d_cur", "d_cur_slots", "d_refer_pose", "d_model", "d_refer", "d_refer_slots",
                "par", "opt", "d_assign", "d_result", "d_refer_result")
    GIDS = ("d_last_slot_gid", "d_refer_slot_gid", "d_cur_slot_gid")
    GUARD = ("d_refer_kf", "d_prev_update")

    def __init__(self):
        from lorb_slam_amd import _abi as A
        self.buf = (ctypes.c_uint8 * 65536)()
        q = ctypes.c_void_p(ctypes.addressof(self.buf))
        self.keep = (A.FrameParams(), A.FrameOut(), A.FrameSlots(q, q, q), A.TrackMotionParams(15.0, 30.0, 20, 1.0),
                     A.LMOptions.default())
        fps, frame, slots, par, opt = self.keep
        self.v = dict(ctx=q, cur=ctypes.byref(fps), d_cur_pose=q, d_cur=ctypes.byref(frame), n_max_cur=I32(10),
                      d_cur_slots=ctypes.byref(slots), first_slots_given=I32(0), d_refer_pose=q, d_model=q,
                      d_refer=ctypes.byref(frame), n_max_refer=I32(10), d_refer_slots=ctypes.byref(slots), d_refer_outlier=None,
                      d_last_slot_gid=q, n_max_last=I32(10), d_refer_slot_gid=q, d_cur_slot_gid=q, refer_kf=I32(0),
                      d_refer_kf=q, d_prev_update=q, par=ctypes.byref(par), opt=ctypes.byref(opt), d_assign=q, d_result=q,
                      d_refer_result=q)

    def call(self, L, **null):
        v = dict(self.v, **null)
        return getattr(L, SYMBOL)(*[v[k] for k in self.NAMES])


def test_null_arguments_are_rejected():
    L, a = library(), Args()
    for name in Args.REQUIRED:
        assert a.call(L, **{name: None}) == INVALID, name


def test_a_partial_gid_group_is_rejected():
    L, a = library(), Args()
    for k in (1, 2):
        for missing in itertools.combinations(Args.GIDS, k):
            assert a.call(L, **{m: None for m in missing}) == INVALID, missing


def test_a_partial_guard_pair_is_rejected():
    L, a = library(), Args()
    for missing in Args.GUARD:
        assert a.call(L, **{missing: None}) == INVALID, missing
    # with either group partial and the other absent
    assert a.call(L, d_refer_kf=None, d_last_slot_gid=None, d_refer_slot_gid=None, d_cur_slot_gid=None) == INVALID
    assert a.call(L, d_last_slot_gid=None, d_refer_kf=None, d_prev_update=None) == INVALID
