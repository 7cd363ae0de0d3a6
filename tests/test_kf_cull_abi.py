"""CPU: the public surface of the points' life and of the map-point culling on the keyframe store -- the header
declares and liblorb.so exports lorb_kf_store_life_write / _life_read / _life_view / _frame_word_view,
lorb_kf_store_observe_dev and lorb_kf_store_cull_dev, the ctypes mirrors agree with the header's structs (the compiled
probe of tests/test_kf_store_abi.py), the constants match, null arguments are rejected without a device, and the ABI
version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_kf_store_life_write", "lorb_kf_store_life_read", "lorb_kf_store_life_view", "lorb_kf_store_frame_word_view",
           "lorb_kf_store_observe_dev", "lorb_kf_store_cull_dev")
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
    for t in ("lorb_kf_store_life_host", "lorb_kf_observe_result", "lorb_kf_cull_params", "lorb_kf_cull_result"):
        assert f"}} {t};" in h, t
    # the citations the contract rests on, the launch counts, and what stays out of scope
    for c in ("src/local_mapping.cpp:82-108", "src/local_mapping.cpp:24-36", "src/visual_odometry.cpp:165,191", ":153-171", ":188-194",
              "src/map_point.cpp:184-199", "src/frame.cpp:896-899", "include/lorb/local_mapping.hpp:66-71", "src/local_mapping.cpp:62-69",
              "#define LORB_KF_FOUND_NEVER 0", "#define LORB_KF_FOUND_SLOTS 1", "#define LORB_KF_CULL_REFERENCE { 0.25f, 2, 3, 3 }",
              "1 kernel launch", "4 kernel launches", "KeyFramesCulling", "rows are not reclaimed", "Out of scope",
              "MapPointsCulling", "lorb_map_step_dev"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_the_launch_counts_are_stated():
    """observe is 1 launch and cull 4 (an insertion stays at 6): the header, the unit and DESIGN say so."""
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    u = open(os.path.join(ROOT, "lorb_slam_amd", "csrc", "lorb_kfcull.hip")).read()
    assert "1 kernel launch, no stream synchronise" in h and "4 kernel launches, no stream synchronise" in h
    assert "lorb_kf_store_insert_dev maintains the state for keyframe K (still six launches" in h
    assert "`lorb_kf_store_observe_dev`: 1 launch" in d and "`lorb_kf_store_cull_dev`: 4 launches" in d
    assert "observe is ONE launch" in u and "cull is FOUR launches" in u
    assert u.count("hipLaunchKernelGGL(") == 1 + 4


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_and_constants_match_the_header():
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_kf_store_life_host", A.KfStoreLifeHost), ("lorb_kf_observe_result", A.KfObserveResult),
             ("lorb_kf_cull_params", A.KfCullParams), ("lorb_kf_cull_result", A.KfCullResult),
             # additive: the structs the existing calls take keep their layout
             ("lorb_kf_store_host", A.KfStoreHost), ("lorb_kf_store_geom_host", A.KfStoreGeomHost),
             ("lorb_kf_insert_result", A.KfInsertResult), ("lorb_kf_ba_result", A.KfBaResult))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    lines.append(f'_Static_assert(LORB_KF_FOUND_NEVER == {A.LORB_KF_FOUND_NEVER}, "the reference rule");')
    lines.append(f'_Static_assert(LORB_KF_FOUND_SLOTS == {A.LORB_KF_FOUND_SLOTS}, "the slots rule");')
    ratio, age_obs, min_obs, age_out = A.LORB_KF_CULL_REFERENCE
    lines.append("static const lorb_kf_cull_params ref = LORB_KF_CULL_REFERENCE;")
    lines.append(f"int probe(void) {{ return ref.min_found_ratio == {ratio}f && ref.age_obs == {age_obs} && ref.min_obs == {min_obs} && "
                 f"ref.age_out == {age_out}; }}")
    src = "\n".join(lines) + "\nint main(void) { return probe() ? 0 : 1; }\n"
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    import kf_cull_ref as L
    assert tuple(A.LORB_KF_CULL_REFERENCE) == tuple(L.REFERENCE) == (0.25, 2, 3, 3)
    assert (A.LORB_KF_FOUND_NEVER, A.LORB_KF_FOUND_SLOTS) == (L.FOUND_NEVER, L.FOUND_SLOTS)
    assert tuple(f for f, _ in A.KfCullResult._fields_) == L.CULL_FIELDS
    assert tuple(f for f, _ in A.KfObserveResult._fields_) == L.OBSERVE_FIELDS


def test_invalid_arguments_are_rejected_without_a_device():
    """With a null context every entry point that takes one returns LORB_E_INVALID whatever else it is given -- full
    dummy arguments, and each argument nulled in turn; a half-given frame group and bad parameters likewise; the
    read-outs reject a null store and a null struct."""
    from lorb_slam_amd import _abi as A
    L = library()
    keep = []

    def buf(n=1024):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.c_void_p(ctypes.addressof(b))

    cur, slots, lmap = A.FrameOut(), A.FrameSlots(), A.LocalMapArrays()
    cur.counts, slots.state, lmap.l2g, lmap.max_local = buf().value, buf().value, buf().value, 8

    def observe_args(**kw):
        a = dict(ctx=None, store=buf(), frame_id=ctypes.c_int32(3), d_cur=ctypes.byref(cur), n_max_cur=ctypes.c_int32(8),
                 d_cur_slots=ctypes.byref(slots), d_cur_slot_gid=buf(), d_cur_slot_id=buf(), lmap=ctypes.byref(lmap), d_update=buf(),
                 d_in_view=buf(), d_local_status=buf(), found_rule=ctypes.c_int32(0), d_result=buf())
        a.update(kw)
        return list(a.values())

    assert L.lorb_kf_store_observe_dev(*observe_args()) == INVALID
    for drop in ("store", "d_cur", "d_cur_slots", "d_cur_slot_gid", "d_cur_slot_id", "lmap", "d_update", "d_in_view", "d_local_status",
                 "d_result"):
        assert L.lorb_kf_store_observe_dev(*observe_args(**{drop: None})) == INVALID, drop
    assert L.lorb_kf_store_observe_dev(*observe_args(n_max_cur=ctypes.c_int32(0))) == INVALID
    assert L.lorb_kf_store_observe_dev(*observe_args(found_rule=ctypes.c_int32(2))) == INVALID

    par = A.KfCullParams(*A.LORB_KF_CULL_REFERENCE)

    def cull_args(**kw):
        a = dict(ctx=None, store=buf(), d_kf=buf(), d_src_status=buf(), par=ctypes.byref(par), d_cur=ctypes.byref(cur),
                 n_max_cur=ctypes.c_int32(8), d_cur_slots=ctypes.byref(slots), d_cur_slot_gid=buf(), d_result=buf())
        a.update(kw)
        return list(a.values())

    assert L.lorb_kf_store_cull_dev(*cull_args()) == INVALID
    for drop in ("store", "d_kf", "d_src_status", "par", "d_cur", "d_cur_slots", "d_cur_slot_gid", "d_result"):
        assert L.lorb_kf_store_cull_dev(*cull_args(**{drop: None})) == INVALID, drop
    assert L.lorb_kf_store_cull_dev(*cull_args(d_cur=None, d_cur_slots=None)) == INVALID   # a half-given frame group
    for bad in (A.KfCullParams(float("nan"), 2, 3, 3), A.KfCullParams(0.25, -1, 3, 3), A.KfCullParams(0.25, 2, 3, -1)):
        assert L.lorb_kf_store_cull_dev(*cull_args(par=ctypes.byref(bad))) == INVALID
    # the life trio and the frame word
    h, w = A.KfStoreLifeHost(), ctypes.c_void_p()
    for f in (L.lorb_kf_store_life_write, L.lorb_kf_store_life_read, L.lorb_kf_store_life_view):
        assert f(None, ctypes.byref(h)) == INVALID
        assert f(buf(), None) == INVALID
    assert L.lorb_kf_store_frame_word_view(None, ctypes.byref(w)) == INVALID
    assert L.lorb_kf_store_frame_word_view(buf(), None) == INVALID
