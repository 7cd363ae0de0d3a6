"""CPU: the public surface of the growing map store -- the header declares and liblorb.so exports
lorb_kf_store_create / _destroy / _view / _counts / _read and lorb_kf_store_insert_dev, the ctypes mirrors of the
capacities, the host store and the record agree with the header's structs (a compiled probe), null arguments and
bad bounds are rejected without a device, and the ABI version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lorb_kf_store_create", "lorb_kf_store_destroy", "lorb_kf_store_view", "lorb_kf_store_counts", "lorb_kf_store_read",
           "lorb_kf_store_insert_dev")
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
    for t in ("lorb_kf_store_caps", "lorb_kf_store_host", "lorb_kf_insert_result"):
        assert f"}} {t};" in h, t
    assert "typedef struct lorb_kf_store lorb_kf_store;" in h
    for c in ("#define LORB_KF_GATE_RATIO 0", "#define LORB_KF_GATE_NONE  1"):
        assert c in h, c
    # the citations the contract rests on, and the conventions stated as restated
    for c in ("src/visual_odometry.cpp:356-404", "src/local_mapping.cpp:57-70", "src/frame.cpp:801-869", ":754-788",
              "src/map_point.cpp:133-139", "src/map_point.cpp:224-264", "RESTATED, not", "size_t nMax = -1",
              "mConnectedKeyFrameWeights", "the weakest ten"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe), the gate
    constants on their values."""
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_kf_store_caps", A.KfStoreCaps), ("lorb_kf_store_host", A.KfStoreHost),
             ("lorb_kf_insert_result", A.KfInsertResult), ("lorb_map_store", A.MapStore))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    lines.append(f'_Static_assert(LORB_KF_GATE_RATIO == {A.LORB_KF_GATE_RATIO} && LORB_KF_GATE_NONE == {A.LORB_KF_GATE_NONE}, "gates");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def insert_args(A, n_max_cur=100, gate=0, n_levels=8, drop=None):
    """A full argument list of lorb_kf_store_insert_dev over dummy host storage; `drop` nulls one."""
    keep = []

    def buf(n=256):
        b = (ctypes.c_uint8 * n)()
        keep.append(b)
        return ctypes.addressof(b)

    cur = A.FrameOut()
    for side in (cur.left, cur.right):
        for f, _ in A.FrameSide._fields_:
            setattr(side, f, buf())
    cur.u_right, cur.depth, cur.counts = buf(), buf(), buf()
    slots = A.FrameSlots(buf(), buf(), buf())
    fp = A.FrameParams()
    fp.n_levels = n_levels
    keep += [cur, slots, fp]
    a = dict(ctx=None, store=ctypes.c_void_p(buf(1024)), frame=ctypes.byref(fp), d_cur=ctypes.byref(cur),
             n_max_cur=ctypes.c_int32(n_max_cur), d_cur_slots=ctypes.byref(slots), d_cur_slot_gid=ctypes.c_void_p(buf()),
             d_cur_pose=ctypes.c_void_p(buf()), d_src_status=ctypes.c_void_p(buf()), gate=ctypes.c_int32(gate),
             d_refer_kf=ctypes.c_void_p(buf()), d_update=ctypes.c_void_p(buf()), d_result=ctypes.c_void_p(buf()))
    if drop:
        a[drop] = None
    return list(a.values()), keep


def test_invalid_arguments_are_rejected_without_a_device():
    """No entry point touches a device, or its store argument, before it has a context to work on: with a null
    context every call returns LORB_E_INVALID whatever else it is given -- full dummy arguments, each argument nulled
    in turn, the bounds 0 and -1, an unknown gate.  (The same with a live context, where the message names the
    cause, is tests/test_gpu_kf_store.py::test_errors.)"""
    from lorb_slam_amd import _abi as A
    L = library()
    f = L.lorb_kf_store_insert_dev
    args, keep = insert_args(A)
    assert f(*args) == INVALID
    for drop in ("store", "frame", "d_cur", "d_cur_slots", "d_cur_slot_gid", "d_cur_pose", "d_src_status", "d_refer_kf", "d_update",
                 "d_result"):
        args, keep = insert_args(A, drop=drop)
        assert f(*args) == INVALID, drop
    for kw in (dict(n_max_cur=0), dict(n_max_cur=-1), dict(n_max_cur=1 << 30), dict(gate=2), dict(gate=-1), dict(n_levels=0),
               dict(n_levels=17)):
        args, keep = insert_args(A, **kw)
        assert f(*args) == INVALID, kw
    # create / view / counts / read / destroy
    out = ctypes.c_void_p()
    for caps in ((4, 16, 16, 16), (0, 16, 16, 16), (4, 0, 16, 16), (4, 16, 0, 16), (4, 16, 16, 0), (4097, 16, 16, 16), (-1, -1, -1, -1)):
        c = A.KfStoreCaps(*caps)
        assert L.lorb_kf_store_create(None, ctypes.byref(c), None, ctypes.byref(out)) == INVALID and not out.value
    c = A.KfStoreCaps(4, 16, 16, 16)
    init = A.KfStoreHost()
    assert L.lorb_kf_store_create(None, ctypes.byref(c), ctypes.byref(init), ctypes.byref(out)) == INVALID
    assert L.lorb_kf_store_create(None, None, None, ctypes.byref(out)) == INVALID
    assert L.lorb_kf_store_create(None, ctypes.byref(c), None, None) == INVALID
    view, host, cnt = A.MapStore(), A.KfStoreHost(), (ctypes.c_int32 * 6)()
    assert L.lorb_kf_store_view(None, ctypes.byref(view)) == INVALID
    assert L.lorb_kf_store_counts(None, cnt, ctypes.c_int32(6)) == INVALID
    assert L.lorb_kf_store_read(None, ctypes.byref(host)) == INVALID
    assert L.lorb_kf_store_destroy(None) == INVALID
