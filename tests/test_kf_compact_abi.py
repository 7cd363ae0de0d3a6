"""CPU: the public surface of the keyframe store's compaction -- the header declares and liblorb.so exports
lorb_kf_store_compact_dev, the ctypes mirrors agree with the header's structs (the compiled probe of
tests/test_kf_store_abi.py), the constant matches, the launch count is stated, a null context is rejected without a device, and the ABI
version is still 1."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lorb_kf_store_compact_dev"
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
    for t in ("lorb_kf_gid_table", "lorb_kf_compact_result"):
        assert f"}} {t};" in h, t
    # what is read, the on-device order, what is never written, where it must not sit, what stays out of scope
    for c in ("#define LORB_KF_COMPACT_MAX_TABLES 8", "Map::EraseMapPoint", "before the first write", "NOT A BYTE",
              "Nothing at or past the OLD true count is written", "nothing at or past\n * *d_count in a table",
              "NOT between a frame's lorb_local_map_update_dev and its lorb_local_map_ids_back_dev", "the pointers of\n *      "
              "lorb_kf_store_view / _geom_view / _life_view never change", "at rest over the whole capacity",
              "5 kernel launches, no stream synchronise, no device-to-host read and no\n * host-to-device copy",
              "KeyFramesCulling", "remapping a lorb_local_map", "lorb_map_step_dev"):
        assert c in h, c
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_the_launch_count_is_stated():
    """A compaction is 5 launches: the header, the unit and DESIGN say so, and the unit has five launch sites."""
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    u = open(os.path.join(ROOT, "lorb_slam_amd", "csrc", "lorb_kfcompact.hip")).read()
    assert "`lorb_kf_store_compact_dev`: 5 launches" in d
    assert "FIVE launches" in u and u.count("hipLaunchKernelGGL(") == 5
    for word in ("hipStreamSynchronize", "hipMemcpy", "hipDeviceSynchronize"):   # no wait and no copy in the call
        assert word not in u, word


def test_abi_version_is_still_1():
    L = library()
    L.lorb_abi_version.restype = ctypes.c_int
    assert L.lorb_abi_version() == 1


def test_struct_mirrors_and_constants_match_the_header():
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_kf_gid_table", A.KfGidTable), ("lorb_kf_compact_result", A.KfCompactResult),
             # additive: the structs the existing calls take keep their layout
             ("lorb_kf_store_host", A.KfStoreHost), ("lorb_kf_store_geom_host", A.KfStoreGeomHost),
             ("lorb_kf_store_life_host", A.KfStoreLifeHost), ("lorb_kf_insert_result", A.KfInsertResult),
             ("lorb_kf_ba_result", A.KfBaResult), ("lorb_kf_cull_result", A.KfCullResult))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    lines.append(f'_Static_assert(LORB_KF_COMPACT_MAX_TABLES == {A.LORB_KF_COMPACT_MAX_TABLES}, "the table limit");')
    src = "\n".join(lines) + "\nint main(void) { return 0; }\n"
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    import kf_compact_ref as M
    assert tuple(f for f, _ in A.KfCompactResult._fields_) == M.FIELDS
    assert A.LORB_KF_COMPACT_MAX_TABLES == M.MAX_TABLES == 8


def test_a_null_context_is_rejected_without_a_device():
    """With a null context the entry point returns LORB_E_INVALID before it looks at anything else, whatever the other
    arguments are.  That is all a machine without a device can show; the LORB_E_INVALID list of the contract is
    checked with a live context in tests/test_gpu_kf_compact.py::test_compact_errors."""
    from lorb_slam_amd import _abi as A
    L = library()
    b = (ctypes.c_uint8 * 1024)()
    p = ctypes.c_void_p(ctypes.addressof(b))
    t = (A.KfGidTable * 2)(A.KfGidTable(p.value, 8, p.value), A.KfGidTable(p.value + 64, 8, p.value))
    f = getattr(L, SYMBOL)
    assert f(None, p, p, t, ctypes.c_int32(2), p, p) == INVALID
    assert f(None, None, None, None, ctypes.c_int32(0), None, None) == INVALID
