"""CPU: the frame builder's public surface -- the header declares and liblorb.so exports every new
entry point, the ctypes mirrors agree with the header's structs (a compiled probe), null / invalid
arguments are rejected without a device, and lorb::BuildFrame instantiates against the reference's
Frame (compiled as tests/test_compile_boundary.py compiles the friend-patched adapters: g++
-fsyntax-only over the declaration-only stand-ins of tests/compile/shim)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LORB_REFERENCE", "/root/reference")
SYMBOLS = ("lorb_frame_builder_create", "lorb_frame_builder_capacity", "lorb_frame_build_dev", "lorb_frame_build",
           "lorb_frame_builder_destroy")
INVALID = -1


def library():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    return ctypes.CDLL(LIB_PATH)


def test_library_exports_the_builder():
    L = library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing


def test_header_declares_the_builder():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in h, s
    for t in ("lorb_frame_config", "lorb_frame_side", "lorb_frame_out", "lorb_frame_builder"):
        assert f"}} {t};" in h or f"typedef struct {t} {t};" in h, t
    assert "src/frame.cpp:17-63" in h and "AssignFeaturesToGrid" in h
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    pairs = (("lorb_frame_config", A.FrameConfig), ("lorb_frame_side", A.FrameSide), ("lorb_frame_out", A.FrameOut))
    lines = ['#include <stddef.h>', '#include "lorb_c.h"']
    for name, S in pairs:
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(S)}, "{name} size");')
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{name}.{f}");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_rejected_without_a_device():
    """No entry point touches the device before it has a context / builder to work on."""
    from lorb_slam_amd import _abi as A
    L = library()
    for s in SYMBOLS:
        getattr(L, s).restype = ctypes.c_int
    cfg, out, b = A.FrameConfig(), A.FrameOut(), ctypes.c_void_p()
    cap, pb = ctypes.c_int32(7), ctypes.c_int64(7)
    assert L.lorb_frame_builder_create(None, ctypes.byref(cfg), ctypes.byref(b)) == INVALID and not b.value
    assert L.lorb_frame_builder_capacity(None, ctypes.byref(cap), ctypes.byref(pb)) == INVALID
    assert (cap.value, pb.value) == (7, 7)
    img = (ctypes.c_uint8 * 16)()
    assert L.lorb_frame_build_dev(None, img, ctypes.c_int32(4), img, ctypes.c_int32(4), ctypes.byref(out)) == INVALID
    assert L.lorb_frame_build(None, img, ctypes.c_int32(4), img, ctypes.c_int32(4), ctypes.c_int32(0),
                              ctypes.byref(out)) == INVALID
    assert L.lorb_frame_builder_destroy(None) == INVALID


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference tree absent")
def test_build_frame_instantiates_on_the_reference_frame(tmp_path):
    """tests/compile/frame_tu.cpp against the reference's headers with the friend declarations of
    INTEGRATION.md §4 (mDescriptors / mDescriptorsRight are private)."""
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(REF, "include"), inc)
    fwd = "namespace lorb { template <class> struct FrameTraits; template <class> struct PointTraits; }\n"
    for name, cls, frd in (("frame.h", "Frame", "friend struct lorb::FrameTraits<Frame>;"),
                           ("map_point.h", "MapPoint", "friend struct lorb::PointTraits<MapPoint>;")):
        s = (inc / name).read_text()
        s = s.replace("namespace Simple_ORB_SLAM", fwd + "namespace Simple_ORB_SLAM", 1)
        s2 = re.sub(r"(class %s\s*\{\s*public:)" % cls, r"\1\n\t%s\npublic:" % frd, s, count=1)
        assert s2 != s, name
        (inc / name).write_text(s2)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-Wno-sign-compare", "-Wno-reorder",
           "-Wno-unused-but-set-variable", "-DLORB_REFERENCE_FRIENDS", "-I", os.path.join(ROOT, "tests", "compile", "shim"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration", "Simple_ORB_SLAM"),
           "-I", str(inc), os.path.join(ROOT, "tests", "compile", "frame_tu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
