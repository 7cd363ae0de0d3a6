"""CPU: the motion-tracking chain's public surface -- liblorb.so exports the four new entry points
and lorb::EstimatePoseMotion instantiates against the reference's unchanged headers (compiled as
tests/test_compile_boundary.py compiles the drop-ins: g++ -fsyntax-only over the declaration-only
stand-ins of tests/compile/shim)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LORB_REFERENCE", "/root/reference")
SYMBOLS = ("lorb_search_by_projection_frame_dev", "lorb_ba_pose_only_dev", "lorb_track_motion_dev",
           "lorb_track_motion")


def test_library_exports_the_chain():
    from lorb_slam_amd.runtime import LIB_PATH
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} not built"
    L = ctypes.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing


def test_header_declares_the_chain():
    h = open(os.path.join(ROOT, "include", "lorb_c.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in h, s
    assert "#define LORB_ABI_VERSION 1" in h  # additive: the version stays


def test_result_struct_mirror_matches_the_header():
    """The ctypes mirror and the C struct agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    R, P = A.TrackMotionResult, A.TrackMotionParams
    src = ('#include <stddef.h>\n#include "lorb_c.h"\n'
           f'_Static_assert(sizeof(lorb_track_motion_result) == {ctypes.sizeof(R)}, "size");\n'
           f'_Static_assert(offsetof(lorb_track_motion_result, pose) == {R.pose.offset}, "pose");\n'
           f'_Static_assert(offsetof(lorb_track_motion_result, summary) == {R.summary.offset}, "summary");\n'
           f'_Static_assert(sizeof(lorb_track_motion_params) == {ctypes.sizeof(P)}, "params");\n'
           f'_Static_assert(offsetof(lorb_track_motion_params, fy_eff) == {P.fy_eff.offset}, "fy_eff");\n')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference tree absent")
def test_adapter_instantiates_on_the_reference_types():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-Wno-sign-compare", "-Wno-reorder",
           "-Wno-unused-but-set-variable", "-I", os.path.join(ROOT, "tests", "compile", "shim"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration", "Simple_ORB_SLAM"),
           "-I", os.path.join(REF, "include"), os.path.join(ROOT, "tests", "compile", "track_motion_tu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference tree absent")
def test_reference_caller_still_compiles_unchanged():
    """src/visual_odometry.cpp builds against the drop-in boundary exactly as before the adapter."""
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "compile", "shim"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration", "Simple_ORB_SLAM"),
           "-I", os.path.join(REF, "include"), os.path.join(REF, "src", "visual_odometry.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
