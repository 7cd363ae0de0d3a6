"""CPU: the local-map tracking chain's public surface -- liblorb.so exports the two new entry points,
the ctypes mirrors agree with the header's structs, and lorb::EstimatePoseLocal instantiates against
the reference's unchanged headers (compiled as tests/test_compile_boundary.py compiles the drop-ins:
g++ -fsyntax-only over the declaration-only stand-ins of tests/compile/shim)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LORB_REFERENCE", "/root/reference")
SYMBOLS = ("lorb_track_local_dev", "lorb_track_local")


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


def test_struct_mirrors_match_the_header():
    """The ctypes mirrors and the C structs agree on size and offsets (checked by compiling a probe)."""
    from lorb_slam_amd import _abi as A
    R, P = A.TrackLocalResult, A.TrackLocalParams
    lines = ['#include <stddef.h>', '#include "lorb_c.h"',
             f'_Static_assert(sizeof(lorb_track_local_result) == {ctypes.sizeof(R)}, "result size");',
             f'_Static_assert(sizeof(lorb_track_local_params) == {ctypes.sizeof(P)}, "params size");']
    for name, S in (("lorb_track_local_result", R), ("lorb_track_local_params", P)):
        for f, _ in S._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, "{f}");')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference tree absent")
def test_adapter_instantiates_on_the_reference_types():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-Wno-sign-compare", "-Wno-reorder",
           "-Wno-unused-but-set-variable", "-I", os.path.join(ROOT, "tests", "compile", "shim"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration", "Simple_ORB_SLAM"),
           "-I", os.path.join(REF, "include"), os.path.join(ROOT, "tests", "compile", "track_local_tu.cpp")]
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
