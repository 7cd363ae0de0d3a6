"""GPU: lorb::EstimatePoseLocal (include/lorb/adapters.hpp) on plain C++ test frames -- a frame that
passes, one that fails the gate and one whose bad held points must leave their slots NULL -- checked
against the oracle composed in C inside tests/cpp/test_track_local.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD = os.path.join(CPP, "_build")
pytestmark = pytest.mark.gpu


def build():
    """The commands of tests/cpp/Makefile's test_adapters rule, for test_track_local.cpp."""
    os.makedirs(BUILD, exist_ok=True)
    objs = []
    for name in ("match", "ba"):
        obj = os.path.join(BUILD, f"tl_{name}.o")
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-std=c99", "-ffp-contract=off", "-c",
                        os.path.join(ROOT, "oracle", f"{name}.c"), "-o", obj], check=True)
        objs.append(obj)
    exe = os.path.join(BUILD, "test_track_local")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-o", exe,
                    os.path.join(CPP, "test_track_local.cpp"), *objs, "-L" + os.path.join(ROOT, "lorb_slam_amd"), "-llorb",
                    "-Wl,-rpath," + os.path.join(ROOT, "lorb_slam_amd"), "-lpthread", "-lm"], check=True)
    return exe


def test_cpp_estimate_pose_local():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "RESULT PASS" in r.stdout, r.stdout + r.stderr
