"""CPU: the hand-built windowed-matcher cases (tests/window_cases.py).  For every semantic case the C
oracle equals the pure-Python restatement (tests/pyref.py) exactly, the properties the case claims
hold, its built distances are what it says, and a hand-derived answer is what both compute.  The path
cases are too large for pure Python: the oracle runs them and their sizes are checked against the
kernel constants they are meant to straddle."""
import numpy as np
import pytest

import oracle as O
import pyref
import window_cases as W


def run_oracle(case):
    fn = O.search_by_projection_frame if case["kind"] == "a4" else O.search_by_projection_local
    return fn(*case["args"])


def run_pyref(case):
    if case["kind"] == "a4":
        return pyref.search_by_projection_frame(*case["args"])
    a, n = pyref.search_by_projection_local(*case["args"])
    return a.astype(np.int32), n  # -1 == LORB_ASSIGN_UNCHANGED; a5 never writes NULL


@pytest.mark.parametrize("name", sorted(W.SEMANTIC))
def test_semantic_case(name):
    case = W.get(name)
    for text, ok in case["claims"].items():
        assert ok, text
    for q, k, d in case["dist"]:
        assert pyref.descriptor_distance(case["qdesc"][q], case["kdesc"][k]) == d, (q, k, d)
    a_o, n_o = run_oracle(case)
    a_p, n_p = run_pyref(case)
    assert n_o == n_p
    assert np.array_equal(a_o, a_p)
    if case["expect"] is not None:
        assert n_o == case["expect"][1]
        assert np.array_equal(a_o, case["expect"][0])
    else:
        assert n_o > 0


@pytest.mark.parametrize("hist,want", [
    ([0] * 30, (-1, -1, -1)),
    ([0, 10, 0, 1, 1] + [0] * 25, (1, 3, 4)),        # 0.1f * 10 == 1: not below, both kept
    ([0, 11, 0, 1] + [0] * 26, (1, -1, -1)),
    ([20, 0, 2, 0, 1] + [0] * 25, (0, 2, -1)),
    ([0, 3, 3, 0, 3, 3] + [0] * 24, (1, 2, 4)),      # ties go to the lower bins
    ([0] * 29 + [7], (29, -1, -1)),
    ([5, 0, 9] + [0] * 27, (2, 0, -1)),
    ([1, 2, 3, 4] + [0] * 26, (3, 2, 1)),
])
def test_compute_three_maxima(hist, want):
    assert O.compute_three_maxima(hist) == want
    assert pyref.compute_three_maxima(hist) == want


def test_compute_three_maxima_random():
    rng = np.random.default_rng(0)
    for _ in range(300):
        h = rng.integers(0, rng.integers(1, 40), 30) * (rng.uniform(size=30) < rng.uniform(0.05, 1.0))
        assert O.compute_three_maxima(h) == pyref.compute_three_maxima(h), h


@pytest.mark.parametrize("name", sorted(W.PATH))
def test_path_case(name):
    case = W.get(name)
    nq, nk = case["shape"]
    args = case["args"]
    if case["kind"] == "a4":
        assert len(args[4]["has_mp"]) == nq and len(args[2]["x"]) == nk
        live = int(args[4]["has_mp"].sum())
    else:
        assert len(args[3]["proj_x"]) == nq and len(args[1]["x"]) == nk
        live = int(args[3]["track_in_view"].sum())
    assert live <= 3000
    a, n = run_oracle(case)
    assert n >= min(20, live // 4) and (a >= 0).sum() > 0


def test_path_shapes_straddle_the_constants():
    S = W.PATH_SHAPES
    assert S["stage_at"][1] == W.K_STAGE_KPS and S["stage_over"][1] == W.K_STAGE_KPS + 1
    assert S["regc_at"][0] == W.K_REG_QUERIES and S["regc_over"][0] == W.K_REG_QUERIES + 1
    assert S["strided_at"][0] * S["strided_at"][1] == W.K_CAND_STRIDED
    assert W.K_CAND_STRIDED < S["strided_over"][0] * S["strided_over"][1] <= W.K_CAND_STRIDED + S["strided_over"][1]
    for k in ("stage_at", "stage_over", "regc_at", "regc_over", "strided_at"):
        assert S[k][0] * S[k][1] <= W.K_CAND_STRIDED and W.resolve_lds_mode(*S[k]) == 2
    assert S["grid_global"][1] > W.K_GRID_LDS and W.resolve_lds_mode(*S["grid_global"]) == 2
    assert S["resolve_mode1"][1] > W.K_GRID_LDS and W.resolve_lds_mode(*S["resolve_mode1"]) == 1
    assert 4 * S["resolve_mode1"][1] + 2 * S["resolve_mode1"][0] == 30800
    assert W.resolve_lds_mode(*S["resolve_mode0"]) == 0 and sum(S["resolve_mode0"]) == 30800
    assert S["resolve_mode0"][0] * S["resolve_mode0"][1] > W.K_CAND_BOUND
    assert S["resolve_mode1"][0] * S["resolve_mode1"][1] > W.K_CAND_BOUND  # also reads the total back
    # the cluster cases: stride below, at and above the resolver's register set
    assert {1, 7} < set(range(W.K_REG_CAND)) and W.K_REG_CAND == 8


def test_kernel_constants_restated():
    """The constants window_cases.py restates are the ones lorb_window.hip declares."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "lorb_slam_amd", "csrc", "lorb_window.hip")).read()
    assert re.search(r"constexpr int kRegCand = 8;", src)
    assert re.search(r"constexpr int kStageKps = 1024;", src)
    assert re.search(r"const bool regc = np <= 1024;", src)
    assert re.search(r"constexpr size_t kCandStrided = size_t\(1\) << 20;", src)
    assert re.search(r"constexpr int kGridLds = 6144;", src)
    assert re.search(r"constexpr size_t kCandBound = size_t\(8\) << 20;", src)
    assert len(re.findall(r"<= 120 \* 1024", src)) == 2  # resolve_lds_mode: 30720 words


def test_local_map_path_problems():
    """track_local_map inputs at the path shapes: sizes, and a search that finds matches."""
    for name in ("stage_at", "resolve_mode0"):
        pr = W.path_local_map(name)
        nq, nk = W.PATH_SHAPES[name]
        assert len(pr["pts"]["max_dist"]) == nq and len(pr["kps"]["x"]) == nk
        fr, assign, nm = O.track_local_map(pr["fp"], pr["Tcw"], pr["kps"], pr["slot_state"], pr["pts"], 0.5, 1.0)
        assert 0 < fr["in_view"].sum() <= 3000 and nm > 5
