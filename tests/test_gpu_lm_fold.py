"""GPU: the folded LM iteration tail against the k_ba_lm_end kernel it replaces.

A fused iteration of an unsharded plan on the two-sided Cholesky runs the previous iteration's tail
(step validity, tolerances, accept / reject) in the prologue of its k_ba_ls instead of in a kernel of
its own; LORB_NO_FOLD=1, read at every solve, keeps the kernel.  Both forms evaluate the same
expressions on the same inputs, so every comparison here is exact: poses, points, every summary field
and every field of every trace record.  The smallest window that reaches the two-sided Cholesky has
n >= 128 rows: 24 keyframes."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth
from test_gpu_ba import close, lm_match

pytestmark = pytest.mark.gpu


def tol0(**kw):
    return A.LMOptions.default(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0,
                               **{"max_num_iterations": 10, **kw})


@pytest.fixture(scope="module")
def base():
    w = synth.ba_window(seed=1, n_kf=24, n_pts=400, n_fixed=2, fixed_obs_per_kf=50)
    assert len(w["obs_point"]) == 3100
    return w


@pytest.fixture(scope="module")
def cut(base):
    """the base window with points 0-4 cut to their first observation each"""
    keep = np.ones(len(base["obs_point"]), bool)
    for p in range(5):
        keep[np.flatnonzero(base["obs_point"] == p)[1:]] = False
    return dict(base, obs_point=base["obs_point"][keep], obs_frame=base["obs_frame"][keep], obs_uv=base["obs_uv"][keep])


def kernel_nodes(plan):
    from lorb_slam_amd.runtime import lib
    v = (C.c_int32 * 12)()
    plan.ctx.check(lib().lorb_ba_plan_info(plan._p, v, C.c_int32(12)), "lorb_ba_plan_info")
    return int(v[11])


def solve(ctx, wins, opt, monkeypatch, fold):
    """one plan of `wins` solved with the folded tail or (LORB_NO_FOLD=1) the kernel: per window poses,
    points, summary and trace, then the plan's Cholesky kind and the kernel launches of its graph"""
    from lorb_slam_amd.runtime import BAPlan
    plan = BAPlan(ctx, wins)
    try:
        with monkeypatch.context() as m:
            if fold:
                m.delenv("LORB_NO_FOLD", raising=False)
            else:
                m.setenv("LORB_NO_FOLD", "1")
            plan.solve(opt)
        P, X, s = plan.read()
        return P, X, s, [plan.trace(i) for i in range(len(wins))], plan.info()["cholesky"], kernel_nodes(plan)
    finally:
        plan.close()


def identical(a, b, label=""):
    for w in range(len(a[0])):
        assert np.array_equal(a[0][w], b[0][w]) and np.array_equal(a[1][w], b[1][w]), (label, w)
        assert a[2][w] == b[2][w], (label, w, a[2][w], b[2][w])
        assert a[3][w] == b[3][w], (label, w)


def both(ctx, wins, opt, monkeypatch, label=""):
    f, k = solve(ctx, wins, opt, monkeypatch, True), solve(ctx, wins, opt, monkeypatch, False)
    identical(f, k, label)
    return f, k


def outcomes(trace):
    return [r["outcome"] for r in trace]


def test_rejected_steps(ctx, base, monkeypatch):
    opt = tol0(initial_trust_region_radius=1e10)
    Po, Xo, so, ot = O.ba_local_traced(base, opt)
    assert outcomes(ot) == ["accepted"] * 6 + ["rejected"] * 4, outcomes(ot)
    f, k = both(ctx, [base], opt, monkeypatch)
    assert f[4] == 2 and f[5] < k[5], (f[4], f[5], k[5])
    lm_match(f[2][0], so, gt=f[3][0], ot=ot, label="fold, rejected steps")
    assert close(f[0][0], Po), np.abs(f[0][0] - Po).max()
    assert close(f[1][0], Xo), np.abs(f[1][0] - Xo).max()


def test_invalid_steps_and_failure_stop(ctx, cut, monkeypatch):
    """a point block that is not invertible is flagged by the very k_ba_ls that evaluates the previous
    iteration's flag; the unfolded form is the yardstick"""
    opt = tol0(initial_trust_region_radius=1e16)
    _, _, _, ot = O.ba_local_traced(cut, opt)
    i, a = "invalid", "accepted"
    assert outcomes(ot) == [i, i, a, i, a, i, i, a, a, i], outcomes(ot)
    f, k = both(ctx, [cut], opt, monkeypatch, "1e16")
    assert f[4] == 2 and f[5] < k[5]
    print("gpu outcomes at 1e16:", outcomes(f[3][0]))
    opt = tol0(initial_trust_region_radius=1e22, max_trust_region_radius=1e22)
    _, _, so, ot = O.ba_local_traced(cut, opt)
    assert outcomes(ot) == [i] * 5 and so["termination"] == "FAILURE", (outcomes(ot), so)
    f, k = both(ctx, [cut], opt, monkeypatch, "1e22")
    print("gpu outcomes at 1e22:", outcomes(f[3][0]), f[2][0])


def test_tolerance_stop_in_mid_solve(ctx, base, monkeypatch):
    opt = A.LMOptions.default()
    _, _, so, ot = O.ba_local_traced(base, opt)
    assert outcomes(ot) == ["accepted"] * 6 + ["function_tol"], outcomes(ot)
    f, _ = both(ctx, [base], opt, monkeypatch)
    assert f[2][0]["termination"] == so["termination"] and f[2][0]["iterations"] == so["iterations"] == 7, (f[2][0], so)
    assert outcomes(f[3][0]) == outcomes(ot)


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_budget_edges(ctx, base, monkeypatch, n):
    """no folded consumer at all (0, 1), exactly one (2), one behind another (3)"""
    f, k = both(ctx, [base], tol0(max_num_iterations=n), monkeypatch)
    assert f[2][0]["iterations"] == n and len(f[3][0]) == n
    assert k[5] - f[5] == max(n - 1, 0), (n, f[5], k[5])


def test_more_than_64_cameras(ctx, monkeypatch):
    """the second pass of the tail's camera loop.  Tracks of 3 and 4 keyframes (band 23): with the
    default tracks (band 47) a band of 70 cameras does not fit the two-sided Cholesky's LDS, and the
    plan would not run the fused iteration at all"""
    w = synth.ba_window(seed=1, n_kf=70, n_pts=600, n_fixed=2, fixed_obs_per_kf=50, obs_lens=(3, 4))
    f, k = both(ctx, [w], tol0(), monkeypatch)
    assert f[4] == 2 and f[5] < k[5] and f[2][0]["iterations"] == 10


@pytest.fixture(scope="module")
def three(base):
    """the base window, another of its size, and one of 30 keyframes / 300 points; a plan takes one set
    of options, so the three are solved together at tolerance 0 and at the Ceres defaults, which
    stop them at iterations 7, 7 and 9 (the oracle's counts)"""
    return [base, synth.ba_window(seed=2, n_kf=24, n_pts=400, n_fixed=2, fixed_obs_per_kf=50),
            synth.ba_window(seed=4, n_kf=30, n_pts=300, n_fixed=2, fixed_obs_per_kf=50)]


def test_several_windows(ctx, three, monkeypatch):
    """one plan of three windows (the folded k_ba_ls learns its window from the group record); each
    window equals its solo solve, at tolerance 0 and at the Ceres defaults"""
    for opt in (tol0(), A.LMOptions.default()):
        f, k = both(ctx, three, opt, monkeypatch)
        assert f[4] == 2 and f[5] < k[5]
        for i, w in enumerate(three):
            s = solve(ctx, [w], opt, monkeypatch, True)
            assert np.array_equal(f[0][i], s[0][0]) and np.array_equal(f[1][i], s[1][0]), i
            assert f[2][i] == s[2][0] and f[3][i] == s[3][0], i
    assert len({s["iterations"] for s in f[2]}) > 1, f[2]


def test_plan_group(ctx, three, monkeypatch):
    from lorb_slam_amd.runtime import BAGroup, BAPlan, lib
    opt = A.LMOptions.default()
    res = {}
    for fold in (True, False):
        gp = [BAPlan(ctx, [w]) for w in three]
        G = BAGroup(ctx, gp)
        try:
            with monkeypatch.context() as m:
                if fold:
                    m.delenv("LORB_NO_FOLD", raising=False)
                else:
                    m.setenv("LORB_NO_FOLD", "1")
                G.solve(opt)
            rd = [p.read() for p in gp]
            v = (C.c_int32 * 4)()
            ctx.check(lib().lorb_ba_group_info(G._p, v, C.c_int32(4)), "lorb_ba_group_info")
            assert v[1] == 1, list(v)
            res[fold] = ([r[0][0] for r in rd], [r[1][0] for r in rd], [r[2][0] for r in rd],
                         [p.trace(0) for p in gp], 2, int(v[3]))
        finally:
            G.close()
            for p in gp:
                p.close()
    identical(res[True], res[False], "group")
    assert res[False][5] - res[True][5] == opt.max_num_iterations - 1, (res[True][5], res[False][5])
    for i, w in enumerate(three):
        s = solve(ctx, [w], opt, monkeypatch, True)
        assert np.array_equal(res[True][0][i], s[0][0]) and np.array_equal(res[True][1][i], s[1][0]), i
        assert res[True][2][i] == s[2][0] and res[True][3][i] == s[3][0], i


def test_window_without_point_group_takes_the_kernel(ctx, base, monkeypatch):
    """a window with cameras and no point group has no k_ba_ls workgroup to commit its state: the plan
    keeps the k_ba_lm_end kernel (as many launches either way) and solves as before"""
    bare = dict(pose_init=base["pose_init"].copy(), fixed_pose=np.zeros((0, 6), np.float32),
                point_init=np.zeros((0, 3), np.float32), obs_point=np.zeros(0, np.int32),
                obs_frame=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2), np.float32), intr=base["intr"])
    f, k = both(ctx, [base, bare], tol0(), monkeypatch)
    assert f[5] == k[5], (f[5], k[5])
    assert np.array_equal(f[0][1], base["pose_init"].astype(np.float64))
    s = solve(ctx, [base], tol0(), monkeypatch, False)
    assert close(f[0][0], s[0][0]) and close(f[1][0], s[1][0]) and f[2][0]["iterations"] == 10


def test_launch_count(ctx, monkeypatch):
    """a 10-iteration C3-size solve: the folded form drops k_ba_lm_end from 9 of its 10 iterations"""
    w = synth.ba_window(seed=3, n_kf=20, n_pts=4000, n_fixed=2, fixed_obs_per_kf=400)
    f, k = both(ctx, [w], tol0(), monkeypatch)
    assert f[4] == 2 and k[5] - f[5] == 9, (f[5], k[5])
