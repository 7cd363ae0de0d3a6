"""GPU parity: the plan builders (lorb_ba_build.hip) on the windows of plan_edge_cases.py -- long point
runs at chosen wave / workgroup positions, runs of unobserved points, a point with up to kGB - 1
observations (group size bound S down to 1), more than 512 point groups, the camera counts around the
fused covisibility tables' limits, an idle camera, a split covisibility graph, one camera -- against the
oracle's or_ba_local under the options the reference runs (Ceres defaults): iteration-level LM parity,
strict, and the solution within 1e-5 (test_gpu_ba.close).  A wrong run end, a lost camera x point bit or
a mis-cut point group gives a plan that solves a slightly different problem; only parity shows it.

Per case: (a) the sorted upload (k_db_sorted), (b) the same slots with unused ones among them (flag 16:
k_db_keys / scan1 / scatter / segsort / cov) -- equal to (a) bit for bit, (c) shuffled slots
(k_db_segsort's insertion sort above 16 observations), (d) the host builder, (e) unobserved points
returned untouched.  Then the drop-in solver, one plan object rebuilt across cases, the builders'
limits, duplicates inside long runs and the build's error bits."""
import functools

import numpy as np
import pytest

import oracle as O
import plan_edge_cases as E
from lorb_slam_amd import _abi as A
from lorb_slam_amd.runtime import BAPlan, BAPlanDev, BASolver, LorbError
from test_gpu_ba import _dev_window, close, lm_match, plan_traced
from test_gpu_solver import check

pytestmark = pytest.mark.gpu
CASES = list(E.CASES)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """(poses, points, summary, trace) of the oracle on a case, computed once"""
    return O.ba_local_traced(E.case(name)[0], A.LMOptions.default())


def free_all(*dicts):
    for a in {id(v): v for d in dicts for v in d.values()}.values():
        a.free()


def solved(plan):
    plan.solve(A.LMOptions.default())
    (P,), (X,), (s,) = plan.read()
    return dict(P=P, X=X, s=s, trace=plan.trace(0), info=plan.info())


def dev_solve(ctx, w, **kw):
    """one window on a fresh device-built plan"""
    arrays, order = _dev_window(ctx, w, **kw)
    try:
        plan = BAPlanDev(ctx, arrays, len(w["pose_init"]), len(w["fixed_pose"]), w["intr"])
        try:
            return dict(solved(plan), order=order)
        finally:
            plan.close()
    finally:
        free_all(arrays)


_sorted = {}


def sorted_result(ctx, name):
    """(a): the case uploaded as is, solved once for the tests that compare with it"""
    if name not in _sorted:
        _sorted[name] = dev_solve(ctx, E.case(name)[0])
    return _sorted[name]


def against_oracle(r, o, label):
    """strict iteration-level parity and the solution to 1e-5"""
    Po, Xo, so, ot = o
    assert r["s"]["termination"] == so["termination"], (label, r["s"], so)
    assert lm_match(r["s"], so, gt=r["trace"], ot=ot, label=label) is None, label
    assert r["s"]["iterations"] == so["iterations"] and r["s"]["successful_steps"] == so["successful_steps"], (label, r["s"], so)
    assert close(r["P"], Po), (label, np.abs(r["P"] - Po).max())
    assert close(r["X"], Xo), (label, np.abs(r["X"] - Xo).max())


def same_bits(a, b, label):
    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["X"], b["X"]), label
    assert a["s"] == b["s"], (label, a["s"], b["s"])
    assert a["trace"] == b["trace"], label


@pytest.mark.parametrize("name", CASES)
def test_sorted_path(ctx, name):
    """(a) and (e)"""
    w, _ = E.case(name)
    r = sorted_result(ctx, name)
    against_oracle(r, oracle_of(name), f"{name} sorted")
    K, P = len(w["obs_point"]), len(w["point_init"])
    info = r["info"]
    assert info["observations"] == K and info["points"] == P and info["cameras"] == len(w["pose_init"]), info
    S, G, SF, NSG = E.layout(w)
    assert info["point_groups"] == G == (K + P - 1) // S + 1, (info, S, G)
    assert info["partial_runs"] == (NSG if SF > 1 else 0), (info, SF, NSG)
    if name == "partial_runs":
        assert info["point_groups"] > 512 and info["partial_runs"] == (info["point_groups"] + 1) // 2, info
    if name.startswith("gaps"):
        unseen = np.bincount(w["obs_point"], minlength=P) == 0
        assert unseen.sum() > 1000
        assert np.array_equal(r["X"][unseen], w["point_init"][unseen].astype(np.float64))


@pytest.mark.parametrize("name", CASES)
def test_general_path_equals_sorted(ctx, name):
    """(b): unused slots among the same slots, order kept: the general phase builds the same integer
    structure and the same per-point order, so the solve is the sorted upload's bit for bit"""
    w, _ = E.case(name)
    a = sorted_result(ctx, name)
    b = dev_solve(ctx, w, holes=max(41, len(w["obs_point"]) // 7))
    assert b["info"] == a["info"], (a["info"], b["info"])
    same_bits(a, b, f"{name} holes")
    against_oracle(b, oracle_of(name), f"{name} holes")


@pytest.mark.parametrize("name", ["run_lengths", "maxk_255", "maxk_254", "maxk_128"])
def test_shuffled_slots(ctx, name):
    """(c): the counting sort's slots come back in order from k_db_segsort, by insertion above 16"""
    w, _ = E.case(name)
    r = dev_solve(ctx, w, shuffle_seed=5)
    order = r["order"]
    srt = np.argsort(w["obs_point"][order], kind="stable")
    wo = dict(w, obs_point=w["obs_point"][order][srt], obs_frame=w["obs_frame"][order][srt], obs_uv=w["obs_uv"][order][srt])
    assert np.array_equal(wo["obs_point"], w["obs_point"]) and not np.array_equal(wo["obs_frame"], w["obs_frame"])
    against_oracle(r, O.ba_local_traced(wo, A.LMOptions.default()), f"{name} shuffled")
    assert r["info"]["observations"] == len(w["obs_point"]) and r["info"]["point_groups"] == E.layout(w)[1]


@pytest.mark.parametrize("name", CASES)
def test_host_builder(ctx, name):
    """(d) and (e): build_plan on the same window; band and Cholesky kernel as the device plan's"""
    w, _ = E.case(name)
    Po, Xo, so, ot = oracle_of(name)
    plan = BAPlan(ctx, [w])
    try:
        r = solved(plan)
    finally:
        plan.close()
    Pg, Xg, sg, info = r["P"], r["X"], r["s"], r["info"]
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"], (sg, so)
    assert lm_match(sg, so, gt=r["trace"], ot=ot, label=f"{name} host plan") is None
    assert close(Pg, Po), np.abs(Pg - Po).max()
    assert close(Xg, Xo), np.abs(Xg - Xo).max()
    dinfo = sorted_result(ctx, name)["info"]
    assert (info["band"], info["cholesky"]) == (dinfo["band"], dinfo["cholesky"]), (info, dinfo)
    if name.startswith("gaps"):
        unseen = np.bincount(w["obs_point"], minlength=len(w["point_init"])) == 0
        assert np.array_equal(Xg[unseen], w["point_init"][unseen].astype(np.float64))


def test_drop_in_solver(ctx):
    """BASolver.solve on cases 1, 2 and 3: resident device-built plans, no host-built fallback"""
    s = BASolver(ctx)
    try:
        for name in ("run_lengths", "gaps", "gaps_mult64", "maxk_255", "maxk_254", "maxk_128", "run_lengths"):
            check(s, E.case(name)[0], A.LMOptions.default(), label=f"solver {name}", strict=True)
            assert s.info()["host_plan_fallback"] == 0, (name, s.info())
        assert s.info()["resident_plans"] == 2, s.info()
        # a point with kGB = 256 observations: the device build refuses it, the host-built plan takes it
        check(s, E.host_limit(256)[0], A.LMOptions.default(), label="solver 256 observations", strict=True)
        assert s.info()["host_plan_fallback"] == 1, s.info()
        check(s, E.case("run_lengths")[0], A.LMOptions.default(), label="solver run_lengths again", strict=True)
        assert s.info()["host_plan_fallback"] == 0, s.info()
    finally:
        s.close()


def _same_capacity(ctx, wins, **kw):
    """device arrays of several windows of one shape, all with the capacities of the largest"""
    Pm = max(len(w["point_init"]) for w in wins) + 37
    Km = max(len(w["obs_point"]) for w in wins) + 500
    return [_dev_window(ctx, w, extra_pts=Pm - len(w["point_init"]), extra_obs=Km - len(w["obs_point"]) - kw.get("holes", 0),
                        **kw)[0] for w in wins]


def test_rebuild_in_place(ctx):
    """one BAPlanDev rebuilt with update(): case 1 -> case 2 (more points: the group buffers grow) -> case 1
    -> short runs only (S = 247 against 166) -> case 1.  Every result against the oracle; case 1's three are
    equal bit for bit."""
    w1, w2, w3 = E.case("run_lengths")[0], E.case("gaps")[0], E.short_runs()
    a1, a2, a3 = _same_capacity(ctx, [w1, w2, w3])
    plan = None
    try:
        plan = BAPlanDev(ctx, a1, len(w1["pose_init"]), len(w1["fixed_pose"]), w1["intr"])
        res = [solved(plan)]
        for a in (a2, a1, a3, a1):
            plan.update(a)
            res.append(solved(plan))
        for r in (res[0], res[2], res[4]):
            against_oracle(r, oracle_of("run_lengths"), "rebuild case 1")
        against_oracle(res[1], oracle_of("gaps"), "rebuild case 2")
        against_oracle(res[3], O.ba_local_traced(w3, A.LMOptions.default()), "rebuild short runs")
        assert E.layout(w3)[0] != E.layout(w1)[0] and res[1]["info"]["point_groups"] > res[0]["info"]["point_groups"]
        same_bits(res[0], res[2], "third build")
        same_bits(res[0], res[4], "fifth build")
        assert res[0]["info"] == res[2]["info"] == res[4]["info"]
        same_bits(res[0], sorted_result(ctx, "run_lengths"), "fresh plan")
    finally:
        if plan is not None:
            plan.close()
        free_all(a1, a2, a3)


def test_device_plan_observation_limit(ctx):
    """a device plan takes a point with up to kGB - 1 = 255 observations (maxk_255); one with 256 is
    refused at creation and at a rebuild, and the plan object then rebuilds and solves case 1"""
    good, bad = E.device_limit()
    ag, ab = _same_capacity(ctx, [good, bad])
    plan = None
    try:
        with pytest.raises(LorbError, match="observations"):
            BAPlanDev(ctx, ab, len(bad["pose_init"]), len(bad["fixed_pose"]), bad["intr"])
        plan = BAPlanDev(ctx, ag, len(good["pose_init"]), len(good["fixed_pose"]), good["intr"])
        first = solved(plan)
        with pytest.raises(LorbError, match="observations"):
            plan.update(ab)
        plan.update(ag)
        again = solved(plan)
        o = O.ba_local_traced(good, A.LMOptions.default())
        against_oracle(first, o, "before the refused build")
        against_oracle(again, o, "after the refused build")
        same_bits(first, again, "after the refused build")
    finally:
        if plan is not None:
            plan.close()
        free_all(ag, ab)


def test_host_plan_limits(ctx):
    """a host-built plan takes a point with exactly kGB = 256 observations (all 128 cameras: 127 apart in the
    plan's order, the dense graph leaves nothing to renumber) and refuses 257; a point seen by cameras 0
    and 127 of a 128-camera window (the renumbering brings them together) solves too"""
    for w in (E.host_limit(256)[0], E.host_span_127()[0]):
        Po, Xo, so, ot = O.ba_local_traced(w, A.LMOptions.default())
        Pg, Xg, sg, gt = plan_traced(ctx, w, A.LMOptions.default())
        assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"], (sg, so)
        assert lm_match(sg, so, gt=gt, ot=ot, label="host limit") is None
        assert close(Pg, Po), np.abs(Pg - Po).max()
        assert close(Xg, Xo), np.abs(Xg - Xo).max()
    with pytest.raises(LorbError, match="observations"):
        BAPlan(ctx, [E.host_limit(257)[0]])


@pytest.mark.parametrize("name", list(E.DUPS))
def test_duplicate_in_a_long_run(ctx, name):
    """sorted path: an optimised camera twice inside a 72-observation run is "twice"; the plan then solves
    the clean window.  The run's first thread compares the run's frames, read from global memory, so the
    one distinction in the code is whether a copy lies within the 16 observations held in registers
    (two_waves, two_blocks: the first copy does) or both lie past them (beyond_16); the wave and the
    256-slot block of the second copy place the reads, not the branch."""
    clean, dup = E.dup_case(name)
    ac, ad = _same_capacity(ctx, [clean, dup])
    plan = None
    try:
        with pytest.raises(LorbError, match="twice"):
            BAPlanDev(ctx, ad, len(dup["pose_init"]), len(dup["fixed_pose"]), dup["intr"])
        plan = BAPlanDev(ctx, ac, len(clean["pose_init"]), len(clean["fixed_pose"]), clean["intr"])
        with pytest.raises(LorbError, match="twice"):
            plan.update(ad)
        plan.update(ac)
        against_oracle(solved(plan), O.ba_local_traced(clean, A.LMOptions.default()), f"after {name}")
    finally:
        if plan is not None:
            plan.close()
        free_all(ac, ad)


@pytest.mark.parametrize("holes", [0, 50])
def test_error_bits(ctx, holes):
    """db_land's messages: a point index >= n_points, a frame index >= n_poses, live counts above the
    capacities, negative counts.  Every one is found on the host in the build's readback, before any solve
    kernel runs; the counts are clamped to the capacities and a bad index is never used as one.  Each error
    gets a plan of its own: built from the good arrays, rebuilt with the bad ones (the message), rebuilt
    with the good ones, solved: the oracle's solution and the first build's bits.

    holes = 50: unused slots among the live ones, so every build runs the general phase (k_db_keys).
    holes = 0: a sorted upload.  A plan leaves k_db_sorted for good at the first build that sets flag 16
    (slots out of order), hence the fresh plan per error, and the bad uploads are made to stay sorted: the
    bad point index is n_points itself in the last slot, and the n_obs overflow pads the spare slots, which
    the clamped count makes live, with the last point.  By k_db_sorted's code these errors, and the good
    rebuild after them (from a scratch left dirty), then stay on k_db_sorted: point index, frame index,
    n_obs and n_points above the capacity, n_obs = -1.  n_points = -1 cannot: clamped to 0 points, every slot
    lies past the last point, so k_db_sorted (its clamp, its flag 8) also sets flag 16 and the message
    comes from the general phase run after it, as does the rebuild.  Which phase a build ran is not
    reported by the plan; the above is read from the code."""
    w, _ = E.case("idle_and_split")
    K, P, C = len(w["obs_point"]), len(w["point_init"]), len(w["pose_init"])
    k = K - 1 if holes == 0 else K // 2
    bad_point = dict(w, obs_point=np.where(np.arange(K) == k, P + (0 if holes == 0 else 3), w["obs_point"]).astype(np.int32))
    kf = int(np.flatnonzero(w["obs_frame"] >= 0)[len(w["obs_frame"]) // 3])
    bad_frame = dict(w, obs_frame=np.where(np.arange(K) == kf, C, w["obs_frame"]).astype(np.int32))
    good, a_pt, a_fr = _same_capacity(ctx, [w, bad_point, bad_frame], holes=holes)
    cap_obs, cap_pts = good["obs_point"].shape[0], good["point_init"].shape[0]
    one = lambda v: ctx.to_device(np.array([v], np.int32))
    live = int(good["n_obs"].numpy()[0])
    op = good["obs_point"].numpy()
    assert live == K + holes and np.all(op[live:] == 0)
    op[live:] = P - 1  # the spare slots continue the last point's run
    over = dict(good, n_obs=one(cap_obs + 1), obs_point=ctx.to_device(op))
    counts = [over, dict(good, n_points=one(cap_pts + 1)), dict(good, n_obs=one(-1)), dict(good, n_points=one(-1))]
    o = oracle_of("idle_and_split")
    plan = None
    try:
        for arrays, msg in [(a_pt, "point index"), (a_fr, "frame index")] + [(c, "count") for c in counts]:
            plan = BAPlanDev(ctx, good, C, len(w["fixed_pose"]), w["intr"])
            first = solved(plan)
            with pytest.raises(LorbError, match=msg):
                plan.update(arrays)
            plan.update(good)
            r = solved(plan)
            against_oracle(r, o, f"after '{msg}'")
            same_bits(first, r, f"after '{msg}'")
            assert r["info"] == first["info"], (msg, r["info"], first["info"])
            plan.close()
            plan = None
    finally:
        if plan is not None:
            plan.close()
        free_all(good, a_pt, a_fr, *counts)
