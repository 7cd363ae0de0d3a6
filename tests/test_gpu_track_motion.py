"""GPU parity of the device-resident motion-tracking chain (VisualOdometry::EstimatePoseMotion):
the device-pointer a4 and a12, and lorb_track_motion / lorb_track_motion_dev, against the oracle's
calls composed in Python -- a4 at 15, the <= 20 rule, a4 at 30 over emptied slots, the residual list
in slot order, a12.  Match codes and counts must be bit-equal; poses within the project's 1e-5."""
import functools

import numpy as np
import pytest

import oracle as O
import lorb_slam_amd.window  # noqa: F401  (binds Context methods)
from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-5
AA, T0 = [0.01, -0.005, 0.002], [0.05, 0.0, 0.02]  # synth.two_frames' current pose
UNCHANGED, NULL = A.LORB_ASSIGN_UNCHANGED, A.LORB_ASSIGN_NULL


def close(a, b, rtol=RTOL):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


def summaries_agree(a, b):
    assert a["termination"] == b["termination"] and a["iterations"] == b["iterations"], (a, b)
    assert a["successful_steps"] == b["successful_steps"], (a, b)
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-6 * b["final_cost"], (a, b)


def prediction(dx):
    """(pose_init, cur_Tcw) of the motion model's prediction, shifted by dx along x."""
    pi = np.array(AA + [T0[0] + dx, T0[1], T0[2]], np.float32)
    return pi, synth.Tcw_from(AA, [T0[0] + dx, T0[1], T0[2]])


def expected(s, dx, slot_state, slot_pos, kps=None, th_first=15.0, th_retry=30.0, min_matches=20):
    """The reference's three calls composed from the oracle."""
    fp, last = s["fp"], s["last"]
    kps = kps or s["cur_kps"]
    pi, T = prediction(dx)
    n = len(kps["x"])
    ss = np.zeros(n, np.uint8) if slot_state is None else slot_state
    a1, n1 = O.search_by_projection_frame(fp, T, kps, ss, last, th_first)
    if n1 <= min_matches:
        a, n2 = O.search_by_projection_frame(fp, T, kps, np.zeros(n, np.uint8), last, th_retry)
        pass_ = 2 if n2 > min_matches else 0
        has = a >= 0
    else:
        a, n2, pass_ = a1, -1, 1
        has = (a >= 0) | ((a == UNCHANGED) & (ss != A.LORB_SLOT_EMPTY))
    idx = np.nonzero(has)[0]
    pts = np.zeros((len(idx), 3), np.float32)
    m = a[idx] >= 0
    pts[m] = last["mp_pos"][a[idx][m]]
    if (~m).any():
        pts[~m] = slot_pos[idx[~m]]
    obs = np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(np.float32)
    e = dict(assign=a, pass_=pass_, nmatches_first=n1, nmatches_retry=n2, n_residuals=len(idx), first=a1)
    if pass_:
        pb = dict(res_off=np.array([0, len(idx)], np.int32),
                  intr=np.array([[fp["fx"], fp["fx"], fp["cx"], fp["cy"]]], np.float32),  # the PoseCost quirk
                  pose_init=pi[None], pts3d=pts, obs2d=obs)
        po, To, so = O.ba_pose_only(pb)
        e.update(pose=po[0], Tcw=To[0], summary=so[0])
    else:
        e.update(pose=pi.astype(np.float64), Tcw=O.pose_to_Tcw(pi[:3], pi[3:]),
                 summary=A.BASummary().as_dict())
    return e


def check(r, e):
    assert np.array_equal(r["assign"], e["assign"])
    assert (r["pass_"], r["nmatches_first"], r["nmatches_retry"], r["n_residuals"]) == \
        (e["pass_"], e["nmatches_first"], e["nmatches_retry"], e["n_residuals"])
    if e["pass_"] == 0:
        assert np.array_equal(r["pose"], e["pose"])  # pose_init widened, bit for bit
        assert r["summary"] == A.BASummary().as_dict()
    assert close(r["pose"], e["pose"]), np.abs(r["pose"] - e["pose"]).max()
    summaries_agree(r["summary"], e["summary"])
    assert np.allclose(r["Tcw"], e["Tcw"], rtol=1e-5, atol=1e-6)


@functools.lru_cache(maxsize=None)
def frames(n_kps, n_shared, seed, locked_frac=0.5, prefilled=0):
    return synth.two_frames(seed=seed, n_kps=n_kps, n_shared=n_shared, locked_frac=locked_frac, prefilled=prefilled)


def run(ctx, s, dx, slot_state, slot_pos, kps=None, **kw):
    pi, T = prediction(dx)
    return ctx.track_motion(s["fp"], T, pi, kps or s["cur_kps"], slot_state, slot_pos, s["last"], **kw)


# 1 -- the device-pointer a4 -------------------------------------------------------------------
@pytest.mark.parametrize("seed,th,prefilled,locked", [(1, 15.0, 0, 0.5), (2, 30.0, 0, 1.0), (3, 15.0, 60, 0.3),
                                                       (4, 5.0, 20, 0.0)])
def test_search_by_projection_frame_dev(ctx, seed, th, prefilled, locked):
    s = synth.two_frames(seed=seed, n_kps=500, n_shared=200, locked_frac=locked, prefilled=prefilled)
    a_g, n_g = ctx.search_by_projection_frame_dev(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], th)
    a_o, n_o = O.search_by_projection_frame(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], th)
    assert n_g == n_o
    assert np.array_equal(a_g, a_o)


def test_search_by_projection_frame_dev_octave_out_of_range(ctx):
    """A last-frame point with an octave outside [0, n_levels) is inactive: the same as the point
    having no map point."""
    s = frames(500, 200, 1)
    idx = np.nonzero(s["last"]["has_mp"])[0][::7]
    bad = dict(s["last"], octave=s["last"]["octave"].copy())
    bad["octave"][idx[::2]] = s["fp"]["n_levels"]
    bad["octave"][idx[1::2]] = -1
    off = dict(s["last"], has_mp=s["last"]["has_mp"].copy())
    off["has_mp"][idx] = 0
    a_g, n_g = ctx.search_by_projection_frame_dev(s["fp"], s["cur_Tcw"], s["cur_kps"], None, bad, 15.0)
    a_o, n_o = O.search_by_projection_frame(s["fp"], s["cur_Tcw"], s["cur_kps"], np.zeros(500, np.uint8), off, 15.0)
    assert n_g == n_o and np.array_equal(a_g, a_o)


# 2 -- the device-pointer a12 ------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_frames,n_res", [(1, 3, 200), (4, 2, 1500)])  # 1500: past the register-resident 512
def test_ba_pose_only_dev(ctx, seed, n_frames, n_res):
    pb = synth.pose_only_batch(seed=seed, n_frames=n_frames, n_res=n_res)
    pg, sg = ctx.ba_pose_only_dev(pb)
    po, _, so = O.ba_pose_only(pb)
    assert close(pg, po), np.abs(pg - po).max()
    for a, b in zip(sg, so):
        summaries_agree(a, b)


def test_ba_pose_only_dev_empty_frame(ctx):
    pb = synth.pose_only_batch(seed=1, n_frames=1, n_res=8)
    empty = dict(res_off=np.array([0, 0], np.int32), intr=pb["intr"], pose_init=pb["pose_init"],
                 pts3d=np.zeros((0, 3), np.float32), obs2d=np.zeros((0, 2), np.float32))
    pg, sg = ctx.ba_pose_only_dev(empty)
    assert np.array_equal(pg[0], pb["pose_init"][0].astype(np.float64))
    assert sg[0] == A.BASummary().as_dict()


# 3 -- the chain -------------------------------------------------------------------------------
CHAIN = [  # n_kps, n_shared, seed, dx, the oracle's nmatches at 15, at 30 (-1: no retry), pass
    (500, 200, 1, 0.0, 146, -1, 1),
    (300, 120, 2, 0.5, 24, -1, 1),   # just above the rule
    (300, 120, 1, 0.5, 20, 61, 2),   # the boundary: <= 20 retries
    (500, 200, 1, 0.7, 13, 69, 2),
    (500, 200, 1, 1.0, 4, 30, 2),    # one rotation NULL in the retry
    (500, 200, 1, 1.5, 1, 14, 0),
    (500, 200, 1, 3.0, 0, 0, 0),     # no residual at all
]


@pytest.mark.parametrize("n_kps,n_shared,seed,dx,n15,n30,pass_", CHAIN)
def test_track_motion(ctx, n_kps, n_shared, seed, dx, n15, n30, pass_):
    s = frames(n_kps, n_shared, seed)
    if dx == 0.0:
        assert np.array_equal(prediction(0.0)[1], s["cur_Tcw"])
    e = expected(s, dx, None, None)
    assert (e["nmatches_first"], e["nmatches_retry"], e["pass_"]) == (n15, n30, pass_)  # synth drift
    if dx == 1.0:
        assert (e["assign"] == NULL).sum() == 1
    if dx == 3.0:
        assert e["n_residuals"] == 0
    check(run(ctx, s, dx, None, None), e)


# 4 -- rotation null-out and pre-filled slots ----------------------------------------------------
def rotated(s, n=12):
    """180 degrees on the current-frame angle of the first n slots the oracle matches at th 15."""
    a, _ = O.search_by_projection_frame(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], 15.0)
    j = np.nonzero(a >= 0)[0][:n]
    ang = s["cur_kps"]["angle"].copy()
    ang[j] = np.mod(ang[j] + np.float32(180), np.float32(360)).astype(np.float32)
    return dict(s["cur_kps"], angle=ang)


@pytest.mark.parametrize("seed,prefilled,n_after", [(1, 0, 134), (3, 60, 122)])
def test_track_motion_rotation_and_prefilled(ctx, seed, prefilled, n_after):
    s = frames(500, 200, seed, 0.5, prefilled)
    kps = rotated(s)
    ss = s["slot_state"]
    slot_pos = np.random.default_rng(seed).uniform(-4, 4, (500, 3)).astype(np.float32)
    slot_pos[:, 2] = np.abs(slot_pos[:, 2]) + 2
    e = expected(s, 0.0, ss, slot_pos, kps)
    a = e["assign"]
    assert e["pass_"] == 1 and e["nmatches_first"] == n_after
    assert (a == NULL).sum() >= 5
    if prefilled:
        assert ((a == UNCHANGED) & (ss != 0)).sum() >= 1 and ((a >= 0) & (ss != 0)).sum() >= 1
        assert e["n_residuals"] > (a >= 0).sum()  # the kept slots' points are residuals too
    check(run(ctx, s, 0.0, ss, slot_pos, kps), e)
    if prefilled:  # the retry ignores every pre-filled slot
        e = expected(s, 0.7, ss, slot_pos, kps)
        assert e["pass_"] == 2 and e["n_residuals"] == (e["assign"] >= 0).sum()
        check(run(ctx, s, 0.7, ss, slot_pos, kps), e)


# 5 -- large: the count / scan / write candidate path, more than 512 residuals --------------------
def test_track_motion_large(ctx):
    s = frames(2000, 1200, 9, 0.7, 100)
    ss = s["slot_state"]
    slot_pos = np.random.default_rng(9).uniform(-4, 4, (2000, 3)).astype(np.float32)
    slot_pos[:, 2] = np.abs(slot_pos[:, 2]) + 2
    e = expected(s, 0.0, ss, slot_pos)
    assert e["nmatches_first"] == 886 and (e["assign"] >= 0).sum() == 885 and (e["assign"] == NULL).sum() == 2
    assert e["n_residuals"] > 512
    check(run(ctx, s, 0.0, ss, slot_pos), e)
    e = expected(s, 1.2, None, None)
    assert (e["nmatches_first"], e["nmatches_retry"], e["pass_"]) == (10, 156, 2)
    check(run(ctx, s, 1.2, None, None), e)


# 6 -- edges -----------------------------------------------------------------------------------
def cut(d, n):
    return {k: (v if k == "Tcw" else v[:n]) for k, v in d.items()}


@pytest.mark.parametrize("device_resident", [True, False])
@pytest.mark.parametrize("edge", ["n_cur=0", "n_last=0", "no map point", "n_cur=1"])
def test_track_motion_edges(ctx, edge, device_resident):
    s = frames(500, 200, 1)
    s = dict(s)
    if edge == "n_cur=0":
        s["cur_kps"] = cut(s["cur_kps"], 0)
    elif edge == "n_cur=1":
        s["cur_kps"] = cut(s["cur_kps"], 1)
    elif edge == "n_last=0":
        s["last"] = cut(s["last"], 0)
    else:
        s["last"] = dict(s["last"], has_mp=np.zeros(500, np.uint8))
    r = run(ctx, s, 0.0, None, None, device_resident=device_resident)
    n = len(s["cur_kps"]["x"])
    if edge == "n_cur=1":  # the one keypoint may well match: whatever the oracle says
        check(r, expected(s, 0.0, None, None))
        return
    pi = prediction(0.0)[0]
    assert r["pass_"] == 0 and r["nmatches_first"] == 0 and r["nmatches_retry"] == 0 and r["n_residuals"] == 0
    assert len(r["assign"]) == n and np.all(r["assign"] == UNCHANGED)
    assert np.array_equal(r["pose"], pi.astype(np.float64))
    assert r["summary"] == A.BASummary().as_dict()


# 7 -- the host-array form and the device form agree ----------------------------------------------
@pytest.mark.parametrize("n_kps,n_shared,seed,dx", [(500, 200, 1, 0.0), (300, 120, 1, 0.5)])
def test_track_motion_host_form_identical(ctx, n_kps, n_shared, seed, dx):
    s = frames(n_kps, n_shared, seed)
    d = run(ctx, s, dx, None, None, device_resident=True)
    h = run(ctx, s, dx, None, None, device_resident=False)
    assert np.array_equal(d["assign"], h["assign"])
    for k in ("pass_", "nmatches_first", "nmatches_retry", "n_residuals", "summary"):
        assert d[k] == h[k], k
    assert np.array_equal(d["pose"], h["pose"]) and np.array_equal(d["Tcw"], h["Tcw"])
    check(h, expected(s, dx, None, None))


# 8 -- the context's all-EMPTY slot states survive an extractor call --------------------------------
def orb_count_with_locked_byte(c):
    """An orb_detect call whose level-0 keypoint count (512 .. 767) has LORB_SLOT_LOCKED as its second
    byte.  Returns the keypoint indices such a byte would land on if the extractor's per-level counts
    (int l at bytes 4 l ..) were written over slot states."""
    nd = np.array(O.orb_features_per_level(1000))
    nd[0] = 600
    g = c.orb_detect(synth.orb_problem(seed=61, n_kps=1)["pyr"], nd, synth.scale_factors())
    counts = np.diff(g["level_off"])
    hit = [4 * l + b for l, n in enumerate(counts) for b in (0, 1) if (int(n) >> (8 * b)) & 255 == A.LORB_SLOT_LOCKED]
    assert hit, counts
    return hit


@pytest.mark.parametrize("chain", ["motion", "local"])
def test_empty_slot_states_survive_orb(chain):
    """slot_state=None reads a zeroed buffer the context keeps from call to call: an extractor call in
    between must not write it.  A context of its own: nothing an earlier test left can hide a fault."""
    import test_gpu_track_local as TL
    from lorb_slam_amd.runtime import Context
    if chain == "motion":
        s = frames(500, 200, 2)
        e = expected(s, 0.0, None, None)
        go = lambda c: check(run(c, s, 0.0, None, None), e)
    else:
        s = dict(TL.problem(40, 500, 2000, 300), slot_state=None, slot_pos=None)
        e = TL.expected(s)
        go = lambda c: TL.check(TL.run(c, s), e)
    c = Context(0)
    try:
        go(c)
        hit = orb_count_with_locked_byte(c)
        assert any(e["assign"][j] >= 0 for j in hit), (hit, e["assign"][:32])  # a match a LOCKED byte there would remove
        go(c)
    finally:
        c.close()
