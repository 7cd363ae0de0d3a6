"""GPU parity of the device-resident local-map tracking chain (VisualOdometry::EstimatePoseLocal
after UpdateLocalMap): lorb_track_local / lorb_track_local_dev against the oracle's calls composed
in Python -- a8 + a5 (O.track_local_map), the <= 20 gate, the residual list in slot order, a12.
Fields, codes and counts must be bit-equal; poses within the project's 1e-5."""
import functools

import numpy as np
import pytest

import oracle as O
import lorb_slam_amd.window  # noqa: F401  (binds Context methods)
from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth
from lorb_slam_amd.runtime import LorbError

pytestmark = pytest.mark.gpu
RTOL = 1e-5
AA, T0 = [0.01, -0.02, 0.005], [0.1, -0.05, 0.2]  # synth.local_map_problem's pose
UNCHANGED = A.LORB_ASSIGN_UNCHANGED
FIELDS = ("proj_x", "proj_y", "proj_xr", "view_cos")
COUNTS = ("ok", "nmatches", "n_in_view", "n_residuals")


def close(a, b, rtol=RTOL):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


def summaries_agree(a, b):
    assert a["termination"] == b["termination"] and a["iterations"] == b["iterations"], (a, b)
    assert a["successful_steps"] == b["successful_steps"], (a, b)
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-6 * b["final_cost"], (a, b)


def prediction(dx):
    """(pose_init, Tcw) of the pose stage 1 left, shifted by dx along x."""
    pi = np.array(AA + [T0[0] + dx, T0[1], T0[2]], np.float32)
    return pi, synth.Tcw_from(AA, [T0[0] + dx, T0[1], T0[2]])


def slot_positions(s, seed):
    """The map point each slot would hold: keypoint j back-projected at a depth of its own under the
    problem's own pose, so that the kept slots are consistent with the scene."""
    fp, k, T = s["fp"], s["kps"], s["Tcw"].astype(np.float64)
    z = np.random.default_rng(seed + 100).uniform(2, 12, len(k["x"]))
    Xc = np.stack([(k["x"] - fp["cx"]) / fp["fx"] * z, (k["y"] - fp["cy"]) / fp["fy"] * z, z], 1)
    return ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)  # world = R^T (Xc - t)


@functools.lru_cache(maxsize=None)
def problem(seed, n_kps, n_pts, n_true):
    s = synth.local_map_problem(seed=seed, n_kps=n_kps, n_pts=n_pts, n_true=n_true)
    s["slot_pos"] = slot_positions(s, seed)
    return s


def expected(s, dx=0.0, th=1.0, min_matches=20):
    """The reference's sequence composed from the oracle."""
    fp, kps, pts = s["fp"], s["kps"], s["pts"]
    pi, T = prediction(dx)
    n = len(kps["x"])
    ss = np.zeros(n, np.uint8) if s["slot_state"] is None else s["slot_state"]
    fr, a, nm = O.track_local_map(fp, T, kps, ss, pts, 0.5, th)
    has = (a >= 0) | ((a == UNCHANGED) & (ss != A.LORB_SLOT_EMPTY))
    idx = np.nonzero(has)[0]
    X = np.zeros((len(idx), 3), np.float32)
    m = a[idx] >= 0
    X[m] = pts["pos"][a[idx][m]]
    if (~m).any():
        X[~m] = s["slot_pos"][idx[~m]]
    obs = np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(np.float32).reshape(-1, 2)
    e = dict(fr, assign=a, ok=int(nm > min_matches), nmatches=nm, n_in_view=int(fr["in_view"].sum()),
             n_residuals=len(idx))
    if e["ok"]:
        pb = dict(res_off=np.array([0, len(idx)], np.int32),
                  intr=np.array([[fp["fx"], fp["fx"], fp["cx"], fp["cy"]]], np.float32),  # the PoseCost quirk
                  pose_init=pi[None], pts3d=X, obs2d=obs)
        po, To, so = O.ba_pose_only(pb)
        e.update(pose=po[0], Tcw=To[0], summary=so[0])
    else:
        e.update(pose=pi.astype(np.float64), Tcw=O.pose_to_Tcw(pi[:3], pi[3:]), summary=A.BASummary().as_dict())
    return e


def check(r, e):
    assert np.array_equal(r["assign"], e["assign"])
    assert np.array_equal(r["in_view"], e["in_view"])
    iv = e["in_view"].astype(bool)
    for k in FIELDS + ("pred_level",):
        assert np.array_equal(r[k][iv], e[k][iv]), k
    assert tuple(r[k] for k in COUNTS) == tuple(e[k] for k in COUNTS)
    if not e["ok"]:
        assert np.array_equal(r["pose"], e["pose"])  # pose_init widened, bit for bit
        assert r["summary"] == A.BASummary().as_dict()
    assert close(r["pose"], e["pose"]), np.abs(r["pose"] - e["pose"]).max()
    summaries_agree(r["summary"], e["summary"])
    assert np.allclose(r["Tcw"], e["Tcw"], rtol=1e-5, atol=1e-6)


def run(ctx, s, dx=0.0, **kw):
    pi, T = prediction(dx)
    return ctx.track_local(s["fp"], T, pi, s["kps"], s["slot_state"], s["slot_pos"], s["pts"], **kw)


def identical(d, h):
    for k in ("assign", "in_view", "pose", "Tcw"):
        assert np.array_equal(d[k], h[k]), k
    iv = d["in_view"].astype(bool)
    for k in FIELDS + ("pred_level",):
        assert np.array_equal(d[k][iv], h[k][iv]), k
    for k in COUNTS + ("summary",):
        assert d[k] == h[k], k


# 1 -- the chain -------------------------------------------------------------------------------
CHAIN = [  # seed, n_kps, n_pts, n_true, dx, th, then the oracle's nm, n_in_view (or None), n_residuals, iterations
    (31, 500, 2000, 300, 0.0, 1.0, 186, 1180, 258, 2),    # live size: LDS grid + strided
    (31, 500, 2000, 300, 0.05, 1.0, 152, None, 229, None),  # the LM does real work
    (33, 300, 400, 57, 0.0, 1.0, 20, None, None, 0),       # the gate's boundary: fails
    (33, 300, 400, 58, 0.0, 1.0, 21, None, None, None),    # and passes
    (32, 300, 400, 100, 0.3, 1.0, 0, None, 100, 0),        # nothing matches: the kept slots stay unoptimised
    (32, 300, 400, 100, 0.3, 3.0, 25, None, 117, 3),       # a wider radius
    (11, 2000, 3000, 1200, 0.0, 1.0, 774, 1761, 855, None),  # past 512 residuals and past kCandStrided
    (34, 1024, 1024, 400, 0.0, 1.0, 240, None, 329, None),  # the last size with the grid in LDS, np nk = kCandStrided
    (35, 1100, 1000, 400, 0.0, 1.0, 236, None, 326, None),  # past both: grid launch, count / scan / write
    (35, 1100, 900, 400, 0.0, 1.0, 245, None, 334, None),   # a grid launch with the strided pass
]


@pytest.mark.parametrize("seed,n_kps,n_pts,n_true,dx,th,nm,n_in_view,n_res,iters", CHAIN)
def test_track_local(ctx, seed, n_kps, n_pts, n_true, dx, th, nm, n_in_view, n_res, iters):
    s = problem(seed, n_kps, n_pts, n_true)
    e = expected(s, dx, th)
    assert e["nmatches"] == nm and e["ok"] == int(nm > 20)  # synth drift
    for want, got in ((n_in_view, e["n_in_view"]), (n_res, e["n_residuals"]), (iters, e["summary"]["iterations"])):
        assert want is None or want == got, (want, got)
    if (seed, dx) == (31, 0.0):
        ss, a = s["slot_state"], e["assign"]
        assert ((a == UNCHANGED) & (ss != 0)).sum() == 72 and ((a >= 0) & (ss != 0)).sum() == 28
    if (seed, dx) == (31, 0.05):
        assert e["summary"]["initial_cost"] > 10 * e["summary"]["final_cost"]
    if nm == 0:
        assert np.all(e["assign"] == UNCHANGED)
    check(run(ctx, s, dx, th=th), e)


# 2 -- two unlocked points on one slot ------------------------------------------------------------
def test_track_local_two_points_one_slot(ctx):
    s = problem(31, 500, 2000, 300)
    a0 = expected(s)["assign"]
    first = list(dict.fromkeys(a0[a0 >= 0].tolist()))[:12]
    pts = {k: np.concatenate([v, v[first]]) for k, v in s["pts"].items()}
    both = np.array(first + list(range(2000, 2012)))
    pts["locked"][both] = 0
    pts["in_frame"][both] = 0
    s2 = dict(s, pts=pts)
    e = expected(s2)
    a = e["assign"]
    assert e["nmatches"] == 198 and (a >= 0).sum() == 186 and (a >= 2000).sum() == 12
    r = run(ctx, s2)
    check(r, e)
    assert r["nmatches"] - (r["assign"] >= 0).sum() == 12
    ss = s["slot_state"]
    assert r["n_residuals"] == ((r["assign"] >= 0) | ((r["assign"] == UNCHANGED) & (ss != 0))).sum()


# 3 -- edges, in both forms ----------------------------------------------------------------------
def cut(d, n):
    return {k: v[:n] for k, v in d.items()}


@pytest.mark.parametrize("device_resident", [True, False])
@pytest.mark.parametrize("edge", ["n_kps=0", "n_pts=0", "all in frame", "no slots", "no flags"])
def test_track_local_edges(ctx, edge, device_resident):
    s = dict(problem(33, 300, 400, 58))
    if edge == "n_kps=0":
        s.update(kps=cut(s["kps"], 0), slot_state=s["slot_state"][:0], slot_pos=s["slot_pos"][:0])
    elif edge == "n_pts=0":
        s["pts"] = cut(s["pts"], 0)
    elif edge == "all in frame":
        s["pts"] = dict(s["pts"], in_frame=np.ones(400, np.uint8))
    elif edge == "no slots":
        s.update(slot_state=None, slot_pos=None)
    else:
        s["pts"] = dict(s["pts"], is_bad=None, in_frame=None)
    e = expected(s)
    r = run(ctx, s, device_resident=device_resident)
    check(r, e)
    pi = prediction(0.0)[0]
    if edge == "n_kps=0":  # the fields are still computed, nothing is matched
        assert r["n_in_view"] > 100 and (r["nmatches"], r["n_residuals"], len(r["assign"])) == (0, 0, 0)
    if edge == "all in frame":
        assert (r["n_in_view"], r["nmatches"], r["ok"]) == (0, 0, 0)
    if edge in ("no slots", "no flags"):
        assert r["ok"] == 1
        if edge == "no slots":
            assert r["n_residuals"] == (r["assign"] >= 0).sum()
    else:  # the gate fails: the start pose comes back untouched
        assert r["ok"] == 0 and np.array_equal(r["pose"], pi.astype(np.float64))
        assert r["summary"] == A.BASummary().as_dict()


# 4 -- forms and regressions ----------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_kps,n_pts,n_true,dx", [(31, 500, 2000, 300, 0.05), (11, 2000, 3000, 1200, 0.0)])
def test_track_local_host_form_identical(ctx, seed, n_kps, n_pts, n_true, dx):
    s = problem(seed, n_kps, n_pts, n_true)
    d = run(ctx, s, dx, device_resident=True)
    h = run(ctx, s, dx, device_resident=False)
    identical(d, h)
    check(h, expected(s, dx))


@pytest.mark.parametrize("seed,n_kps,n_pts,n_true", [(31, 500, 2000, 300), (35, 1100, 1000, 400)])
def test_track_local_fields_equal_track_local_map(ctx, seed, n_kps, n_pts, n_true):
    """The frustum test fused into the candidate kernel moves no bit of k_frustum's fields."""
    s = problem(seed, n_kps, n_pts, n_true)
    r = run(ctx, s)
    m = ctx.track_local_map(s["fp"], s["Tcw"], s["kps"], s["slot_state"], s["pts"])
    assert np.array_equal(prediction(0.0)[1], s["Tcw"])
    assert np.array_equal(r["in_view"], m["in_view"]) and np.array_equal(r["assign"], m["assign"])
    assert r["nmatches"] == m["nmatches"]
    iv = m["in_view"].astype(bool)
    for k in FIELDS + ("pred_level",):
        assert np.array_equal(r[k][iv], m[k][iv]), k


@pytest.mark.parametrize("device_resident", [True, False])
def test_track_local_invalid_arguments(ctx, device_resident):
    s = problem(33, 300, 400, 58)
    pi, T = prediction(0.0)
    with pytest.raises(LorbError, match=r"rc=-1: min_matches"):  # LORB_E_INVALID
        run(ctx, s, min_matches=-1, device_resident=device_resident)
    with pytest.raises(LorbError, match=r"rc=-1: null array"):
        ctx.track_local(s["fp"], T, pi, s["kps"], s["slot_state"], None, s["pts"], device_resident=device_resident)
