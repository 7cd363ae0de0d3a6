"""Stores with geometry for the local bundle adjustment on the keyframe store: the hand case with its answer written
out (tests/test_kf_ba_ref.py checks the restatement tests/kf_ba_ref.py against it on the CPU), generated stores at
the sizes where the gather's kernels change path, and the solve scene.  tests/test_gpu_kf_ba.py checks the device
against the restatement on all of them.

A case is dict(store, geom, kf) (+ want for the hand case); store as tests/kf_store_cases.py builds it."""
import numpy as np

import kf_store_cases as KC
import kf_store_ref as R
from lorb_slam_amd import synth

F = np.float32


def geometry_for(store, seed=0):
    """A geometry that keeps the invariant: every observation (p, f) names the LOWEST slot of f that holds p; a
    keyframe that observes p without holding it gets a slot appended.  Poses and keypoints are random."""
    rng = np.random.default_rng(6000 + seed)
    slots = [list(r) for r in store["kf_slots"]]
    obs_slot = []
    for p, obs in enumerate(store["obs"]):
        row = []
        for f in obs:
            if p not in slots[f]:
                slots[f].append(p)
            row.append(slots[f].index(p))
        obs_slot.append(row)
    store["kf_slots"] = slots
    nk = len(slots)
    return dict(kf_pose=list((rng.normal(size=(nk, 6)) * 0.1).astype(F)),
                kf_slot_uv=[rng.uniform(0, 700, (len(r), 2)).astype(F) for r in slots], obs_slot=obs_slot)


def hand_case():
    """Six keyframes, kf 2 bad, K = 5, cov[5] = [3, 2, 1].  row5 = [7, -1, 4, 7, 9] with point 9 bad, row3 = [4, 2, 7],
    row1 = [0, 2]; kf 0 holds p7, kf 2 and kf 4 hold p4.  Observations: p7 {0, 3, 5}, p4 {2, 3, 4, 5}, p2 {1, 3},
    p0 {1}, p9 {5}.
      frames   local = [5, 3, 1] (kf 2 is bad: skipped and counted)
      points   row5 gives 7, 4 (slot 3 holds 7 again, 9 is bad), row3 gives 2, row1 gives 0: l2g = [7, 4, 2, 0]
      obs      p7: kf0 fixed 0 -> -1, kf3 -> 1, kf5 -> 0;  p4: kf2 bad (skipped), kf3 -> 1, kf4 fixed 1 -> -2, kf5 -> 0;
               p2: kf1 -> 2, kf3 -> 1;  p0: kf1 -> 2.  fixed = [0, 4].
      uv       slot j of keyframe f is (100 f + j, 100 f + j + 0.5): p7 in K comes from slot 0, not slot 3."""
    rows = [[7], [0, 2], [4], [4, 2, 7], [4], [7, -1, 4, 7, 9]]
    obs = [[] for _ in range(10)]
    obs[7], obs[4], obs[2], obs[0], obs[9] = [0, 3, 5], [2, 3, 4, 5], [1, 3], [1], [5]
    is_bad = np.zeros(10, np.uint8)
    is_bad[9] = 1
    cov = [[], [3], [], [1, 5], [], [3, 2, 1]]
    store = KC.make_store(obs, [0, 0, 1, 0, 0, 0], rows, cov, [{} for _ in rows], is_bad=is_bad, seed=50)
    slot = {(7, 0): 0, (7, 3): 2, (7, 5): 0, (4, 2): 0, (4, 3): 0, (4, 4): 0, (4, 5): 2, (2, 1): 1, (2, 3): 1, (0, 1): 0, (9, 5): 4}
    geom = dict(kf_pose=[np.full(6, 0.01 * (f + 1), F) * np.arange(1, 7, dtype=F) for f in range(6)],
                kf_slot_uv=[np.array([[100 * f + j, 100 * f + j + 0.5] for j in range(len(r))], F).reshape(-1, 2)
                            for f, r in enumerate(rows)],
                obs_slot=[[slot[(p, f)] for f in o] for p, o in enumerate(obs)])
    want = dict(local_kf=[5, 3, 1], l2g=[7, 4, 2, 0], fixed_kf=[0, 4], obs_point=[0, 0, 0, 1, 1, 1, 2, 2, 3],
                obs_frame=[-1, 1, 0, 1, -2, 0, 2, 1, 2],
                obs_uv=[[0, 0.5], [302, 302.5], [500, 500.5], [300, 300.5], [400, 400.5], [502, 502.5], [101, 101.5], [301, 301.5],
                        [100, 100.5]],
                rec=dict(status=0, kf=5, n_poses=3, n_fixed=2, n_points=4, n_obs=9, n_cov_bad=1, n_obs_bad_kf=1, n_obs_bad_slot=0,
                         written=0))
    return dict(store=store, geom=geom, kf=5, want=want)


def random_case(n_kf, n_points, seed, kf=None, **kw):
    """KC.random_store plus geometry; K's covisibility row is its weight map's keys in R.ordered's order, so that
    bad keyframes, repeated points and bad points all occur."""
    s = KC.random_store(n_kf, n_points, seed, **kw)
    g = geometry_for(s, seed)
    kf = n_kf - 1 if kf is None else kf
    s["cov"][kf] = R.ordered(s["conn"][kf])
    return dict(store=s, geom=g, kf=kf)


def star_case(n_local, pts_per_kf, seed=0, n_obs_of_p0=1, n_fixed=0, row_len=None, extra=0, spare=False):
    """K = the last keyframe with n_local - 1 covisible keyframes before it, `pts_per_kf` points of its own per local
    frame; point 0 (held by K) is observed by n_obs_of_p0 keyframes in all; n_fixed further keyframes of one slot
    each observe one point of K each (fixed frames); `extra` further points are seen by K alone; row_len pads K's
    row with empty slots up to that length; `spare` appends a keyframe with one point of its own and no neighbour."""
    n_extra = max(n_obs_of_p0 - 1 - (n_local - 1), 0)           # observers of p0 beyond K and its local frames
    nk = n_local + n_extra + n_fixed
    K = nk - 1
    local = list(range(n_local - 1))
    rows, obs = [[] for _ in range(nk)], []
    for f in local + [K]:
        for _ in range(pts_per_kf):
            rows[f].append(len(obs))
            obs.append([f])
    for _ in range(extra):
        rows[K].append(len(obs))
        obs.append([K])
    p0 = rows[K][0]
    others = (local + list(range(n_local - 1, n_local - 1 + n_extra)))[:max(n_obs_of_p0 - 1, 0)]
    for f in others:
        rows[f].append(p0)
        obs[p0].append(f)
    for i in range(n_fixed):
        f = n_local - 1 + n_extra + i
        p = rows[K][i % pts_per_kf]
        if f not in obs[p]:
            rows[f].append(p)
            obs[p].append(f)
    obs = [sorted(o) for o in obs]
    if row_len:
        rows[K] = rows[K] + [-1] * (row_len - len(rows[K]))
    cov = [[] for _ in range(nk)]
    cov[K] = local
    if spare:
        rows.append([len(obs)])
        obs.append([nk])
        cov.append([])
        nk += 1
    s = KC.make_store(obs, [0] * nk, rows, cov, [{} for _ in range(nk)], seed=seed)
    return dict(store=s, geom=geometry_for(s, seed), kf=K)


def size_cases():
    """The sizes at which the gather takes another path (kT = 1024 positions per tile, 128 local frames, 256
    observations per point, 4096 keyframes per row)."""
    out = {}
    for n in (1023, 1024, 1025):                                 # one scan tile of window points and its neighbours
        out[f"points_{n}"] = star_case(3, 341, seed=n, extra=n - 1023)
    out["row_1025"] = star_case(2, 5, seed=11, row_len=1025)     # a keyframe row of 1025 slots
    for n in (64, 65, 128):
        out[f"local_{n}"] = star_case(n, 2, seed=n)
    out["obs_255"] = star_case(4, 2, seed=12, n_obs_of_p0=255)
    out["fixed_1025"] = star_case(2, 8, seed=13, n_fixed=1025)   # 1025 fixed keyframes, rows of one slot each
    return out


def status_cases():
    return dict(local_129=star_case(129, 1, seed=14, spare=True), obs_256=star_case(4, 2, seed=15, n_obs_of_p0=256, spare=True))


def solve_scene():
    """The store of the solve test, from synth.ba_window(seed=3, n_kf=6, n_pts=300, n_fixed=2, fixed_obs_per_kf=60,
    obs_lens=(3, 4)): the two fixed keyframes are store keyframes 0 and 1, window keyframe c is store keyframe 2 + c,
    K = 7 is the newest.  A fixed keyframe keeps at most two of its observations of points K sees, so it shares
    fewer than 3 points with K and stays out of K's covisibility row, which is R.ordered over K's shared-point
    counts of 3 or more.  40 further points are seen by K alone, as an insertion creates them."""
    w = synth.ba_window(seed=3, n_kf=6, n_pts=300, n_fixed=2, fixed_obs_per_kf=60, obs_lens=(3, 4))
    n_fixed, n_win, n_pts = len(w["fixed_pose"]), len(w["pose_init"]), len(w["point_init"])
    nk, K = n_fixed + n_win, n_fixed + n_win - 1
    kf_of = lambda fr: n_fixed + int(fr) if fr >= 0 else -1 - int(fr)   # noqa: E731
    seen_by_K = {int(p) for p, fr in zip(w["obs_point"], w["obs_frame"]) if kf_of(fr) == K}
    rows, uvs, obs, shared = [[] for _ in range(nk)], [[] for _ in range(nk)], [[] for _ in range(n_pts)], [0] * nk
    for p, fr, uv in zip(w["obs_point"], w["obs_frame"], w["obs_uv"]):
        f, p = kf_of(fr), int(p)
        if f < n_fixed and p in seen_by_K:
            if shared[f] == 2:
                continue
            shared[f] += 1
        rows[f].append(p)
        uvs[f].append(uv)
        obs[p].append(f)
    pos = [np.asarray(x, F) for x in w["point_init"]]
    rng = np.random.default_rng(9)
    fx, fy, cx, cy = (float(v) for v in w["intr"])
    aa, t = w["true_poses"][n_win - 1][:3], w["true_poses"][n_win - 1][3:]
    Rk = synth.rodrigues(aa)
    for _ in range(40):                                          # seen by K alone: its true projection + 0.5 px noise
        X = np.array([rng.uniform(-4, 6), rng.uniform(-2, 2), rng.uniform(5, 18)])
        pc = Rk @ X + t
        rows[K].append(len(obs))
        uvs[K].append(np.array([fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy], F) + rng.normal(0, 0.5, 2).astype(F))
        obs.append([K])
        pos.append(np.asarray(X + rng.normal(0, 5e-2, 3), F))
    obs = [sorted(o) for o in obs]
    weight = {}
    for p in rows[K]:
        for f in obs[p]:
            if f != K:
                weight[f] = weight.get(f, 0) + 1
    cov = [[] for _ in range(nk)]
    cov[K] = R.ordered({f: v for f, v in weight.items() if v >= 3})
    assert all(weight.get(f, 0) < 3 for f in range(n_fixed)) and len(cov[K]) >= 2
    s = KC.make_store(obs, [0] * nk, rows, cov, [{} for _ in range(nk)], seed=60)
    s["pos"] = np.asarray(pos, F).reshape(-1, 3)
    pose = np.concatenate([w["fixed_pose"], w["pose_init"]]).astype(F)
    geom = dict(kf_pose=list(pose), kf_slot_uv=[np.asarray(u, F).reshape(-1, 2) for u in uvs],
                obs_slot=[[rows[f].index(p) for f in o] for p, o in enumerate(obs)])
    return dict(store=s, geom=geom, kf=K, fp=dict(synth.frame_params(), fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy)))


def chain_scene():
    """solve_scene() with K taken out again and handed back as the frame to insert: its slots hold the points the
    other keyframes see (LOCKED, with their store indices) and then the 40 points of its own (FREE with gid -1: the
    insertion adopts them), its keypoints are K's observations.  -> dict(store, geom, case, pose6, fp): case is a
    tests/kf_store_cases.py case under LORB_KF_GATE_NONE."""
    sc = solve_scene()
    s, g, K = sc["store"], sc["geom"], sc["kf"]
    row, uv = s["kf_slots"][K], np.asarray(g["kf_slot_uv"][K], F)
    own = [p for p in row if s["obs"][p] == [K]]
    n_old = s["n_points"] - len(own)
    assert own == list(range(n_old, s["n_points"])) and row[-len(own):] == own
    obs = [[f for f in o if f != K] for o in s["obs"][:n_old]]
    store = KC.make_store(obs, [0] * K, s["kf_slots"][:K], [[] for _ in range(K)], [{} for _ in range(K)], seed=61)
    store["pos"] = s["pos"][:n_old].copy()
    geom = dict(kf_pose=g["kf_pose"][:K], kf_slot_uv=g["kf_slot_uv"][:K],
                obs_slot=[[j for f, j in zip(o, js) if f != K] for o, js in zip(s["obs"][:n_old], g["obs_slot"][:n_old])])
    n, held = len(row), len(row) - len(own)
    state = [KC.LOCKED] * held + [KC.FREE] * len(own)
    c = KC.case(store, state, row[:held] + [-1] * len(own), {}, gate=R.GATE_NONE, seed=61, slack=8)
    c["frame"]["x"], c["frame"]["y"] = uv[:, 0].copy(), uv[:, 1].copy()
    c["slots"]["pos"][held:] = s["pos"][n_old:]
    assert c["n_cur"] == n
    return dict(store=store, geom=geom, case=c, pose6=np.asarray(g["kf_pose"][K], F), fp=sc["fp"])
