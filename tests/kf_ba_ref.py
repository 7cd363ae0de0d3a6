"""The store's geometry and the window lorb_kf_store_ba_gather_dev gathers, restated in plain Python on the store
dict of tests/kf_store_ref.py: BA::LocalPoseOptimization's frames, points and observations
(src/bundle_adjust.cpp:210-303), steps b-e of the contract in lorb_c.h.

The geometry of a store is dict(kf_pose: per keyframe its 6 floats mRvec | mTvec; kf_slot_uv: per keyframe an
(n_slots, 2) float32 array, GetKp2d of each slot; obs_slot: per point the slot of each of its observations,
parallel to store["obs"]).  Keyframe index order stands for std::map<Frame*, size_t> order."""
import numpy as np

import kf_store_ref as R

F = R.F
MAX_LOCAL, MAX_OBS = 128, 256
FIELDS = ("status", "kf", "n_poses", "n_fixed", "n_points", "n_obs", "n_cov_bad", "n_obs_bad_kf", "n_obs_bad_slot", "written")


def empty_geometry():
    return dict(kf_pose=[], kf_slot_uv=[], obs_slot=[])


def check_invariant(store, geom):
    """kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p for every observation o of p in f."""
    assert len(geom["kf_pose"]) == len(geom["kf_slot_uv"]) == len(store["kf_bad"])
    assert len(geom["obs_slot"]) == store["n_points"]
    for f, row in enumerate(store["kf_slots"]):
        assert len(geom["kf_slot_uv"][f]) == len(row), f
    for p, (obs, slots) in enumerate(zip(store["obs"], geom["obs_slot"])):
        assert len(obs) == len(slots), p
        for f, j in zip(obs, slots):
            assert 0 <= j < len(store["kf_slots"][f]) and store["kf_slots"][f][j] == p, (p, f, j)


def insert_geometry(geom, result, frame, pose6, n_cur):
    """The geometry after the insertion that R.insert_keyframe restated as `result`: K's pose vector (the bits of
    d_cur_pose->pose), K's uv row (the frame's left x, y of the slots j < n_cur), and the slot of every observation
    K added -- the lowest slot that holds a point the store already had, the slot that adopted or created a new
    one.  A refused insertion leaves the geometry as it is."""
    if not result["inserted"]:
        return geom
    s, K = result["store"], result["kf"]
    row = s["kf_slots"][K]
    assert len(row) == n_cur
    uv = np.stack([np.asarray(frame["x"], F)[:n_cur], np.asarray(frame["y"], F)[:n_cur]], axis=1).reshape(n_cur, 2)
    g = dict(kf_pose=list(geom["kf_pose"]) + [np.asarray(pose6, F).reshape(6)], kf_slot_uv=list(geom["kf_slot_uv"]) + [uv],
             obs_slot=[list(x) for x in geom["obs_slot"]])
    lowest = {}
    for j, p in enumerate(row):
        if p >= 0:
            lowest.setdefault(p, j)
    for p, obs in enumerate(s["obs"]):
        if p >= len(g["obs_slot"]):
            g["obs_slot"].append([])
        if len(obs) > len(g["obs_slot"][p]):   # K joined the list, last (src/map_point.cpp:133-139)
            assert obs[-1] == K and len(obs) == len(g["obs_slot"][p]) + 1
            g["obs_slot"][p].append(lowest[p])
    return g


def flat_geometry(geom):
    """The three arrays as the device keeps them."""
    uv = [np.asarray(r, F).reshape(-1, 2) for r in geom["kf_slot_uv"]]
    return dict(kf_pose=np.asarray(geom["kf_pose"], F).reshape(-1, 6),
                kf_slot_uv=np.concatenate(uv) if uv else np.zeros((0, 2), F),
                obs_slot=np.asarray([j for row in geom["obs_slot"] for j in row], np.int32))


def gather(store, geom, kf, src_status=0):
    """-> dict(rec: the record's fields that are written; and for status 0 / 3 the window: local_kf, fixed_kf, l2g,
    pose_init, fixed_pose, point_init, obs_point, obs_frame, obs_uv)."""
    nk, P = len(store["kf_bad"]), store["n_points"]
    # a. status
    if src_status != 0 or not 0 <= kf < nk:
        return dict(rec=dict(status=1))
    # b. frames, :210-220
    local, n_cov_bad = [kf], 0                                  # the reference does not ask whether kf is bad
    for f in store["cov"][kf]:                                  # the whole mvpOrderedKeyFrames, in row order
        if not 0 <= f < nk or f == kf:
            continue
        if store["kf_bad"][f]:                                  # :215-217
            n_cov_bad += 1
            continue
        if f not in local:
            local.append(f)
    if len(local) > MAX_LOCAL:
        return dict(rec=dict(status=2))
    rank = {f: r for r, f in enumerate(local)}
    # c. points, :224-241: first appearance over the local frames in list order, slots in slot order
    l2g, seen = [], set()
    for f in local:
        for p in store["kf_slots"][f]:
            if 0 <= p < P and not store["is_bad"][p] and p not in seen:
                seen.add(p)
                l2g.append(p)
    # d. observations, :270-303
    rows, fixed, bad_kf, bad_slot, maxk = [], set(), 0, 0, 0
    for i, p in enumerate(l2g):
        n = 0
        for f, j in zip(store["obs"][p], geom["obs_slot"][p]):  # ascending keyframe index
            if not 0 <= f < nk:
                bad_slot += 1
                continue
            if store["kf_bad"][f]:                              # :278
                bad_kf += 1
                continue
            if not 0 <= j < len(store["kf_slots"][f]):
                bad_slot += 1
                continue
            rows.append((i, f, j))
            n += 1
            if f not in rank:
                fixed.add(f)
        maxk = max(maxk, n)
    fixed = sorted(fixed)                                       # numbered in ascending keyframe index
    fid = {f: k for k, f in enumerate(fixed)}
    status = 3 if not l2g or not rows else 4 if maxk >= MAX_OBS else 0
    rec = dict(status=status, kf=kf, n_poses=len(local), n_fixed=len(fixed), n_points=len(l2g), n_obs=len(rows),
               n_cov_bad=n_cov_bad, n_obs_bad_kf=bad_kf, n_obs_bad_slot=bad_slot, written=0)
    pose = np.asarray(geom["kf_pose"], F).reshape(-1, 6)
    out = dict(rec=rec, local_kf=np.asarray(local, np.int32), fixed_kf=np.asarray(fixed, np.int32), l2g=np.asarray(l2g, np.int32),
               pose_init=pose[local].reshape(-1, 6), fixed_pose=pose[fixed].reshape(-1, 6),                        # e.
               point_init=np.asarray(store["pos"], F).reshape(-1, 3)[l2g].reshape(-1, 3))
    if status != 4:
        out.update(obs_point=np.asarray([i for i, _, _ in rows], np.int32),
                   obs_frame=np.asarray([rank[f] if f in rank else -1 - fid[f] for _, f, _ in rows], np.int32),
                   obs_uv=np.asarray([geom["kf_slot_uv"][f][j] for _, f, j in rows], F).reshape(-1, 2))
    return out
