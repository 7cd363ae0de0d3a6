"""lorb_kf_store_refresh_dev restated in plain Python / numpy on the store dict of tests/kf_store_ref.py, the geometry
of tests/kf_ba_ref.py and the appearance: MapPoint::UpdateNormalAndDepth (src/map_point.cpp:224-264) and
MapPoint::ComputeDescriptor (:69-129) over the points of a gathered window, steps b-d of the contract in lorb_c.h.

The appearance of a store is dict(kf_slot_desc: per keyframe an (n_slots, 32) uint8 array, GetDescriptor of each
slot; kf_slot_octave: per keyframe its slots' octaves; kf_center: (n_kf, 3) float32, mptCameraCenter).  The centres
are an INPUT: the device's double sin / cos are not libm's, so the store's own centres are what the points are
checked against (centers() gives the host's value of step b).  All arithmetic is written with explicit np.float32 /
np.float64 scalars."""
import numpy as np

import kf_store_ref as R

F, D = R.F, R.D
CENTERS, NORMAL_DEPTH, DESCRIPTOR, ALL = 1, 2, 4, 7
MAX_LEVELS = 16
FIELDS = ("status", "kf", "n_points", "n_refreshed", "n_bad", "n_empty", "n_obs_bad_slot", "n_desc_changed", "n_centers")


def flat_appearance(app):
    """The three arrays as the device keeps them."""
    d = [np.asarray(r, np.uint8).reshape(-1, 32) for r in app["kf_slot_desc"]]
    o = [np.asarray(r, np.int32).reshape(-1) for r in app["kf_slot_octave"]]
    return dict(kf_slot_desc=np.concatenate(d) if d else np.zeros((0, 32), np.uint8),
                kf_slot_octave=np.concatenate(o) if o else np.zeros(0, np.int32),
                kf_center=np.asarray(app["kf_center"], F).reshape(-1, 3))


def insert_appearance(app, result, frame, pose, n_cur):
    """The appearance after the insertion that R.insert_keyframe restated as `result`: K's descriptor and octave rows
    are the frame's of the slots j < n_cur, its centre the translation column of pose["Twc"].  A refused insertion
    leaves the appearance as it is."""
    if not result["inserted"]:
        return app
    Twc = np.asarray(pose["Twc"], F).reshape(16)
    return dict(kf_slot_desc=list(app["kf_slot_desc"]) + [np.asarray(frame["desc"], np.uint8).reshape(-1, 32)[:n_cur].copy()],
                kf_slot_octave=list(app["kf_slot_octave"]) + [np.asarray(frame["octave"], np.int32)[:n_cur].copy()],
                kf_center=np.concatenate([np.asarray(app["kf_center"], F).reshape(-1, 3), Twc[[3, 7, 11]].reshape(1, 3)]))


def centers(kf_pose, local, kf_center, pose_to_Tcw, inv4):
    """Step b with the host's arithmetic: kf_center with the rows of `local` replaced by the translation column of
    inv4(pose_to_Tcw(rvec, tvec)) (oracle.pose_to_Tcw / oracle.inv4_f32)."""
    out = np.array(kf_center, F).reshape(-1, 3).copy()
    for f in local:
        p = np.asarray(kf_pose[f], F).reshape(6)
        Twc = np.asarray(inv4(pose_to_Tcw(p[:3], p[3:]))[0], F).reshape(16)
        out[f] = Twc[[3, 7, 11]]
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def choose(descs):
    """ComputeDescriptor's choice among n >= 1 descriptors (:84-124): element (n - 1) // 2 of every sorted row of the
    all-pairs matrix, self-distance included; the smallest median, the first index of equals."""
    n = len(descs)
    best, best_median = 0, None
    for i in range(n):
        row = sorted(hamming(descs[i], descs[j]) for j in range(n))
        median = row[(n - 1) // 2]
        if best_median is None or median < best_median:
            best, best_median = i, median
    return best


def split(store, geom, p):
    """Point p's observations as (keyframe, slot) inside the store, in list order, and the number outside it."""
    nk = len(store["kf_bad"])
    inside, outside = [], 0
    for f, j in zip(store["obs"][p], geom["obs_slot"][p]):
        if 0 <= f < nk and 0 <= j < len(store["kf_slots"][f]):
            inside.append((f, j))
        else:
            outside += 1
    return inside, outside


def normal_and_depth(pos, obs, kf_center, app, fp):
    """UpdateNormalAndDepth over the observations obs = [(keyframe, slot)] (all of them: bad keyframes count),
    :241-262 with OpenCV's arithmetic: cv::norm accumulates the squares in double, a Mat divided by a scalar is
    multiplied by the float reciprocal, and a Mat sum is a float add per component."""
    C = np.asarray(kf_center, F).reshape(-1, 3)
    s = [F(0), F(0), F(0)]
    for f, _ in obs:
        d = [F(pos[k]) - C[f][k] for k in range(3)]
        with np.errstate(divide="ignore", invalid="ignore"):
            nd = np.sqrt(D(d[0]) * D(d[0]) + D(d[1]) * D(d[1]) + D(d[2]) * D(d[2]))
            inv = F(D(1.0) / nd)
            s = [F(s[k] + F(d[k] * inv)) for k in range(3)]
    invn = F(D(1.0) / D(len(obs)))
    normal = np.array([F(s[k] * invn) for k in range(3)], F)
    rf, rj = obs[0]                                               # mpRefKF: the first entry of the list
    d = [F(pos[k]) - C[rf][k] for k in range(3)]
    dist = F(np.sqrt(D(d[0]) * D(d[0]) + D(d[1]) * D(d[1]) + D(d[2]) * D(d[2])))
    sf = np.asarray(fp["scale_factors"], F)
    lvl = min(max(int(app["kf_slot_octave"][rf][rj]), 0), MAX_LEVELS - 1)
    top = min(max(int(fp["n_levels"]) - 1, 0), MAX_LEVELS - 1)
    mx = F(dist * sf[lvl])
    return normal, mx, F(mx / sf[top])


def refresh(store, geom, app, window, kf_center, fp, what=ALL, ba_status=0, written=0):
    """-> dict(rec: the record's fields that are written; normal, max_dist, min_dist, desc: the columns afterwards
    (copies); chosen: per window point the position, among its usable observations, of the one whose descriptor it
    took, or -1).  window: dict(kf, local_kf, l2g) of the gather; kf_center: the centres the points are computed
    from (after step b)."""
    cols = {k: np.array(store[k]).copy() for k in ("normal", "max_dist", "min_dist", "desc")}
    if ba_status != 0:
        return dict(rec=dict(status=1), chosen=[], **cols)
    rec = dict(status=0, kf=int(window["kf"]), n_points=len(window["l2g"]), n_refreshed=0, n_bad=0, n_empty=0, n_obs_bad_slot=0,
               n_desc_changed=0, n_centers=len(window["local_kf"]) if (what & CENTERS) and written == 1 else 0)
    chosen = []
    for g in (int(v) for v in window["l2g"]):
        chosen.append(-1)
        if store["is_bad"][g]:                                     # :230
            rec["n_bad"] += 1
            continue
        obs, outside = split(store, geom, g)
        rec["n_obs_bad_slot"] += outside
        if not obs:                                                # :238
            rec["n_empty"] += 1
            continue
        rec["n_refreshed"] += 1
        if what & NORMAL_DEPTH:
            cols["normal"][g], cols["max_dist"][g], cols["min_dist"][g] = normal_and_depth(store["pos"][g], obs, kf_center, app, fp)
        if what & DESCRIPTOR:
            use = [(f, j) for f, j in obs if not store["kf_bad"][f]]   # :77-78
            if use:                                                # none: the descriptor stays
                descs = [np.asarray(app["kf_slot_desc"][f][j], np.uint8) for f, j in use]
                chosen[-1] = choose(descs)
                rec["n_desc_changed"] += hamming(cols["desc"][g], descs[chosen[-1]])
                cols["desc"][g] = descs[chosen[-1]]
    return dict(rec=rec, chosen=chosen, **cols)
