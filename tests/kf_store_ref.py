"""The growing map store and lorb_kf_store_insert_dev restated in plain Python / numpy -- the model the GPU tests
compare with: VisualOdometry::AddKeyFrame (src/visual_odometry.cpp:356-404) and the map part of Initialize
(:86-103), LocalMapping::ProcessNewFrames step 1 (src/local_mapping.cpp:57-70), Frame::UpdateConnections
(src/frame.cpp:801-869) with AddConnection and UpdateBestCovisibleFrames (:754-788).

A store is the dict of tests/local_map_ref.py (n_points; the columns pos, normal, max_dist, min_dist, desc, locked,
is_bad; obs, kf_bad, kf_slots, cov as lists per row) plus conn: per keyframe {keyframe: weight}
(mConnectedKeyFrameWeights).  Keyframe index order stands for std::map<Frame*, ...> order.  Step d's arithmetic
is written with explicit np.float32 / np.float64 scalars."""
import copy

import numpy as np

EMPTY, FREE, LOCKED = 0, 1, 2
GATE_RATIO, GATE_NONE = 0, 1
F, D = np.float32, np.float64
COLS = ("pos", "normal", "max_dist", "min_dist", "desc", "locked", "is_bad")
FIELDS = ("status", "inserted", "n_cur", "n_map", "kf", "n_observed", "n_adopted", "n_created", "n_connected", "n_points",
          "n_kf", "n_obs")


def empty_store():
    return dict(n_points=0, pos=np.zeros((0, 3), F), normal=np.zeros((0, 3), F), max_dist=np.zeros(0, F), min_dist=np.zeros(0, F),
                desc=np.zeros((0, 32), np.uint8), locked=np.zeros(0, np.uint8), is_bad=np.zeros(0, np.uint8), obs=[],
                kf_bad=np.zeros(0, np.uint8), kf_slots=[], cov=[], conn=[])


def counts(s):
    return dict(n_kf=len(s["kf_bad"]), n_points=s["n_points"], n_obs=sum(len(o) for o in s["obs"]),
                n_kf_slots=sum(len(k) for k in s["kf_slots"]), n_cov=sum(len(c) for c in s["cov"]),
                n_conn=sum(len(c) for c in s["conn"]))


def unproject(fp, Twc, x, y, z):
    """Frame::UnprojectStereo (src/frame.cpp:335-356) under a given Twc: camera coordinates in float, the product
    accumulated in double as cv::gemm on CV_32F does, one rounding; the origin without depth (:352-355)."""
    x, y, z = F(x), F(y), F(z)
    if not z > 0:
        return np.zeros(3, F)
    xx = (x - F(fp["cx"])) * z / F(fp["fx"])
    yy = (y - F(fp["cy"])) * z / F(fp["fy"])
    T = np.asarray(Twc, F).reshape(16)
    out = np.zeros(3, F)
    for r in range(3):
        s = D(T[4 * r]) * D(xx) + D(T[4 * r + 1]) * D(yy) + D(T[4 * r + 2]) * D(z) + D(T[4 * r + 3]) * D(F(1.0))
        out[r] = F(s)
    return out


def normal_and_depth(pos, Ow, octave, fp):
    """UpdateNormalAndDepth over one observation (src/map_point.cpp:224-264), OpenCV's arithmetic restated:
    cv::norm accumulates the squares in double; the division of the Mat is a multiply by the float reciprocal."""
    d = [F(pos[k]) - F(Ow[k]) for k in range(3)]
    nd = np.sqrt(D(d[0]) * D(d[0]) + D(d[1]) * D(d[1]) + D(d[2]) * D(d[2]))
    inv = F(D(1.0) / nd)
    normal = np.array([d[0] * inv, d[1] * inv, d[2] * inv], F)
    dist = F(nd)
    sf = np.asarray(fp["scale_factors"], F)
    max_dist = dist * sf[int(octave)]                    # :260
    min_dist = max_dist / sf[int(fp["n_levels"]) - 1]    # :261
    return normal, F(max_dist), F(min_dist)


def ordered(weights):
    """UpdateBestCovisibleFrames (src/frame.cpp:754-774): ALL of a weight map, ascending by (weight, index)."""
    return [kf for w, kf in sorted((w, kf) for kf, w in weights.items())]


def insert_keyframe(store, caps, fp, frame, pose, slots, gid, n_cur, n_max_cur, gate=GATE_RATIO, src_status=0):
    """-> dict(rec: the record's fields that are written; store: the store afterwards (a copy; the same content when
    nothing was inserted); state, pos, desc, gid: the slots afterwards (all given entries); inserted; kf).
    caps: dict(max_kf, max_points, max_obs, max_kf_slots); frame: dict(x, y, depth, octave, desc); pose: dict(Twc,
    status); slots: dict(state, pos, desc)."""
    st, sp, sd = np.array(slots["state"], np.uint8), np.array(slots["pos"], F).reshape(-1, 3), np.array(slots["desc"], np.uint8)
    g = np.array(gid, np.int32)
    out = dict(store=store, state=st, pos=sp, desc=sd, gid=g, inserted=False, kf=-1)
    # a. status
    if n_cur < 0 or n_cur > n_max_cur or pose["status"] != 0 or src_status != 0:
        out["rec"] = dict(status=1)
        return out
    n = n_cur
    K, P = len(store["kf_bad"]), store["n_points"]
    c0 = counts(store)
    # b. the gate, :360-372
    n_map = int(sum(st[j] != EMPTY for j in range(n)))             # :361-368
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = F(n_map) / F(n)                                     # :369, NaN for an empty frame
    if gate == GATE_RATIO and ratio > F(0.35):                      # :370-372
        out["rec"] = dict(status=0, inserted=0, n_map=n_map)
        return out
    # d's cases, counted first: c decides before anything is written
    kind, held = [], {}
    for j in range(n):
        gj = int(g[j]) if 0 <= g[j] < P else -1                     # an index outside the store counts as -1
        if st[j] != EMPTY:
            if gj < 0:
                kind.append(("adopt", -1))
            elif store["is_bad"][gj]:
                kind.append(("bad", gj))                            # src/local_mapping.cpp:60-61
            else:
                kind.append(("observe", gj))
                held.setdefault(gj, j)                              # the lowest slot adds the observation
        else:
            kind.append(("create", -1) if frame["depth"][j] >= 0 else ("stay", -1))   # :88-89
    n_observed = len(held)
    n_adopted, n_created = sum(k == "adopt" for k, _ in kind), sum(k == "create" for k, _ in kind)
    n_new = n_adopted + n_created
    if (K + 1 > caps["max_kf"] or P + n_new > caps["max_points"] or c0["n_obs"] + n_observed + n_new > caps["max_obs"]
            or c0["n_kf_slots"] + n > caps["max_kf_slots"]):
        out["rec"] = dict(status=2, inserted=0, n_cur=n, n_map=n_map, kf=-1, n_observed=n_observed, n_adopted=n_adopted,
                          n_created=n_created, n_connected=0, n_points=P, n_kf=K, n_obs=c0["n_obs"])
        return out
    s = copy.deepcopy(store)
    Twc = np.asarray(pose["Twc"], F).reshape(16)
    Ow = (Twc[3], Twc[7], Twc[11])
    new = {k: [] for k in COLS}
    row = []
    for j in range(n):
        k, gj = kind[j]
        if k == "bad":
            row.append(gj)
        elif k == "observe":                                        # src/local_mapping.cpp:62-65
            if held[gj] == j:
                s["obs"][gj].append(K)                              # src/map_point.cpp:133-139: once; K is the largest
            s["locked"][gj] = 1
            st[j] = LOCKED
            row.append(gj)
        elif k in ("adopt", "create"):
            if k == "create":                                       # :91-97
                sp[j] = unproject(fp, Twc, frame["x"][j], frame["y"][j], frame["depth"][j])
                sd[j] = frame["desc"][j]
            st[j] = LOCKED
            nrm, mx, mn = normal_and_depth(sp[j], Ow, frame["octave"][j], fp)
            for key, v in zip(COLS, (sp[j].copy(), nrm, mx, mn, sd[j].copy(), 1, 0)):
                new[key].append(v)
            idx = P + len(new["pos"]) - 1
            s["obs"].append([K])
            g[j] = idx
            row.append(idx)
        else:
            g[j] = -1
            row.append(-1)
    if n_new:
        for key in COLS:
            add = np.asarray(new[key], s[key].dtype).reshape((n_new,) + s[key].shape[1:])
            s[key] = np.concatenate([s[key], add])
    s["n_points"] = P + n_new
    # e. K's row
    s["kf_slots"].append(row)
    s["kf_bad"] = np.concatenate([s["kf_bad"], np.zeros(1, np.uint8)])
    # f. UpdateConnections(K), src/frame.cpp:801-869
    counter = {}                                                    # :804
    for j in range(n):                                              # :808, per slot
        p = row[j]
        if st[j] == EMPTY or p < 0 or s["is_bad"][p]:               # :811-814
            continue
        for kf in s["obs"][p]:                                      # :816-821
            if kf != K:
                counter[kf] = counter.get(kf, 0) + 1
    pairs = []
    best = None
    for kf in sorted(counter):                                      # :828, std::map order
        w = counter[kf]
        if best is None or w > best[0]:                             # the strictly largest count, the first of equals
            best = (w, kf)
        if w >= 3:                                                  # :838-842
            pairs.append((w, kf))
    if not pairs and best is not None:                              # :845-849 restated (lorb_c.h)
        pairs.append(best)
    for w, kf in pairs:                                             # f.AddConnection(K, w), :777-788
        s["conn"][kf][K] = w
        s["cov"][kf] = ordered(s["conn"][kf])                       # :786, from ALL of the map
    s["conn"].append(dict(counter))                                 # :855
    s["cov"].append([kf for w, kf in sorted(pairs)])                # :851, :856-862
    c1 = counts(s)
    out.update(store=s, inserted=True, kf=K,
               rec=dict(status=0, inserted=1, n_cur=n, n_map=n_map, kf=K, n_observed=n_observed, n_adopted=n_adopted,
                        n_created=n_created, n_connected=len(pairs), n_points=c1["n_points"], n_kf=K + 1, n_obs=c1["n_obs"]))
    return out
