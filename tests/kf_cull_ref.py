"""The life of the store's points, lorb_kf_store_observe_dev and lorb_kf_store_cull_dev restated in plain Python /
numpy -- the model the GPU tests compare with: the MapPoint constructors (src/map_point.cpp:16-17,33-34), the list
LocalMapping::ProcessNewFrames keeps (src/local_mapping.cpp:57-70), the tracker's two IncreaseVisible sites
(src/visual_odometry.cpp:153-171, :176-195), LocalMapping::MapPointsCulling (src/local_mapping.cpp:82-108) in the
verdict order of include/lorb/local_mapping.hpp:63-74, MapPoint::SetBadFlag (src/map_point.cpp:184-199) and
Frame::EraseMapPoint (src/frame.cpp:896-899).

A store is the dict of tests/kf_store_ref.py.  Its life is a dict(visible, found, first_fid: int32 per point; recent:
uint8 per point, the membership of mvpRecentAddPoints; kf_fid: int32 per keyframe; frame_word: the id of the frame the
tracker last observed).  obs_slot is a list per point, parallel to store["obs"]: the slot of the point in that
keyframe."""
import copy

import numpy as np

import kf_store_ref as R

EMPTY = R.EMPTY
F = np.float32
FOUND_NEVER, FOUND_SLOTS = 0, 1
REFERENCE = (0.25, 2, 3, 3)  # min_found_ratio, age_obs, min_obs, age_out: src/local_mapping.cpp:92,98,104
LIFE = ("visible", "found", "first_fid", "recent", "kf_fid")
OBSERVE_FIELDS = ("status", "n_held", "n_in_view", "n_found")
CULL_FIELDS = ("status", "kf", "n_examined", "n_bad_before", "n_culled_ratio", "n_culled_obs", "n_aged_out", "n_recent",
               "n_obs_removed", "n_slots_erased", "n_frame_slots_emptied", "n_obs_bad_slot", "n_obs")
VERDICTS = ("bad_before", "ratio", "obs", "aged_out", "stays")


def new_life(n_kf, n_points):
    """A store from create: mnVisible = mnFound = 1, everything else 0."""
    return dict(visible=np.ones(n_points, np.int32), found=np.ones(n_points, np.int32), first_fid=np.zeros(n_points, np.int32),
                recent=np.zeros(n_points, np.uint8), kf_fid=np.zeros(n_kf, np.int32), frame_word=0)


def copy_life(life):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in life.items()}


def insert_life(life, store, frame, slots, gid, res):
    """The life after lorb_kf_store_insert_dev.  store, frame, slots, gid: the call's inputs as kf_store_ref.
    insert_keyframe took them (the store BEFORE the call); res: what it returned.  Nothing inserted: unchanged."""
    out = copy_life(life)
    if not res["inserted"]:
        return out
    P, n, fid = store["n_points"], res["rec"]["n_cur"], int(life["frame_word"])
    first, new_recent = {}, []
    for j in range(n):
        g = int(gid[j]) if 0 <= gid[j] < P else -1
        if slots["state"][j] != EMPTY:
            if g < 0:
                new_recent.append(0)                       # adopted: AddObservation, not pushed (:62-65)
            elif not store["is_bad"][g]:                   # a held bad point changes nothing (:60-61)
                if g in first:
                    out["recent"][g] = 1                   # a later slot finds IsInFrame true: pushed (:66-69)
                first.setdefault(g, j)
        elif frame["depth"][j] >= 0:
            new_recent.append(1)                           # created with K as an observation: pushed
    k = len(new_recent)
    assert k == res["rec"]["n_adopted"] + res["rec"]["n_created"]
    out["visible"] = np.concatenate([out["visible"], np.ones(k, np.int32)])
    out["found"] = np.concatenate([out["found"], np.ones(k, np.int32)])
    out["first_fid"] = np.concatenate([out["first_fid"], np.full(k, fid, np.int32)])
    out["recent"] = np.concatenate([out["recent"], np.asarray(new_recent, np.uint8)])
    out["kf_fid"] = np.concatenate([out["kf_fid"], np.asarray([fid], np.int32)])
    return out


def observe(life, n_points, frame_id, n_cur, n_max_cur, state, gid, lid, l2g, n_local, max_local, in_view, update_status=0,
            local_status=0, found_rule=FOUND_NEVER):
    """-> (life afterwards, the record's fields that are written)."""
    out = copy_life(life)
    if (n_cur < 0 or n_cur > n_max_cur or local_status != 0 or update_status != 0 or n_local < 0 or n_local > max_local):
        return out, dict(status=1)                                    # a. nothing else, the frame word included
    out["frame_word"] = int(frame_id)                                 # b.
    rec = dict(status=0, n_held=0, n_in_view=0, n_found=0)
    for j in range(n_cur):                                            # c. :153-171, per slot
        if 0 <= gid[j] < n_points:
            out["visible"][gid[j]] += 1
            rec["n_held"] += 1
    for k in range(n_local):                                          # d. :188-194
        if in_view[k] and 0 <= l2g[k] < n_points:
            out["visible"][l2g[k]] += 1
            rec["n_in_view"] += 1
    if found_rule == FOUND_SLOTS:                                     # e. ORB-SLAM2's TrackLocalMap intent
        for j in range(n_cur):
            if state[j] == EMPTY:
                continue
            g = -1
            if lid[j] < 0:
                g = gid[j]
            elif lid[j] < n_local:
                g = l2g[lid[j]]
            if 0 <= g < n_points:
                out["found"][g] += 1
                rec["n_found"] += 1
    return out, rec


def verdict(found, visible, age, n_obs, is_bad, params=REFERENCE):
    """One list entry, in the order of include/lorb/local_mapping.hpp:66-71."""
    ratio, age_obs, min_obs, age_out = params
    if is_bad:
        return "bad_before"
    if F(found) / F(visible) < F(ratio):
        return "ratio"
    if age >= age_obs and n_obs < min_obs:
        return "obs"
    if age >= age_out:
        return "aged_out"
    return "stays"


def cull(store, obs_slot, life, kf, params=REFERENCE, src_status=0, frame=None):
    """-> dict(store, obs_slot, life: afterwards (copies); rec: the record's fields that are written; verdicts: {point:
    verdict}; culled: the points culled by this call; state, gid: the frame's slots afterwards when frame =
    dict(n_cur, n_max_cur, state, gid) is given)."""
    s, slot, L = copy.deepcopy(store), [list(x) for x in obs_slot], copy_life(life)
    out = dict(store=s, obs_slot=slot, life=L, verdicts={}, culled=[])
    if frame is not None:
        out.update(state=np.array(frame["state"], np.uint8), gid=np.array(frame["gid"], np.int32))
    nk, P = len(s["kf_bad"]), s["n_points"]
    if src_status != 0 or not 0 <= kf < nk:                           # a.
        out["rec"] = dict(status=1)
        return out
    cur = int(L["kf_fid"][kf])
    rec = dict.fromkeys(CULL_FIELDS, 0)
    rec["kf"] = kf
    for p in range(P):                                                # b.
        if not L["recent"][p]:
            continue
        rec["n_examined"] += 1
        age = (cur - int(L["first_fid"][p])) & 0xffffffff             # size_t arithmetic, as 32 bits
        v = verdict(int(L["found"][p]), int(L["visible"][p]), age, len(s["obs"][p]), s["is_bad"][p], params)
        out["verdicts"][p] = v
        rec[dict(bad_before="n_bad_before", ratio="n_culled_ratio", obs="n_culled_obs", aged_out="n_aged_out", stays="n_recent")[v]] += 1
        if v != "stays":
            L["recent"][p] = 0
        if v in ("ratio", "obs"):
            out["culled"].append(p)
    for p in out["culled"]:                                           # c. SetBadFlag
        s["is_bad"][p] = 1
        for f, sl in zip(s["obs"][p], slot[p]):                       # Frame::EraseMapPoint, bad keyframe or not
            if 0 <= f < nk and 0 <= sl < len(s["kf_slots"][f]) and s["kf_slots"][f][sl] == p:
                s["kf_slots"][f][sl] = -1
                rec["n_slots_erased"] += 1
            else:
                rec["n_obs_bad_slot"] += 1
        rec["n_obs_removed"] += len(s["obs"][p])
        s["obs"][p], slot[p] = [], []
    if frame is not None and 0 <= frame["n_cur"] <= frame["n_max_cur"]:   # d.
        gone = set(out["culled"])
        for j in range(frame["n_cur"]):
            if int(out["gid"][j]) in gone:
                out["state"][j] = EMPTY
                out["gid"][j] = -1
                rec["n_frame_slots_emptied"] += 1
    rec["n_obs"] = sum(len(o) for o in s["obs"])                      # e.
    out["rec"] = rec
    return out
