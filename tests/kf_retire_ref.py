"""lorb_kf_store_retire_dev restated in plain Python -- the model the GPU tests compare with.  It is LITERAL and
SEQUENTIAL: the list is taken in order and every keyframe of it runs Frame::SetBadFlag as written
(src/frame.cpp:684-714), with dict-per-point observations and dict-per-keyframe weights: Frame::EraseConnection per
key of the weight map with its re-sort (:791-798, :754-774), MapPoint::EraseObservation per held slot with the cascade
at mnObs <= 2 into MapPoint::SetBadFlag (src/map_point.cpp:141-153, :184-199).  The device retires the list as a set;
that the two agree, in every order of the list, is what the tests prove.

What the header states beyond the reference, stated here in the same words:
  the guard     if(mnId == 0) return; (:686-687) reads kf_fid[f] == 0
  the verdict   is taken from the lists alone: EraseObservation acts where the point's list names f, and after the
                held slots every point whose list names f while no slot of f's row holds it gets the same call (on a
                sound store there is none)
  the row       the whole slot row of a retired keyframe becomes -1
  the counters  n_slots_erased and n_obs_bad_slot count the cascade's observations of keyframes OUTSIDE V (a keyframe
                of V loses its whole row whatever the cascade does); n_conn_erased and n_rows_reordered count keyframes
                outside V, a row once however often the sequence re-sorts it

A store is the dict of tests/kf_store_ref.py, obs_slot a list per point parallel to store["obs"], life the dict of
tests/kf_cull_ref.py (only kf_fid is read)."""
import copy

import kf_store_ref as R

MAX_LIST, MAX_PROTECT = 1024, 4
FIELDS = ("status", "n_skip_range", "n_skip_dup", "n_skip_bad", "n_skip_first", "n_skip_protected", "n_retired", "n_obs_erased",
          "n_points_bad", "n_obs_removed", "n_slots_erased", "n_obs_bad_slot", "n_conn_erased", "n_rows_reordered", "n_obs", "n_cov",
          "n_conn")


def classify(store, life, lst, protect=()):
    """Step b: -> (V in list order, the five skip counters)."""
    nk = len(store["kf_bad"])
    skip = dict(n_skip_range=0, n_skip_dup=0, n_skip_bad=0, n_skip_first=0, n_skip_protected=0)
    V, seen = [], set()
    for f in lst:
        f = int(f)
        if not 0 <= f < nk:
            skip["n_skip_range"] += 1
            continue
        if f in seen:
            skip["n_skip_dup"] += 1
        elif store["kf_bad"][f]:
            skip["n_skip_bad"] += 1
        elif int(life["kf_fid"][f]) == 0:                             # :686-687
            skip["n_skip_first"] += 1
        elif f in [int(x) for x in protect]:
            skip["n_skip_protected"] += 1
        else:
            V.append(f)
        seen.add(f)
    return V, skip


def retire(store, obs_slot, life, lst, n_list=None, n_max_list=None, protect=(), src_status=0, caps=None):
    """-> dict(store, obs_slot: afterwards (copies); rec: the record's fields that are written; V; dead: the points the
    cascade ran on).  lst: the list's entries (n_list defaults to all of them, n_max_list to their number); caps:
    dict(max_kf, max_points, max_obs, max_kf_slots) or None."""
    s, slot = copy.deepcopy(store), [list(x) for x in obs_slot]
    out = dict(store=s, obs_slot=slot, V=[], dead=[])
    n_list = len(lst) if n_list is None else n_list
    n_max_list = max(len(lst), 1) if n_max_list is None else n_max_list
    cn, nk = R.counts(s), len(s["kf_bad"])
    full = caps is not None and (nk > caps["max_kf"] or cn["n_points"] > caps["max_points"] or cn["n_obs"] > caps["max_obs"]
                                 or cn["n_kf_slots"] > caps["max_kf_slots"])
    if src_status != 0 or not 0 <= n_list <= n_max_list or full:     # a.
        out["rec"] = dict(status=1)
        return out
    V, skip = classify(s, life, lst[:n_list], protect)                # b.
    inV = set(V)
    rec = dict.fromkeys(FIELDS, 0)
    rec.update(skip, n_retired=len(V))
    lost, reordered = {}, set()

    def set_bad_point(p):                                             # MapPoint::SetBadFlag, src/map_point.cpp:184-199
        s["is_bad"][p] = 1
        for f, sl in zip(s["obs"][p], slot[p]):                       # Frame::EraseMapPoint(it->second)
            ok = 0 <= f < nk and 0 <= sl < len(s["kf_slots"][f]) and s["kf_slots"][f][sl] == p
            if ok:
                s["kf_slots"][f][sl] = -1
            if f not in inV:
                rec["n_slots_erased" if ok else "n_obs_bad_slot"] += 1
        rec["n_obs_removed"] += len(s["obs"][p])
        s["obs"][p], slot[p] = [], []
        out["dead"].append(p)

    def erase_observation(p, f):                                      # MapPoint::EraseObservation, :141-153
        if f in s["obs"][p]:
            i = s["obs"][p].index(f)
            del s["obs"][p][i], slot[p][i]                            # mpRefKF stays the first entry of the list (:147-148)
            rec["n_obs_removed"] += 1
            lost[p] = lost.get(p, 0) + 1
            if len(s["obs"][p]) <= 2:                                 # :151-152
                set_bad_point(p)

    for f in V:                                                       # Frame::SetBadFlag of each, in list order
        for g in sorted(s["conn"][f]):                                # :690-693, std::map order
            if f in s["conn"][g]:                                     # Frame::EraseConnection, :791-798
                del s["conn"][g][f]
                s["cov"][g] = R.ordered(s["conn"][g])                 # UpdateBestCovisibleFrames: ALL of the map
                if g not in inV:
                    rec["n_conn_erased"] += 1
                    reordered.add(g)
        for p in list(s["kf_slots"][f]):                              # :696-703, per held slot
            if 0 <= p < s["n_points"]:
                erase_observation(p, f)
        for p in range(s["n_points"]):                                # the lists alone: a damaged row
            erase_observation(p, f)
        s["conn"][f], s["cov"][f] = {}, []                            # :705-707
        s["kf_bad"][f] = 1                                            # :709
        s["kf_slots"][f] = [-1] * len(s["kf_slots"][f])               # the header's divergence
    dead = set(out["dead"])
    rec["n_points_bad"] = len(out["dead"])
    rec["n_obs_erased"] = sum(n for p, n in lost.items() if p not in dead)
    rec["n_rows_reordered"] = len(reordered)
    c1 = R.counts(s)
    rec.update(n_obs=c1["n_obs"], n_cov=c1["n_cov"], n_conn=c1["n_conn"])
    out.update(rec=rec, V=V)
    return out
