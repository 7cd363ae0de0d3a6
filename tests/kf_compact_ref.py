"""lorb_kf_store_compact_dev restated in plain Python / numpy -- the model the GPU tests compare with (the contract is
in include/lorb_c.h).  A point p below the true n_points is DROPPED when all of these hold: is_bad[p]; its observation
list is empty; no keyframe slot below the true n_kf_slots names it; no examined entry (j < count) of a caller's gid
table names it.  Every other point is kept and takes the index new(p) = the number of kept points below p.

Two forms of the same rule:
  compact_store   on the store dict of tests/kf_store_ref.py with obs_slot (a list per point) and the life dict of
                  tests/kf_cull_ref.py: what the calls behind a compaction are restated on;
  compact_arrays  on the device's arrays over their whole capacity (the dict tests/test_gpu_kf_cull.all_arrays reads):
                  every byte the call may and may not write, the rows that return to a fresh store's state included.
A table is dict(gid: int32 array over the whole buffer, n_max, count)."""
import copy

import numpy as np

FIELDS = ("status", "n_points_before", "n_dropped", "n_points", "n_bad_kept", "n_kf_slots_mapped", "n_gids_mapped")
MAX_TABLES = 8
POINT_ROWS = ("pos", "normal", "max_dist", "min_dist", "desc", "locked", "is_bad", "life_visible", "life_found", "life_first_fid",
              "life_recent")   # obs_off moves too, by its own rule
LIFE_ROWS = ("visible", "found", "first_fid", "recent")


def refused(tables, src_status):
    """a. the status, decided before the first write"""
    return src_status != 0 or any(not 0 <= t["count"] <= t["n_max"] for t in tables)


def verdict(P, is_bad, obs_len, slot_points, tables):
    """-> (keep: bool per point, held: bool per point).  slot_points: kf_slot_point below the true n_kf_slots."""
    held = np.zeros(P, bool)
    for g in slot_points:                                      # b. a keyframe slot
        if 0 <= g < P and is_bad[g]:
            held[g] = True
    for t in tables:                                           # b. an examined table entry
        for g in t["gid"][:t["count"]]:
            if 0 <= g < P and is_bad[g]:
                held[g] = True
    keep = np.array([not (is_bad[p] and obs_len[p] == 0 and not held[p]) for p in range(P)], bool)   # c.
    return keep, held


def index_map(keep):
    """new(p) = the kept points below p; -1 for a dropped point"""
    m = np.cumsum(keep) - keep
    return np.where(keep, m, -1).astype(np.int32)


def map_tables(tables, m, rec, go):
    out = []
    P = len(m)
    for t in tables:
        g = np.array(t["gid"], np.int32)
        if go:
            for j in range(t["count"]):
                if 0 <= g[j] < P:
                    assert m[g[j]] >= 0                        # an examined entry keeps its point
                    g[j] = m[g[j]]
                    rec["n_gids_mapped"] += 1
        out.append(dict(t, gid=g))
    return out


def compact_store(store, obs_slot, life, tables=(), src_status=0):
    """-> dict(store, obs_slot, life, tables: afterwards (copies); map: old -> new or None when refused; rec: the
    record's fields that are written; dropped: the points that went)."""
    s, slot, L = copy.deepcopy(store), [list(x) for x in obs_slot], {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in life.items()}
    out = dict(store=s, obs_slot=slot, life=L, tables=[dict(t, gid=np.array(t["gid"], np.int32)) for t in tables], map=None, dropped=[])
    if refused(tables, src_status):
        out["rec"] = dict(status=1)
        return out
    P = s["n_points"]
    flat = [g for row in s["kf_slots"] for g in row]
    keep, _ = verdict(P, s["is_bad"], [len(o) for o in s["obs"]], flat, tables)
    m = index_map(keep)
    n = int(keep.sum())
    rec = dict(status=0, n_points_before=P, n_dropped=P - n, n_points=n, n_bad_kept=int(sum(1 for p in range(P) if keep[p] and s["is_bad"][p])),
               n_kf_slots_mapped=0, n_gids_mapped=0)
    out.update(map=m, rec=rec, dropped=[p for p in range(P) if not keep[p]])
    if n == P:                                                 # nothing to drop: not a byte changes
        return out
    for k in ("pos", "normal", "max_dist", "min_dist", "desc", "locked", "is_bad"):   # e.
        s[k] = s[k][keep]
    for k in LIFE_ROWS:
        L[k] = L[k][keep]
    s["obs"] = [o for p, o in enumerate(s["obs"]) if keep[p]]
    out["obs_slot"] = [o for p, o in enumerate(slot) if keep[p]]
    s["n_points"] = n
    for row in s["kf_slots"]:                                  # f.
        for j, g in enumerate(row):
            if 0 <= g < P:
                assert m[g] >= 0
                row[j] = int(m[g])
                rec["n_kf_slots_mapped"] += 1
    out["tables"] = map_tables(tables, m, rec, True)
    return out


def compact_arrays(arrays, counts, tables=(), src_status=0, d_map=None):
    """arrays: name -> numpy array over the whole capacity (a life array under "life_" + its name); counts: the true
    n_points, n_obs, n_kf_slots.  d_map: the caller's buffer as it stands, or None.
    -> dict(arrays, tables, d_map: afterwards (copies); rec; n_points)."""
    a = {k: np.array(v) for k, v in arrays.items()}
    out = dict(arrays=a, tables=[dict(t, gid=np.array(t["gid"], np.int32)) for t in tables], d_map=None if d_map is None else np.array(d_map),
               n_points=counts["n_points"])
    if refused(tables, src_status):
        out["rec"] = dict(status=1)
        return out
    P, O, S = counts["n_points"], counts["n_obs"], counts["n_kf_slots"]
    off = np.clip(a["obs_off"][:P + 1].astype(np.int64), 0, O)
    obs_len = [max(int(off[p + 1]) - int(off[p]), 0) for p in range(P)]
    keep, _ = verdict(P, a["is_bad"], obs_len, a["kf_slot_point"][:S], tables)
    m = index_map(keep)
    n = int(keep.sum())
    rec = dict(status=0, n_points_before=P, n_dropped=P - n, n_points=n, n_bad_kept=int((keep & (a["is_bad"][:P] != 0)).sum()),
               n_kf_slots_mapped=0, n_gids_mapped=0)
    out["rec"] = rec
    if out["d_map"] is not None:                               # d. the identity when nothing is dropped
        out["d_map"][:P] = m
    if n == P:
        return out
    for k in POINT_ROWS:                                       # e. the rows, and a fresh store's state behind them
        a[k][:n] = arrays[k][:P][keep]
        a[k][n:P] = 1 if k == "is_bad" else 0
    a["obs_off"][:n] = arrays["obs_off"][:P][keep]
    a["obs_off"][n] = O
    a["obs_off"][n + 1:P + 1] = 0
    sp = a["kf_slot_point"]                                    # f.
    for i in range(S):
        if 0 <= sp[i] < P:
            assert m[sp[i]] >= 0
            sp[i] = m[sp[i]]
            rec["n_kf_slots_mapped"] += 1
    out["tables"] = map_tables(tables, m, rec, True)
    out["n_points"] = n
    return out
