"""VisualOdometry::UpdateLocalMap (src/visual_odometry.cpp:234-340) restated in plain Python / numpy on
the flattened map store lorb_local_map_update_dev reads -- the model the GPU tests compare with.

A store is a dict: n_points; is_bad (n_points uint8) or None; obs: per point the list of observing
keyframe indices (MapPoint::GetObservations); kf_bad (n_kf uint8, Frame::IsBad); kf_slots: per keyframe
the list of its slots' global point indices, -1 for NULL (Frame::GetMapPoints); cov: per keyframe its
ordered covisible keyframes (mvpOrderedKeyFrames); and the point columns pos, normal, max_dist,
min_dist, desc, locked for the gather.  Keyframe index order stands for std::map<Frame*, ...> order,
point index order for std::set<MapPoint*> order."""
import numpy as np

EMPTY = 0
UNCHANGED, NULL = -1, -2
COLS = ("pos", "normal", "max_dist", "min_dist", "desc", "locked")


def entry_gids(gid, n_cur, n_points, ids=None):
    """Step b: the slots' global ids on entry.  ids: None (gid as given) or dict(assign, pass_, given,
    last_gid) -- the rule documented for lorb_track_local_id_source, over global ids."""
    g = np.asarray(gid[:n_cur], np.int64).copy()
    if ids is not None:
        keep = ids["pass_"] == 1 and bool(ids["given"])
        for j in range(n_cur):
            c = int(ids["assign"][j])
            if c >= 0:
                g[j] = ids["last_gid"][c] if c < len(ids["last_gid"]) else -1
            elif c == NULL or not keep:
                g[j] = -1
    g[(g < 0) | (g >= n_points)] = -1  # a point outside the store
    return g.astype(np.int32)


def update_local_map(store, state, gid, n_cur, max_local, ids=None):
    """-> dict(state, gid: the n_cur slots after step 1.1; votes (n_kf); local_kf (list); refer_kf;
    n_held, n_nulled, n_voted, n_local; status 0 / 2; l2g (list), g2l (n_points); slot_id (n_cur local
    rows, None under status 2); rows: the gathered columns (n_local rows each, none under status 2))."""
    n_points, n_kf = store["n_points"], len(store["kf_bad"])
    bad = store.get("is_bad")
    st = np.asarray(state[:n_cur], np.uint8).copy()
    g = entry_gids(gid, n_cur, n_points, ids)
    # step 1.1, :241-259
    votes = np.zeros(n_kf, np.int32)      # :238 frameCounter
    n_nulled = 0
    for i in range(n_cur):                # :241
        if st[i] == EMPTY:                # :244 pMP != NULL
            continue
        if g[i] < 0:                      # a point UpdateFrame created: no observations (:248-252 adds nothing)
            continue
        if bad is not None and bad[g[i]]:  # :246, :254-257
            st[i], g[i] = EMPTY, -1
            n_nulled += 1
            continue
        for kf in store["obs"][g[i]]:     # :248-252
            votes[kf] += 1
    # steps 1.2-1.3.1, :263-280
    local_kf, n_max, refer = [], 0, -1    # :263, :266-267
    for kf in range(n_kf):                # :268 std::map order = index order
        if votes[kf] == 0:                # not in the map
            continue
        if store["kf_bad"][kf]:           # :271-272
            continue
        if n_max < votes[kf]:             # :274 strict: the first of equals stays
            n_max, refer = int(votes[kf]), kf   # :276-277
        local_kf.append(kf)               # :279
    n_voted = len(local_kf)
    # the expansion, :282-307, as an index loop over the growing list (the reference iterates by
    # iterator while it push_backs)
    i = 0
    while i < len(local_kf):              # :282
        if len(local_kf) > 10:            # :285-286
            break
        for b in store["cov"][local_kf[i]][:10]:   # :291 GetBestCovisibleFrames(10), src/frame.cpp:735-741
            if store["kf_bad"][b]:        # :295
                continue
            if b not in local_kf:         # :298-299
                local_kf.append(b)        # :301
                break                     # :302
        i += 1
    # step 2, :315-336
    local = set()                         # :315
    for kf in local_kf:                   # :316
        for p in store["kf_slots"][kf]:   # :319-321
            if p < 0:                     # :324
                continue
            if bad is not None and bad[p]:  # :326
                continue
            local.add(int(p))             # :329-334
    l2g = sorted(local)                   # std::set order = index order
    n_local = len(l2g)
    out = dict(state=st, gid=g, votes=votes, local_kf=local_kf, refer_kf=refer, n_held=int((st != EMPTY).sum()),
               n_nulled=n_nulled, n_voted=n_voted, n_local=n_local, n_cur=n_cur)
    g2l = np.full(n_points, -1, np.int32)
    if n_local > max_local:
        out.update(status=2, l2g=[], g2l=g2l, slot_id=None, rows={})
        return out
    g2l[l2g] = np.arange(n_local, dtype=np.int32)
    sid = np.where((st != EMPTY) & (g >= 0), g2l[np.maximum(g, 0)] if n_points else -1, -1).astype(np.int32)
    rows = {k: np.asarray(store[k])[l2g] for k in COLS} if n_local else {}
    out.update(status=0, l2g=l2g, g2l=g2l, slot_id=sid, rows=rows)
    return out


def ids_back(state, slot_id, gid, l2g):
    """lorb_local_map_ids_back_dev: the gids after the local stage."""
    g = np.asarray(gid, np.int32).copy()
    for j in range(len(g)):
        if slot_id[j] >= 0:
            g[j] = l2g[slot_id[j]]
        elif state[j] == EMPTY:
            g[j] = -1
    return g
