"""Stores with geometry and life for lorb_kf_store_retire_dev: hand-written stores whose answers are written out in
tests/test_kf_retire_ref.py, and fabricated stores at the smallest sizes at which the call's kernels can go wrong.
tests/test_gpu_kf_retire.py checks the device against the restatement tests/kf_retire_ref.py on all of them.

A case is dict(store, geom, obs_slot, life, list, protect): store as tests/kf_store_cases.py builds it, geom as
lorb_slam_amd.frame.KeyframeStore takes it, life as tests/kf_cull_ref.py keeps it, list the keyframes to retire."""
import numpy as np

import kf_cull_cases as CC
import kf_cull_ref as L
import kf_store_cases as KC
import kf_store_ref as R

TILE = 1024  # points per tile, threads per workgroup and the longest list (kT in lorb_kfretire.hip)


def life_for(store, kf_fid=None):
    """The life create leaves, with mnId = index + 1 per keyframe unless kf_fid says otherwise."""
    nk = len(store["kf_bad"])
    life = L.new_life(nk, store["n_points"])
    life["kf_fid"] = np.arange(1, nk + 1, dtype=np.int32) if kf_fid is None else np.asarray(kf_fid, np.int32)
    life["frame_word"] = nk + 1
    return life


def build(n_kf, obs, conn=None, cov=None, is_bad=None, kf_bad=None, kf_fid=None, rows=None, lst=(), protect=(), seed=0):
    """A sound store from the observation lists: keyframe f's row holds the points that observe it in ascending order
    (or `rows`), every observation names the lowest slot that holds its point.  conn defaults to empty maps, cov to the
    ordered entries of weight 3 and more."""
    if rows is None:
        rows = [[p for p, o in enumerate(obs) if f in o] for f in range(n_kf)]
    conn = [{} for _ in range(n_kf)] if conn is None else conn
    cov = [R.ordered({f: w for f, w in c.items() if w >= 3}) for c in conn] if cov is None else cov
    s = KC.make_store(obs, [0] * n_kf if kf_bad is None else kf_bad, rows, cov, conn, is_bad=is_bad, seed=seed)
    g = CC.geometry_for(s, seed)
    return dict(store=s, geom=g, obs_slot=g["obs_slot"], life=life_for(s, kf_fid), list=list(lst), protect=list(protect))


def generated(n_points, n_kf, seed, lst, affected=(), protect=(), obs_per_point=4, conn_per_kf=6, all_good=False):
    """KC.random_store (asymmetric weight maps, a few bad keyframes and points) with geometry.  affected: points forced
    to observe lst[0] beside what they observe already."""
    s = KC.random_store(n_kf, n_points, seed, obs_per_point=obs_per_point, conn_per_kf=min(conn_per_kf, n_kf))
    if all_good:
        s["kf_bad"][:] = 0
    for f in lst:
        if 0 <= f < n_kf:
            s["kf_bad"][f] = 0
    for p in affected:
        s["obs"][p] = sorted(set(s["obs"][p]) | {lst[0]})
    s["kf_slots"] = [[p for p, o in enumerate(s["obs"]) if f in o] for f in range(n_kf)]
    g = CC.geometry_for(s, seed)
    return dict(store=s, geom=g, obs_slot=g["obs_slot"], life=life_for(s), list=list(lst), protect=list(protect))


def every_point_dies(n_points=1030, seed=21):
    """Every point observes keyframe 0 and at most two others: retiring 0 leaves no observation at all."""
    rng = np.random.default_rng(seed)
    obs = [[0] + sorted(rng.choice([1, 2, 3], size=int(rng.integers(0, 3)), replace=False).tolist()) for _ in range(n_points)]
    conn = [{1: 5, 2: 2}, {0: 5, 2: 4}, {0: 2, 1: 4}, {}]
    return build(4, obs, conn=conn, lst=[0], seed=seed)


def nobody_affected(seed=22):
    """The retired keyframe observes nothing and has an empty weight map: isolated."""
    c = generated(1100, 6, seed, lst=[5])
    s = c["store"]
    s["obs"] = [[f for f in o if f != 5] for o in s["obs"]]
    s["conn"] = [{f: w for f, w in m.items() if f != 5} for m in s["conn"]]
    s["conn"][5] = {}
    s["cov"] = [R.ordered({f: w for f, w in m.items() if w >= 3}) for m in s["conn"]]
    s["kf_slots"] = [[p for p, o in enumerate(s["obs"]) if f in o] for f in range(6)]
    s["kf_slots"][5] = [-1, -1, -1]
    g = CC.geometry_for(s, seed)
    return dict(c, geom=g, obs_slot=g["obs_slot"])


def long_point_list(n_lost, seed=23):
    """Point 1027 of 1030 is observed by 300 of 310 keyframes and loses n_lost of them; point 3 loses one."""
    V = [int(v) for v in np.linspace(0, 299, n_lost).round()]
    assert len(set(V)) == n_lost
    c = generated(1030, 310, seed, lst=V, affected=(3,), obs_per_point=3, conn_per_kf=4, all_good=True)
    s = c["store"]
    s["obs"][1027] = list(range(300))
    s["kf_slots"] = [[p for p, o in enumerate(s["obs"]) if f in o] for f in range(310)]
    g = CC.geometry_for(s, seed)
    return dict(c, geom=g, obs_slot=g["obs_slot"])


def long_slot_row(seed=24):
    """Keyframe 1 holds 1025 points (one of them twice, behind the others)."""
    rng = np.random.default_rng(seed)
    obs = [[1] + sorted(rng.choice([0, 2, 3, 4], size=int(rng.integers(1, 5)), replace=False).tolist()) for _ in range(1024)]
    obs = [sorted(o) for o in obs]
    rows = [[p for p, o in enumerate(obs) if f in o] for f in range(5)]
    rows[1].append(7)
    assert len(rows[1]) == TILE + 1
    return build(5, obs, conn=[{1: 9}, {0: 9, 2: 1}, {1: 1}, {}, {}], rows=rows, lst=[1], seed=seed)


def long_weight_row(seed=25):
    """Keyframe 1029 of 1030 (max_kf 1100) has the keys 0 .. 1024 in its weight map and loses its first, its last and
    one in the middle; every one of them names it back."""
    n = 1030
    conn = [{} for _ in range(n)]
    rng = np.random.default_rng(seed)
    conn[1029] = {f: int(rng.integers(1, 9)) for f in range(1025)}
    for f in (0, 512, 1024):
        conn[f] = {1029: conn[1029][f]}
    conn[3] = {1029: 2}  # named by a keyframe that is not retired
    obs = [[0, 1, 2, 1029], [512, 1029], [1024, 5, 6, 7, 8]]
    c = build(n, obs, conn=conn, lst=[0, 512, 1024], seed=seed)
    c["max_kf"] = 1100
    return c


def long_list(n, n_kf=40, seed=26):
    """A list of n entries over a store of n_kf keyframes: duplicates, entries outside the store, bad keyframes,
    keyframes with kf_fid 0 and protected ones mixed in."""
    rng = np.random.default_rng(seed + n)
    lst = [int(v) for v in rng.integers(-3, n_kf + 3, n)] if n > 1 else [7]
    c = generated(600, n_kf, seed, lst=[7], affected=(0, 599))
    c["store"]["kf_bad"][[2, 11]] = 1
    c["life"]["kf_fid"][[0, 9, 11]] = 0
    return dict(c, list=lst, protect=[5, 9, 2, n_kf + 1])


def cases():
    c = {}
    for n in (1023, 1024, 1025):                                       # the first and the last point
        c[f"points_{n}"] = generated(n, 6, seed=n, lst=[2, 4], affected=(0, 5, n // 2, n - 1))
    c["points_2049_tile_edges"] = generated(2 * TILE + 1, 5, seed=7, lst=[1], affected=(0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE))
    c["every_point_dies"] = every_point_dies()
    c["nobody_affected"] = nobody_affected()
    for k in (1, 150, 298):
        c[f"point_of_300_loses_{k}"] = long_point_list(k)
    c["slot_row_1025"] = long_slot_row()
    c["weight_row_1025"] = long_weight_row()
    c["list_of_1"] = long_list(1)
    c["list_of_1024"] = long_list(1024)
    return c
