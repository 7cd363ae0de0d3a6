"""Stores with geometry and life for the map-point culling on the keyframe store: the hand case with its answer written
out in tests/test_kf_cull_ref.py, generated stores at the sizes where the cull's kernels change path, fabricated
inputs for the observe call, and the chain scene.  tests/test_gpu_kf_cull.py checks the device against the
restatement tests/kf_cull_ref.py on all of them.

A cull case is dict(store, geom, obs_slot, life, kf, params, frame): store as tests/kf_store_cases.py builds it, geom
as lorb_slam_amd.frame.KeyframeStore takes it, frame = dict(n_cur, n_max_cur, state, gid) or None."""
import numpy as np

import kf_cull_ref as L
import kf_store_cases as KC
import kf_store_ref as R

F = np.float32
EMPTY, FREE, LOCKED = R.EMPTY, R.FREE, R.LOCKED
TILE = 1024  # points per tile of the cull's kernels (kT in lorb_kfcull.hip)


def geometry_for(store, seed=0):
    """A geometry that keeps the invariant: every observation (p, f) names the lowest slot of f that holds p; a
    keyframe that observes p without holding it gets a slot appended.  Poses and keypoints are random."""
    rng = np.random.default_rng(8000 + seed)
    slots = [list(r) for r in store["kf_slots"]]
    where = [{} for _ in slots]
    for f, r in enumerate(slots):
        for j, p in enumerate(r):
            where[f].setdefault(p, j)
    obs_slot = []
    for p, obs in enumerate(store["obs"]):
        row = []
        for f in obs:
            if p not in where[f]:
                where[f][p] = len(slots[f])
                slots[f].append(p)
            row.append(where[f][p])
        obs_slot.append(row)
    store["kf_slots"] = slots
    nk = len(slots)
    return dict(kf_pose=list((rng.normal(size=(nk, 6)) * 0.1).astype(F)),
                kf_slot_uv=[rng.uniform(0, 700, (len(r), 2)).astype(F) for r in slots], obs_slot=obs_slot)


def hand_case():
    """Four keyframes with frame ids 0, 1, 2, 5; the cull runs for kf 3, so cur = 5.  Seven points:
         p0  in the list, already bad                                  -> leaves the list
         p1  found / visible = 1 / 5, age 5, one observation           -> culled, counted as ratio
         p2  1 / 4 (kept by the ratio), age 2 = age_obs, two obs < 3   -> culled by the observation rule
         p3  age 1 = age_obs - 1, one observation                      -> stays
         p4  age 3 = age_out, three observations                       -> leaves the list
         p5  age 2 = age_out - 1, three observations                   -> stays
         p6  not in the list (1 / 100): not examined
       rows: kf0 = [0, 1, 2, 4, 5, 6], kf1 = [2, 4, 5], kf2 = [4, 5], kf3 = [3, 6].
       The tracker's frame holds p1, p0, p2, p5, a created point and an index outside the store."""
    obs = [[0], [0], [0, 1], [3], [0, 1, 2], [0, 1, 2], [0, 3]]
    obs_slot = [[0], [1], [2, 0], [0], [3, 1, 0], [4, 2, 1], [5, 1]]
    rows = [[0, 1, 2, 4, 5, 6], [2, 4, 5], [4, 5], [3, 6]]
    store = KC.make_store(obs, [0, 0, 0, 0], rows, [[1], [0], [], []], [{1: 3}, {0: 3}, {}, {}], is_bad=[1, 0, 0, 0, 0, 0, 0], seed=70)
    rng = np.random.default_rng(70)
    geom = dict(kf_pose=list((rng.normal(size=(4, 6)) * 0.1).astype(F)),
                kf_slot_uv=[rng.uniform(0, 700, (len(r), 2)).astype(F) for r in rows], obs_slot=obs_slot)
    life = dict(visible=np.array([1, 5, 4, 1, 1, 1, 100], np.int32), found=np.ones(7, np.int32),
                first_fid=np.array([0, 0, 3, 4, 2, 3, 0], np.int32), recent=np.array([1, 1, 1, 1, 1, 1, 0], np.uint8),
                kf_fid=np.array([0, 1, 2, 5], np.int32), frame_word=5)
    frame = dict(n_cur=6, n_max_cur=8, state=np.array([LOCKED, LOCKED, FREE, LOCKED, FREE, LOCKED], np.uint8),
                 gid=np.array([1, 0, 2, 5, -1, 9], np.int32))
    return dict(store=store, geom=geom, obs_slot=obs_slot, life=life, kf=3, params=L.REFERENCE, frame=frame)


def generated(n_points, n_kf, seed, cull=(), all_culled=False, none_culled=False, long_list=None, n_cur=40, params=L.REFERENCE,
              obs_per_point=3):
    """KC.random_store with geometry and a random life.  cull: points forced to fail the ratio (in the list, not bad,
    1 / 9); long_list = (p, n): point p observed by the first n keyframes; the frame's slots hold culled points,
    points that are bad already, other points, created points and indices outside the store."""
    rng = np.random.default_rng(9000 + seed)
    s = KC.random_store(n_kf, n_points, seed, obs_per_point=obs_per_point, conn_per_kf=min(6, n_kf))
    if long_list:
        s["obs"][long_list[0]] = list(range(long_list[1]))
    g = geometry_for(s, seed)
    cur = 50
    life = dict(visible=rng.integers(1, 7, n_points).astype(np.int32), found=rng.integers(1, 3, n_points).astype(np.int32),
                first_fid=(cur - rng.integers(0, 5, n_points)).astype(np.int32), recent=(rng.uniform(size=n_points) < 0.5).astype(np.uint8),
                kf_fid=np.sort(rng.integers(0, cur, n_kf)).astype(np.int32), frame_word=cur)
    life["kf_fid"][-1] = cur
    if all_culled:
        s["is_bad"][:] = 0
        cull = range(n_points)
    if none_culled:
        life["visible"][:], life["found"][:], life["first_fid"][:] = 1, 1, cur
    for p in cull:
        s["is_bad"][p], life["recent"][p], life["visible"][p], life["found"][p] = 0, 1, 9, 1
    bad = [int(p) for p in np.nonzero(s["is_bad"])[0][:5]]
    want = [int(p) for p in list(cull)[:12]] + bad + [int(p) for p in rng.integers(0, n_points, 12)]
    gid = np.full(n_cur, -1, np.int32)
    state = np.full(n_cur, EMPTY, np.uint8)
    at = rng.permutation(n_cur)[:min(len(want), n_cur)]
    gid[at] = want[:len(at)]
    state[at] = LOCKED
    rest = np.setdiff1d(np.arange(n_cur), at)
    gid[rest[::3]] = n_points + 4          # outside the store
    state[rest[1::3]] = FREE               # a created point, gid -1
    frame = dict(n_cur=n_cur, n_max_cur=n_cur + 5, state=state, gid=gid)
    return dict(store=s, geom=g, obs_slot=g["obs_slot"], life=life, kf=n_kf - 1, params=params, frame=frame)


def cull_cases():
    """The sizes at which the kernels take another path (1024 points per tile), and the edges of the lists."""
    c = dict(hand=hand_case())
    for n in (1023, 1024, 1025):
        c[f"points_{n}"] = generated(n, 6, seed=n, cull=(0, 5, n // 2, n - 1))                      # the first and the last point
    c["points_2049_tile_edge"] = generated(2 * TILE + 1, 2, seed=7, cull=(TILE - 1, TILE, 2 * TILE - 1, 2 * TILE),
                                           n_cur=TILE + 1)                                          # both sides of a tile edge
    c["all_culled"] = generated(1030, 4, seed=8, all_culled=True)
    c["none_culled"] = generated(1100, 5, seed=9, none_culled=True)
    c["obs_300"] = generated(1030, 310, seed=10, cull=(3, 1027), long_list=(1027, 300))
    c["other_params"] = generated(300, 5, seed=11, cull=(7,), params=(0.5, 1, 2, 4))
    c["no_frame"] = dict(generated(200, 4, seed=12, cull=(0, 199)), frame=None)
    return c


def observe_cases():
    """Fabricated inputs of lorb_kf_store_observe_dev on a store of 1500 points (life as create leaves it): n_cur and
    n_local on both sides of the 1024 threads of the walk, a point in two slots, gids and local rows outside the
    store, local ids outside the local rows."""
    out = {}
    P = 1500
    for n_cur, n_local in ((1023, 1025), (1024, 1024), (1025, 1023), (7, 3)):
        rng = np.random.default_rng(100 + n_cur)
        gid = rng.integers(-1, P + 3, n_cur).astype(np.int32)   # -1, P .. P + 2: outside
        gid[1] = gid[0] = 5                                     # a point in two slots
        state = rng.choice([EMPTY, FREE, LOCKED], size=n_cur).astype(np.uint8)
        state[:2] = LOCKED
        lid = rng.integers(-1, n_local + 2, n_cur).astype(np.int32)
        l2g = rng.integers(0, P + 2, n_local).astype(np.int32)
        l2g[-1] = P + 1
        in_view = (rng.uniform(size=n_local) < 0.6).astype(np.uint8)
        in_view[-1] = 1
        out[f"cur_{n_cur}_local_{n_local}"] = dict(n_points=P, frame_id=1000 + n_cur, n_cur=n_cur, n_max_cur=n_cur + 3, state=state,
                                                   gid=gid, lid=lid, l2g=l2g, n_local=n_local, max_local=n_local + 2, in_view=in_view)
    return out


# -- the chain: keyframe K1 creates points, two frames see some of them, K2 is inserted, culled and adjusted ----------
CHAIN_PARAMS = (0.25, 2, 2, 3)  # min_obs = 2: a created point K2 holds again has the two observations it needs
N_CREATED = 12


def chain_frames(sc):
    """sc: tests/kf_ba_cases.chain_scene().  -> (k1, k2, caps): two tests/kf_store_cases.py cases under
    LORB_KF_GATE_NONE on sc's store.  K1 (frame id 20) holds six old points and creates c0 .. c11 = P .. P + 11.
    Frames 21 and 22 hold c0 .. c5 in their slots and see c0, c1 among the local points as well.  K2 (frame id 24,
    sc's frame) holds c0 .. c5 behind its own slots and sees c0, c1 in the same way.  At K2's cull, under CHAIN_PARAMS:
       c0, c1    visible 1 + 3 * 2 = 7 (held and in view), found 1        -> culled by the ratio
       c2 .. c5  visible 1 + 2 + 1 = 4 (1 / 4 is kept), two observations, age 4 -> leave the list, alive
       c6 .. c11 never seen again: age 4, one observation                -> culled by the observation rule"""
    store, c2 = sc["store"], sc["case"]
    P = store["n_points"]
    old = [p for p in range(P) if not store["is_bad"][p] and store["obs"][p]][:6]
    n1 = len(old) + N_CREATED + 2
    k1 = KC.case(store, [LOCKED] * len(old) + [EMPTY] * (N_CREATED + 2), old + [-1] * (N_CREATED + 2), {},
                 depth=[KC.NO] * len(old) + [2.0 + j for j in range(N_CREATED)] + [KC.NO, KC.NO], gate=R.GATE_NONE, seed=80)
    created = list(range(P, P + N_CREATED))
    n2 = c2["n_cur"]
    rng = np.random.default_rng(81)
    k2 = dict(c2)
    k2["frame"] = {k: np.concatenate([v, rng.uniform(0, 500, (6,) + v.shape[1:]).astype(v.dtype)]) for k, v in c2["frame"].items()}
    k2["frame"]["depth"][n2:] = KC.NO
    k2["frame"]["octave"][n2:] = 0
    k2["slots"] = dict(state=np.concatenate([c2["slots"]["state"], np.full(6, LOCKED, np.uint8)]),
                       pos=np.concatenate([c2["slots"]["pos"], rng.normal(size=(6, 3)).astype(F)]),
                       desc=np.concatenate([c2["slots"]["desc"], rng.integers(0, 256, (6, 32), dtype=np.uint8)]))
    k2["gid"] = np.concatenate([c2["gid"], np.asarray(created[:6], np.int32)])
    k2["n_cur"], k2["n_max_cur"] = n2 + 6, n2 + 9
    cn = R.counts(store)
    caps = dict(max_kf=cn["n_kf"] + 4, max_points=P + N_CREATED + n2 + 20, max_obs=cn["n_obs"] + n1 + n2 + 40,
                max_kf_slots=cn["n_kf_slots"] + n1 + n2 + 30)
    k1["caps"] = k2["caps"] = caps
    seen = dict(n_points=None, n_cur=6, n_max_cur=8, state=np.full(6, LOCKED, np.uint8), gid=np.asarray(created[:6], np.int32),
                lid=np.full(6, -1, np.int32), l2g=np.asarray(created[:2] + [0], np.int32), n_local=3, max_local=16,
                in_view=np.array([1, 1, 0], np.uint8))
    return k1, k2, caps, seen, created
