"""Hand-built stores and frames for the keyframe insertion, each with the answer written out by hand (`want`):
tests/test_kf_store_ref.py checks the restatement (tests/kf_store_ref.py) against these answers on the CPU,
tests/test_gpu_kf_store.py checks the device against the restatement.  size_cases() are generated stores at the
sizes that cross the kernels' limits; they have no hand answer.

A case is dict(store, caps, fp, frame, pose, slots, gid, n_cur, n_max_cur, gate, want).  `want` holds only what
was worked out by hand; keys: the record's fields, and gid, state, row (K's slot row), obs, cov, conn, locked."""
import numpy as np

import kf_store_ref as R
from lorb_slam_amd import synth

EMPTY, FREE, LOCKED = R.EMPTY, R.FREE, R.LOCKED
NO = -1.0  # a keypoint without depth


def make_store(obs, kf_bad, kf_slots, cov, conn, is_bad=None, seed=0):
    rng = np.random.default_rng(2000 + seed)
    n = len(obs)
    assert len(kf_slots) == len(cov) == len(conn) == len(kf_bad)
    return dict(n_points=n, obs=[list(o) for o in obs], kf_bad=np.asarray(kf_bad, np.uint8), kf_slots=[list(s) for s in kf_slots],
                cov=[list(c) for c in cov], conn=[dict(c) for c in conn],
                is_bad=np.zeros(n, np.uint8) if is_bad is None else np.asarray(is_bad, np.uint8),
                pos=rng.normal(size=(n, 3)).astype(np.float32), normal=rng.normal(size=(n, 3)).astype(np.float32),
                max_dist=rng.uniform(5, 9, n).astype(np.float32), min_dist=rng.uniform(1, 2, n).astype(np.float32),
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), locked=rng.integers(0, 2, n).astype(np.uint8))


def pose_block():
    """Twc of a camera turned 0.1 rad about y, centre (0.3, -0.2, 1.5): all the insertion reads of a pose."""
    c, s = np.float32(np.cos(0.1)), np.float32(np.sin(0.1))
    Twc = np.array([[c, 0, s, 0.3], [0, 1, 0, -0.2], [-s, 0, c, 1.5], [0, 0, 0, 1]], np.float32)
    return dict(Twc=Twc.reshape(16), status=0)


def case(store, state, gid, want, depth=None, caps=None, gate=R.GATE_RATIO, seed=0, slack=3):
    """A frame of len(state) keypoints; depth defaults to none anywhere.  Capacities default to what the insertion
    needs plus `slack` rows, so that there is room behind every count for sentinel bytes."""
    rng = np.random.default_rng(3000 + seed)
    n = len(state)
    fp = synth.frame_params()
    depth = np.full(n, NO, np.float32) if depth is None else np.asarray(depth, np.float32)
    frame = dict(x=rng.uniform(0, float(fp["max_x"]), n).astype(np.float32), y=rng.uniform(0, float(fp["max_y"]), n).astype(np.float32),
                 depth=depth, octave=rng.integers(0, fp["n_levels"], n).astype(np.int32),
                 desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    slots = dict(state=np.asarray(state, np.uint8), pos=(rng.normal(size=(n, 3)) * 4 + [0, 0, 9]).astype(np.float32),
                 desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    c = R.counts(store)
    if caps is None:
        caps = dict(max_kf=c["n_kf"] + 1 + slack, max_points=c["n_points"] + n + slack, max_obs=c["n_obs"] + n + slack,
                    max_kf_slots=c["n_kf_slots"] + n + 1 + slack)
    return dict(store=store, caps=caps, fp=fp, frame=frame, pose=pose_block(), slots=slots, gid=np.asarray(gid, np.int32), n_cur=n,
                n_max_cur=n + 1, gate=gate, want=want)


def held(gids, n, state=LOCKED):
    """n slots: the first len(gids) hold those points, the rest are EMPTY."""
    return [state] * len(gids) + [EMPTY] * (n - len(gids)), list(gids) + [-1] * (n - len(gids))


def gate_cases():
    """7 of 20 held: (float)7 / (float)20 is the float 0.35f itself, not above it -> inserted.  8 of 20 -> refused.
    Eight points seen by kf0; the held ones take K = 1: the counter gives kf0 the weight 7."""
    def store():
        return make_store([[0]] * 8, [0], [list(range(8))], [[]], [{}], seed=1)
    st, g = held(range(7), 20)
    yes = case(store(), st, g, dict(status=0, inserted=1, n_cur=20, n_map=7, kf=1, n_observed=7, n_adopted=0, n_created=0,
                                    n_connected=1, n_points=8, n_kf=2, n_obs=15, row=list(range(7)) + [-1] * 13,
                                    obs=[[0, 1]] * 7 + [[0]], cov=[[1], [0]], conn=[{1: 7}, {0: 7}]), seed=1)
    st, g = held(range(8), 20)
    no = case(store(), st, g, dict(status=0, inserted=0, n_map=8), seed=2)
    return dict(gate_7_of_20=yes, gate_8_of_20=no)


def empty_frame_case():
    """n_cur = 0: the ratio is NaN, the comparison false -> an empty keyframe with no connection."""
    s = make_store([[0]], [0], [[0]], [[]], [{}], seed=3)
    return case(s, [], [], dict(status=0, inserted=1, n_cur=0, n_map=0, kf=1, n_observed=0, n_adopted=0, n_created=0,
                                n_connected=0, n_points=1, n_kf=2, n_obs=1, row=[], obs=[[0]], cov=[[], []], conn=[{}, {}]), seed=3)


def two_slots_case():
    """p0 sits in slots 0 and 1: ONE observation, but the counter takes it per slot -> kf0 = 2 (p0) + 1 (p2) = 3,
    kf1 = 1 (p2).  kf0 enters the pairs; its map {1: 1} takes {2: 3} and its list is rebuilt [1, 2]."""
    s = make_store([[0], [1], [0, 1]], [0, 0], [[0, 2], [1, 2]], [[1], [0]], [{1: 1}, {0: 1}], seed=4)
    return case(s, [LOCKED, FREE, LOCKED] + [EMPTY] * 6, [0, 0, 2] + [-1] * 6,
                dict(status=0, inserted=1, n_map=3, kf=2, n_observed=2, n_connected=1, n_points=3, n_kf=3, n_obs=6,
                     obs=[[0, 2], [1], [0, 1, 2]], cov=[[1, 2], [0], [0]], conn=[{1: 1, 2: 3}, {0: 1}, {0: 3, 1: 1}],
                     state=[LOCKED] * 3 + [EMPTY] * 6, row=[0, 0, 2] + [-1] * 6), seed=4)


def held_bad_case():
    """Slot 1 holds bad p1: nothing is added, slot, gid and K's row keep it.  p0 gives kf0 the count 1: no pair, so
    the largest-count fallback connects K and kf0 with weight 1."""
    s = make_store([[0], [0]], [0], [[0, 1]], [[]], [{}], is_bad=[0, 1], seed=5)
    return case(s, [LOCKED, FREE] + [EMPTY] * 4, [0, 1, -1, -1, -1, -1],
                dict(status=0, inserted=1, n_map=2, kf=1, n_observed=1, n_adopted=0, n_created=0, n_connected=1, n_points=2,
                     n_obs=3, obs=[[0, 1], [0]], cov=[[1], [0]], conn=[{1: 1}, {0: 1}], state=[LOCKED, FREE] + [EMPTY] * 4,
                     gid=[0, 1, -1, -1, -1, -1], row=[0, 1, -1, -1, -1, -1]), seed=5)


def gid_outside_case(caps=None, want=None):
    """Slot 0 holds gid 7, outside a store of 2 points: counts as -1 -> adopted (point 2), as is slot 1 (gid -1,
    point 3); slot 2 is EMPTY with depth -> created (point 4); slot 3 is EMPTY without depth but carries a stale
    gid, which becomes -1; slot 4 holds p1 (observed).  kf0 sees p1: count 1 -> the fallback."""
    s = make_store([[0], [0]], [0], [[0, 1]], [[]], [{}], seed=6)
    want = want or dict(status=0, inserted=1, n_cur=9, n_map=3, kf=1, n_observed=1, n_adopted=2, n_created=1, n_connected=1,
                        n_points=5, n_kf=2, n_obs=6, gid=[2, 3, 4, -1, 1, -1, -1, -1, -1], row=[2, 3, 4, -1, 1, -1, -1, -1, -1],
                        state=[LOCKED] * 3 + [EMPTY, LOCKED] + [EMPTY] * 4, obs=[[0], [0, 1], [1], [1], [1]],
                        cov=[[1], [0]], conn=[{1: 1}, {0: 1}])
    return case(s, [LOCKED, FREE, EMPTY, EMPTY, FREE] + [EMPTY] * 4, [7, -1, 0, 1, 1, -1, -1, -1, -1], want,
                depth=[NO, 3.0, 5.0, NO, NO, NO, NO, NO, NO], caps=caps, seed=6)


def capacity_cases():
    """The frame of gid_outside needs 2 keyframes, 5 points, 6 observations and 2 + 9 slots: each capacity one short
    of that is status 2 with the counts found and nothing written; all four exact is fine."""
    need = dict(max_kf=2, max_points=5, max_obs=6, max_kf_slots=11)
    full = dict(status=2, inserted=0, n_cur=9, n_map=3, kf=-1, n_observed=1, n_adopted=2, n_created=1, n_connected=0,
                n_points=2, n_kf=1, n_obs=2)
    out = dict(cap_exact=gid_outside_case(caps=dict(need)))
    for k in need:
        out["cap_" + k] = gid_outside_case(caps=dict(need, **{k: need[k] - 1}), want=full)
    return out


def weights_case():
    """Counts kf0 = 2, kf1 = 3, kf2 = 3: the pairs are kf1 and kf2, ordered by index on the tie; kf0 stays in K's
    weight map only, and its own map and list are not touched."""
    s = make_store([[0], [0], [1], [1], [1], [2], [2], [2]], [0, 0, 0], [[0, 1], [2, 3, 4], [5, 6, 7]], [[], [], []], [{}, {}, {}],
                   seed=7)
    st, g = held(range(8), 23)
    return case(s, st, g, dict(status=0, inserted=1, n_map=8, kf=3, n_observed=8, n_connected=2, cov=[[], [3], [3], [1, 2]],
                               conn=[{}, {3: 3}, {3: 3}, {0: 2, 1: 3, 2: 3}], n_obs=16), seed=7)


def fallback_case():
    """Counts kf0 = 1, kf1 = 2, kf2 = 2: none reaches 3; the first keyframe with the strictly largest count (kf1)
    gets the one connection, weight 2.  kf1's map {0: 4} becomes {0: 4, 3: 2}: list [3, 0]."""
    s = make_store([[0], [1, 2], [1, 2]], [0, 0, 0], [[0], [1, 2], [1, 2]], [[1], [0], []], [{1: 4}, {0: 4}, {}], seed=8)
    st, g = held(range(3), 9)
    return case(s, st, g, dict(status=0, inserted=1, n_map=3, kf=3, n_observed=3, n_connected=1, cov=[[1], [3, 0], [], [1]],
                               conn=[{1: 4}, {0: 4, 3: 2}, {}, {0: 1, 1: 2, 2: 2}]), seed=8)


def below3_case():
    """kf0's map {1: 2, 2: 5} had the list [2] (its own UpdateConnections left the 2 out).  K = 3 joins with weight
    3: AddConnection rebuilds the list from ALL of the map -> [1, 3, 2]."""
    s = make_store([[0], [0], [0]], [0, 0, 0], [[0, 1, 2], [], []], [[2], [], [0]], [{1: 2, 2: 5}, {0: 2}, {0: 5}], seed=9)
    st, g = held(range(3), 9)
    return case(s, st, g, dict(status=0, inserted=1, kf=3, n_connected=1, cov=[[1, 3, 2], [], [0], [0]],
                               conn=[{1: 2, 2: 5, 3: 3}, {0: 2}, {0: 5}, {0: 3}]), seed=9)


def empty_store_case():
    """Initialize: an empty store under LORB_KF_GATE_NONE.  Slots with depth >= 0 (0.0 included: the origin) are
    created in slot order; the keyframe has nobody to connect to."""
    return case(R.empty_store(), [EMPTY] * 5, [-1] * 5,
                dict(status=0, inserted=1, n_cur=5, n_map=0, kf=0, n_observed=0, n_adopted=0, n_created=4, n_connected=0,
                     n_points=4, n_kf=1, n_obs=4, gid=[0, -1, 1, 2, 3], row=[0, -1, 1, 2, 3], obs=[[0]] * 4, cov=[[]], conn=[{}],
                     state=[LOCKED, EMPTY, LOCKED, LOCKED, LOCKED], locked=[1, 1, 1, 1]),
                depth=[1.0, NO, 2.5, 0.0, 3.0], gate=R.GATE_NONE, seed=10)


def all_cases():
    c = dict(empty_frame=empty_frame_case(), two_slots=two_slots_case(), held_bad=held_bad_case(), gid_outside=gid_outside_case(),
             weights_2_3_3=weights_case(), fallback_largest=fallback_case(), below3_enters=below3_case(),
             empty_store_none=empty_store_case())
    c.update(gate_cases())
    c.update(capacity_cases())
    return c


# -- four frames behind one another, from an empty store (tests/test_gpu_kf_store_chain.py) ----------------------------
CHAIN_CAPS = dict(max_kf=6, max_points=80, max_obs=120, max_kf_slots=100)
CHAIN_N_MAX = 31  # one bound for every frame


def chain_frames():
    """The four frames, worked out by hand (the store's indices are deterministic):
       0  LORB_KF_GATE_NONE, 12 keypoints, 10 with depth            -> K = 0, points 0-9
       1  holds p0-p4 and one created point (6 of 20 <= 0.35), 4 keypoints with depth
                                                                     -> K = 1, point 10 adopted, 11-14 created; kf0: 5
       2  5 of 10 held                                               -> refused
       3  holds p0, p1, p2, p10-p13 and p2 again, 2 created points (10 of 30), 5 with depth
                                                                     -> K = 2; kf0: 4, kf1: 8 (p2 counts twice)"""
    def frame(state, gid, depth, gate, seed):
        c = case(R.empty_store(), state, gid, {}, depth=depth, caps=CHAIN_CAPS, gate=gate, seed=seed)
        c["n_max_cur"] = CHAIN_N_MAX
        return c

    d0 = [1.0 + j for j in range(10)] + [NO, NO]
    f0 = frame([EMPTY] * 12, [-1] * 12, d0, R.GATE_NONE, 40)
    f1 = frame([LOCKED] * 5 + [FREE] + [EMPTY] * 14, [0, 1, 2, 3, 4, -1] + [-1] * 14, [NO] * 6 + [2.0, 3.0, 4.0, 5.0] + [NO] * 10,
               R.GATE_RATIO, 41)
    f2 = frame([LOCKED] * 5 + [EMPTY] * 5, [5, 6, 7, 8, 9] + [-1] * 5, [NO] * 5 + [1.0] * 5, R.GATE_RATIO, 42)
    f3 = frame([LOCKED] * 8 + [FREE] * 2 + [EMPTY] * 20, [0, 1, 2, 10, 11, 12, 13, 2, -1, -1] + [-1] * 20,
               [NO] * 10 + [6.0, 7.0, 8.0, 9.0, 10.0] + [NO] * 15, R.GATE_RATIO, 43)
    return [f0, f1, f2, f3]


def chain_restate(fs):
    """The restatement applied to the frames in turn -> the results, each on the store the one before left."""
    s, out = R.empty_store(), []
    for c in fs:
        r = R.insert_keyframe(s, CHAIN_CAPS, c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], CHAIN_N_MAX, c["gate"])
        out.append(r)
        s = r["store"]
    return out


# -- generated stores at the kernels' limits -------------------------------------------------------------------------
def random_store(n_kf, n_points, seed, obs_per_point=3, conn_per_kf=6):
    rng = np.random.default_rng(4000 + seed)
    obs = [sorted(rng.choice(n_kf, size=min(n_kf, int(rng.integers(0, obs_per_point + 1))), replace=False).tolist())
           for _ in range(n_points)]
    slots = [[] for _ in range(n_kf)]
    for p, o in enumerate(obs):
        for k in o:
            slots[k].append(p)
    conn = []
    for k in range(n_kf):
        others = [f for f in rng.choice(n_kf, size=min(n_kf, conn_per_kf), replace=False).tolist() if f != k]
        conn.append({int(f): int(rng.integers(1, 9)) for f in others})
    cov = [R.ordered({f: w for f, w in c.items() if w >= 3}) for c in conn]
    is_bad = (rng.uniform(size=n_points) < 0.05).astype(np.uint8)
    return make_store(obs, (rng.uniform(size=n_kf) < 0.1).astype(np.uint8), slots, cov, conn, is_bad=is_bad, seed=seed)


def size_cases(walk, tile, window, wave=64):
    """walk: threads of the slot walk; tile: points per scan tile; window: keyframes per counter window.
       walk_plus:   n_cur = walk + 6 slots of every kind, held points repeated
       two_tiles:   n_points = 2 * tile + 3, held points on both sides of both tile borders
       window_plus: n_kf = window + 1; observers in the first and the second counter window; one neighbour whose
                    weight map has wave + 6 entries and one with every other keyframe (window entries: with K more than
                    one key per thread of the sort)"""
    out = {}
    rng = np.random.default_rng(77)
    # walk_plus
    n = walk + 6
    s = random_store(12, 900, seed=20)
    state = rng.choice([EMPTY, FREE, LOCKED], size=n, p=[0.7, 0.1, 0.2]).astype(np.uint8)
    gid = np.where(rng.uniform(size=n) < 0.8, rng.integers(0, 300, n), -1).astype(np.int32)
    depth = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0.5, 30, n), NO).astype(np.float32)
    out["walk_plus"] = case(s, state, gid, {}, depth=depth, seed=20)
    # two_tiles
    P = 2 * tile + 3
    s = random_store(5, P, seed=21)
    s["is_bad"][:] = 0
    pts = [0, 5, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 2, 5, tile]
    st, g = held(pts, 40)
    dp = np.full(40, NO, np.float32)
    dp[20:24] = [2.0, 7.5, 0.0, 11.0]
    out["two_tiles"] = case(s, st, g, {}, depth=dp, seed=21)
    # window_plus
    nk = window + 1
    s = random_store(nk, 60, seed=22, conn_per_kf=3)
    s["is_bad"][:] = 0
    s["kf_bad"][:] = 0
    for p in range(12):  # the held points: seen from both windows, kf3 and the last keyframe by at least three
        s["obs"][p] = sorted(set([3, window - 1, window] + s["obs"][p][:1]))
    s["conn"][3] = {int(f): int(rng.integers(1, 9)) for f in range(10, 10 + wave + 6)}
    s["conn"][window] = {int(f): int(rng.integers(1, 40)) for f in range(window)}
    st, g = held(range(12), 40)
    out["window_plus"] = case(s, st, g, {}, seed=22)
    return out
