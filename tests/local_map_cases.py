"""Hand-built map stores and frames for UpdateLocalMap, each with the answer written out by hand
(`want`): tests/test_local_map_ref.py checks the restatement (tests/local_map_ref.py) against these
answers on the CPU, tests/test_gpu_local_map.py checks the device against the restatement.

A case is dict(store, state, gid, n_cur, max_local, ids, want).  `want` holds only what was worked out
by hand; keys: status, votes, local_kf, refer_kf, n_voted, n_held, n_nulled, l2g, slot_id, state, gid."""
import numpy as np

EMPTY, FREE, LOCKED = 0, 1, 2
UNCHANGED, NULL = -1, -2


def make_store(n_points, obs, kf_bad, kf_slots, cov, is_bad=None, seed=0):
    rng = np.random.default_rng(1000 + seed)
    n = n_points
    assert len(obs) == n and len(kf_slots) == len(cov) == len(kf_bad)
    return dict(n_points=n, obs=[list(o) for o in obs], kf_bad=np.asarray(kf_bad, np.uint8),
                kf_slots=[list(s) for s in kf_slots], cov=[list(c) for c in cov],
                is_bad=None if is_bad is None else np.asarray(is_bad, np.uint8),
                pos=rng.normal(size=(n, 3)).astype(np.float32), normal=rng.normal(size=(n, 3)).astype(np.float32),
                max_dist=rng.uniform(5, 9, n).astype(np.float32), min_dist=rng.uniform(1, 2, n).astype(np.float32),
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), locked=rng.integers(0, 2, n).astype(np.uint8))


def case(store, state, gid, want, max_local=None, ids=None, n_cur=None):
    n_cur = len(state) if n_cur is None else n_cur
    return dict(store=store, state=np.asarray(state, np.uint8), gid=np.asarray(gid, np.int32), n_cur=n_cur,
                max_local=max(store["n_points"], 1) if max_local is None else max_local, ids=ids, want=want)


def votes_case():
    """1: kf1 and kf3 tie at 2 votes -> the first index (kf1) is pFMax; kf2 has the most votes (4) but is
    bad: skipped, never pFMax.  p4 has no observations, p5 is not held."""
    obs = [[0, 1, 2], [1, 2, 3], [2, 3], [2], [], [4]]
    s = make_store(6, obs, [0, 0, 1, 0, 0], [[0, -1, 5], [5, 1], [3], [], [2]], [[]] * 5, seed=1)
    return case(s, [LOCKED, FREE, LOCKED, LOCKED, FREE], [0, 1, 2, 3, 4],
                dict(status=0, votes=[1, 2, 4, 2, 0], local_kf=[0, 1, 3], refer_kf=1, n_voted=3, n_held=5, n_nulled=0,
                     l2g=[0, 1, 5], slot_id=[0, 1, -1, -1, -1]))


def bad_point_case():
    """2: slot 1 holds bad p1 -> nulled, no vote.  Slot 2 is EMPTY (its gid is not looked at), slot 3 holds a
    created point (gid -1), slot 5 a gid outside the store (counts as -1)."""
    s = make_store(4, [[0], [0, 1], [1], [1]], [0, 0], [[0, 1], [2, -1, 3]], [[], []], is_bad=[0, 1, 0, 0], seed=2)
    return case(s, [LOCKED, FREE, EMPTY, LOCKED, FREE, LOCKED], [0, 1, 2, -1, 2, 7],
                dict(status=0, votes=[1, 1], local_kf=[0, 1], refer_kf=0, n_voted=2, n_held=4, n_nulled=1, l2g=[0, 2, 3],
                     slot_id=[0, -1, -1, -1, 1, -1], state=[LOCKED, EMPTY, EMPTY, LOCKED, FREE, LOCKED],
                     gid=[0, -1, 2, -1, 2, -1]))


def _one_point_per_kf(n_kf, voted, cov, kf_bad=None, seed=3):
    """Point k is observed by keyframe k and sits in its slot 0; the frame holds the points of `voted`."""
    kf_bad = [0] * n_kf if kf_bad is None else kf_bad
    cov = [cov.get(k, []) for k in range(n_kf)]
    s = make_store(n_kf, [[k] for k in range(n_kf)], kf_bad, [[k, -1] for k in range(n_kf)], cov, seed=seed)
    return s, [LOCKED] * len(voted), list(voted)


def expansion_cases():
    """3: every voted keyframe has one vote, so pFMax is the lowest voted index; the local points are the
    local keyframes' own points, ascending."""
    out = {}

    def add(name, n_kf, voted, cov, local_kf, kf_bad=None):
        s, st, gid = _one_point_per_kf(n_kf, voted, cov, kf_bad)
        v = [1 if k in voted else 0 for k in range(n_kf)]
        out[name] = case(s, st, gid, dict(status=0, votes=v, local_kf=local_kf, refer_kf=min(voted), n_voted=len(voted),
                                          l2g=sorted(local_kf), n_held=len(voted), n_nulled=0))

    # 9 voted: entry 0 appends 20 (10 entries), entry 1 appends 21 (11); entry 2 finds more than 10 and stops
    add("grow_9_to_11", 24, range(9), {0: [20], 1: [21], 2: [22], 3: [23]}, list(range(9)) + [20, 21])
    # 12 voted: more than 10 from the start, nothing is appended
    add("twelve_no_expansion", 24, range(12), {0: [20], 1: [21]}, list(range(12)))
    # kf0's first covisible (1) is listed: the next (5) is taken; kf1's are both listed by then; kf5 has none
    add("first_already_listed", 8, [0, 1], {0: [1, 5], 1: [0, 5]}, [0, 1, 5])
    # all covisibles bad
    add("all_covisibles_bad", 6, [0], {0: [3, 4]}, [0], kf_bad=[0, 0, 0, 1, 1, 0])
    # a chain: each appended frame is visited and appends its own covisible, until 11 entries
    add("appended_is_expanded", 14, [0], {k: [k + 1] for k in range(13)}, list(range(11)))
    # 12 covisibles: ten bad ones, then 12 (good), then 13 (bad) -- only the first 10 are read
    add("eleventh_not_taken", 14, [0], {0: list(range(2, 12)) + [12, 13]}, [0],
        kf_bad=[0, 0] + [1] * 10 + [0, 1])
    return out


def dedupe_case(max_local=None, status=0):
    """4 (and 6): p3 sits in slots of all three local keyframes -> once; p4 is bad -> left out; -1 ignored."""
    s = make_store(6, [[0], [1], [2], [0, 1, 2], [0], [2]], [0, 0, 0], [[3, -1, 0], [3, 4, -1], [-1, 3, 5]], [[], [], []],
                   is_bad=[0, 0, 0, 0, 1, 0], seed=4)
    want = dict(status=status, votes=[2, 2, 1], local_kf=[0, 1, 2], refer_kf=0, n_voted=3, n_held=3, n_nulled=0, n_local=3)
    if status == 0:
        want.update(l2g=[0, 3, 5], slot_id=[0, -1, 1])
    return case(s, [LOCKED, FREE, LOCKED], [0, 1, 3], want, max_local=max_local)


def compaction_case(n_points, mode):
    """5: one keyframe, voted through point 0; its slots hold all / none / the even points."""
    held = dict(all=list(range(n_points)), none=[], alternating=list(range(0, n_points, 2)))[mode]
    s = make_store(n_points, [[0]] + [[]] * (n_points - 1), [0], [held], [[]], seed=5)
    return case(s, [FREE], [0], dict(status=0, votes=[1], local_kf=[0], refer_kf=0, n_voted=1, l2g=held,
                                     slot_id=[0 if held else -1]))


def empty_cases():
    """7: an empty store under a frame of created points; a store under a frame with no held slot."""
    e = make_store(0, [], [], [], [], seed=6)
    a = case(e, [FREE, LOCKED], [-1, -1], dict(status=0, votes=[], local_kf=[], refer_kf=-1, n_voted=0, n_held=2, l2g=[],
                                               slot_id=[-1, -1]), max_local=4)
    s = make_store(3, [[0], [0], [1]], [0, 0], [[0, 1], [2]], [[1], [0]], seed=7)
    b = case(s, [EMPTY, EMPTY, EMPTY], [0, 1, 2], dict(status=0, votes=[0, 0], local_kf=[], refer_kf=-1, n_voted=0, n_held=0,
                                                        l2g=[], slot_id=[-1, -1, -1]), max_local=4)
    return dict(empty_store=a, no_held_slot=b)


def ids_case():
    """9: the motion stage's codes over global ids.  Slot 0 copies last slot 2 (gid 1), slot 1 is NULLed,
    slot 2 is UNCHANGED with pass 1 and given slots (keeps its gid 3), slot 3 copies last slot 0 (gid -1:
    a created point), slot 4 copies last slot 1 (gid 0).  The same frame with the gids passed directly is
    `direct`."""
    s = make_store(4, [[0], [0, 1], [1], [1]], [0, 0], [[0, 1], [2, 3]], [[], []], seed=8)
    ids = dict(assign=np.array([2, NULL, UNCHANGED, 0, 1], np.int32), pass_=1, given=1, last_gid=np.array([-1, 0, 1], np.int32))
    state = [LOCKED, EMPTY, FREE, FREE, LOCKED]
    want = dict(status=0, votes=[2, 2], local_kf=[0, 1], refer_kf=0, n_voted=2, n_held=4, l2g=[0, 1, 2, 3],
                slot_id=[1, -1, 3, -1, 0], gid=[1, -1, 3, -1, 0])
    return dict(given=case(s, state, [9, 9, 3, 9, 9], want, ids=ids), direct=case(s, state, [1, -1, 3, -1, 0], want))


def many_keyframes_case():
    """More keyframes than one vote window (4096) and than one compaction pass (1024): votes at 0, 1500,
    4095, 4096 and 4100 (twice: pFMax); kf4100's covisible 3000 joins through the expansion."""
    n_kf = 4101
    slots, cov = [[] for _ in range(n_kf)], [[] for _ in range(n_kf)]
    slots[0], slots[3000], slots[4100], cov[4100] = [0], [3], [1, -1, 2], [3000]
    s = make_store(4, [[0, 4095], [4096, 4100], [4100, 1500], [2000]], [0] * n_kf, slots, cov, seed=9)
    v = np.zeros(n_kf, np.int32)
    v[[0, 1500, 4095, 4096]], v[4100] = 1, 2
    return case(s, [LOCKED, FREE, LOCKED], [0, 1, 2],
                dict(status=0, votes=v, local_kf=[0, 1500, 4095, 4096, 4100, 3000], refer_kf=4100, n_voted=5, n_held=3,
                     l2g=[0, 1, 2, 3], slot_id=[0, 1, 2]))


def all_cases():
    c = dict(votes=votes_case(), bad_point=bad_point_case(), dedupe=dedupe_case(), exact_fit=dedupe_case(max_local=3),
             overflow=dedupe_case(max_local=2, status=2), many_keyframes=many_keyframes_case())
    c.update(expansion_cases())
    c.update(empty_cases())
    for k, v in ids_case().items():
        c["ids_" + k] = v
    for n in (1, 1023, 1024, 1025, 3 * 1024 + 1):
        for mode in ("all", "none", "alternating"):
            c[f"compact_{n}_{mode}"] = compaction_case(n, mode)
    return c
