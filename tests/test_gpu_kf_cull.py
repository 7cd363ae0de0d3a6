"""GPU: the life of the keyframe store's points, lorb_kf_store_observe_dev and lorb_kf_store_cull_dev
(lorb_slam_amd.frame.KeyframeStore.read_life / write_life, keyframe_observe, keyframe_cull), bit for bit against the
restatement tests/kf_cull_ref.py.

1. Life after insertion: after every case of tests/kf_store_cases.py and after chain_frames()' four insertions behind
   one wait, visible, found, first_fid, recent and kf_fid equal the restatement; every output the existing insertion
   tests compare keeps its bits; the bytes past the counts are untouched.
2. Observe (1 launch) on fabricated gids, local rows, in_view and records: both found rules, both sides of the 1024
   threads of the walk, every status-1 path (nothing is written, the frame word included).
3. Cull (4 launches) against the restatement: every store, geometry and life array (integers equal, floats as bytes),
   the record, the frame's slots and gids, sentinel bytes past every true count; the sizes where the kernels change
   path; a failed call followed by a good one.
4. Chain: insert -> cull -> local BA on the insertion's record words with nothing between them equals the same with a
   wait after each; the BA window and lorb_local_map_update_dev see no culled point."""
import copy
import ctypes as C

import numpy as np
import pytest

import kf_ba_cases as BC
import kf_ba_ref as B
import kf_cull_cases as CC
import kf_cull_ref as L
import kf_store_cases as KC
import kf_store_ref as R
import test_gpu_kf_ba as KB
import test_gpu_kf_store as KS
import test_gpu_kf_store_chain as CH
import test_gpu_local_map as LM
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, DeviceSlots, KeyframeStore, LocalMap, _sentinel, keyframe_ba_record,
                                 keyframe_ba_result, keyframe_cull, keyframe_cull_record, keyframe_cull_result, keyframe_insert,
                                 keyframe_insert_result, keyframe_local_ba, keyframe_observe, keyframe_observe_record)
from lorb_slam_amd.runtime import LorbError, lib

pytestmark = pytest.mark.gpu

G, SENT, FILL, SENT_I32 = KS.G, KS.SENT, KS.FILL, KS.SENT_I32
raw, sentinel = KS.raw, KS.sentinel
OBS_REC, CULL_REC = C.sizeof(A.KfObserveResult), C.sizeof(A.KfCullResult)
CULL = CC.cull_cases()
OBSERVE = CC.observe_cases()


def h2d(ctx, dev, values, dtype=np.int32):
    v = np.ascontiguousarray(values, dtype)
    ctx.check(lib().lorb_memcpy_h2d(ctx.handle, dev.ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes)), "h2d")


def memset(ctx, dev, nbytes, value=SENT):
    ctx.check(lib().lorb_memset_dev(ctx.handle, dev.ptr, C.c_int(value), C.c_size_t(nbytes)), "memset")


def life_arrays(store):
    """Every life array over its whole capacity, and the frame word."""
    return {k: v.numpy() for k, v in store.life.items()}


def same_life(store, life, cn):
    """read_life and the whole-capacity views against a restatement's life; sentinel bytes past the true counts."""
    got, a = store.read_life(), life_arrays(store)
    for k in L.LIFE:
        assert got[k].dtype == life[k].dtype and np.array_equal(got[k], life[k]), k
        m = cn["n_kf"] if k == "kf_fid" else cn["n_points"]
        assert np.array_equal(a[k][:m], life[k]) and sentinel(a[k][m:]), k
    assert got["frame_word"] == life["frame_word"]


def same_record(rec, want, fields):
    for f in fields:
        assert getattr(rec, f) == want.get(f, SENT_I32), (f, getattr(rec, f), want.get(f))


def all_arrays(store):
    a = KB.arrays_of(store)
    a.update({"life_" + k: v for k, v in life_arrays(store).items()})
    return a


# -- 1. life after insertion -----------------------------------------------------------------------------------------
def set_frame_word(ctx, store, fid):
    h2d(ctx, store.life["frame_word"], [fid])


@pytest.mark.parametrize("name", sorted(KS.CASES))
def test_life_after_insertion(ctx, name):
    c = copy.deepcopy(KS.CASES[name])
    g0 = BC.geometry_for(c["store"], seed=len(name))
    rig = KB.GeomRig(ctx, c, g0)
    try:
        cn0 = R.counts(c["store"])
        rig.store.fill_life(cn0)
        life0 = L.new_life(cn0["n_kf"], cn0["n_points"])
        same_life(rig.store, life0, cn0)          # what create leaves
        set_frame_word(ctx, rig.store, 33)
        life0["frame_word"] = 33
        rig.insert()
        r = rig.read()
        ref = KS.reference(c)
        KS.check(rig, r, ref)                     # the existing read-outs keep their bits
        KB.same_geometry(rig.store, B.insert_geometry(g0, ref, c["frame"], KB.POSE6, c["n_cur"]))
        same_life(rig.store, L.insert_life(life0, c["store"], c["frame"], c["slots"], c["gid"], ref), R.counts(ref["store"]))
    finally:
        rig.free()


class Nothing:
    """The inputs of an observe call that holds and sees nothing: it only moves the frame word."""

    def __init__(self, ctx):
        self.frame = LM.Counts(ctx, 0)
        self.slots = DeviceSlots(ctx, 1, state=0)
        self.ints = ctx.to_device(np.zeros(8, np.int32))
        self.update = ctx.to_device(np.frombuffer(bytes(A.LocalMapResult()), np.uint8).copy())
        self.view = A.LocalMapArrays()
        self.view.l2g, self.view.max_local = self.ints.ptr.value, 1
        self.rec = keyframe_observe_record(ctx)

    def observe(self, ctx, store, fid):
        keyframe_observe(ctx, store, fid, self.frame, self.slots, self.ints, self.ints, self.view, self.update, self.ints, self.rec,
                         n_max_cur=1)

    def free(self):
        for a in (self.frame, self.slots, self.ints, self.update, self.rec):
            a.free()


def test_life_after_four_insertions_behind_one_wait(ctx):
    fs = KC.chain_frames()
    refs = KC.chain_restate(fs)
    store = KeyframeStore(ctx, **KC.CHAIN_CAPS)
    empty = R.counts(R.empty_store())
    store.fill(empty)
    store.fill_geometry(empty)
    store.fill_life(empty)
    steps = [CH.Step(ctx, c, [0]) for c in fs]
    no = Nothing(ctx)
    try:
        for i, st in enumerate(steps):  # eight calls, no wait: each frame has its own id
            no.observe(ctx, store, 10 * (i + 1))
            keyframe_insert(ctx, store, st.c["fp"], st.frame, st.slots, st.gid, st.pose, st.rec, n_max_cur=KC.CHAIN_N_MAX,
                            gate=st.c["gate"])
        ctx.sync()
        life, s = L.new_life(0, 0), R.empty_store()
        for i, (c, ref) in enumerate(zip(fs, refs)):
            life["frame_word"] = 10 * (i + 1)
            life = L.insert_life(life, s, c["frame"], c["slots"], c["gid"], ref)
            s = ref["store"]
        assert list(life["kf_fid"]) == [10, 20, 40] and life["recent"].sum() == 10 + 4 + 5   # the created points (p2, held twice, is one)
        KS.same_store(store.read(), s)
        same_life(store, life, R.counts(s))
    finally:
        for st in steps:
            st.free()
        no.free()
        store.free()


# -- 2. observe ------------------------------------------------------------------------------------------------------
class ObserveRig:
    def __init__(self, ctx, c):
        self.ctx, self.c = ctx, c
        P = c["n_points"]
        s = KC.random_store(3, P, seed=30)
        self.cn = R.counts(s)
        self.store = KeyframeStore(ctx, 5, P + 7, self.cn["n_obs"] + 5, self.cn["n_kf_slots"] + 5, init=s)
        self.store.fill_life(self.cn)
        nc, nl = c["n_max_cur"], c["max_local"]
        self.frame = LM.Counts(ctx, c["n_cur"])
        self.slots = DeviceSlots(ctx, nc, state=c["state"])

        def guarded(a, n, dt=np.int32):
            h = np.full(n + G, FILL, np.int32).astype(dt)
            h[:len(a)] = a
            return ctx.to_device(h)

        self.gid, self.lid, self.l2g = guarded(c["gid"], nc), guarded(c["lid"], nc), guarded(c["l2g"], nl)
        self.in_view = guarded(c["in_view"], nl, np.uint8)
        self.update = ctx.to_device(np.full(C.sizeof(A.LocalMapResult) + G, SENT, np.uint8))
        self.status = ctx.to_device(np.array([0] + [FILL] * G, np.int32))
        self.view = A.LocalMapArrays()
        self.view.l2g, self.view.max_local = self.l2g.ptr.value, nl
        self.rec = keyframe_observe_record(ctx)
        self.set()

    def set(self, n_cur=None, n_local=None, update_status=0, local_status=0):
        u = A.LocalMapResult()
        u.status, u.n_local = update_status, self.c["n_local"] if n_local is None else n_local
        h2d(self.ctx, self.update, np.frombuffer(bytes(u), np.uint8), np.uint8)
        h2d(self.ctx, self.status, [local_status])
        self.frame.set(self.c["n_cur"] if n_cur is None else n_cur)

    def run(self, rule, frame_id=None, status_word=True):
        memset(self.ctx, self.rec, OBS_REC)
        keyframe_observe(self.ctx, self.store, self.c["frame_id"] if frame_id is None else frame_id, self.frame, self.slots, self.gid,
                         self.lid, self.view, self.update, self.in_view, self.rec, n_max_cur=self.c["n_max_cur"],
                         d_local_status=self.status.ptr.value if status_word else None, found_rule=rule)
        b = self.rec.numpy()
        assert sentinel(b[OBS_REC:])
        return A.KfObserveResult.from_buffer_copy(b.tobytes()[:OBS_REC])

    def free(self):
        for a in (self.store, self.frame, self.slots, self.gid, self.lid, self.l2g, self.in_view, self.update, self.status, self.rec):
            a.free()


@pytest.mark.parametrize("name", sorted(OBSERVE))
def test_observe(ctx, name):
    c = OBSERVE[name]
    rig = ObserveRig(ctx, c)
    try:
        life = L.new_life(rig.cn["n_kf"], rig.cn["n_points"])
        inputs = {k: v.numpy() for k, v in dict(gid=rig.gid, lid=rig.lid, l2g=rig.l2g, in_view=rig.in_view).items()}
        for i, rule in enumerate((L.FOUND_NEVER, L.FOUND_SLOTS, L.FOUND_NEVER)):   # the counters accumulate
            rec = rig.run(rule, frame_id=c["frame_id"] + i, status_word=i != 2)
            life, want = L.observe(life, found_rule=rule, **dict(c, frame_id=c["frame_id"] + i))
            same_record(rec, want, L.OBSERVE_FIELDS)
            assert want["status"] == 0 and want["n_held"] >= 2 and (rule == 1 or want["n_found"] == 0)
            if c["n_cur"] > 1000:
                assert want["n_in_view"] > 0 and (want["n_found"] > 0) == (rule == 1)
            same_life(rig.store, life, rig.cn)
        assert life["visible"][5] >= 1 + 3 * 2                                       # the point in two slots
        for k, v in inputs.items():                                                  # read only
            assert np.array_equal(getattr(rig, k).numpy(), v), k
    finally:
        rig.free()


@pytest.mark.parametrize("fail", ["count_above", "count_negative", "n_local_above", "n_local_negative", "update_status", "local_status"])
def test_observe_status_1_writes_nothing(ctx, fail):
    c = OBSERVE["cur_7_local_3"]
    rig = ObserveRig(ctx, c)
    try:
        memset(ctx, rig.store.life["frame_word"], 4)
        rig.set(**dict(count_above=dict(n_cur=c["n_max_cur"] + 1), count_negative=dict(n_cur=-1),
                       n_local_above=dict(n_local=c["max_local"] + 1), n_local_negative=dict(n_local=-1),
                       update_status=dict(update_status=2), local_status=dict(local_status=1))[fail])
        before = life_arrays(rig.store)
        rec = rig.run(L.FOUND_SLOTS)
        same_record(rec, dict(status=1), L.OBSERVE_FIELDS)
        after = life_arrays(rig.store)
        for k in before:
            assert np.array_equal(after[k], before[k]), k
        assert int(after["frame_word"][0]) == SENT_I32
        rig.set()                                                                    # the next call is fine
        rec = rig.run(L.FOUND_SLOTS)
        life, want = L.observe(L.new_life(rig.cn["n_kf"], rig.cn["n_points"]), found_rule=L.FOUND_SLOTS, **c)
        same_record(rec, want, L.OBSERVE_FIELDS)
        same_life(rig.store, life, rig.cn)
    finally:
        rig.free()


# -- 3. cull ---------------------------------------------------------------------------------------------------------
class CullRig:
    """A store with geometry and life a few rows larger than its counts, sentinel bytes behind every count; the
    tracker's frame; the device words the call reads and its record."""

    def __init__(self, ctx, case, slack=5):
        self.ctx, self.case = ctx, case
        s = case["store"]
        cn = self.cn = R.counts(s)
        self.store = KeyframeStore(ctx, cn["n_kf"] + slack, cn["n_points"] + slack, cn["n_obs"] + slack, cn["n_kf_slots"] + slack,
                                   init=s, geom=case["geom"])
        self.store.fill(cn)
        self.store.fill_geometry(cn)
        self.store.fill_life(cn)
        self.store.write_life(case["life"])
        set_frame_word(ctx, self.store, case["life"]["frame_word"])
        self.words = ctx.to_device(np.array([case["kf"], 0] + [FILL] * G, np.int32))   # d_kf, d_src_status
        self.rec = keyframe_cull_record(ctx)
        f = self.f = case["frame"]
        self.frame = self.slots = self.gid = None
        if f is not None:
            self.frame = LM.Counts(ctx, f["n_cur"])
            self.slots = DeviceSlots(ctx, f["n_max_cur"], state=f["state"])
            g = np.full(f["n_max_cur"] + G, FILL, np.int32)
            g[:f["n_cur"]] = f["gid"]
            self.gid = ctx.to_device(g)

    def set(self, kf, src_status=0):
        h2d(self.ctx, self.words, [kf, src_status])

    def run(self, params=None, status_word=True):
        memset(self.ctx, self.rec, CULL_REC)
        d = self.words.ptr.value
        keyframe_cull(self.ctx, self.store, d, self.rec, d_src_status=d + 4 if status_word else None,
                      params=self.case["params"] if params is None else params, cur=self.frame, cur_slots=self.slots,
                      slot_gid=self.gid, n_max_cur=None if self.f is None else self.f["n_max_cur"])
        b = self.rec.numpy()
        assert sentinel(b[CULL_REC:])
        return A.KfCullResult.from_buffer_copy(b.tobytes()[:CULL_REC])

    def free(self):
        for a in (self.store, self.words, self.rec, self.frame, self.slots, self.gid):
            if a is not None:
                a.free()


def check_cull(rig, ref, before):
    """Everything the device holds after a cull against the restatement's result.  rig.cn: the counts when the
    sentinel bytes were written (entries between the new and that n_obs hold what the lists held before)."""
    case, s = rig.case, ref["store"]
    cn = R.counts(s)
    assert rig.store.counts() == cn
    KS.same_store(rig.store.read(), s)
    KB.same_geometry(rig.store, dict(case["geom"], obs_slot=ref["obs_slot"]))
    same_life(rig.store, ref["life"], cn)
    B.check_invariant(s, dict(case["geom"], obs_slot=ref["obs_slot"]))
    after = all_arrays(rig.store)
    # rows past the true counts keep the sentinel fill; between the new and the old n_obs the old entries stay
    past = dict(obs_off=cn["n_points"] + 1, obs_kf=rig.cn["n_obs"], obs_slot=rig.cn["n_obs"], kf_slot_off=cn["n_kf"] + 1,
                kf_slot_point=cn["n_kf_slots"], cov_off=cn["n_kf"] + 1, cov_kf=cn["n_cov"], kf_bad=cn["n_kf"], kf_pose=cn["n_kf"],
                kf_slot_uv=cn["n_kf_slots"])
    for k, v in after.items():
        if k.startswith("life_"):
            continue
        tail = v[past.get(k, cn["n_points"]):]
        assert (tail == 1).all() if k in ("is_bad", "kf_bad") else sentinel(tail), k
    # left as they are, as in the reference
    for k in ("locked", "pos", "normal", "max_dist", "min_dist", "desc", "cov_off", "cov_kf", "kf_bad", "kf_slot_off", "kf_pose",
              "kf_slot_uv", "life_visible", "life_found", "life_first_fid", "life_kf_fid", "life_frame_word"):
        assert np.array_equal(raw(after[k]), raw(before[k])), k
    if rig.f is not None:
        n = rig.f["n_cur"]
        st, g = rig.slots.numpy(), rig.gid.numpy()
        assert np.array_equal(st["state"][:n], ref["state"]) and sentinel(st["state"][n:])
        assert sentinel(st["pos"]) and sentinel(st["desc"])
        assert np.array_equal(g[:n], ref["gid"]) and (g[n:] == FILL).all()


def restate(case, **kw):
    return L.cull(case["store"], case["obs_slot"], case["life"], kw.pop("kf", case["kf"]), kw.pop("params", case["params"]),
                  frame=case["frame"], **kw)


@pytest.mark.parametrize("name", sorted(CULL))
def test_cull(ctx, name):
    case = CULL[name]
    ref = restate(case)
    n, culled = case["store"]["n_points"], ref["culled"]
    # the case is what its name says
    if name in ("points_1023", "points_1024", "points_1025"):
        assert n == int(name.split("_")[1]) and 0 in culled and n - 1 in culled
    if name == "points_2049_tile_edge":
        assert {CC.TILE - 1, CC.TILE, 2 * CC.TILE - 1, 2 * CC.TILE} <= set(culled) and case["frame"]["n_cur"] == 1025
        assert max(len(r) for r in case["store"]["kf_slots"]) >= 1025
    if name == "all_culled":
        assert ref["rec"]["n_obs"] == 0 and len(culled) + ref["rec"]["n_bad_before"] == n and ref["rec"]["n_obs_removed"] > 0
    if name == "none_culled":
        assert not culled and ref["rec"]["n_examined"] > 0
        assert ref["rec"]["n_recent"] == ref["rec"]["n_examined"] - ref["rec"]["n_bad_before"]
    if name == "obs_300":
        assert 1027 in culled and len(case["store"]["obs"][1027]) == 300 and ref["rec"]["n_obs_removed"] >= 300
    if case["frame"] is not None and culled:
        assert ref["rec"]["n_frame_slots_emptied"] > 0
        held_bad = [j for j in range(case["frame"]["n_cur"]) if 0 <= case["frame"]["gid"][j] < n
                    and case["store"]["is_bad"][case["frame"]["gid"][j]]]
        assert name == "all_culled" or (held_bad and all(ref["gid"][j] == case["frame"]["gid"][j] for j in held_bad))
    rig = CullRig(ctx, case)
    try:
        before = all_arrays(rig.store)
        rec = rig.run()
        same_record(rec, ref["rec"], L.CULL_FIELDS)
        check_cull(rig, ref, before)
        if not culled:   # the CSR is not rewritten: not a byte of it, nor of any other array but recent, moved
            after = all_arrays(rig.store)
            for k in after:
                if k != "life_recent":
                    assert np.array_equal(raw(after[k]), raw(before[k])), k
        # a second call finds nobody to cull: the marks are back at rest, the lists stand
        ref2 = L.cull(ref["store"], ref["obs_slot"], ref["life"], case["kf"], case["params"],
                      frame=None if case["frame"] is None else dict(case["frame"], state=ref["state"], gid=ref["gid"]))
        assert not ref2["culled"]
        mid = all_arrays(rig.store)
        rec = rig.run()
        same_record(rec, ref2["rec"], L.CULL_FIELDS)
        check_cull(rig, ref2, mid)
    finally:
        rig.free()


def test_every_verdict_branch_is_taken():
    seen = set()
    for case in CULL.values():
        seen |= set(restate(case)["verdicts"].values())
    assert seen == set(L.VERDICTS)


@pytest.mark.parametrize("fail", ["kf_negative", "kf_above", "src_status"])
def test_failed_cull_then_a_good_one(ctx, fail):
    """Status 1 stores the status and nothing else; the good call behind it equals the good call alone."""
    case = CULL["hand"]
    rig = CullRig(ctx, case)
    try:
        nk = rig.cn["n_kf"]
        rig.set(*dict(kf_negative=(-1, 0), kf_above=(nk, 0), src_status=(case["kf"], 2))[fail])
        before = all_arrays(rig.store)
        slots, gid = rig.slots.numpy(), rig.gid.numpy()
        rec = rig.run()
        same_record(rec, dict(status=1), L.CULL_FIELDS)
        after = all_arrays(rig.store)
        for k in before:
            assert np.array_equal(raw(after[k]), raw(before[k])), k
        assert np.array_equal(rig.slots.numpy()["state"], slots["state"]) and np.array_equal(rig.gid.numpy(), gid)
        rig.set(case["kf"])
        ref = restate(case)
        rec = rig.run(status_word=fail != "src_status")
        same_record(rec, ref["rec"], L.CULL_FIELDS)
        check_cull(rig, ref, before)
    finally:
        rig.free()


def test_cull_errors(ctx):
    case = CULL["hand"]
    rig = CullRig(ctx, case)
    bare = KeyframeStore(ctx, 8, 16, 32, 32, init=case["store"])   # no geometry for its keyframes
    try:
        d = rig.words.ptr.value

        def call(match, **kw):
            a = dict(store=rig.store, params=L.REFERENCE, cur=rig.frame, cur_slots=rig.slots, slot_gid=rig.gid, n_max_cur=8)
            a.update(kw)
            with pytest.raises(LorbError, match=match):
                keyframe_cull(ctx, a.pop("store"), d, rig.rec, **a)

        call("geometry", store=bare)
        call("in part", cur=None)
        call("in part", slot_gid=None)
        call("positive", n_max_cur=0)
        call("parameters", params=(float("nan"), 2, 3, 3))
        call("parameters", params=(0.25, -1, 3, 3))
        call("parameters", params=(0.25, 2, 3, -2))
        # the life write-in: counts that are not the true ones, and values no MapPoint can hold
        life = case["life"]
        with pytest.raises(LorbError, match="counts"):
            rig.store.write_life(dict(visible=np.ones(6, np.int32)), n_points=6)
        with pytest.raises(LorbError, match=r"visible\[2\] = 0"):
            rig.store.write_life(dict(life, visible=np.array([1, 1, 0, 1, 1, 1, 1], np.int32)))
        with pytest.raises(LorbError, match=r"found\[6\] = -1"):
            rig.store.write_life(dict(life, found=np.array([1, 1, 1, 1, 1, 1, -1], np.int32)))
        # an observe call with an unknown rule or no bound
        no = Nothing(ctx)
        try:
            with pytest.raises(LorbError, match="unknown found rule"):
                keyframe_observe(ctx, rig.store, 1, no.frame, no.slots, no.ints, no.ints, no.view, no.update, no.ints, no.rec,
                                 n_max_cur=1, found_rule=2)
            with pytest.raises(LorbError, match="positive"):
                keyframe_observe(ctx, rig.store, 1, no.frame, no.slots, no.ints, no.ints, no.view, no.update, no.ints, no.rec,
                                 n_max_cur=0)
        finally:
            no.free()
        ref = restate(case)   # the next call is fine
        before = all_arrays(rig.store)
        same_record(rig.run(), ref["rec"], L.CULL_FIELDS)
        check_cull(rig, ref, before)
    finally:
        bare.free()
        rig.free()


# -- 4. chain --------------------------------------------------------------------------------------------------------
class ChainArm:
    """One store from the chain scene with K1 inserted and frames 21 and 22 observed (waited for: the set-up), and the
    objects of K2's insertion, cull and local BA."""

    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        k1, k2, caps, seen, self.created = CC.chain_frames(sc)
        self.k1, self.k2, self.seen = k1, k2, seen
        s = sc["store"]
        self.store = KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=s,
                                   geom=sc["geom"])
        cn = R.counts(s)
        self.store.fill(cn)
        self.store.fill_geometry(cn)
        self.store.fill_life(cn)
        self.no = Nothing(ctx)
        self.s1, self.s2 = self.step(k1, KB.POSE6), self.step(k2, sc["pose6"])
        P1 = s["n_points"] + CC.N_CREATED
        self.seen_dev = dict(frame=LM.Counts(ctx, seen["n_cur"]), slots=DeviceSlots(ctx, seen["n_max_cur"], state=seen["state"]),
                             gid=ctx.to_device(np.concatenate([seen["gid"], [FILL] * 4]).astype(np.int32)),
                             lid=ctx.to_device(np.concatenate([seen["lid"], [FILL] * 4]).astype(np.int32)),
                             l2g=ctx.to_device(np.concatenate([seen["l2g"], [FILL] * 16]).astype(np.int32)),
                             in_view=ctx.to_device(np.concatenate([seen["in_view"], [0] * 16]).astype(np.uint8)))
        u = A.LocalMapResult()
        u.status, u.n_local = 0, seen["n_local"]
        self.seen_dev["update"] = ctx.to_device(np.frombuffer(bytes(u), np.uint8).copy())
        self.view = A.LocalMapArrays()
        self.view.l2g, self.view.max_local = self.seen_dev["l2g"].ptr.value, seen["max_local"]
        self.orec, self.crec, self.brec = keyframe_observe_record(ctx), keyframe_cull_record(ctx), keyframe_ba_record(ctx)
        self.P1 = P1
        # the set-up: frame 20 becomes K1, frames 21 and 22 see some of its points
        self.no.observe(ctx, self.store, 20)
        self.insert(self.s1, k1)
        for fid in (21, 22):
            d = self.seen_dev
            keyframe_observe(ctx, self.store, fid, d["frame"], d["slots"], d["gid"], d["lid"], self.view, d["update"], d["in_view"],
                             self.orec, n_max_cur=seen["n_max_cur"])
        ctx.sync()
        assert keyframe_insert_result(self.s1["rec"]).n_created == CC.N_CREATED

    def step(self, c, pose6):
        ctx, nc = self.ctx, c["n_max_cur"]
        g = np.full(nc + G, FILL, np.int32)
        g[:c["n_cur"]] = c["gid"]
        sl = c["slots"]
        return dict(frame=KS.Frame(ctx, c), slots=DeviceSlots(ctx, nc, state=sl["state"], pos=sl["pos"], desc=sl["desc"]),
                    gid=ctx.to_device(g), pose=DeviceBlock(ctx, A.FramePose, KB.pose_value(c["pose"], pose6)),
                    rec=_sentinel(ctx, KS.REC + G, np.uint8))

    def insert(self, st, c):
        keyframe_insert(self.ctx, self.store, c["fp"], st["frame"], st["slots"], st["gid"], st["pose"], st["rec"], n_max_cur=c["n_max_cur"],
                        gate=c["gate"])

    def observe_k2(self):
        """K2's own frame, id 24: its slots as the tracker left them (the gids the insertion will read)."""
        d, c = self.seen_dev, self.k2
        keyframe_observe(self.ctx, self.store, 24, self.s2["frame"], self.s2["slots"], self.s2["gid"], d["lid"], self.view, d["update"],
                         d["in_view"], self.orec, n_max_cur=c["n_max_cur"])

    def insert_k2(self):
        self.insert(self.s2, self.k2)

    def cull(self):
        rec = self.s2["rec"].ptr.value
        keyframe_cull(self.ctx, self.store, rec + A.KfInsertResult.kf.offset, self.crec, d_src_status=rec + A.KfInsertResult.status.offset,
                      params=CC.CHAIN_PARAMS, cur=self.s2["frame"], cur_slots=self.s2["slots"], slot_gid=self.s2["gid"],
                      n_max_cur=self.k2["n_max_cur"])

    def local_ba(self):
        rec = self.s2["rec"].ptr.value
        keyframe_local_ba(self.ctx, self.store, self.sc["fp"], rec + A.KfInsertResult.kf.offset, self.brec,
                          d_src_status=rec + A.KfInsertResult.status.offset)

    def free(self):
        for st in (self.s1, self.s2):
            for a in st.values():
                a.free()
        for a in (*self.seen_dev.values(), self.orec, self.crec, self.brec, self.no, self.store):
            a.free()


def chain_restatement(sc):
    """The same steps on the restatement -> dict(store, geom, life: after K2's cull; cull: L.cull's result; ...)."""
    k1, k2, caps, seen, created = CC.chain_frames(sc)
    s, g = sc["store"], sc["geom"]
    life = L.new_life(len(s["kf_bad"]), s["n_points"])
    life, _ = L.observe(life, s["n_points"], 20, 0, 1, [], [], [], [0], 0, 1, [0])
    r1 = R.insert_keyframe(s, caps, k1["fp"], k1["frame"], k1["pose"], k1["slots"], k1["gid"], k1["n_cur"], k1["n_max_cur"], k1["gate"])
    g = B.insert_geometry(g, r1, k1["frame"], KB.POSE6, k1["n_cur"])
    life = L.insert_life(life, s, k1["frame"], k1["slots"], k1["gid"], r1)
    s = r1["store"]
    for fid in (21, 22):
        life, rec = L.observe(life, **dict(seen, n_points=s["n_points"], frame_id=fid))
        assert rec["n_held"] == 6 and rec["n_in_view"] == 2
    # K2's own frame: lid, l2g, in_view as frames 21 and 22 (c0 and c1 among the local points)
    life, rec = L.observe(life, s["n_points"], 24, k2["n_cur"], k2["n_max_cur"], k2["slots"]["state"], k2["gid"], seen["lid"], seen["l2g"],
                          seen["n_local"], seen["max_local"], seen["in_view"])
    r2 = R.insert_keyframe(s, caps, k2["fp"], k2["frame"], k2["pose"], k2["slots"], k2["gid"], k2["n_cur"], k2["n_max_cur"], k2["gate"])
    g = B.insert_geometry(g, r2, k2["frame"], sc["pose6"], k2["n_cur"])
    life = L.insert_life(life, s, k2["frame"], k2["slots"], k2["gid"], r2)
    cull = L.cull(r2["store"], g["obs_slot"], life, r2["kf"], CC.CHAIN_PARAMS,
                  frame=dict(n_cur=k2["n_cur"], n_max_cur=k2["n_max_cur"], state=r2["state"], gid=r2["gid"]))
    return dict(cull=cull, geom=dict(g, obs_slot=cull["obs_slot"]), created=created, r2=r2, k2=k2)


def test_chain_insert_cull_local_ba(ctx):
    sc = BC.chain_scene()
    ref = chain_restatement(sc)
    cull, created = ref["cull"], ref["created"]
    # non-vacuity, from the restatement: created points that are culled, and created points that survive
    assert [cull["verdicts"][p] for p in created] == ["ratio"] * 2 + ["aged_out"] * 4 + ["obs"] * 6
    assert set(cull["culled"]) == set(created[:2] + created[6:]) and not cull["store"]["is_bad"][created[2]]
    assert cull["rec"]["n_frame_slots_emptied"] == 2
    chained, waited = ChainArm(ctx, sc), ChainArm(ctx, sc)
    try:
        chained.observe_k2()   # nothing between the four calls
        chained.insert_k2()
        chained.cull()
        chained.local_ba()
        waited.observe_k2()
        ctx.sync()
        waited.insert_k2()
        ctx.sync()
        assert keyframe_insert_result(waited.s2["rec"]).inserted == 1
        waited.cull()
        ctx.sync()
        # the store after the cull is the restatement's
        s = cull["store"]
        KS.same_store(waited.store.read(), s)
        KB.same_geometry(waited.store, ref["geom"])
        same_life(waited.store, cull["life"], R.counts(s))
        same_record(keyframe_cull_result(waited.crec), cull["rec"], L.CULL_FIELDS)
        waited.local_ba()
        ctx.sync()
        a, b = all_arrays(chained.store), all_arrays(waited.store)
        for k in a:
            assert np.array_equal(raw(a[k]), raw(b[k])), k
        assert bytes(keyframe_cull_result(chained.crec)) == bytes(keyframe_cull_result(waited.crec))
        ra, rb = keyframe_ba_result(chained.brec), keyframe_ba_result(waited.brec)
        assert bytes(ra) == bytes(rb) and ra.status == 0 and ra.written == 1 and ra.kf == ref["r2"]["kf"]
        # the BA window: K1 is a local frame, its surviving created points are in, no culled point is
        win = chained.store.ba_window(ra)
        assert ref["r2"]["kf"] - 1 in win["local_kf"] and not set(win["l2g"]) & set(cull["culled"])
        assert set(created[2:6]) <= set(win["l2g"])
        want = B.gather(s, ref["geom"], ref["r2"]["kf"])
        assert np.array_equal(win["l2g"], want["l2g"]) and np.array_equal(win["obs_point"], want["obs_point"])
        # the emptied frame slots are what the next motion stage reads
        k2 = ref["k2"]
        n = k2["n_cur"]
        for arm in (chained, waited):
            st, g = arm.s2["slots"].numpy(), arm.s2["gid"].numpy()
            assert np.array_equal(st["state"][:n], cull["state"]) and np.array_equal(g[:n], cull["gid"])
            assert list(st["state"][n - 6:n]) == [R.EMPTY] * 2 + [R.LOCKED] * 4 and list(g[n - 6:n]) == [-1, -1] + created[2:6]
        # the next frame's UpdateLocalMap no longer lists them: a frame that still holds c0, c6 and c2
        gids = [created[0], created[6], created[2], 0, 1, 2]
        probe = CH.Probe(ctx, gids)
        probe.lmap.free()
        caps = k2["caps"]
        probe.lmap = LocalMap(ctx, 1024, caps["max_kf"], caps["max_points"])
        probe.lmap.fill()
        try:
            probe.update(chained.store)
            got = probe.read()
        finally:
            probe.free()
        up = A.LocalMapResult.from_buffer_copy(got["rec"].tobytes()[:C.sizeof(A.LocalMapResult)])
        assert up.status == 0 and up.n_nulled == 2 and list(got["gid"][:3]) == [-1, -1, created[2]]
        local = set(int(p) for p in got["l2g"][:up.n_local])
        assert created[2] in local and not local & set(cull["culled"])
    finally:
        chained.free()
        waited.free()
