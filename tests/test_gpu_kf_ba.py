"""GPU: the keyframe store's geometry and the local bundle adjustment fed from the store (lorb_kf_store_create_geom /
_geom_read, lorb_kf_store_ba_gather_dev, lorb_kf_store_local_ba_dev, lorb_kf_ba_window_read;
lorb_slam_amd.frame.KeyframeStore / keyframe_local_ba).

1. Insertion geometry: after the cases of tests/kf_store_cases.py, and after chain_frames()' four insertions behind
   one wait, kf_pose, kf_slot_uv and obs_slot equal the restatement (tests/kf_ba_ref.py) bit for bit, the invariant
   holds, every output the existing insertion tests compare keeps its bits, and the bytes past the counts are
   untouched.
2. Gather: the window equals the restatement -- integer arrays equal, float arrays equal as bytes -- on the hand
   case, generated stores and the sizes where the kernels change path; the statuses; the store is not touched.
3. Solve: the kf_pose rows of the local frames and the pos rows of l2g agree with oracle.ba_local run on the window
   read back, |gpu - float32(oracle)| <= 1e-5 max(|oracle|, 1) (RTOL of tests/test_gpu_ba.py), with the oracle's
   iteration count and termination and its final cost within 1e-8; every other byte of the store is unchanged.
4. Chain: an insertion and the local BA on its record's kf and status words, nothing between them, equal
   insert -> wait -> local BA; lorb_local_map_update_dev on the view afterwards gathers the refined pos rows.
Sentinel bytes sit past every count in the old and the new arrays."""
import copy
import ctypes as C

import numpy as np
import pytest

import kf_ba_cases as BC
import kf_ba_ref as B
import kf_store_cases as KC
import kf_store_ref as R
import oracle as O
import test_gpu_kf_store as KS
import test_gpu_kf_store_chain as CH
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, KeyframeStore, LocalMap, keyframe_ba_record, keyframe_ba_result, keyframe_insert,
                                 keyframe_insert_result, keyframe_local_ba)
from lorb_slam_amd.runtime import LorbError, lib

pytestmark = pytest.mark.gpu

G, SENT, FILL, SENT_I32 = KS.G, KS.SENT, KS.FILL, KS.SENT_I32
REC = C.sizeof(A.KfBaResult)
RTOL = 1e-5  # tests/test_gpu_ba.py
POSE6 = np.array([0.02, -0.01, 0.03, 0.3, -0.2, 1.5], np.float32)
raw, sentinel = KS.raw, KS.sentinel
WINDOW_INT, WINDOW_FLOAT = ("local_kf", "fixed_kf", "l2g", "obs_point", "obs_frame"), ("pose_init", "fixed_pose", "point_init", "obs_uv")


def pose_value(pose, pose6):
    p = KS.pose_value(pose)
    p.pose[:] = [float(v) for v in pose6]
    return p


def arrays_of(store):
    a = {k: v.numpy() for k, v in store.arrays.items()}
    a.update({k: v.numpy() for k, v in store.geometry.items()})
    return a


def geometry_tails_untouched(store, cn):
    past = dict(kf_pose=cn["n_kf"], kf_slot_uv=cn["n_kf_slots"], obs_slot=cn["n_obs"])
    for k, arr in store.geometry.items():
        assert sentinel(arr.numpy()[past[k]:]), k


def same_geometry(store, geom):
    got, want = store.read_geometry(), B.flat_geometry(geom)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(raw(got[k]), raw(want[k])), k


# -- 1. insertion geometry -------------------------------------------------------------------------------------------
class GeomRig(KS.Rig):
    """KS.Rig on a store made with geometry, the pose block carrying a pose vector."""

    def __init__(self, ctx, c, geom, pose6=POSE6):
        super().__init__(ctx, c)
        s, k = c["store"], c["caps"]
        has = bool(len(s["kf_bad"]) or s["n_points"])
        self.store.free()
        self.store = KeyframeStore(ctx, k["max_kf"], k["max_points"], k["max_obs"], k["max_kf_slots"], init=s if has else None,
                                   geom=geom if has else None)
        self.store.fill(R.counts(s))
        self.store.fill_geometry(R.counts(s))
        self.pose.free()
        self.pose = DeviceBlock(ctx, A.FramePose, pose_value(c["pose"], pose6))


@pytest.mark.parametrize("name", sorted(KS.CASES))
def test_insertion_geometry(ctx, name):
    c = copy.deepcopy(KS.CASES[name])
    rows = copy.deepcopy(c["store"]["kf_slots"])
    g0 = BC.geometry_for(c["store"], seed=len(name))
    assert c["store"]["kf_slots"] == rows  # the hand cases hold every point they observe
    rig = GeomRig(ctx, c, g0)
    try:
        before = {k: v.numpy() for k, v in rig.store.geometry.items()}
        rig.insert()
        r = rig.read()
        ref = KS.reference(c)
        KS.check(rig, r, ref)  # every output the insertion tests compare keeps its bits
        g = B.insert_geometry(g0, ref, c["frame"], POSE6, c["n_cur"])
        B.check_invariant(ref["store"], g)
        same_geometry(rig.store, g)
        geometry_tails_untouched(rig.store, R.counts(ref["store"]))
        # the invariant on what the device holds
        st, dg = r["store"], rig.store.read_geometry()
        off = st["csr"]["kf_slot_off"]
        o = 0
        for p, obs in enumerate(st["obs"]):
            for f in obs:
                assert st["csr"]["kf_slot_point"][off[f] + dg["obs_slot"][o]] == p, (p, f)
                o += 1
        if not ref["inserted"]:
            for k, v in rig.store.geometry.items():
                assert np.array_equal(raw(v.numpy()), raw(before[k])), k
    finally:
        rig.free()


def test_chain_insertion_geometry_behind_one_wait(ctx):
    fs = KC.chain_frames()
    refs = KC.chain_restate(fs)
    store = KeyframeStore(ctx, **KC.CHAIN_CAPS)
    store.fill(R.counts(R.empty_store()))
    store.fill_geometry(R.counts(R.empty_store()))
    steps = [CH.Step(ctx, c, [0]) for c in fs]
    poses = [POSE6 * (i + 1) for i in range(len(fs))]
    try:
        for st, p in zip(steps, poses):
            st.pose.upload(pose_value(st.c["pose"], p))
        for st in steps:  # four calls, no wait
            keyframe_insert(ctx, store, st.c["fp"], st.frame, st.slots, st.gid, st.pose, st.rec, n_max_cur=KC.CHAIN_N_MAX,
                            gate=st.c["gate"])
        ctx.sync()
        g = B.empty_geometry()
        for c, ref, p in zip(fs, refs, poses):
            g = B.insert_geometry(g, ref, c["frame"], p, c["n_cur"])
        final = refs[-1]["store"]
        B.check_invariant(final, g)
        KS.same_store(store.read(), final)
        same_geometry(store, g)
        geometry_tails_untouched(store, R.counts(final))
    finally:
        for st in steps:
            st.free()
        store.free()


# -- 2. gather -------------------------------------------------------------------------------------------------------
class BaRig:
    """A store with geometry a few rows larger than its counts, sentinel bytes behind every count; the device words
    the call reads and its record."""

    def __init__(self, ctx, case, slack=5, geom=True):
        self.ctx, self.case = ctx, case
        s = case["store"]
        cn = self.cn = R.counts(s)
        self.store = KeyframeStore(ctx, cn["n_kf"] + slack, cn["n_points"] + slack, cn["n_obs"] + slack, cn["n_kf_slots"] + slack,
                                   init=s, geom=case["geom"] if geom else None)
        self.store.fill(cn)
        self.store.fill_geometry(cn)
        self.words = ctx.to_device(np.array([case["kf"], 0] + [FILL] * G, np.int32))  # d_kf, d_src_status
        self.rec = keyframe_ba_record(ctx)
        self.fp = case.get("fp") or KC.synth.frame_params()

    def set(self, kf, src_status=0):
        v = np.array([kf, src_status], np.int32)
        self.ctx.check(lib().lorb_memcpy_h2d(self.ctx.handle, self.words.ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(8)), "h2d")

    def run(self, **kw):
        self.ctx.check(lib().lorb_memset_dev(self.ctx.handle, self.rec.ptr, C.c_int(SENT), C.c_size_t(REC)), "memset")
        d = self.words.ptr.value
        return keyframe_local_ba(self.ctx, self.store, self.fp, d, self.rec, d_src_status=d + 4, **kw)

    def record(self):
        b = self.rec.numpy()
        assert sentinel(b[REC:])
        return A.KfBaResult.from_buffer_copy(b.tobytes()[:REC])

    def free(self):
        for a in (self.store, self.words, self.rec):
            a.free()


def same_record(rec, want):
    for f in B.FIELDS:
        assert getattr(rec, f) == want.get(f, SENT_I32), (f, getattr(rec, f), want.get(f))


def same_window(got, ref):
    for k in WINDOW_INT:
        assert np.array_equal(got[k], ref[k]), k
    for k in WINDOW_FLOAT:
        assert got[k].shape == ref[k].shape and np.array_equal(raw(got[k]), raw(np.asarray(ref[k], np.float32))), k


def gather_and_compare(rig, kf=None, src_status=0):
    case = rig.case
    kf = case["kf"] if kf is None else kf
    rig.set(kf, src_status)
    before = arrays_of(rig.store)
    rig.run(gather_only=True)
    rec = rig.record()
    ref = B.gather(case["store"], case["geom"], kf, src_status)
    same_record(rec, ref["rec"])
    if ref["rec"]["status"] in (0, 3):
        same_window(rig.store.ba_window(rec), ref)
    after = arrays_of(rig.store)
    for k in before:  # the gather reads the store
        assert np.array_equal(raw(after[k]), raw(before[k])), k
    return rec, ref


def gather_cases():
    c = dict(hand=BC.hand_case(), random_a=BC.random_case(9, 300, seed=1), random_b=BC.random_case(40, 2500, seed=2, obs_per_point=6),
             random_mid=BC.random_case(12, 700, seed=3, kf=5))
    c.update(BC.size_cases())
    return c


GATHER = gather_cases()


@pytest.mark.parametrize("name", sorted(GATHER))
def test_gather(ctx, name):
    rig = BaRig(ctx, GATHER[name])
    try:
        rec, ref = gather_and_compare(rig)
        assert rec.status == 0, name
        if name == "hand":
            w = rig.store.ba_window(rec)
            for k, v in rig.case["want"].items():
                if k != "rec":
                    assert w[k].tolist() == v, k
    finally:
        rig.free()


def test_gather_statuses(ctx):
    """kf = -1, a keyframe past the count and a non-zero source status: status 1 and nothing else, no error.  A window
    without points: status 3.  Then a good call on the same store."""
    rig = BaRig(ctx, BC.hand_case())
    try:
        for kf, src in ((-1, 0), (6, 0), (5, 7)):
            rec, _ = gather_and_compare(rig, kf, src)
            assert rec.status == 1 and rec.kf == SENT_I32
        with pytest.raises(LorbError, match="no window"):
            rig.store.ba_window(A.KfBaResult())
        rec, _ = gather_and_compare(rig)
        assert rec.status == 0 and rec.n_points == 4
    finally:
        rig.free()
    s = KC.make_store([[0]], [0], [[0]], [[]], [{}], is_bad=[1])
    g = dict(kf_pose=[np.zeros(6, np.float32)], kf_slot_uv=[np.zeros((1, 2), np.float32)], obs_slot=[[0]])
    rig = BaRig(ctx, dict(store=s, geom=g, kf=0))
    try:
        rec, _ = gather_and_compare(rig)
        assert rec.status == 3 and rec.n_points == 0
        assert rig.run(summary=True) == A.BASummary().as_dict() and rig.record().written == 0  # nothing is solved
    finally:
        rig.free()


@pytest.mark.parametrize("name,status", [("local_129", 2), ("obs_256", 4)])
def test_unsupported_windows(ctx, name, status):
    """129 local frames -> status 2 and nothing else written; a point with 256 usable observations -> status 4.  Both
    return LORB_E_UNSUPPORTED with the store untouched, from the gather and from the solving call, and the next good
    call gives the window it gives alone."""
    rig = BaRig(ctx, BC.status_cases()[name])
    try:
        before = arrays_of(rig.store)
        for kw in (dict(gather_only=True), dict()):
            with pytest.raises(LorbError, match="rc=-4"):
                rig.run(**kw)
            rec = rig.record()
            assert rec.status == status and rec.written in (0, SENT_I32)
            if status == 2:
                same_record(rec, dict(status=2))
            after = arrays_of(rig.store)
            for k in before:
                assert np.array_equal(raw(after[k]), raw(before[k])), k
        rec, _ = gather_and_compare(rig, len(rig.case["store"]["kf_bad"]) - 1)  # the spare keyframe
        assert rec.status == 0 and rec.n_points == 1
    finally:
        rig.free()


def test_a_store_without_geometry_is_refused(ctx):
    rig = BaRig(ctx, BC.hand_case(), geom=False)
    try:
        for kw in (dict(gather_only=True), dict()):
            with pytest.raises(LorbError, match="rc=-1.*geometry"):
                rig.run(**kw)
        assert sentinel(rig.rec.numpy())
    finally:
        rig.free()
    with pytest.raises(LorbError, match=r"geom: obs_slot\[8\] = 1 \(point 7 in keyframe 3\) names a slot that holds 2"):
        c = BC.hand_case()
        c["geom"]["obs_slot"][7][1] = 1
        BaRig(ctx, c)
    with pytest.raises(LorbError, match="outside the keyframe's 3 slots"):
        c = BC.hand_case()
        c["geom"]["obs_slot"][7][1] = 3
        BaRig(ctx, c)


# -- 3. solve --------------------------------------------------------------------------------------------------------
def close(a, b):
    b32 = np.asarray(b, np.float64).astype(np.float32).astype(np.float64)
    return np.abs(np.asarray(a, np.float64) - b32) <= RTOL * np.maximum(np.abs(np.asarray(b, np.float64)), 1.0)


def check_solution(store, win, summary, before, moved=True):
    """The store after the write-back against the oracle on the window that was solved, and against `before`
    everywhere else."""
    Po, Xo, so = O.ba_local([win])
    after = arrays_of(store)
    pose, pos = after["kf_pose"][win["local_kf"]], after["pos"][win["l2g"]]
    ep = np.abs(pose - Po[0].astype(np.float32)) / np.maximum(np.abs(Po[0]), 1.0)
    ex = np.abs(pos - Xo[0].astype(np.float32)) / np.maximum(np.abs(Xo[0]), 1.0)
    print(f"local BA on the store: max relative difference poses {ep.max():.3e} points {ex.max():.3e}; gpu {summary}; oracle {so[0]}")
    assert close(pose, Po[0]).all() and close(pos, Xo[0]).all()
    assert summary["iterations"] == so[0]["iterations"] and summary["termination"] == so[0]["termination"], (summary, so)
    assert abs(summary["final_cost"] - so[0]["final_cost"]) <= 1e-8 * so[0]["final_cost"], (summary, so)
    assert np.array_equal(raw(pose), raw(before["kf_pose"][win["local_kf"]])) != moved  # something was refined
    # every other byte: rows outside the window, all other columns, lists, counts' tails
    want = {k: v.copy() for k, v in before.items()}
    want["kf_pose"][win["local_kf"]] = pose
    want["pos"][win["l2g"]] = pos
    for k in want:
        assert np.array_equal(raw(after[k]), raw(want[k])), k


def test_local_ba_against_the_oracle(ctx):
    rig = BaRig(ctx, BC.solve_scene())
    try:
        before = arrays_of(rig.store)
        counts = rig.store.counts()
        summary = rig.run(summary=True)
        rec = rig.record()
        ref = B.gather(rig.case["store"], rig.case["geom"], rig.case["kf"])
        same_record(rec, dict(ref["rec"], written=1))
        win = rig.store.ba_window(rec)
        same_window(win, ref)
        check_solution(rig.store, win, summary, before)
        assert rig.store.counts() == counts
        # a second call: the camera count is resident, the window is gathered from the refined store, on which the
        # LM ends at once as the oracle's does (no successful step: the rows keep their bits)
        before = arrays_of(rig.store)
        summary = rig.run(summary=True)
        win2 = rig.store.ba_window(rig.record())
        assert np.array_equal(raw(win2["pose_init"]), raw(before["kf_pose"][win["local_kf"]]))
        check_solution(rig.store, win2, summary, before, moved=summary["successful_steps"] > 0)
    finally:
        rig.free()


# -- 4. chain --------------------------------------------------------------------------------------------------------
class ChainArm:
    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        self.rig = GeomRig(ctx, sc["case"], sc["geom"], sc["pose6"])
        self.store = self.rig.store
        self.ba_rec = keyframe_ba_record(ctx)

    def insert(self):
        self.rig.insert()

    def local_ba(self):
        rec = self.rig.rec.ptr.value
        keyframe_local_ba(self.ctx, self.store, self.sc["fp"], rec + A.KfInsertResult.kf.offset, self.ba_rec,
                          d_src_status=rec + A.KfInsertResult.status.offset)

    def free(self):
        self.rig.free()
        self.ba_rec.free()


def test_chain_insertion_then_local_ba(ctx):
    sc = BC.chain_scene()
    chained, waited = ChainArm(ctx, sc), ChainArm(ctx, sc)
    try:
        chained.insert()   # nothing between the two calls
        chained.local_ba()
        waited.insert()
        ctx.sync()
        assert keyframe_insert_result(waited.rig.rec).inserted == 1
        mid = arrays_of(waited.store)
        waited.local_ba()
        ctx.sync()
        a, b = arrays_of(chained.store), arrays_of(waited.store)
        for k in a:
            assert np.array_equal(raw(a[k]), raw(b[k])), k
        ra, rb = keyframe_ba_result(chained.ba_rec), keyframe_ba_result(waited.ba_rec)
        assert bytes(ra) == bytes(rb) and ra.status == 0 and ra.written == 1 and ra.kf == 7 and ra.n_points == 340
        win = chained.store.ba_window(ra)
        assert not np.array_equal(raw(b["pos"][win["l2g"]]), raw(mid["pos"][win["l2g"]]))
        # the next frame's UpdateLocalMap reads the refined rows
        gids = [int(p) for p in win["l2g"][[0, 1, 2, -3, -2, -1]]]
        probe = CH.Probe(ctx, gids)
        probe.lmap.free()
        caps = sc["case"]["caps"]
        probe.lmap = LocalMap(ctx, 512, caps["max_kf"], caps["max_points"])
        probe.lmap.fill()
        try:
            probe.update(chained.store)
            got = probe.read()
        finally:
            probe.free()
        n_local = A.LocalMapResult.from_buffer_copy(got["rec"].tobytes()[:C.sizeof(A.LocalMapResult)]).n_local
        assert n_local >= len(gids)
        for p in gids:
            row = int(np.nonzero(got["l2g"][:n_local] == p)[0][0])
            assert np.array_equal(raw(got["pos"][row]), raw(a["pos"][p])), p
    finally:
        chained.free()
        waited.free()
