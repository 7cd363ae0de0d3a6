"""GPU: lorb_kf_store_retire_dev in the chain, on the scene of tests/kf_store_cases.py.

chain_frames()' four insertions grow a store from empty to three keyframes; two more frames (LORB_KF_GATE_NONE) hold
p0, p1, p2, p10, p11 and p15 again, so that the store has five keyframes and points with five observations.  Every
frame has its own id (the frame word), so every keyframe can be retired.  Then, enqueued with nothing between them
and ONE wait at the end:
    retire [4, 0] with the last insertion's kf word protected (keyframe 4 is skipped, keyframe 0 goes: p0, p1, p2 keep
    four observations and a new first observer, p3 .. p9 die)
    -> lorb_local_map_update_dev            against the same call on the restated store
    -> lorb_kf_store_ba_gather_dev          the window is the restatement's; keyframe 0 is neither pose nor fixed frame
    -> lorb_kf_store_refresh_dev            bit-exact against tests/kf_refresh_ref.py on the restated lists
    -> lorb_kf_store_compact_dev            every point the cascade killed is dropped
    -> lorb_kf_store_insert_dev once more   UpdateConnections never counts keyframe 0; the store is the restatement's
One case runs the call behind a failed insertion's status word and expects a no-op."""
import ctypes as C

import numpy as np
import pytest

import kf_ba_ref as B
import kf_compact_ref as M
import kf_cull_ref as L
import kf_refresh_ref as RR
import kf_retire_ref as T
import kf_store_cases as KC
import kf_store_ref as R
import test_gpu_kf_ba as KB
import test_gpu_kf_cull as CU
import test_gpu_kf_store as KS
import test_gpu_kf_store_chain as CH
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (KeyframeStore, keyframe_ba_record, keyframe_ba_result, keyframe_compact_record,
                                 keyframe_compact_result, keyframe_insert, keyframe_insert_result, keyframe_local_ba,
                                 keyframe_refresh, keyframe_refresh_record, keyframe_refresh_result, keyframe_retire,
                                 keyframe_retire_record, keyframe_retire_result)

pytestmark = pytest.mark.gpu

G, FILL, SENT_I32 = KS.G, KS.FILL, KS.SENT_I32
raw = KS.raw
CAPS, N_MAX = KC.CHAIN_CAPS, KC.CHAIN_N_MAX
HELD = [0, 1, 2, 10, 11, 15]
PROBE = [0, 1, 2, 10, 11, 15]      # six points that live on
LIST = [4, 0]
STAGES = ("update", "gather", "refresh", "compact", "insert")


def extra_frame(seed, gate=R.GATE_NONE):
    c = KC.case(R.empty_store(), [KC.LOCKED] * 6 + [KC.EMPTY] * 4, HELD + [-1] * 4, {}, caps=CAPS, gate=gate, seed=seed)
    c["n_max_cur"] = N_MAX
    return c


def scene():
    """The six frames and the restated store, geometry, life and appearance after them."""
    fs = KC.chain_frames() + [extra_frame(44), extra_frame(45)]
    poses = [KB.POSE6 * (i + 1) for i in range(len(fs))]
    s, g, life, app, refs = R.empty_store(), B.empty_geometry(), L.new_life(0, 0), dict(kf_slot_desc=[], kf_slot_octave=[],
                                                                                         kf_center=np.zeros((0, 3), np.float32)), []
    for i, (c, p) in enumerate(zip(fs, poses)):
        life["frame_word"] = 10 * (i + 1)
        ref = R.insert_keyframe(s, CAPS, c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], N_MAX, c["gate"])
        g = B.insert_geometry(g, ref, c["frame"], p, c["n_cur"])
        life = L.insert_life(life, s, c["frame"], c["slots"], c["gid"], ref)
        app = RR.insert_appearance(app, ref, c["frame"], c["pose"], c["n_cur"])
        s = ref["store"]
        refs.append(ref)
    assert len(s["kf_bad"]) == 5 and s["obs"][0] == [0, 1, 2, 3, 4] and s["obs"][3] == [0, 1] and list(life["kf_fid"]) == [10, 20, 40, 50, 60]
    return dict(fs=fs, poses=poses, store=s, geom=g, life=life, app=app, refs=refs)


class Chain:
    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        self.store = KeyframeStore(ctx, **CAPS)
        empty = R.counts(R.empty_store())
        self.store.fill(empty)
        self.store.fill_geometry(empty)
        self.store.fill_life(empty)
        self.steps = [CH.Step(ctx, c, PROBE) for c in sc["fs"]]
        self.no = CU.Nothing(ctx)
        self.list = ctx.to_device(np.array(LIST + [len(LIST)] + [FILL] * G, np.int32))   # the list, then its count word
        self.trec, self.brec, self.rrec, self.mrec = (keyframe_retire_record(ctx), keyframe_ba_record(ctx),
                                                     keyframe_refresh_record(ctx), keyframe_compact_record(ctx))
        self.last = extra_frame(46)
        self.last_step = CH.Step(ctx, self.last, PROBE)
        for st, p in zip(self.steps, sc["poses"]):
            st.pose.upload(KB.pose_value(st.c["pose"], p))

    def insertions(self):
        for i, st in enumerate(self.steps):
            self.no.observe(self.ctx, self.store, 10 * (i + 1))
            keyframe_insert(self.ctx, self.store, st.c["fp"], st.frame, st.slots, st.gid, st.pose, st.rec, n_max_cur=N_MAX, gate=st.c["gate"])

    def retire(self, status_of=None):
        ir = self.steps[-1].rec.ptr.value
        keyframe_retire(self.ctx, self.store, self.list, self.list.ptr.value + 4 * len(LIST), self.trec, n_max_list=len(LIST),
                        protect=ir + A.KfInsertResult.kf.offset, n_protect=1,
                        d_src_status=(ir if status_of is None else status_of) + A.KfInsertResult.status.offset)

    def run(self, stage):
        """Everything up to `stage`, no wait; then the one wait."""
        ctx, st, fp = self.ctx, self.store, self.sc["fs"][0]["fp"]
        ir = self.steps[-1].rec.ptr.value
        d_kf, d_st = ir + A.KfInsertResult.kf.offset, ir + A.KfInsertResult.status.offset
        self.insertions()
        self.retire()
        if stage == "update":
            self.steps[-1].probe.update(st)
        if stage in ("gather", "refresh"):
            keyframe_local_ba(ctx, st, fp, d_kf, self.brec, d_src_status=d_st, gather_only=True)
        if stage == "refresh":
            keyframe_refresh(ctx, st, fp, self.brec, self.rrec)
        if stage == "compact":
            st.compact(self.mrec, d_src_status=d_st)
        if stage == "insert":
            s = self.last_step
            keyframe_insert(ctx, st, s.c["fp"], s.frame, s.slots, s.gid, s.pose, s.rec, n_max_cur=N_MAX, gate=s.c["gate"])
        ctx.sync()

    def free(self):
        for a in (self.store, self.no, self.list, self.trec, self.brec, self.rrec, self.mrec, self.last_step, *self.steps):
            a.free()


def restated_retire(sc):
    ref = T.retire(sc["store"], sc["geom"]["obs_slot"], sc["life"], LIST, protect=[4])
    r = ref["rec"]
    assert ref["V"] == [0] and r["n_skip_protected"] == 1 and sorted(ref["dead"]) == list(range(3, 10))
    assert ref["store"]["obs"][0] == [1, 2, 3, 4] and r["n_obs_erased"] == 3 and r["n_conn_erased"] > 0
    return ref


@pytest.mark.parametrize("stage", STAGES)
def test_retire_in_the_chain(ctx, stage):
    sc = scene()
    ref = restated_retire(sc)
    s1, geom1 = ref["store"], dict(sc["geom"], obs_slot=ref["obs_slot"])
    ch = Chain(ctx, sc)
    try:
        ch.run(stage)
        CU.same_record(keyframe_retire_result(ch.trec), ref["rec"], T.FIELDS)
        if stage == "update":
            # the retired keyframe is in no list and gets no vote that counts: the call on the restated store
            assert s1["kf_bad"][0] == 1 and not any(0 in c for c in s1["cov"])
            CH.assert_same_update(ch.steps[-1].probe.read(), CH.exact_update(ctx, s1, PROBE), s1, bounds=True)
            KS.same_store(ch.store.read(), s1)
            KB.same_geometry(ch.store, geom1)
            CU.same_life(ch.store, sc["life"], R.counts(s1))
        if stage in ("gather", "refresh"):
            rec = keyframe_ba_result(ch.brec)
            want = B.gather(s1, geom1, 4)
            KB.same_record(rec, want["rec"])
            win = ch.store.ba_window(rec)
            KB.same_window(win, want)
            assert rec.status == 0 and 0 not in list(win["local_kf"]) and 0 not in list(win["fixed_kf"]) and rec.n_obs_bad_kf == 0
        if stage == "refresh":
            rr = RR.refresh(s1, geom1, sc["app"], dict(kf=4, local_kf=win["local_kf"], l2g=win["l2g"]), sc["app"]["kf_center"],
                            sc["fs"][0]["fp"])
            got = keyframe_refresh_result(ch.rrec)
            for f in RR.FIELDS:
                assert getattr(got, f) == rr["rec"].get(f, SENT_I32), f
            assert got.n_refreshed > 0 and {0, 1, 2} <= set(int(v) for v in win["l2g"])    # their mpRefKF is keyframe 1 now
            after = ch.store.read()
            for k in ("normal", "max_dist", "min_dist", "desc"):
                assert np.array_equal(raw(after[k]), raw(np.asarray(rr[k], after[k].dtype))), k
        if stage == "compact":
            cm = M.compact_store(s1, ref["obs_slot"], sc["life"])
            got = keyframe_compact_result(ch.mrec)
            for f in M.FIELDS:
                assert getattr(got, f) == cm["rec"].get(f, SENT_I32), f
            assert set(ref["dead"]) <= set(cm["dropped"]) and got.n_dropped >= len(ref["dead"])
            assert got.n_bad_kept == sum(1 for p in range(s1["n_points"]) if s1["is_bad"][p] and p not in cm["dropped"])
            KS.same_store(ch.store.read(), cm["store"])
            KB.same_geometry(ch.store, dict(geom1, obs_slot=cm["obs_slot"]))
        if stage == "insert":
            c = ch.last
            ins = R.insert_keyframe(s1, CAPS, c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], N_MAX, c["gate"])
            got = keyframe_insert_result(ch.last_step.rec)
            for f in R.FIELDS:
                assert getattr(got, f) == ins["rec"].get(f, SENT_I32), f
            assert got.inserted == 1 and got.kf == 5 and 0 not in ins["store"]["conn"][5] and 0 not in ins["store"]["cov"][5]
            KS.same_store(ch.store.read(), ins["store"])
    finally:
        ch.free()


def test_retire_behind_a_failed_insertion_is_a_no_op(ctx):
    """The last insertion's count is out of range: its record says status 1, and the retirement wired to that word
    stores status 1 and nothing else."""
    sc = scene()
    ch = Chain(ctx, sc)
    try:
        ch.insertions()
        s = ch.last_step
        s.frame.set(N_MAX + 1)
        keyframe_insert(ctx, ch.store, s.c["fp"], s.frame, s.slots, s.gid, s.pose, s.rec, n_max_cur=N_MAX, gate=s.c["gate"])
        ch.retire(status_of=s.rec.ptr.value)
        ctx.sync()
        assert keyframe_insert_result(s.rec).status == 1
        CU.same_record(keyframe_retire_result(ch.trec), dict(status=1), T.FIELDS)
        KS.same_store(ch.store.read(), sc["store"])
        KB.same_geometry(ch.store, sc["geom"])
        CU.same_life(ch.store, sc["life"], R.counts(sc["store"]))
    finally:
        ch.free()
