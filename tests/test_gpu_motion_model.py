"""GPU: the pose hand-over between frames in device memory -- lorb_track_motion_frames_pose_dev (the motion
stage with its three poses read from lorb_frame_pose / lorb_motion_model blocks, the motion-model
prediction in its first launch) and lorb_frame_pose_finish_dev (the frame's block and mTcc from the local
stage's record) -- so that any number of frames is enqueued behind one another and waited for once.

The scene is tests/test_gpu_track_local_frames.py's (case "320x256", frame A INITIALIZE-filled at the
identity, B the same bands DX further), the map store tests/test_gpu_local_map_chain.py's.  What a result
is compared with: the blocks against the numpy restatement tests/motion_model_ref.py (Tcw, Twc, Tcc and the
translation bit for bit, the Rodrigues vector within its derived tolerance); every other output against
lorb_track_motion_frames_dev on the same poses as host values, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lorb_slam_amd.window as W
import motion_model_ref as M
import test_gpu_local_map_chain as LMC
import test_gpu_track_frames as TR
import test_gpu_track_local_frames as TLF
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceMapStore, LocalFramesOut, LocalMap, enqueue_track_motion_frames,
                                 enqueue_track_motion_frames_pose, fill_slots, frame_pose_finish, frame_pose_from_Tcw,
                                 local_map_buffers, local_map_ids_back, local_map_update, model_block,
                                 motion_record_addresses, pose_block, track_local_frames)
from test_gpu_track_frames import builders  # noqa: F401 -- the module-scoped builder fixture

pytestmark = pytest.mark.gpu

G, SENT, FILL, I4 = W.ORB_GUARD, W.ORB_SENTINEL, TR.FILL, TR.I4
EMPTY = A.LORB_SLOT_EMPTY
INIT = A.LORB_SLOTS_INITIALIZE
DX, TH = TLF.DX, LMC.TH
LOCAL_MIN = 5  # the local stage's min_matches in the whole-frame tests: behind a motion stage that has matched most of
# the scene the search at th = 2 finds 15, 9 and 9 new points in the three frames (20, the default, would fail the gate)
DX_RETRY = 0.9  # a prediction this far off leaves pass 1 with 15 matches, the retry with 36 (the oracle; asserted below)
MREC, LREC = C.sizeof(A.TrackFramesResult), C.sizeof(A.TrackLocalFramesResult)
POSE, MODEL = C.sizeof(A.FramePose), C.sizeof(A.MotionModel)
SENT_I32 = TLF.SENT_I32
same = TLF.same


def shift(dx=0.0, dz=0.0):
    T = I4.copy()
    T[0, 3], T[2, 3] = dx, dz
    return T


def mat(a):
    return np.array(a[:], np.float32).reshape(4, 4)


def block_dict(b):
    """An A.FramePose as the restatement's dict."""
    return dict(Tcw=mat(b.Tcw), Twc=mat(b.Twc), pose=np.array(b.pose[:], np.float32), status=b.status)


def assert_block(got, ref, what, s=None):
    """A device block against the restatement: everything bit for bit, or -- with s, the restatement's
    |r| / 2 -- the Rodrigues vector within M.vec_tol."""
    g = block_dict(got)
    assert g["status"] == ref["status"] == 0, what
    assert same(g["Tcw"], ref["Tcw"]) and same(g["Twc"], ref["Twc"]) and same(g["pose"][3:], ref["pose"][3:]), what
    if s is None:
        assert same(g["pose"][:3], ref["pose"][:3]), what
    else:
        err = np.abs(g["pose"][:3].astype(np.float64) - ref["pose"][:3].astype(np.float64))
        print(what, "s", s, "|dev - ref|", err, "tolerance", M.vec_tol(ref["pose"][:3], s))
        assert M.vec_close(g["pose"][:3], ref["pose"][:3], s), what


class Stage:
    """The motion stage's device objects on a Built pair: the last frame's slots INITIALIZE-filled at the
    identity, the current frame's, assign and the record, each with its guard band."""

    def __init__(self, ctx, bt, S, N, cur_entry=None):
        self.ctx, self.bt, self.S, self.N = ctx, bt, S, N
        self.ls = bt.slots(N, TR.entry_slots(N))
        fill_slots(ctx, S["fp"], I4, bt.fa, self.ls, INIT)
        self.cs = bt.slots(N, cur_entry or TR.entry_slots(N))
        self.masg = ctx.to_device(np.full(N + G, FILL, np.int32))
        self.mrec = ctx.to_device(np.full(MREC + G, SENT, np.uint8))
        bt.held += [self.masg, self.mrec]

    def pose_form(self, cur_pose, last_pose, model, **kw):
        enqueue_track_motion_frames_pose(self.ctx, self.S["fp"], cur_pose, self.bt.fb, self.cs, last_pose, model, self.bt.fa,
                                         self.ls, self.masg, self.mrec, n_max_cur=self.N, n_max_last=self.N, **kw)

    def host_form(self, cur_Tcw, pose_init, last_Tcw, **kw):
        enqueue_track_motion_frames(self.ctx, self.S["fp"], cur_Tcw, pose_init, self.bt.fb, self.cs, last_Tcw, self.bt.fa,
                                    self.ls, self.masg, self.mrec, n_max_cur=self.N, n_max_last=self.N, **kw)

    def read(self):
        raw = self.mrec.numpy()
        return dict(rec=A.TrackFramesResult.from_buffer_copy(raw.tobytes()[:MREC]), mrec=raw, masg=self.masg.numpy(),
                    cur=self.cs.numpy(), last=self.ls.numpy())


def assert_same_stage(a, b, what):
    assert same(a["mrec"], b["mrec"]), (what, "record")
    assert same(a["masg"], b["masg"]), (what, "assign")
    for side in ("cur", "last"):
        for k in ("state", "pos", "desc"):
            assert same(a[side][k], b[side][k]), (what, side, k)


def bound(S):
    return max(S["n_last"], S["n_cur"]) + 1


# 1 -- the prediction block ---------------------------------------------------------------------------------------
def test_prediction_block(ctx, builders):
    """d_model given: d_cur_pose = Frame::SetPose(last.Tcw * Tcc) for the hand poses and five seeded ones
    as the last frame's pose, the model a translation of DX along x."""
    S = TLF.scene()
    Tcc = shift(DX)
    poses = M.hand_poses() + [(f"seeded_{i}", T) for i, T in enumerate(M.seeded_poses(5, 77))]
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        st = Stage(ctx, bt, S, bound(S))
        model = model_block(ctx, Tcc)
        bt.held.append(model)
        for name, T in poses:
            last = M.set_pose(T)
            ref = M.predict(last, Tcc)
            assert ref["s"] is None or abs(ref["s"] - 1e-5) > 1e-9, name  # both sides take the same branch
            lp, cp = pose_block(ctx, T), pose_block(ctx)
            bt.held += [lp, cp]
            st.pose_form(cp, lp, model)
            r = st.read()
            assert r["rec"].status == 0, name
            raw = cp.numpy()
            assert (raw[POSE:] == SENT).all(), name
            assert_block(cp.read(), ref, name, s=ref["s"] or 0.0)
            assert same(lp.numpy()[:POSE], np.frombuffer(bytes(frame_pose_from_Tcw(T)), np.uint8)), name  # read only
            assert same(model.numpy()[:MODEL + G], model.numpy()) and model.read().status == 0


# 2 -- the pose form equals the host form ---------------------------------------------------------------------------
def motion_direction(fp, cur_Tcw, last_Tcw):
    """(mode_forward, mode_backward) of src/matcher.cpp:74-87 in float64 (the cases sit far from the
    threshold)."""
    Rcw, tcw = cur_Tcw[:3, :3].astype(np.float64), cur_Tcw[:3, 3].astype(np.float64)
    tlc = last_Tcw[:3, :3].astype(np.float64) @ (-Rcw.T @ tcw) + last_Tcw[:3, 3].astype(np.float64)
    return bool(tlc[2] > fp["b"]), bool(-tlc[2] > fp["b"])


@pytest.mark.parametrize("case", ["first_pass", "retry", "slots_given", "forward", "backward"])
def test_pose_form_equals_host_form(ctx, builders, case):
    """d_model = NULL and uploaded blocks against lorb_track_motion_frames_dev on the same values: assign,
    the record, both slot sets and every guard band, byte for byte; the blocks are left as uploaded."""
    S = TLF.scene()
    fp, N = S["fp"], bound(S)
    b = float(fp["b"])
    cur_T = dict(first_pass=shift(DX), retry=shift(DX_RETRY), slots_given=shift(DX), forward=shift(DX, -1.5 * b),
                 backward=shift(DX, 1.5 * b))[case]
    fwd, bwd = motion_direction(fp, cur_T, I4)
    assert (fwd, bwd) == dict(forward=(True, False), backward=(False, True)).get(case, (False, False))
    entry, given = None, False
    if case == "slots_given":
        entry, given = TR.entry_slots(N, *TR.given_slots(TLF.NAME, DX)), True
    cur_blk, last_blk = frame_pose_from_Tcw(cur_T), frame_pose_from_Tcw(I4)
    assert same(np.array(cur_blk.pose[:], np.float32), np.array([0, 0, 0, cur_T[0, 3], 0, cur_T[2, 3]], np.float32))
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        host = Stage(ctx, bt, S, N, cur_entry=entry)
        host.host_form(cur_T, np.array(cur_blk.pose[:], np.float32), I4, cur_slots_given=given)
        h = host.read()
        dev = Stage(ctx, bt, S, N, cur_entry=entry)
        cp, lp = pose_block(ctx, cur_T), pose_block(ctx, I4)
        bt.held += [cp, lp]
        before = cp.numpy(), lp.numpy()
        dev.pose_form(cp, lp, None, cur_slots_given=given)
        d = dev.read()
        assert_same_stage(d, h, case)
        assert same(cp.numpy(), before[0]) and same(lp.numpy(), before[1])
        # the case is the case it names
        m = h["rec"].motion
        assert h["rec"].status == 0 and (h["masg"][S["n_cur"]:] == FILL).all() and (h["mrec"][MREC:] == SENT).all()
        print(case, "pass", m.pass_, "first", m.nmatches_first, "retry", m.nmatches_retry, "residuals", m.n_residuals)
        if case == "retry":
            assert (m.nmatches_first, m.nmatches_retry, m.pass_) == (15, 36, 2)
        elif case in ("first_pass", "slots_given"):
            assert m.pass_ == 1 and m.nmatches_first > 20 and m.nmatches_retry == -1
        if case == "slots_given":
            kept = (h["masg"][:S["n_cur"]] == A.LORB_ASSIGN_UNCHANGED) & (entry["state"][:S["n_cur"]] != EMPTY)
            assert kept.sum() >= 5 and (h["cur"]["state"][:S["n_cur"]][kept] != EMPTY).all()
        if case in ("forward", "backward"):  # the octave window differs from the symmetric one
            plain = Stage(ctx, bt, S, N)
            plain.host_form(shift(DX), TR.prediction(DX)[0], I4)
            assert not np.array_equal(plain.read()["masg"], h["masg"])


# 3 -- status ---------------------------------------------------------------------------------------------------------
def assert_untouched(r, entry_cur, entry_last, N):
    """Record status 1 and every other byte of the record, assign and both slot sets at its fill."""
    assert r["rec"].status == 1
    rec = A.TrackFramesResult.from_buffer_copy(r["mrec"].tobytes()[:MREC])
    rec.status = SENT_I32
    assert (np.frombuffer(bytes(rec), np.uint8) == SENT).all() and (r["mrec"][MREC:] == SENT).all()
    assert (r["masg"] == FILL).all()
    for side, entry in (("cur", entry_cur), ("last", entry_last)):
        for k in ("state", "pos", "desc"):
            assert same(r[side][k], entry[k]), (side, k)


def assert_pose_status_only(blk):
    raw = blk.numpy()
    p = A.FramePose.from_buffer_copy(raw.tobytes()[:POSE])
    assert p.status == 1
    p.status = SENT_I32
    assert (np.frombuffer(bytes(p), np.uint8) == SENT).all() and (raw[POSE:] == SENT).all()


@pytest.mark.parametrize("fail", ["last_pose", "model", "count_above"])
def test_status(ctx, builders, fail):
    """A failing status word or count stores status 1 in the record and in d_cur_pose and nothing else;
    the next call on the same context is correct."""
    S = TLF.scene()
    N = bound(S)
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        st = Stage(ctx, bt, S, N)
        ctx.sync()
        entry_cur, entry_last = st.cs.numpy(), st.ls.numpy()
        lastp, mod = frame_pose_from_Tcw(I4), A.MotionModel()
        mod.Tcc[:] = [float(v) for v in shift(DX).reshape(16)]
        if fail == "last_pose":
            lastp.status = 1
        if fail == "model":
            mod.status = 1
        lp, cp, mb = pose_block(ctx), pose_block(ctx), model_block(ctx)
        lp.upload(lastp)
        mb.upload(mod)
        bt.held += [lp, cp, mb]
        counts = bt.fb.counts.numpy()
        if fail == "count_above":
            bad = counts.copy()
            bad[0] = N + 1
            LMC.h2d(ctx, bt.fb.counts, bad)
        st.pose_form(cp, lp, mb)
        r = st.read()
        LMC.h2d(ctx, bt.fb.counts, counts)
        assert_untouched(r, entry_cur, entry_last, N)
        assert_pose_status_only(cp)
        # the next call on the same context: the good blocks, the host form's bits
        lp.upload(frame_pose_from_Tcw(I4))
        mod.status = 0
        mb.upload(mod)
        st.pose_form(cp, lp, mb)
        d = st.read()
        ref = Stage(ctx, bt, S, N)
        ref.host_form(shift(DX), TR.prediction(DX)[0], I4)
        assert_same_stage(d, ref.read(), "after " + fail)
        assert cp.read().status == 0


def test_finish_status(ctx):
    """A local record with status 1: cur.status = 1, nothing else in the block, the model untouched."""
    rec = A.TrackLocalFramesResult()
    rec.status = 1
    drec = ctx.to_device(np.frombuffer(bytes(rec), np.uint8).copy())
    lp, cp, mb = pose_block(ctx, I4), pose_block(ctx), model_block(ctx)
    try:
        frame_pose_finish(ctx, drec, lp, cp, mb)
        assert_pose_status_only(cp)
        assert (mb.numpy() == SENT).all()
    finally:
        for h in (drec, lp, cp, mb):
            h.free()


# 4, 5 -- whole frames ---------------------------------------------------------------------------------------------------
class Tracked:
    """Everything one tracked frame owns on the device: slots, global and local slot ids, the records and
    outputs of its stages, its pose block and the motion model its finish leaves."""

    def __init__(self, ctx, bt, N, n_local, gid=None, Tcw=None):
        self.slots = bt.slots(N, TR.entry_slots(N))
        self.gid, self.sid, self.urec = local_map_buffers(ctx, N, gid, FILL)
        self.masg = ctx.to_device(np.full(N + G, FILL, np.int32))
        self.mrec = ctx.to_device(np.full(MREC + G, SENT, np.uint8))
        self.out = LocalFramesOut(ctx, n_local, N, FILL)
        self.pose, self.model = pose_block(ctx, Tcw), model_block(ctx)
        bt.held += [self.gid, self.sid, self.urec, self.masg, self.mrec, self.out, self.pose, self.model]

    def read(self):
        o = self.out
        d = dict(masg=self.masg.numpy(), mrec=self.mrec.numpy(), urec=self.urec.numpy(), lrec=o.record.numpy(),
                 assign=o.assign.numpy(), in_view=o.in_view.numpy(), track=o.track.numpy(), level=o.level.numpy(),
                 gid=self.gid.numpy(), sid=self.sid.numpy(), pose=self.pose.numpy(), model=self.model.numpy())
        d.update({"slots_" + k: v for k, v in self.slots.numpy().items()})
        return d


class Loop:
    """The frame loop's shared objects: the map store, the local map, frame 0 (image A, INITIALIZE-filled
    at the identity, its global ids the store's)."""

    def __init__(self, ctx, bt, S):
        self.ctx, self.bt, self.S, self.fp, self.N = ctx, bt, S, S["fp"], bound(S)
        store, last_gid = LMC.build_store(S)
        self.dstore = DeviceMapStore(ctx, store, store["obs"], store["kf_bad"], store["kf_slots"], store["cov"])
        self.lmap = LocalMap(ctx, store["n_points"] - 3, 8, store["n_points"] + 5)
        bt.held += [self.dstore, self.lmap]
        self.last_gid = last_gid

    def first(self):
        f = Tracked(self.ctx, self.bt, self.N, self.lmap.n, gid=self.last_gid, Tcw=I4)
        fill_slots(self.ctx, self.fp, I4, self.bt.fa, f.slots, INIT)
        return f

    def new(self):
        return Tracked(self.ctx, self.bt, self.N, self.lmap.n)

    def track(self, img, cur, last_img, last, model=None, host_pose=None, local_min=LOCAL_MIN):
        """One tracked frame enqueued -- motion (pose form with `model`, or host form with host_pose =
        (cur_Tcw, pose_init, last_Tcw)), UpdateLocalMap, the local stage, ids back, finish -- and no wait."""
        ctx, fp, N = self.ctx, self.fp, self.N
        if host_pose is None:
            enqueue_track_motion_frames_pose(ctx, fp, cur.pose, img, cur.slots, last.pose, model, last_img, last.slots, cur.masg,
                                             cur.mrec, n_max_cur=N, n_max_last=N)
        else:
            enqueue_track_motion_frames(ctx, fp, host_pose[0], host_pose[1], img, cur.slots, host_pose[2], last_img, last.slots,
                                        cur.masg, cur.mrec, n_max_cur=N, n_max_last=N)
        d_pose, d_mstatus = motion_record_addresses(cur.mrec)
        ids = A.TrackLocalIdSource(cur.masg.ptr.value, cur.mrec.ptr.value, last.gid.ptr.value, N, 0)
        d_ustatus = local_map_update(ctx, self.lmap, self.dstore, img, cur.slots, cur.gid, cur.sid, cur.urec, n_max_cur=N,
                                     d_src_status=d_mstatus, id_source=ids)
        track_local_frames(ctx, fp, img, cur.slots, cur.sid, d_pose, self.lmap, out=cur.out, n_max_cur=N,
                           d_src_status=d_ustatus, th=TH, min_matches=local_min)
        local_map_ids_back(ctx, self.lmap, img, cur.slots, cur.sid, cur.gid, n_max_cur=N,
                           d_local_status=cur.out.record.ptr.value + A.TrackLocalFramesResult.status.offset)
        frame_pose_finish(ctx, cur.out.record, last.pose, cur.pose, cur.model)


@pytest.mark.parametrize("gate", ["passes", "fails"])
def test_finish(ctx, builders, gate):
    """After a whole tracked frame the block and mTcc are the restatement applied to the local record; a
    frame whose local gate fails (min_matches above the match count) hands on Tcw_in and pose_in."""
    S = TLF.scene()
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        loop = Loop(ctx, bt, S)
        f0, f1 = loop.first(), loop.new()
        m0 = model_block(ctx, shift(DX))
        bt.held.append(m0)
        loop.track(bt.fb, f1, bt.fa, f0, model=m0, local_min=LOCAL_MIN if gate == "passes" else 100000)
        rec = f1.out.result()  # the one wait
        mrec = A.TrackFramesResult.from_buffer_copy(f1.mrec.numpy().tobytes()[:MREC])
        assert rec.status == 0 and mrec.status == 0 and mrec.motion.pass_ == 1
        print(gate, "local matches", rec.local.nmatches, "ok", rec.local.ok, "residuals", rec.local.n_residuals)
        assert rec.local.ok == (1 if gate == "passes" else 0) and rec.local.nmatches > LOCAL_MIN
        last = M.set_pose(I4)
        cur, Tcc = M.finish(mat(rec.Tcw), rec.local.ok, rec.local.pose[:], rec.pose_in[:], last)
        assert_block(f1.pose.read(), cur, gate)
        model = f1.model.read()
        assert model.status == 0 and same(mat(model.Tcc), Tcc)
        assert (f1.pose.numpy()[POSE:] == SENT).all() and (f1.model.numpy()[MODEL:] == SENT).all()
        if gate == "fails":
            assert same(mat(rec.Tcw), mat(rec.Tcw_in)) and same(np.array(f1.pose.read().pose[:], np.float32),
                                                                np.array(rec.pose_in[:], np.float32))
        else:
            assert not same(np.array(rec.local.pose[:]), np.array(rec.pose_in[:], np.float32).astype(np.float64))
        assert same(f0.pose.numpy()[:POSE], np.frombuffer(bytes(frame_pose_from_Tcw(I4)), np.uint8))  # read only


def test_three_frames_one_wait(ctx, builders):
    """B against A (model = DX), A's image against B, B's against that: fifteen calls enqueued with the pose
    blocks handed on in device memory and ONE wait, against the stepwise loop that waits after every frame,
    reads the device's own predicted block back (the definition of the prediction) and hands its Tcw and
    pose to the host-pose lorb_track_motion_frames_dev.  Bit for bit, for every frame."""
    S = TLF.scene()
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        loop = Loop(ctx, bt, S)
        imgs = [bt.fa, bt.fb, bt.fa, bt.fb]

        # the chain: nothing waits until the end
        fr = [loop.first()] + [loop.new() for _ in range(3)]
        m0 = model_block(ctx, shift(DX))
        bt.held.append(m0)
        for k in (1, 2, 3):
            loop.track(imgs[k], fr[k], imgs[k - 1], fr[k - 1], model=m0 if k == 1 else fr[k - 1].model)
        ctx.sync()  # the one wait
        chain = [f.read() for f in fr]

        # the stepwise loop
        st = [loop.first()] + [loop.new() for _ in range(3)]
        for k in (1, 2, 3):
            model = m0 if k == 1 else st[k - 1].model
            # the device's own prediction: the pose form on copies of the slots, its block read back
            snap = st[k - 1].slots.numpy()
            tl = bt.slots(loop.N, {q: snap[q] for q in ("state", "pos", "desc")})
            tc, tp = bt.slots(loop.N, TR.entry_slots(loop.N)), pose_block(ctx)
            tasg, trec = ctx.to_device(np.full(loop.N + G, FILL, np.int32)), ctx.to_device(np.full(MREC + G, SENT, np.uint8))
            bt.held += [tp, tasg, trec]
            enqueue_track_motion_frames_pose(ctx, loop.fp, tp, imgs[k], tc, st[k - 1].pose, model, imgs[k - 1], tl, tasg, trec,
                                             n_max_cur=loop.N, n_max_last=loop.N)
            pred, last = tp.read(), st[k - 1].pose.read()
            assert pred.status == 0 and last.status == 0
            loop.track(imgs[k], st[k], imgs[k - 1], st[k - 1],
                       host_pose=(mat(pred.Tcw), np.array(pred.pose[:], np.float32), mat(last.Tcw)))
            ctx.sync()  # the frame's wait
        step = [f.read() for f in st]

    for k in range(4):
        for key in chain[k]:
            if k == 0 and key in ("pose", "model"):
                continue  # frame 0's block is uploaded, its model never written
            assert same(chain[k][key], step[k][key]), (k, key)
    for k in (1, 2, 3):
        mrec = A.TrackFramesResult.from_buffer_copy(chain[k]["mrec"].tobytes()[:MREC])
        lrec = A.TrackLocalFramesResult.from_buffer_copy(chain[k]["lrec"].tobytes()[:LREC])
        pose = A.FramePose.from_buffer_copy(chain[k]["pose"].tobytes()[:POSE])
        print("frame", k, "pass", mrec.motion.pass_, "first", mrec.motion.nmatches_first, "retry", mrec.motion.nmatches_retry,
              "local", lrec.local.nmatches, "ok", lrec.local.ok, "t", pose.pose[3:6])
        assert mrec.status == 0 and lrec.status == 0 and pose.status == 0
        assert mrec.motion.pass_ != 0 and lrec.local.ok == 1 and lrec.local.nmatches > LOCAL_MIN
        # the blocks are the restatement applied to the records
        last = block_dict(A.FramePose.from_buffer_copy(chain[k - 1]["pose"].tobytes()[:POSE]))
        cur, Tcc = M.finish(mat(lrec.Tcw), lrec.local.ok, lrec.local.pose[:], lrec.pose_in[:], last)
        assert_block(pose, cur, f"frame {k}")
        assert same(mat(A.MotionModel.from_buffer_copy(chain[k]["model"].tobytes()[:MODEL]).Tcc), Tcc)
