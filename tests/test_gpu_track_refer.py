"""GPU: the second motion attempt on the reference keyframe, decided on the device
(lorb_track_motion_refer_pose_dev; VisualOdometry::Run, src/visual_odometry.cpp:50-54), enqueued directly
behind lorb_track_motion_frames_pose_dev with nothing read back in between.

The scene is tests/test_gpu_motion_model.py's (TLF.scene(), "320x256", bound max(n_last, n_cur) + 1, guard
bands and sentinels on every buffer).  A failing first attempt: the last frame is image A, INITIALIZE-filled
at the identity, but its pose block is uploaded as a translation of 2.0 - DX, and the model is shift(DX), so
the first prediction is dx = 2.0 (pass 0: 6 matches at 15, 11 at 30, 11 slots left held).  The refer frame is
a second slot set of image A, INITIALIZE-filled; its block's translation x makes the second prediction
dx = x + DX.  d_refer_slot_gid = the last frame's gids + 1000, so that the two sources cannot be confused.

What a result is compared with: every output of an attempt that ran, bit for bit, with
lorb_track_motion_frames_pose_dev called by the host on what the first attempt left (cur_slots_given = 1,
the refer objects as the last frame); the match figures and the codes with the oracle (TR.expected) at the
pose the device reports; the gids with a numpy restatement of the call's steps c and e; an attempt that is
skipped with the bytes every object had before the call."""
import ctypes as C
import functools

import numpy as np
import pytest

import lorb_slam_amd.window as W
import test_gpu_local_map_chain as LMC
import test_gpu_motion_model as MM
import test_gpu_track_frames as TR
import test_gpu_track_local_frames as TLF
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, enqueue_track_motion_frames_pose, enqueue_track_motion_refer_pose, fill_slots,
                                 frame_pose_finish, frame_pose_from_Tcw, local_map_ids_back, local_map_update, model_block,
                                 motion_record_addresses, pose_block, refer_kf_word, track_local_frames)
from test_gpu_track_frames import builders  # noqa: F401 -- the module-scoped builder fixture

pytestmark = pytest.mark.gpu

G, SENT, FILL, I4 = W.ORB_GUARD, W.ORB_SENTINEL, TR.FILL, TR.I4
UNCHANGED, NULL, EMPTY = A.LORB_ASSIGN_UNCHANGED, A.LORB_ASSIGN_NULL, A.LORB_SLOT_EMPTY
INIT = A.LORB_SLOTS_INITIALIZE
DX, TH, LOCAL_MIN = TLF.DX, LMC.TH, MM.LOCAL_MIN
MREC, POSE, RREC = C.sizeof(A.TrackFramesResult), C.sizeof(A.FramePose), C.sizeof(A.TrackReferResult)
X_FAIL = 2.0 - DX     # the last block's translation that makes the first prediction dx = 2.0
GID_OFF = 1000        # refer gids = last gids + GID_OFF
REFER_KF = 0          # the keyframe index of the refer frame (the store's kf0)
# the second prediction's block translation -> (pass, matches at 15, at 30, residuals or None), the oracle's figures
SECOND = {0.0: (1, 185, -1, 196), 0.8: (2, 15, 36, None), 1.9: (0, 4, 11, None)}
FIRST = (0, 6, 11)    # the first attempt at dx = 2.0: pass, matches at 15, at 30
N_KEPT = 11           # slots the failed first attempt leaves held
same, shift, bound = TLF.same, MM.shift, MM.bound


# ---- the host model ------------------------------------------------------------------------------------------------
def init_image(S, N):
    """Image A's slots INITIALIZE-filled at the identity, as a guarded host image of N entries."""
    return TR.filled(S["fp"], I4, S["ca"]["o"], TR.entry_slots(N), INIT)[0]


@functools.lru_cache(maxsize=None)
def oracle_attempt(dx, after_dx=None):
    """TR.expected for image B against INITIALIZE-filled A at prediction dx (a float32's value): the current
    slots not given, or -- after_dx -- given as the attempt at after_dx left them."""
    S = TLF.scene()
    N = bound(S)
    oa, ob = S["ca"]["o"], S["cb"]["o"]
    if after_dx is None:
        return TR.expected(oa, ob, S["fp"], dx, init_image(S, N), TR.entry_slots(N))
    return TR.expected(oa, ob, S["fp"], dx, init_image(S, N), oracle_attempt(after_dx)["cur_slots"], given=True)


def step_c(masg, pass_, given, last_gid, entry_gid, n_cur):
    """Step c: the slots' gids from the first attempt's codes (the rule of lorb_track_local_id_source)."""
    return TLF.entry_ids(masg, pass_, given, last_gid, entry_gid, n_cur)


def step_e(masg, pass_, refer_gid, gid_c, n_cur):
    """Step e's tail: the final codes applied to the gids step c left (cur_slots_given = 1)."""
    a = masg[:n_cur]
    g = np.full(n_cur, -1, np.int32)
    g[a >= 0] = refer_gid[a[a >= 0]]
    keep = (a == UNCHANGED) & (pass_ == 1)
    g[keep] = gid_c[keep]
    return g


def figures(rec):
    m = rec.motion
    return m.pass_, m.nmatches_first, m.nmatches_retry


# ---- the device side -----------------------------------------------------------------------------------------------
class Rig:
    """Both attempts' device objects on a Built pair: the motion stage's (MM.Stage: last slots of image A
    INITIALIZE-filled, current slots, assign, record), the refer frame's slot set, the three pose blocks, the
    model, the three gid arrays, the reference-frame word, the previous frame's local-map record and the
    refer record."""

    def __init__(self, ctx, bt, S, x_refer=0.0, x_last=X_FAIL, given=False, prev_kf=-1, prev_status=0):
        self.ctx, self.bt, self.S, self.given = ctx, bt, S, given
        N = self.N = bound(S)
        entry = None
        self.gid_entry = np.full(N + G, FILL, np.int32)
        if given:
            entry = TR.entry_slots(N, *TR.given_slots(TLF.NAME, DX))
            self.gid_entry[:S["n_cur"]] = 5000 + np.arange(S["n_cur"])
        self.st = MM.Stage(ctx, bt, S, N, cur_entry=entry)
        self.rs = bt.slots(N, TR.entry_slots(N))
        fill_slots(ctx, S["fp"], I4, bt.fa, self.rs, INIT)
        self.lp, self.rp, self.cp = pose_block(ctx, shift(x_last)), pose_block(ctx, shift(x_refer)), pose_block(ctx)
        self.model = model_block(ctx, shift(DX))
        self.last_gid_h = LMC.build_store(S)[1]
        self.refer_gid_h = np.where(self.last_gid_h >= 0, self.last_gid_h + GID_OFF, -1).astype(np.int32)
        self.last_gid = ctx.to_device(TR.guarded(self.last_gid_h, N))
        self.refer_gid = ctx.to_device(TR.guarded(self.refer_gid_h, N))
        self.cur_gid = ctx.to_device(self.gid_entry)
        self.kf = refer_kf_word(ctx, REFER_KF)
        upd = A.LocalMapResult()
        upd.status, upd.refer_kf = prev_status, prev_kf
        self.upd = DeviceBlock(ctx, A.LocalMapResult, upd)
        self.rrec = DeviceBlock(ctx, A.TrackReferResult)
        bt.held += [self.lp, self.rp, self.cp, self.model, self.last_gid, self.refer_gid, self.cur_gid, self.kf, self.upd,
                    self.rrec]

    def first(self):
        self.st.pose_form(self.cp, self.lp, self.model, cur_slots_given=self.given)

    def refer(self, n_max_refer=None):
        enqueue_track_motion_refer_pose(
            self.ctx, self.S["fp"], self.cp, self.bt.fb, self.st.cs, self.rp, self.model, self.bt.fa, self.rs, self.st.masg,
            self.st.mrec, self.rrec, first_slots_given=self.given, n_max_cur=self.N,
            n_max_refer=self.N if n_max_refer is None else n_max_refer, last_gid=self.last_gid, n_max_last=self.N,
            refer_gid=self.refer_gid, cur_gid=self.cur_gid, refer_kf=REFER_KF, kf_word=self.kf, prev_update=self.upd)

    def host_second(self):
        """What the host would issue after reading a pass 0: the plain pose form on the refer frame."""
        enqueue_track_motion_frames_pose(self.ctx, self.S["fp"], self.cp, self.bt.fb, self.st.cs, self.rp, self.model, self.bt.fa,
                                         self.rs, self.st.masg, self.st.mrec, n_max_cur=self.N, n_max_last=self.N,
                                         cur_slots_given=True)

    def read(self):
        """Every byte of every object (the first fetch waits for the stream)."""
        d = dict(mrec=self.st.mrec.numpy(), masg=self.st.masg.numpy(), cp=self.cp.numpy(), lp=self.lp.numpy(),
                 rp=self.rp.numpy(), model=self.model.numpy(), last_gid=self.last_gid.numpy(), refer_gid=self.refer_gid.numpy(),
                 cur_gid=self.cur_gid.numpy(), kf=self.kf.numpy(), upd=self.upd.numpy(), rrec=self.rrec.numpy())
        for name, s in (("cur", self.st.cs), ("last", self.st.ls), ("refer", self.rs)):
            d.update({f"{name}_{k}": v for k, v in s.numpy().items()})
        return d


STAGE_KEYS = ("mrec", "masg", "cp", "lp", "rp", "model", "cur_state", "cur_pos", "cur_desc", "last_state", "last_pos",
              "last_desc", "refer_state", "refer_pos", "refer_desc")


def record(r):
    return A.TrackFramesResult.from_buffer_copy(r["mrec"].tobytes()[:MREC])


def refer_record(r):
    assert (r["rrec"][RREC:] == SENT).all()
    q = A.TrackReferResult.from_buffer_copy(r["rrec"].tobytes()[:RREC])
    return q.due, q.ran, q.stale, q.first_nmatches_first, q.first_nmatches_retry


def assert_unchanged(after, before, but=()):
    for k in before:
        if k not in but:
            assert same(after[k], before[k]), k


def assert_gids(r, want, n_cur):
    assert np.array_equal(r["cur_gid"][:n_cur], want) and (r["cur_gid"][n_cur:] == FILL).all()


def dx_of(r):
    """The prediction the device reports: the translation of d_cur_pose along x (a float32's value)."""
    blk = A.FramePose.from_buffer_copy(r["cp"].tobytes()[:POSE])
    assert blk.status == 0
    return float(np.float32(blk.Tcw[3]))


# 1 -- skipped -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True])
def test_skipped(ctx, builders, given):
    """The first attempt passes: d_assign, the record, both current slot arrays, the refer slots, the three
    pose blocks, the model and every guard band are byte-identical to before; due = ran = stale = 0; the
    gids are the id-source rule on the first attempt's codes."""
    S = TLF.scene()
    n_cur = S["n_cur"]
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        rig = Rig(ctx, bt, S, x_last=0.0, given=given)
        rig.first()
        before = rig.read()
        rec = record(before)
        assert rec.status == 0 and rec.motion.pass_ == 1
        rig.refer()
        after = rig.read()
    assert_unchanged(after, before, but=("rrec", "cur_gid"))
    assert refer_record(after) == (0, 0, 0, rec.motion.nmatches_first, rec.motion.nmatches_retry)
    want = TLF.entry_ids(before["masg"], 1, given, rig.last_gid_h, rig.gid_entry, n_cur)
    assert_gids(after, want, n_cur)
    a = before["masg"][:n_cur]
    assert (want[a >= 0] == rig.last_gid_h[a[a >= 0]]).all() and (want[a == NULL] == -1).all()
    if given:  # UNCHANGED slots keep the ids they came with
        assert (a == UNCHANGED).sum() >= 5 and (want[a == UNCHANGED] == rig.gid_entry[:n_cur][a == UNCHANGED]).all()
    else:
        assert (want[a == UNCHANGED] == -1).all()


# 2 -- runs ---------------------------------------------------------------------------------------------------------------
def run_both(ctx, bt, S, x_refer, **kw):
    """(the chain: first attempt + refer call, no wait in between; what the first attempt left; the host's
    second call on that)."""
    dev = Rig(ctx, bt, S, x_refer=x_refer, **kw)
    dev.first()
    dev.refer()
    d = dev.read()
    host = Rig(ctx, bt, S, x_refer=x_refer, **kw)
    host.first()
    h1 = host.read()
    host.host_second()
    return dev, d, h1, host.read()


def assert_ran(dev, d, h1, h, S):
    n_cur = S["n_cur"]
    first, second = record(h1), record(h)
    assert first.status == 0 and first.motion.pass_ == 0
    for k in STAGE_KEYS:
        assert same(d[k], h[k]), k
    assert refer_record(d) == (1, 1, 0, first.motion.nmatches_first, first.motion.nmatches_retry)
    gid_c = step_c(h1["masg"], 0, dev.given, dev.last_gid_h, dev.gid_entry, n_cur)
    assert_gids(d, step_e(h["masg"], second.motion.pass_, dev.refer_gid_h, gid_c, n_cur), n_cur)
    assert same(d["last_gid"], h["last_gid"]) and same(d["refer_gid"], h["refer_gid"])
    assert same(d["kf"], h["kf"]) and same(d["upd"], h["upd"])
    return first, second, gid_c


@pytest.mark.parametrize("x_refer", list(SECOND))
def test_runs(ctx, builders, x_refer):
    """The first attempt fails at dx = 2.0; the second, from the slots it left, lands on pass 1 (x = 0), pass
    2 (x = 0.8) and pass 0 (x = 1.9).  Every output equals the host-issued pose form's; the figures and the
    codes are the oracle's at the poses the device reports."""
    S = TLF.scene()
    n_cur = S["n_cur"]
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        dev, d, h1, h = run_both(ctx, bt, S, x_refer)
    first, second, gid_c = assert_ran(dev, d, h1, h, S)
    dx1, dx2 = dx_of(h1), dx_of(d)
    print("x_refer", x_refer, "dx", dx1, dx2, "first", figures(first), "second", figures(second), "residuals",
          second.motion.n_residuals)
    assert abs(dx1 - 2.0) < 1e-6 and abs(dx2 - (x_refer + DX)) < 1e-6
    # the first attempt: the oracle at the reported pose, and the figures the set-up was chosen by
    e1 = oracle_attempt(dx1)
    assert figures(first) == (e1["pass_"], e1["nmatches_first"], e1["nmatches_retry"]) == FIRST
    assert np.array_equal(h1["masg"][:n_cur], e1["assign"])
    held = h1["cur_state"][:n_cur] != EMPTY
    assert held.sum() == N_KEPT and same(h1["cur_state"], e1["cur_slots"]["state"])
    # the second attempt, from those slots
    e2 = oracle_attempt(dx2, after_dx=dx1)
    want = SECOND[x_refer]
    assert figures(second) == (e2["pass_"], e2["nmatches_first"], e2["nmatches_retry"]) == want[:3]
    assert second.motion.n_residuals == e2["n_residuals"] and np.array_equal(d["masg"][:n_cur], e2["assign"])
    for k in ("state", "pos", "desc"):
        assert same(d["cur_" + k], e2["cur_slots"][k]) and same(d["refer_" + k], e2["last_slots"][k]), k
    a, g = d["masg"][:n_cur], d["cur_gid"][:n_cur]
    if second.motion.pass_ == 1:
        kept = (a == UNCHANGED) & held
        assert second.motion.n_residuals == want[3] and kept.sum() == N_KEPT
        assert not np.array_equal(e2["assign"], oracle_attempt(dx2)["assign"])  # the slots given change the search
        # the kept slots carry last-frame gids, the hits refer gids
        assert same(g[kept], gid_c[kept]) and (g[kept] < GID_OFF).all() and (g[kept] >= 0).any()
        assert (g[a >= 0] == dev.refer_gid_h[a[a >= 0]]).all() and (g[a >= 0] >= GID_OFF).sum() > 100
    else:  # the retry starts from emptied slots: nothing of the first attempt's is kept
        assert (g[a < 0] == -1).all() and (d["cur_state"][:n_cur][a < 0] == EMPTY).all()
    if second.motion.pass_ == 0:  # the second prediction and the second retry's slots stay
        assert (d["cur_state"][:n_cur] != EMPTY).sum() == (a >= 0).sum() > 0


# 3 -- status ---------------------------------------------------------------------------------------------------------------
def status_only(after_bytes, before_bytes, ctype, n):
    """after = before but for the struct's status word, which is 1."""
    a, b = ctype.from_buffer_copy(after_bytes.tobytes()[:n]), ctype.from_buffer_copy(before_bytes.tobytes()[:n])
    assert a.status == 1
    a.status = b.status
    assert bytes(a) == bytes(b) and same(after_bytes[n:], before_bytes[n:])


@pytest.mark.parametrize("case", ["first_failed", "refer_count", "refer_pose", "not_due_count", "not_due_pose"])
def test_status(ctx, builders, case):
    """A first record with status 1: nothing but the zeroed refer record.  Due with a refer count above its
    bound or d_refer_pose->status = 1: status 1 in the record and in d_cur_pose, the gids of step c and the
    refer record, nothing else.  The same bad refer objects while not due: a clean skip.  The next call on
    the context is correct."""
    S = TLF.scene()
    n_cur = S["n_cur"]
    due = case in ("refer_count", "refer_pose")
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        rig = Rig(ctx, bt, S, x_last=X_FAIL if due or case == "first_failed" else 0.0)
        if case == "first_failed":
            bad = frame_pose_from_Tcw(shift(X_FAIL))
            bad.status = 1
            rig.lp.upload(bad)
        if case.endswith("pose"):
            bad = frame_pose_from_Tcw(I4)
            bad.status = 1
            rig.rp.upload(bad)
        rig.first()
        before = rig.read()
        rec = record(before)
        rig.refer(n_max_refer=S["n_last"] - 1 if case.endswith("count") else None)
        after = rig.read()
        # afterwards: a good pair of attempts on the same context
        dev, d, h1, h = run_both(ctx, bt, S, 0.0)
    if case == "first_failed":
        assert rec.status == 1
        assert_unchanged(after, before, but=("rrec",))
        assert refer_record(after) == (0, 0, 0, 0, 0)
    elif due:
        assert rec.status == 0 and rec.motion.pass_ == 0
        assert_unchanged(after, before, but=("rrec", "cur_gid", "mrec", "cp"))
        status_only(after["mrec"], before["mrec"], A.TrackFramesResult, MREC)
        status_only(after["cp"], before["cp"], A.FramePose, POSE)
        assert refer_record(after) == (1, 1, 0, rec.motion.nmatches_first, rec.motion.nmatches_retry)
        assert_gids(after, step_c(before["masg"], 0, False, rig.last_gid_h, rig.gid_entry, n_cur), n_cur)
    else:
        assert rec.status == 0 and rec.motion.pass_ == 1
        assert_unchanged(after, before, but=("rrec", "cur_gid"))
        assert refer_record(after) == (0, 0, 0, rec.motion.nmatches_first, rec.motion.nmatches_retry)
        assert_gids(after, step_c(before["masg"], 1, False, rig.last_gid_h, rig.gid_entry, n_cur), n_cur)
    _, second, _ = assert_ran(dev, d, h1, h, S)
    assert figures(second) == SECOND[0.0][:3]


# 4 -- the guard ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["moved", "minus_one", "update_failed"])
def test_guard(ctx, builders, case):
    """While due: the previous frame's UpdateLocalMap named another keyframe -- stale = 1, ran = 0, the word
    is updated and everything else is untouched.  refer_kf = -1 and a status != 0 leave the word as it was,
    and the attempt runs."""
    S = TLF.scene()
    n_cur = S["n_cur"]
    prev = dict(moved=(REFER_KF + 3, 0), minus_one=(-1, 0), update_failed=(REFER_KF + 3, 1))[case]
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        if case == "moved":
            rig = Rig(ctx, bt, S, prev_kf=prev[0], prev_status=prev[1])
            rig.first()
            before = rig.read()
            rig.refer()
            after = rig.read()
        else:
            dev, d, h1, h = run_both(ctx, bt, S, 0.0, prev_kf=prev[0], prev_status=prev[1])
    if case == "moved":
        rec = record(before)
        assert rec.status == 0 and rec.motion.pass_ == 0
        assert_unchanged(after, before, but=("rrec", "cur_gid", "kf"))
        assert refer_record(after) == (1, 0, 1, rec.motion.nmatches_first, rec.motion.nmatches_retry)
        assert int(after["kf"][:4].view(np.int32)[0]) == REFER_KF + 3 and same(after["kf"][4:], before["kf"][4:])
        assert_gids(after, step_c(before["masg"], 0, False, rig.last_gid_h, rig.gid_entry, n_cur), n_cur)
    else:
        _, second, _ = assert_ran(dev, d, h1, h, S)
        assert figures(second) == SECOND[0.0][:3]
        assert int(d["kf"][:4].view(np.int32)[0]) == REFER_KF and (d["kf"][4:] == SENT).all()


# 5 -- the whole loop -------------------------------------------------------------------------------------------------------
class ReferLoop(MM.Loop):
    """MM.Loop with the refer frame's objects: a second slot set of image A INITIALIZE-filled at the identity,
    its pose block, its gids, the reference-frame word and the refer records of the frames."""

    def __init__(self, ctx, bt, S):
        super().__init__(ctx, bt, S)
        N = self.N
        self.rs = bt.slots(N, TR.entry_slots(N))
        fill_slots(ctx, self.fp, I4, bt.fa, self.rs, INIT)
        self.rp = pose_block(ctx, I4)
        self.refer_gid_h = np.where(self.last_gid >= 0, self.last_gid + GID_OFF, -1).astype(np.int32)
        self.refer_gid = ctx.to_device(TR.guarded(self.refer_gid_h, N))
        self.kf = refer_kf_word(ctx, REFER_KF)
        none = A.LocalMapResult()
        none.refer_kf = -1
        self.no_update = DeviceBlock(ctx, A.LocalMapResult, none)  # frame 1 has no previous UpdateLocalMap
        self.rrecs = []
        bt.held += [self.rp, self.refer_gid, self.kf, self.no_update]

    def first(self):
        f = super().first()
        f.pose.upload(frame_pose_from_Tcw(shift(X_FAIL)))  # the set-up: the block is moved, the slots are not
        return f

    def rest(self, img, cur):
        """The calls behind the motion stage: UpdateLocalMap (ids = NULL: the gids are in place), the local
        stage, ids back, finish."""
        ctx, N = self.ctx, self.N
        d_pose, d_mstatus = motion_record_addresses(cur.mrec)
        d_ustatus = local_map_update(ctx, self.lmap, self.dstore, img, cur.slots, cur.gid, cur.sid, cur.urec, n_max_cur=N,
                                     d_src_status=d_mstatus)
        track_local_frames(ctx, self.fp, img, cur.slots, cur.sid, d_pose, self.lmap, out=cur.out, n_max_cur=N,
                           d_src_status=d_ustatus, th=TH, min_matches=LOCAL_MIN)
        local_map_ids_back(ctx, self.lmap, img, cur.slots, cur.sid, cur.gid, n_max_cur=N,
                           d_local_status=cur.out.record.ptr.value + A.TrackLocalFramesResult.status.offset)

    def motion(self, img, cur, last_img, last, model):
        enqueue_track_motion_frames_pose(self.ctx, self.fp, cur.pose, img, cur.slots, last.pose, model, last_img, last.slots,
                                         cur.masg, cur.mrec, n_max_cur=self.N, n_max_last=self.N)

    def refer(self, img, cur, last, model, prev_update):
        rrec = DeviceBlock(self.ctx, A.TrackReferResult)
        self.bt.held.append(rrec)
        self.rrecs.append(rrec)
        enqueue_track_motion_refer_pose(
            self.ctx, self.fp, cur.pose, img, cur.slots, self.rp, model, self.bt.fa, self.rs, cur.masg, cur.mrec, rrec,
            n_max_cur=self.N, n_max_refer=self.N, last_gid=last.gid, n_max_last=self.N, refer_gid=self.refer_gid,
            cur_gid=cur.gid, refer_kf=REFER_KF, kf_word=self.kf, prev_update=prev_update)

    def finish(self, cur, last):
        frame_pose_finish(self.ctx, cur.out.record, last.pose, cur.pose, cur.model)

    def objects(self):
        d = dict(kf=self.kf.numpy(), rp=self.rp.numpy())
        d.update({"refer_" + k: v for k, v in self.rs.numpy().items()})
        return d


def test_whole_loop(ctx, builders):
    """Frame 1 (image B against A, the failing set-up) runs the second attempt, frame 2 (image A against B)
    skips it: frame build, motion, refer, UpdateLocalMap, the local stage, ids back and finish for each --
    fourteen calls and ONE wait -- against the stepwise loop, which waits on each motion record and lets the
    host decide whether to issue the plain pose form on the refer frame, and keeps the gids in numpy.  Every
    object of every frame matches bit for bit.  Frame 1's own mTcc is formed against the last frame's block,
    which the set-up moved to make the first attempt fail; frame 2 therefore predicts with an uploaded model
    (DX from frame 1's pose), in both loops."""
    S = TLF.scene()
    n = {1: S["n_cur"], 2: S["n_last"]}
    images = {1: S["cb"], 2: S["ca"]}
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        m1, m2 = model_block(ctx, shift(DX)), model_block(ctx, shift(DX))
        bt.held += [m1, m2]
        models = {1: m1, 2: m2}

        def build(k):
            f = bt.b.build_device(images[k]["left"], images[k]["right"])
            bt.held.append(f)
            return f

        # the chain: seven calls per frame, nothing waits until the end
        loop = ReferLoop(ctx, bt, S)
        fr, img = [loop.first(), loop.new(), loop.new()], {0: bt.fa}
        for k in (1, 2):
            img[k] = build(k)
            loop.motion(img[k], fr[k], img[k - 1], fr[k - 1], models[k])
            loop.refer(img[k], fr[k], fr[k - 1], models[k], loop.no_update if k == 1 else fr[k - 1].urec)
            loop.rest(img[k], fr[k])
            loop.finish(fr[k], fr[k - 1])
        ctx.sync()  # the one wait
        chain = [f.read() for f in fr]
        chain_obj, chain_rrec = loop.objects(), [refer_record(dict(rrec=r.numpy())) for r in loop.rrecs]

        # the stepwise loop
        step_loop = ReferLoop(ctx, bt, S)
        st, simg, issued = [step_loop.first(), step_loop.new(), step_loop.new()], {0: bt.fa}, []
        for k in (1, 2):
            simg[k] = build(k)
            step_loop.motion(simg[k], st[k], simg[k - 1], st[k - 1], models[k])
            first = A.TrackFramesResult.from_buffer_copy(st[k].mrec.numpy().tobytes()[:MREC])  # the motion record's wait
            assert first.status == 0
            last_gid = st[k - 1].gid.numpy()
            gid = st[k].gid.numpy()
            g = step_c(st[k].masg.numpy(), first.motion.pass_, False, last_gid, gid, n[k])
            issued.append(first.motion.pass_ == 0)
            if first.motion.pass_ == 0:  # the host's decision
                enqueue_track_motion_frames_pose(ctx, step_loop.fp, st[k].pose, simg[k], st[k].slots, step_loop.rp, models[k],
                                                 bt.fa, step_loop.rs, st[k].masg, st[k].mrec, n_max_cur=step_loop.N,
                                                 n_max_last=step_loop.N, cur_slots_given=True)
                second = A.TrackFramesResult.from_buffer_copy(st[k].mrec.numpy().tobytes()[:MREC])
                g = step_e(st[k].masg.numpy(), second.motion.pass_, step_loop.refer_gid_h, g, n[k])
            gid[:n[k]] = g
            LMC.h2d(ctx, st[k].gid, gid)
            step_loop.rest(simg[k], st[k])
            step_loop.finish(st[k], st[k - 1])
            ctx.sync()
        step = [f.read() for f in st]
        step_obj = step_loop.objects()

    assert issued == [True, False]
    assert chain_rrec[0][:3] == (1, 1, 0) and chain_rrec[0][3:] == FIRST[1:] and chain_rrec[1][:3] == (0, 0, 0)
    for k in range(3):
        for key in chain[k]:
            if k == 0 and key == "model":
                continue  # frame 0's model is never written
            assert same(chain[k][key], step[k][key]), (k, key)
    for key in chain_obj:
        assert same(chain_obj[key], step_obj[key]), key
    assert int(chain_obj["kf"][:4].view(np.int32)[0]) == REFER_KF
    for k in (1, 2):
        mrec = A.TrackFramesResult.from_buffer_copy(chain[k]["mrec"].tobytes()[:MREC])
        lrec = A.TrackLocalFramesResult.from_buffer_copy(chain[k]["lrec"].tobytes()[:MM.LREC])
        print("frame", k, "motion", figures(mrec), "local", lrec.local.nmatches, "ok", lrec.local.ok)
        assert mrec.status == 0 and lrec.status == 0 and mrec.motion.pass_ != 0
        if k == 1:  # the local stage passes its gate behind the second attempt
            assert lrec.local.ok == 1 and lrec.local.nmatches > LOCAL_MIN
    assert figures(A.TrackFramesResult.from_buffer_copy(chain[1]["mrec"].tobytes()[:MREC])) == SECOND[0.0][:3]
