"""GPU: local-map tracking straight from a built frame (lorb_track_local_frames_dev;
lorb_slam_amd.frame.track_local_frames) enqueued behind lorb_track_motion_frames_dev with ONE wait.

The base scene is the one tests/test_gpu_track_frames.py::test_chain_into_track_local pins: case
"320x256", dx = 0.1, frame A INITIALIZE-filled, A's initialised points as the local map, ids = the
position of each initialised slot in that table.  The motion stage stands at pass 1; stage 2 finds 19
matches at th = 1 (the gate fails) and 22 at th = 2 (the pose is optimised).

What a result is compared with: the slots the motion stage left are read from a motion-only run on the
same frames (its record must equal the chain's byte for byte); the ids on entry, the held-slot loop, the
in_frame mask and the slot write-back are numpy over those; the search and the pose are (1)
lorb_track_local_dev given the record's Tcw_in / pose_in / n_cur and the host's mask and slots -- bit for
bit -- and (2) the oracle composition stage2() of tests/test_gpu_track_frames.py on the same Tcw_in --
codes, flags and counts bit for bit, the pose by that module's close()."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import lorb_slam_amd.window as W
import test_gpu_frame as TF
import test_gpu_track_frames as TR
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DevicePoints, LocalFramesOut, enqueue_track_motion_frames, fill_slots,
                                 motion_record_addresses, track_local_frames)
from lorb_slam_amd.runtime import LorbError, lib
from test_gpu_track_frames import builders  # noqa: F401 -- the module-scoped builder fixture
from test_gpu_track_motion import close, summaries_agree

pytestmark = pytest.mark.gpu

UNCHANGED, NULL = A.LORB_ASSIGN_UNCHANGED, A.LORB_ASSIGN_NULL
EMPTY, FREE, LOCKED = A.LORB_SLOT_EMPTY, A.LORB_SLOT_FREE, A.LORB_SLOT_LOCKED
INIT = A.LORB_SLOTS_INITIALIZE
G, SENT, FILL, I4 = W.ORB_GUARD, W.ORB_SENTINEL, TR.FILL, TR.I4
NAME, DX = "320x256", 0.1
REC = C.sizeof(A.TrackLocalFramesResult)
SENT_I32 = int(np.full(4, SENT, np.uint8).view(np.int32)[0])


@functools.lru_cache(maxsize=None)
def scene():
    """The base scene's host side: frames, A's INITIALIZE image, the local map and the last frame's ids."""
    ca, cb = TR.frames(NAME)
    fp, oa, ob = ca["fp"], ca["o"], cb["o"]
    n_last, n_cur = int(oa["counts"][0]), int(ob["counts"][0])
    init, _ = TR.filled(fp, I4, oa, TR.entry_slots(n_last + 1), INIT)
    idx = np.nonzero(init["state"][:n_last] == LOCKED)[0]
    idx = idx[np.linalg.norm(init["pos"][:n_last][idx].astype(np.float64), axis=1) > 0]
    pts = {k: v for k, v in TR.local_points(init, n_last, np.zeros(0, np.int32)).items() if k != "in_frame"}
    assert len(pts["pos"]) == len(idx) and same(pts["pos"], init["pos"][:n_last][idx])
    last_id = np.full(n_last, -1, np.int32)
    last_id[idx] = np.arange(len(idx), dtype=np.int32)
    kps = dict({k: ob["left"][k] for k in ("x", "y", "octave", "angle", "desc")}, u_right=ob["u_right"])
    return dict(ca=ca, cb=cb, fp=fp, n_last=n_last, n_cur=n_cur, pts=pts, last_id=last_id, kps=kps)


def same(a, b):
    return TR.same_bytes(np.asarray(a), np.asarray(b))


def padded(pts, n):
    """pts with points behind the camera appended up to n entries: never in view, never a candidate."""
    m = n - len(pts["pos"])
    assert m > 0
    out = dict(pts)
    out["pos"] = np.concatenate([pts["pos"], np.tile(np.array([[0.5, -0.5, -6.0]], np.float32), (m, 1))])
    out["normal"] = np.concatenate([pts["normal"], np.tile(np.array([[0, 0, -1]], np.float32), (m, 1))])
    out["max_dist"] = np.concatenate([pts["max_dist"], np.full(m, 12, np.float32)])
    out["min_dist"] = np.concatenate([pts["min_dist"], np.full(m, 2, np.float32)])
    out["desc"] = np.concatenate([pts["desc"], np.full((m, 32), 0x5a, np.uint8)])
    out["locked"] = np.concatenate([pts["locked"], np.zeros(m, np.uint8)])
    if pts.get("is_bad") is not None:
        out["is_bad"] = np.concatenate([pts["is_bad"], np.zeros(m, np.uint8)])
    return out


# ---- the host model -----------------------------------------------------------------------------------
def entry_ids(masg, pass_, given, last_id, cur_id, n_cur):
    """Slot ids on entry by the id-source rule (the rule the motion tail applied to the slots)."""
    a = masg[:n_cur]
    ids = np.full(n_cur, -1, np.int32)
    ids[a >= 0] = last_id[a[a >= 0]]
    keep = (a == UNCHANGED) & (pass_ == 1) & bool(given)
    if keep.any():
        ids[keep] = cur_id[:n_cur][keep]
    return ids


def step_c(state, ids, pts):
    """src/visual_odometry.cpp:153-171: (states, ids, in_frame mask) after the held-slot loop."""
    st, ids, npt = state.copy(), ids.copy(), len(pts["pos"])
    ids[(ids < 0) | (ids >= npt)] = -1
    bad = (st != EMPTY) & (ids >= 0)
    if pts.get("is_bad") is not None and npt:
        bad &= pts["is_bad"][np.maximum(ids, 0)] != 0
    else:
        bad[:] = False
    st[bad] = EMPTY
    ids[bad] = -1
    inf = np.zeros(npt, np.uint8)
    inf[ids[(st != EMPTY) & (ids >= 0)]] = 1
    return st, ids, inf


def applied(slots_m, st, ids, a2, pts, n_cur):
    """The whole guarded slot arrays and the ids after a5's codes were applied (gate or no gate)."""
    out = {k: v.copy() for k, v in slots_m.items()}
    out["state"][:n_cur] = st
    idf = ids.copy()
    hit = a2 >= 0
    k = a2[hit]
    out["state"][:n_cur][hit] = np.where(pts["locked"][k] != 0, LOCKED, FREE)
    out["pos"][:n_cur][hit] = pts["pos"][k]
    out["desc"][:n_cur][hit] = pts["desc"][k]
    idf[hit] = k
    return out, idf


# ---- the device side ----------------------------------------------------------------------------------
class Rig:
    """One chain's device objects on a Built pair: slot sets (the last one INITIALIZE-filled), ids, the
    motion call's outputs, the local map and the new call's outputs.  Everything is freed with bt."""

    def __init__(self, ctx, bt, S, nc, pts, cur_entry=None, cur_id=None, given=False, fb=None):
        self.ctx, self.bt, self.S, self.nc, self.pts, self.given = ctx, bt, S, nc, pts, given
        self.fb = fb or bt.fb
        nl = self.nl = S["n_last"] + 1
        self.ls = bt.slots(nl, TR.entry_slots(nl))
        fill_slots(ctx, S["fp"], I4, bt.fa, self.ls, INIT)
        self.cs = bt.slots(nc, cur_entry or TR.entry_slots(nc))
        self.id_entry = TR.guarded(np.zeros(0, np.int32) if cur_id is None else np.asarray(cur_id, np.int32), nc)
        self.ids = ctx.to_device(self.id_entry)
        self.last_ids = ctx.to_device(TR.guarded(S["last_id"], nl))
        self.masg = ctx.to_device(np.full(nc + G, FILL, np.int32))
        self.mrec = ctx.to_device(np.full(C.sizeof(A.TrackFramesResult), SENT, np.uint8))
        self.dp = DevicePoints(ctx, pts)
        self.out = LocalFramesOut(ctx, self.dp.n, nc, FILL)
        bt.held += [self.ids, self.last_ids, self.masg, self.mrec, self.dp, self.out]

    def motion(self, **kw):
        pi, T = TR.prediction(DX)
        enqueue_track_motion_frames(self.ctx, self.S["fp"], T, pi, self.fb, self.cs, I4, self.bt.fa, self.ls, self.masg,
                                    self.mrec, cur_slots_given=self.given, **kw)

    def id_source(self):
        return A.TrackLocalIdSource(self.masg.ptr.value, self.mrec.ptr.value, self.last_ids.ptr.value, self.nl,
                                    1 if self.given else 0)

    def local(self, th, id_source=True, d_pose=None, d_status="motion", **kw):
        pose, status = motion_record_addresses(self.mrec)
        return track_local_frames(self.ctx, self.S["fp"], self.fb, self.cs, self.ids, d_pose or pose, self.dp, out=self.out,
                                  n_max_cur=self.nc, d_src_status=status if d_status == "motion" else d_status,
                                  id_source=self.id_source() if id_source else None, th=th, **kw)

    def read(self):
        """Everything the chain left, fetched after ONE wait (the record's fetch)."""
        rec = self.out.result()
        o = self.out
        return dict(rec=rec, rec_bytes=o.record.numpy(), mrec=self.mrec.numpy(), masg=self.masg.numpy(),
                    slots=self.cs.numpy(), ids=self.ids.numpy(), in_view=o.in_view.numpy(), track=o.track.numpy(),
                    level=o.level.numpy(), assign=o.assign.numpy())


def motion_only(ctx, bt, S, nc, cur_entry=None, given=False, fb=None, **kw):
    """The motion stage alone on fresh slot sets: what the new call finds (TR.run's dict)."""
    nl = S["n_last"] + 1
    ls = bt.slots(nl, TR.entry_slots(nl))
    fill_slots(ctx, S["fp"], I4, bt.fa, ls, INIT)
    cs = bt.slots(nc, cur_entry or TR.entry_slots(nc))
    pi, T = TR.prediction(DX)
    return TR.track_motion_frames(ctx, S["fp"], T, pi, fb or bt.fb, cs, I4, bt.fa, ls, assign_fill=FILL, cur_slots_given=given,
                                  **kw)


def two_call(ctx, fb, fp, rec, st, sp, pts, inf, th):
    """lorb_track_local_dev on the same device frame with the record's Tcw_in / pose_in / n_cur as host
    values and the host's slots-after-step-c and in_frame mask uploaded."""
    n_cur, npt = rec.n_cur, len(pts["pos"])
    dp = DevicePoints(ctx, pts)
    held = [dp, ctx.to_device(A.u8(inf)), ctx.to_device(A.u8(st)), ctx.to_device(A.f32(sp)),
            ctx.empty(npt, np.uint8), ctx.empty((4, npt), np.float32), ctx.empty(npt, np.int32), ctx.empty(n_cur, np.int32),
            ctx.to_device(np.zeros(C.sizeof(A.TrackLocalResult), np.uint8))]
    _, dinf, dst, dsp, iv, tr, lv, asg, drec = held
    try:
        dp.c.in_frame = dinf.ptr
        fps, opt, par = A.make_frame_params(fp), A.LMOptions.default(), A.TrackLocalParams(0.5, th, 20, fp["fx"])
        T16, pi = np.array(rec.Tcw_in[:], np.float32), np.array(rec.pose_in[:], np.float32)
        k = fb.keypoints(n_cur)
        ctx.check(lib().lorb_track_local_dev(ctx.handle, C.byref(fps), A.ptr(T16, C.c_float), A.ptr(pi, C.c_float),
                                             C.byref(k), dst.ptr, dsp.ptr, C.byref(dp.c), C.byref(par), C.byref(opt), iv.ptr,
                                             tr.ptr, lv.ptr, asg.ptr, drec.ptr), "lorb_track_local_dev")
        return dict(rec=A.TrackLocalResult.from_buffer_copy(drec.numpy().tobytes()), assign=asg.numpy(),
                    in_view=iv.numpy(), track=tr.numpy(), level=lv.numpy())
    finally:
        for h in held:
            h.free()


def local_fields(rec):
    return (rec.ok, rec.nmatches, rec.n_in_view, rec.n_residuals)


def check_outputs(r, w, npt, nc):
    """The chain's outputs r against the two-call sequence's w, bit for bit, and r's guard bands."""
    rec, n_cur = r["rec"], r["rec"].n_cur
    assert rec.status == 0
    assert np.array_equal(r["assign"][:n_cur], w["assign"][:n_cur]) and (r["assign"][n_cur:] == FILL).all()
    assert len(r["assign"]) == nc + G
    iv = r["in_view"][:npt]
    assert np.array_equal(iv, w["in_view"][:npt]) and set(np.unique(iv)) <= {0, 1}
    m = iv != 0
    assert same(r["track"][:4 * npt].reshape(4, npt)[:, m], w["track"].reshape(4, npt)[:, m])
    assert np.array_equal(r["level"][:npt][m], w["level"][:npt][m])
    for k, n in (("in_view", npt), ("track", 4 * npt), ("level", npt)):
        assert (np.ascontiguousarray(r[k][n:]).view(np.uint8) == SENT).all(), k
    assert (r["rec_bytes"][REC:] == SENT).all()
    assert local_fields(rec.local) == local_fields(w["rec"])
    assert same(np.array(rec.local.pose[:]), np.array(w["rec"].pose[:]))
    assert rec.local.summary.as_dict() == w["rec"].summary.as_dict()


def check_oracle(r, S, st, sp, pts, inf, th):
    """stage2(): the oracle composition given the record's Tcw_in and pose_in."""
    rec = r["rec"]
    pi2, T2 = np.array(rec.pose_in[:], np.float32), np.array(rec.Tcw_in[:], np.float32).reshape(4, 4)
    w = TR.stage2(S["fp"], S["kps"], st, sp, dict(pts, in_frame=inf), pi2, T2, th)
    n_cur = rec.n_cur
    assert np.array_equal(r["assign"][:n_cur], w["assign"]) and np.array_equal(r["in_view"][:len(inf)], w["in_view"])
    assert local_fields(rec.local) == w["counts"]
    if rec.local.ok:
        assert close(np.array(rec.local.pose[:]), w["pose"])
        summaries_agree(rec.local.summary.as_dict(), w["summary"])
    else:
        assert same(np.array(rec.local.pose[:]), pi2.astype(np.float64))
        assert rec.local.summary.as_dict() == A.BASummary().as_dict()
    return w


def check_chain(ctx, rig, r, m, th, oracle=True):
    """One chain's read-back r against everything the model gives from the motion-only run m."""
    S, pts, nc = rig.S, rig.pts, rig.nc
    rec, n_cur, npt = r["rec"], r["rec"].n_cur, len(rig.pts["pos"])
    assert rec.status == 0 and n_cur == m["n_cur"]
    assert same(r["mrec"], m["record_bytes"]) and np.array_equal(r["masg"], m["assign"])  # the same motion stage
    ids0 = entry_ids(m["assign"], m["pass_"], rig.given, S["last_id"], rig.id_entry, n_cur)
    st, ids, inf = step_c(m["cur_slots"]["state"][:n_cur], ids0, pts)
    sp = m["cur_slots"]["pos"][:n_cur].copy()
    assert (rec.n_held, rec.n_in_frame) == (int((st != EMPTY).sum()), int(inf.sum()))
    w = two_call(ctx, rig.fb, S["fp"], rec, st, sp, pts, inf, th)
    check_outputs(r, w, npt, nc)
    if oracle:
        check_oracle(r, S, st, sp, pts, inf, th)
    want_slots, want_ids = applied(m["cur_slots"], st, ids, r["assign"][:n_cur], pts, n_cur)
    TR.check_slots(r["slots"], want_slots, nc, "cur")
    assert np.array_equal(r["ids"][:n_cur], want_ids) and same(r["ids"][n_cur:], rig.id_entry[n_cur:])
    check_pose(r)
    return dict(st=st, ids=ids, inf=inf, want_ids=want_ids)


def check_pose(r, pose64=None):
    """The pose hand-over: pose_in = float32 of the doubles; Tcw_in / Tcw against O.pose_to_Tcw -- the
    translation column and the last row bit for bit, each rotation entry within 2^-23 (entries lie in
    [-1, 1], where a float ulp is at most 2^-23, and the two double evaluations differ by a few double
    ulps).  Returns how many rotation entries were not bit-equal."""
    rec = r["rec"]
    if pose64 is None:
        pose64 = np.array(A.TrackFramesResult.from_buffer_copy(r["mrec"].tobytes()).motion.pose[:], np.float64)
    pin = np.array(rec.pose_in[:], np.float32)
    assert same(pin, pose64.astype(np.float32))
    off = 0
    for T, p in ((rec.Tcw_in, pin), (rec.Tcw, np.array(rec.local.pose[:], np.float64).astype(np.float32))):
        T, w = np.array(T[:], np.float32).reshape(4, 4), O.pose_to_Tcw(p[:3], p[3:])
        assert same(T[:, 3], w[:, 3]) and same(T[3], w[3])
        d = np.abs(T[:3, :3].astype(np.float64) - w[:3, :3].astype(np.float64))
        print("Tcw rotation entries not bit-equal to the host's:", int((T[:3, :3] != w[:3, :3]).sum()), "max", d.max())
        assert d.max() <= 2.0 ** -23
        off += int((T[:3, :3] != w[:3, :3]).sum())
    if not rec.local.ok:
        assert same(np.array(rec.Tcw[:]), np.array(rec.Tcw_in[:]))
    return off


def run_base(ctx, bt, S, th, nc=None, pts=None):
    nc = nc or S["n_cur"] + 1
    rig = Rig(ctx, bt, S, nc, pts or S["pts"])
    rig.motion()
    rig.local(th)
    return rig, rig.read()


# 1 -- the chain equals the two-call sequence and the oracle ------------------------------------------------
@pytest.mark.parametrize("th", [1.0, 2.0])
def test_chain_equals_two_calls(ctx, builders, th):
    S = scene()
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = S["n_cur"] + 1
        m = motion_only(ctx, bt, S, nc)
        assert m["pass_"] == 1
        rig, r = run_base(ctx, bt, S, th)
        c = check_chain(ctx, rig, r, m, th)
        assert c["inf"].sum() >= 20 and (c["st"] == LOCKED).sum() >= 20
        assert local_fields(r["rec"].local)[:2] == ((0, 19) if th == 1.0 else (1, 22))
        assert (r["assign"][:S["n_cur"]] >= 0).sum() >= 19  # the writes are kept at th = 1 too (checked by check_chain)


# 2 -- the pose hand-over at a rotation angle near 3 rad ------------------------------------------------------
def test_pose_near_pi(ctx, builders):
    S = scene()
    axis = np.array([0.6, -0.48, 0.64])
    pose = np.concatenate([2.999 * axis / np.linalg.norm(axis), [0.1, -0.2, 0.3]]).astype(np.float64)
    pose[0] += 1e-9  # not representable in float: the rounding is at work
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        rig = Rig(ctx, bt, S, S["n_cur"] + 1, S["pts"], cur_id=np.full(S["n_cur"], -1, np.int32))
        dpose = ctx.to_device(pose)
        bt.held.append(dpose)
        rig.motion()
        rig.local(1.0, id_source=False, d_pose=dpose.ptr.value, d_status=None)
        r = rig.read()
        assert r["rec"].status == 0 and not same(pose.astype(np.float32).astype(np.float64), pose)
        assert abs(np.linalg.norm(np.array(r["rec"].pose_in[:3], np.float64)) - 2.999) < 1e-6
        check_pose(r, pose)


# 3 -- slot write-back and ids ------------------------------------------------------------------------------
def test_ids_passed_directly(ctx, builders):
    """Ids computed on the host from the motion stage's codes and passed directly give what the id
    source gives."""
    S, th = scene(), 2.0
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = S["n_cur"] + 1
        m = motion_only(ctx, bt, S, nc)
        _, ra = run_base(ctx, bt, S, th)
        ids0 = entry_ids(m["assign"], m["pass_"], False, S["last_id"], None, S["n_cur"])
        rig = Rig(ctx, bt, S, nc, S["pts"], cur_id=ids0)
        rig.motion()
        rig.local(th, id_source=False)
        rb = rig.read()
        for k in ("rec_bytes", "slots", "ids", "in_view", "track", "level", "assign"):
            if k == "slots":
                assert all(same(ra[k][q], rb[k][q]) for q in ("state", "pos", "desc"))
            else:
                assert same(ra[k], rb[k]), k


def test_given_slots_keep_their_ids(ctx, builders):
    """cur_slots_given = 1 with pre-held slots carrying ids: an UNCHANGED code keeps the id already in
    d_cur_slot_id (pass 1 stood), so that point is in the frame and leaves a8."""
    S, th = scene(), 2.0
    n_cur, npt = S["n_cur"], len(S["pts"]["pos"])
    state, pos, desc = TR.given_slots(NAME, DX)
    cur_id = np.full(n_cur, -1, np.int32)
    heldj = np.nonzero(state != EMPTY)[0]
    cur_id[heldj[::2]] = (np.arange(len(heldj[::2])) * 7) % npt  # every other pre-held slot names a table point
    nc = n_cur + 1
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        entry = TR.entry_slots(nc, state, pos, desc)
        m = motion_only(ctx, bt, S, nc, cur_entry=entry, given=True)
        kept = (m["assign"][:n_cur] == UNCHANGED) & (state != EMPTY) & (cur_id >= 0)
        assert m["pass_"] == 1 and kept.sum() >= 5
        rig = Rig(ctx, bt, S, nc, S["pts"], cur_entry=entry, cur_id=cur_id, given=True)
        rig.motion()
        rig.local(th)
        r = rig.read()
        c = check_chain(ctx, rig, r, m, th)
        assert np.array_equal(c["ids"][kept], cur_id[kept]) and c["inf"][cur_id[kept]].all()
        assert not r["in_view"][:npt][cur_id[kept]].any()


# 4 -- a bad held point ---------------------------------------------------------------------------------------
def test_bad_held_point(ctx, builders):
    S, th = scene(), 2.0
    n_cur = S["n_cur"]
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = n_cur + 1
        m = motion_only(ctx, bt, S, nc)
        _, base = run_base(ctx, bt, S, th)
        ids0 = entry_ids(m["assign"], m["pass_"], False, S["last_id"], None, n_cur)
        j = int(np.nonzero((m["cur_slots"]["state"][:n_cur] != EMPTY) & (ids0 >= 0))[0][3])
        k = int(ids0[j])
        assert (ids0 == k).sum() == 1
        pts = dict(S["pts"], is_bad=np.zeros(len(S["pts"]["pos"]), np.uint8))
        pts["is_bad"][k] = 1
        rig, r = run_base(ctx, bt, S, th, pts=pts)
        c = check_chain(ctx, rig, r, m, th)
        assert c["st"][j] == EMPTY and c["ids"][j] == -1 and c["inf"][k] == 0 and not r["in_view"][k]
        assert r["rec"].n_held == base["rec"].n_held - 1 and r["rec"].n_in_frame == base["rec"].n_in_frame - 1
        if np.array_equal(r["assign"][:n_cur], base["assign"][:n_cur]):  # the search was not disturbed: one residual fewer
            assert r["assign"][j] == UNCHANGED and r["slots"]["state"][j] == EMPTY and r["ids"][j] == -1
            assert r["rec"].local.n_residuals == base["rec"].local.n_residuals - 1


# 5 -- paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["guard_of_one", "capacity", "count_scan_write"])
@pytest.mark.parametrize("th", [1.0, 2.0])
def test_paths(ctx, builders, path, th):
    S = scene()
    n_cur, npt0 = S["n_cur"], len(S["pts"]["pos"])
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        _, base = run_base(ctx, bt, S, th)
        nc, pts = n_cur + 1, S["pts"]
        if path == "capacity":
            nc = bt.b.capacity
            assert nc > 1024 and npt0 * nc <= 1 << 20  # the k_grid_build path, still one strided pass
        elif path == "count_scan_write":
            pts = padded(S["pts"], (1 << 20) // nc + 8)
            assert 1 << 20 < len(pts["pos"]) * nc <= 8 << 20
        m = motion_only(ctx, bt, S, nc)
        rig, r = run_base(ctx, bt, S, th, nc=nc, pts=pts)
        check_chain(ctx, rig, r, m, th)
        # the same results as the base path
        assert np.array_equal(r["assign"][:n_cur], base["assign"][:n_cur])
        assert np.array_equal(r["in_view"][:npt0], base["in_view"][:npt0]) and not r["in_view"][npt0:len(pts["pos"])].any()
        assert bytes(r["rec"].local)[:16 + 48] == bytes(base["rec"].local)[:16 + 48]  # counts and pose
        assert r["rec"].local.summary.as_dict() == base["rec"].local.summary.as_dict()
        assert np.array_equal(r["ids"][:n_cur], base["ids"][:n_cur])
        for k in ("state", "pos", "desc"):
            assert same(r["slots"][k][:n_cur], base["slots"][k][:n_cur]), k


# 6 -- edges --------------------------------------------------------------------------------------------------
def test_motion_stage_fails(ctx, builders):
    """pass == 0 (the motion stage's min_matches above the keypoint count): stage 2 starts from pose_init
    widened and runs over the slots the retry rule left."""
    S, th = scene(), 2.0
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = S["n_cur"] + 1
        m = motion_only(ctx, bt, S, nc, min_matches=100000)
        assert m["pass_"] == 0 and same(m["pose"], TR.prediction(DX)[0].astype(np.float64))
        rig = Rig(ctx, bt, S, nc, S["pts"])
        rig.motion(min_matches=100000)
        rig.local(th)
        r = rig.read()
        check_chain(ctx, rig, r, m, th)
        assert same(np.array(r["rec"].pose_in[:], np.float32), TR.prediction(DX)[0])


def test_blank_current_frame(ctx, builders):
    """n_cur = 0: the fields are still computed, nothing matches, ok is 0."""
    S, th = scene(), 1.0
    geom = (256, 320, 8, 500)
    none = TF.blank_case(*geom, "left")
    assert int(none["o"]["counts"][0]) == 0
    with TR.Built(ctx, builders, dict(S["ca"], geom=geom), none) as bt:
        nc = 2
        m = motion_only(ctx, bt, S, nc)
        assert m["n_cur"] == 0 and m["pass_"] == 0
        rig = Rig(ctx, bt, S, nc, S["pts"])
        rig.motion()
        rig.local(th)
        r = rig.read()
        check_chain(ctx, rig, r, m, th, oracle=False)  # the oracle is not asked about empty frames
        rec = r["rec"]
        assert (rec.n_cur, rec.n_held, rec.n_in_frame, rec.local.ok, rec.local.nmatches) == (0, 0, 0, 0, 0)
        assert rec.local.n_in_view == int(r["in_view"][:len(S["pts"]["pos"])].sum()) > 0


def test_no_points(ctx, builders):
    """d_pts->n = 0."""
    S, th = scene(), 1.0
    pts = {k: (None if v is None else v[:0]) for k, v in S["pts"].items()}
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = S["n_cur"] + 1
        m = motion_only(ctx, bt, S, nc)
        rig, r = run_base(ctx, bt, S, th, pts=pts)
        check_chain(ctx, rig, r, m, th, oracle=False)
        rec = r["rec"]
        assert (rec.local.ok, rec.local.nmatches, rec.local.n_in_view, rec.n_in_frame) == (0, 0, 0, 0)
        assert (r["assign"][:S["n_cur"]] == UNCHANGED).all() and rec.n_held > 0


# 7 -- status ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fail", ["count_above", "count_negative", "src_status"])
def test_status(ctx, builders, fail):
    """A failing input stores status = 1 and nothing else: every other output byte keeps its fill
    pattern, the record included; the next call on the same context is correct."""
    S, th = scene(), 2.0
    n_cur = S["n_cur"]
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = n_cur + 1
        m = motion_only(ctx, bt, S, nc)
        ids0 = entry_ids(m["assign"], m["pass_"], False, S["last_id"], None, n_cur)
        rig = Rig(ctx, bt, S, nc, S["pts"], cur_id=ids0)
        rig.motion()
        ctx.sync()
        before = dict(slots=rig.cs.numpy(), ids=rig.ids.numpy())
        dpose = ctx.to_device(m["pose"])
        dstat = ctx.to_device(np.array([0 if fail != "src_status" else 3], np.int32))
        bt.held += [dpose, dstat]
        counts = bt.fb.counts.numpy()
        if fail != "src_status":
            bad = counts.copy()
            bad[0] = nc + 1 if fail == "count_above" else -1
            ctx.check(lib().lorb_memcpy_h2d(ctx.handle, bt.fb.counts.ptr, bad.ctypes.data_as(C.c_void_p),
                                            C.c_size_t(bad.nbytes)), "h2d")
        rig.local(th, id_source=False, d_pose=dpose.ptr.value, d_status=dstat.ptr.value)
        r = rig.read()
        ctx.check(lib().lorb_memcpy_h2d(ctx.handle, bt.fb.counts.ptr, counts.ctypes.data_as(C.c_void_p),
                                        C.c_size_t(counts.nbytes)), "h2d")
        assert r["rec"].status == 1
        rec = A.TrackLocalFramesResult.from_buffer_copy(r["rec_bytes"].tobytes()[:REC])
        rec.status = SENT_I32
        assert (np.frombuffer(bytes(rec), np.uint8) == SENT).all() and (r["rec_bytes"][REC:] == SENT).all()
        assert (r["assign"] == FILL).all()
        for k in ("in_view", "track", "level"):
            assert (np.ascontiguousarray(r[k]).view(np.uint8) == SENT).all(), k
        assert all(same(r["slots"][q], before["slots"][q]) for q in ("state", "pos", "desc")) and same(r["ids"], before["ids"])
        # the next call on the same context
        rig2, r2 = run_base(ctx, bt, S, th)
        check_chain(ctx, rig2, r2, m, th)


# 8 -- context reuse ----------------------------------------------------------------------------------------------
def test_context_reuse(ctx, builders):
    """Scratch-slot reuse: after the new call the existing chains give their own results on the same
    context -- lorb_track_local_dev (inside check_chain), lorb_track_motion_frames_dev, the motion chain
    on host-built inputs and a4 through search_by_projection_frame_dev."""
    import test_gpu_track_motion as TM
    S, th = scene(), 2.0
    s = TM.frames(500, 200, 1)
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        for nc in (bt.b.capacity, S["n_cur"] + 1):
            m = motion_only(ctx, bt, S, nc)
            rig, r = run_base(ctx, bt, S, th, nc=nc)
            check_chain(ctx, rig, r, m, th)
            m2 = motion_only(ctx, bt, S, nc)
            assert same(m2["record_bytes"], m["record_bytes"]) and np.array_equal(m2["assign"], m["assign"])
            assert all(same(m2["cur_slots"][q], m["cur_slots"][q]) for q in ("state", "pos", "desc"))
            for d in (0.0, 0.7):
                TM.check(TM.run(ctx, s, d, None, None), TM.expected(s, d, None, None))
            a_g, n_g = ctx.search_by_projection_frame_dev(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], 15.0)
            a_o, n_o = O.search_by_projection_frame(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], 15.0)
            assert n_g == n_o and np.array_equal(a_g, a_o)


def test_errors(ctx, builders):
    """With a live context the invalid arguments of tests/test_track_local_frames_abi.py are
    LORB_E_INVALID before anything is enqueued; the next call is fine."""
    S, th = scene(), 2.0
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nc = S["n_cur"] + 1
        m = motion_only(ctx, bt, S, nc)
        rig = Rig(ctx, bt, S, nc, S["pts"])
        rig.motion()
        for kw in (dict(n_max_cur=0), dict(n_max_cur=-1), dict(n_max_cur=(8 << 20) // rig.dp.n + 1), dict(min_matches=-1)):
            with pytest.raises(LorbError):
                track_local_frames(ctx, S["fp"], rig.fb, rig.cs, rig.ids, motion_record_addresses(rig.mrec)[0], rig.dp,
                                   out=rig.out, **dict(dict(n_max_cur=nc), **kw))
        mask = ctx.to_device(np.zeros(rig.dp.n, np.uint8))
        bt.held.append(mask)
        rig.dp.c.in_frame = mask.ptr
        with pytest.raises(LorbError, match="in_frame"):
            rig.local(th)
        rig.dp.c.in_frame = None
        rig.local(th)
        check_chain(ctx, rig, rig.read(), m, th)
