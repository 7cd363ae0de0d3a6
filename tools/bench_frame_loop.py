#!/usr/bin/env python3
"""Per-frame cost of the tracked-frame loop with and without a host step between frames: what the
motion-model hand-over (src/visual_odometry.cpp:65, :119, Frame::SetPose) costs when the host does it,
which needs one wait per frame, against the same hand-over in device memory (lorb_frame_pose /
lorb_motion_model blocks), where a whole round of frames is enqueued and waited for once.

Sizes, images and the store are tools/bench_local_map.py's (480 x 752, 1000 features, 8 levels, bounds
1250, max_local 4096, 4500 points under 12 keyframes).  As there, the last frame is built once,
INITIALIZE-filled and resident at the identity, and every timed frame builds the current frame from the
second image pair and tracks it against that last frame; what is new is that frame k + 1's predicted pose
is last.Tcw * mTcc with the mTcc frame k left (mTcc = last.Twc * cur.Tcw), so frame k + 1 cannot start
before frame k's pose exists.  Every call goes through prebuilt ctypes arguments.

  a  the route before lorb_track_motion_frames_pose_dev, per frame: the host prediction (T_pred =
     T_last * mTcc, lorb_frame_pose_from_Tcw of it: the matrix, its Rodrigues vector), lorb_frame_build_dev,
     lorb_track_motion_frames_dev on those host values, lorb_local_map_update_dev,
     lorb_track_local_frames_dev, lorb_local_map_ids_back_dev, lorb_memcpy_d2h of the local record (the
     frame's wait), then lorb_pose_to_Tcw of the rounded pose, lorb_frame_pose_from_Tcw of it (Twc) and
     mTcc = Twc_last * Tcw.  The two 4 x 4 products are numpy's (float32) into preallocated arrays.
  b  per frame: lorb_frame_build_dev, lorb_track_motion_frames_pose_dev with the model block,
     lorb_local_map_update_dev, lorb_track_local_frames_dev, lorb_local_map_ids_back_dev,
     lorb_frame_pose_finish_dev; nothing waits until the round's last frame is enqueued, then one lorb_sync.

Protocol (tools/bench_local_map.py's): warm-up of every arm, then `--repeats` rounds; in every round each
arm runs `--calls` frames, the arms interleaved inside the round; every round starts from mTcc = I and
ends with a check that its last frame's status is 0 (outside the timed region).  Reported per arm: median
and min / max over the rounds of the mean time per frame.  Gate: b's median below a's median by more than
a's own min-max spread.

  python tools/bench_frame_loop.py --out profiles/r16/frame_loop.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_frame_loop.py --only b --repeats 1 --calls 20
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lorb_slam_amd.window  # noqa: E402,F401
from bench_frame import features_per_level  # noqa: E402
from bench_local_map import BOUND, COLS, MAX_LOCAL, N_KF, N_LEVELS, N_POINTS, NFEATURES, ROWS, SEED, make_store  # noqa: E402
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd import synth  # noqa: E402
from lorb_slam_amd.frame import (DeviceMapStore, DeviceSlots, FrameBuilder, LocalFramesOut, LocalMap, fill_slots,  # noqa: E402
                                 frame_pose_from_Tcw, local_map_buffers, local_map_result, model_block,
                                 motion_record_addresses, pose_block)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

F32P = C.POINTER(C.c_float)


def build_arms(ctx):
    L, h = lib(), ctx.handle
    fp = synth.frame_params(width=COLS, height=ROWS)
    fps = A.make_frame_params(fp)
    nd = features_per_level(NFEATURES)
    pat = np.random.default_rng(7).integers(-13, 13, size=1024).astype(np.int32)
    fb = FrameBuilder(ctx, fp, ROWS, COLS, nd, pat)
    last_img = synth.stereo_pair(SEED, ROWS, COLS)
    cur_img = synth.stereo_pair(SEED, ROWS, COLS, shift=2, noise_seed=777)
    fa = fb.build_device(*last_img)  # the last frame: built once, resident
    n_last = int(fa.read_counts()[0])
    held = [fa]

    def keep(d):
        held.append(d)
        return d

    I4 = np.eye(4, dtype=np.float32)
    mpar, lpar, opt = A.TrackMotionParams(15.0, 30.0, 20, fps.fx), A.TrackLocalParams(0.5, 1.0, 20, fps.fx), A.LMOptions.default()
    cols, nb = C.c_int32(COLS), C.c_int32(BOUND)
    mrec_bytes, lrec_bytes = C.sizeof(A.TrackFramesResult), C.sizeof(A.TrackLocalFramesResult)

    # the last frame's slots (INITIALIZE), the store around its initialised points, the local map (the arms run in turn)
    ls = keep(DeviceSlots(ctx, BOUND, state=0))
    fill_slots(ctx, fp, I4, fa, ls, A.LORB_SLOTS_INITIALIZE)
    s0 = ls.numpy()
    idx = np.nonzero(s0["state"][:n_last] == A.LORB_SLOT_LOCKED)[0]
    d = np.linalg.norm(s0["pos"][idx].astype(np.float64), axis=1)
    idx, d = idx[d > 0], d[d > 0]
    pos = s0["pos"][idx]
    npt = len(idx)
    pts0 = dict(pos=pos, normal=(pos / d[:, None]).astype(np.float32), max_dist=(1.6 * d).astype(np.float32),
                min_dist=(0.6 * d).astype(np.float32), desc=s0["desc"][idx], locked=np.ones(npt, np.uint8))
    last_gid = np.full(BOUND, -1, np.int32)
    last_gid[idx] = np.arange(npt, dtype=np.int32)
    d_last_gid = keep(ctx.to_device(last_gid))
    store = keep(DeviceMapStore(ctx, *make_store(pts0, last_gid[:n_last])))
    lmap = keep(LocalMap(ctx, MAX_LOCAL, N_KF, N_POINTS))

    def arm_buffers():
        f = keep(fb.build_device(*cur_img))  # the current frame's buffers; rebuilt in every frame
        b = dict(f=f, l=f._all[-2], r=f._all[-1], cs=keep(DeviceSlots(ctx, BOUND, state=0)),
                 masg=keep(ctx.empty(BOUND, np.int32)), mrec=keep(ctx.empty(mrec_bytes, np.uint8)),
                 out=keep(LocalFramesOut(ctx, MAX_LOCAL, BOUND)))
        b["gid"], b["sid"], b["urec"] = (keep(x) for x in local_map_buffers(ctx, BOUND))
        b["d_pose"], b["d_status"] = (C.c_void_p(v) for v in motion_record_addresses(b["mrec"]))
        b["src"] = A.TrackLocalIdSource(b["masg"].ptr.value, b["mrec"].ptr.value, d_last_gid.ptr.value, BOUND, 0)
        b["d_ustatus"] = C.c_void_p(b["urec"].ptr.value + A.LocalMapResult.status.offset)
        b["d_lstatus"] = C.c_void_p(b["out"].record.ptr.value + A.TrackLocalFramesResult.status.offset)
        return b

    def back(b):  # what both arms enqueue behind the motion stage
        o = b["out"]
        rc = L.lorb_local_map_update_dev(h, lmap._p, C.byref(store.c), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["gid"].ptr,
                                         b["sid"].ptr, b["d_status"], C.byref(b["src"]), b["urec"].ptr)
        rc |= L.lorb_track_local_frames_dev(h, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["sid"].ptr, b["d_pose"],
                                            b["d_ustatus"], None, C.byref(lmap.c), C.byref(lpar), C.byref(opt), o.in_view.ptr,
                                            o.track.ptr, o.level.ptr, o.assign.ptr, o.record.ptr)
        return rc | L.lorb_local_map_ids_back_dev(h, lmap._p, C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["sid"].ptr,
                                                  b["d_lstatus"], b["gid"].ptr)

    # arm a: the host's motion model
    a = arm_buffers()
    last_h = frame_pose_from_Tcw(I4)
    T_last, Twc_last = (np.ctypeslib.as_array(x).reshape(4, 4) for x in (last_h.Tcw, last_h.Twc))
    a_Tcc, a_Tpred, a_Tcw = I4.copy(), I4.copy(), I4.copy()
    a_pred, a_cur, a_lrec = A.FramePose(), A.FramePose(), A.TrackLocalFramesResult()
    a_pose64 = np.ctypeslib.as_array(a_lrec.local.pose)
    a_pose32 = np.zeros(6, np.float32)
    p_Tpred, p_Tcw, p_last = (x.ctypes.data_as(F32P) for x in (a_Tpred, a_Tcw, T_last))
    p_rv, p_tv = a_pose32[:3].ctypes.data_as(F32P), a_pose32[3:].ctypes.data_as(F32P)
    p_pred_T = C.cast(C.addressof(a_pred) + A.FramePose.Tcw.offset, F32P)
    p_pred_pose = C.cast(C.addressof(a_pred) + A.FramePose.pose.offset, F32P)

    def frame_a():
        np.dot(T_last, a_Tcc, out=a_Tpred)  # pF->GetPose() * mTcc
        rc = L.lorb_frame_pose_from_Tcw(p_Tpred, C.byref(a_pred))  # SetPose(Tcw): the vector the LM starts from
        rc |= L.lorb_frame_build_dev(fb._p, a["l"].ptr, cols, a["r"].ptr, cols, C.byref(a["f"].out))
        rc |= L.lorb_track_motion_frames_dev(h, C.byref(fps), p_pred_T, p_pred_pose, C.byref(a["f"].out), nb, C.byref(a["cs"].c),
                                             C.c_int32(0), p_last, C.byref(fa.out), nb, C.byref(ls.c), None, C.byref(mpar),
                                             C.byref(opt), a["masg"].ptr, a["mrec"].ptr)
        rc |= back(a)
        rc |= L.lorb_memcpy_d2h(h, C.byref(a_lrec), a["out"].record.ptr, C.c_size_t(lrec_bytes))  # the frame's wait
        a_pose32[:] = a_pose64  # the write-back's rounding
        L.lorb_pose_to_Tcw(p_rv, p_tv, p_Tcw)  # Frame::SetPose(Tvec, Rvec)
        rc |= L.lorb_frame_pose_from_Tcw(p_Tcw, C.byref(a_cur))  # its Twc
        np.dot(Twc_last, a_Tcw, out=a_Tcc)  # mTcc = mPrevFrame->GetInvPose() * mCurrFrame->GetPose()
        return rc

    def round_a(n):
        a_Tcc[:] = I4
        t0 = time.perf_counter()
        rc = 0
        for _ in range(n):
            rc |= frame_a()
        dt = time.perf_counter() - t0
        assert rc == 0 and a_lrec.status == 0, (rc, a_lrec.status)
        return dt / n * 1e6

    # arm b: the hand-over in device memory
    b = arm_buffers()
    b_last, b_cur, b_model = keep(pose_block(ctx, I4)), keep(pose_block(ctx, I4)), keep(model_block(ctx, I4))
    model_I = A.MotionModel()
    model_I.Tcc[:] = [float(v) for v in I4.reshape(16)]

    def frame_b():
        rc = L.lorb_frame_build_dev(fb._p, b["l"].ptr, cols, b["r"].ptr, cols, C.byref(b["f"].out))
        rc |= L.lorb_track_motion_frames_pose_dev(h, C.byref(fps), b_cur.ptr, C.byref(b["f"].out), nb, C.byref(b["cs"].c),
                                                  C.c_int32(0), b_last.ptr, b_model.ptr, C.byref(fa.out), nb, C.byref(ls.c), None,
                                                  C.byref(mpar), C.byref(opt), b["masg"].ptr, b["mrec"].ptr)
        rc |= back(b)
        return rc | L.lorb_frame_pose_finish_dev(h, b["out"].record.ptr, b_last.ptr, b_cur.ptr, b_model.ptr)

    def round_b(n):
        b_model.upload(model_I)
        t0 = time.perf_counter()
        rc = 0
        for _ in range(n):
            rc |= frame_b()
        rc |= L.lorb_sync(h)  # the round's one wait
        dt = time.perf_counter() - t0
        st = b["out"].result().status
        assert rc == 0 and st == 0, (rc, st)
        return dt / n * 1e6

    def verify():
        """The first two frames of a round in each arm.  Frame 1 starts from mTcc = I in both: the same
        codes, counts and pose, bit for bit.  Frame 2 starts from the model frame 1 left, and the host's
        float32 product may differ from the device's double accumulation in the last bit: the same counts,
        the pose to 1e-6."""
        out = {}
        for n in (1, 2):
            round_a(n)
            round_b(n)
            ra, rb = a["out"].result(), b["out"].result()
            ub = local_map_result(b["urec"])
            mb = A.TrackFramesResult.from_buffer_copy(b["mrec"].numpy().tobytes())
            ma = A.TrackFramesResult.from_buffer_copy(a["mrec"].numpy().tobytes())
            n_cur = rb.n_cur
            assert ra.status == 0 and rb.status == 0 and ub.status == 0 and mb.status == 0
            fa_, fb_ = ((r.local.ok, r.local.nmatches, r.local.n_in_view, r.local.n_residuals) for r in (ra, rb))
            assert fa_ == fb_ and (ma.motion.pass_, ma.motion.nmatches_first) == (mb.motion.pass_, mb.motion.nmatches_first)
            if n == 1:
                assert np.array_equal(a["masg"].numpy()[:n_cur], b["masg"].numpy()[:n_cur])
                assert np.array_equal(a["out"].assign.numpy()[:n_cur], b["out"].assign.numpy()[:n_cur])
            pa, pb = np.array(ra.local.pose[:]), np.array(rb.local.pose[:])
            assert (pa == pb).all() if n == 1 else np.abs(pa - pb).max() < 1e-6, (n, pa, pb)
            out[f"frame{n}"] = dict(motion_nmatches=mb.motion.nmatches_first, local_ok=rb.local.ok, local_nmatches=rb.local.nmatches,
                                    local_n_in_view=rb.local.n_in_view, local_n_residuals=rb.local.n_residuals,
                                    lm_iterations=rb.local.summary.iterations, n_local=ub.n_local, pose=[float(v) for v in pb])
        return dict(n_last=n_last, n_cur=n_cur, bound=BOUND, max_local=MAX_LOCAL, store_points=N_POINTS, store_keyframes=N_KF, **out)

    def cleanup():
        for x in held:
            x.free()
        fb.close()

    return dict(a=round_a, b=round_b), verify, cleanup, (pat, last_h, a_pred, a_cur, a_lrec, model_I, p_pred_T, p_pred_pose)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--only", choices=["a", "b"], help="run one arm only (for a profiler run)")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.calls >= 100 or args.only, "protocol: >= 5 repeats of >= 100 calls"

    ctx = Context(0)
    arms, verify, cleanup, keep = build_arms(ctx)
    info = verify()
    names = [args.only] if args.only else ["a", "b"]
    for a in names:
        arms[a](args.warmup)
    samples = {a: [] for a in names}
    for _ in range(args.repeats):
        for a in names:  # interleaved: every round times every arm
            samples[a].append(arms[a](args.calls))
    rec = dict(tool="tools/bench_frame_loop.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
               unit="us per frame",
               workload="synth.stereo_pair(%d, %d, %d) -> the same, shift 2, noise seed 777; %d features, %d levels" %
               (SEED, ROWS, COLS, NFEATURES, N_LEVELS), **info, arms={})
    for a in names:
        v = samples[a]
        rec["arms"][a] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    if not args.only:
        A_, B_ = rec["arms"]["a"], rec["arms"]["b"]
        spread_a = A_["max"] - A_["min"]
        rec["gate"] = dict(b_below_a_by=A_["median"] - B_["median"], a_spread=spread_a,
                           b_faster_than_a=A_["median"] - B_["median"] > spread_a)
        rec["gate_holds"] = rec["gate"]["b_faster_than_a"]
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    cleanup()
    ctx.close()


if __name__ == "__main__":
    main()
