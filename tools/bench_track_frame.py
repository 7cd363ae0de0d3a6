#!/usr/bin/env python3
"""Per-frame cost of one tracked frame on the GPU, "image pair in -> local-map pose out": the stereo
Frame constructor, VisualOdometry::EstimatePoseMotion and EstimatePoseLocal
(src/visual_odometry.cpp:37-75), the last frame already built, INITIALIZE-filled and resident, the local
map its initialised points.

Two arms on the same two image pairs, every one through prebuilt ctypes arguments (so Python
marshalling is outside the timed region):
  a  what a caller had to do before lorb_track_local_frames_dev: lorb_frame_build_dev,
     lorb_track_motion_frames_dev, lorb_sync, lorb_memcpy_d2h of the record and of assign, the pose
     rounded and lorb_pose_to_Tcw on the host, the in_frame mask worked out from assign (numpy) and
     uploaded (lorb_memcpy_h2d), lorb_track_local_dev, lorb_sync
  b  lorb_frame_build_dev, lorb_track_motion_frames_dev, lorb_track_local_frames_dev (pose, status and
     ids from the motion stage's device outputs), lorb_sync
Both leave assign, the tracking fields and the result record in device memory.  Input:
synth.stereo_pair(500, 480, 752) as the last frame, the same scene 2 pixels further with other pixel
noise as the current one, 1000 features, 8 levels, bounds 1250; last frame at the identity, predicted
pose the identity.

Protocol (tools/bench_track_frames.py's): warm-up of every arm, then `--repeats` rounds; in every round
each arm runs `--calls` calls back to back, the arms interleaved inside the round.  Reported per arm:
median and min / max over the rounds of the mean time per call.  Gate: b's median below a's median by
more than a's own min-max spread.

  python tools/bench_track_frame.py --out profiles/r14/track_frame.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_track_frame.py --only b --repeats 1 --calls 20
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lorb_slam_amd.window  # noqa: E402,F401
from bench_frame import features_per_level, time_calls  # noqa: E402
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd import synth  # noqa: E402
from lorb_slam_amd.frame import (DevicePoints, DeviceSlots, FrameBuilder, LocalFramesOut, fill_slots,  # noqa: E402
                                 motion_record_addresses)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

ROWS, COLS, NFEATURES, N_LEVELS, SEED = 480, 752, 1000, 8, 500
BOUND = NFEATURES + NFEATURES // 4


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

    I = np.eye(4, dtype=np.float32).reshape(16)
    Tp, pi = A.ptr(I, C.c_float), np.zeros(6, np.float32)
    pip = A.ptr(pi, C.c_float)
    mpar, lpar, opt = A.TrackMotionParams(15.0, 30.0, 20, fps.fx), A.TrackLocalParams(0.5, 1.0, 20, fps.fx), A.LMOptions.default()
    cols, nb = C.c_int32(COLS), C.c_int32(BOUND)
    mrec_bytes = C.sizeof(A.TrackFramesResult)

    # the last frame's slots (INITIALIZE, then the motion stage's UpdateFrame fill, which is idempotent) and the
    # local map: its initialised points, plausible normals and distance bounds
    ls = keep(DeviceSlots(ctx, BOUND, state=0))
    fill_slots(ctx, fp, I.reshape(4, 4), fa, ls, A.LORB_SLOTS_INITIALIZE)
    s0 = ls.numpy()
    idx = np.nonzero(s0["state"][:n_last] == A.LORB_SLOT_LOCKED)[0]
    d = np.linalg.norm(s0["pos"][idx].astype(np.float64), axis=1)
    idx, d = idx[d > 0], d[d > 0]
    pos = s0["pos"][idx]
    npt = len(idx)
    pts = dict(pos=pos, normal=(pos / d[:, None]).astype(np.float32), max_dist=(1.6 * d).astype(np.float32),
               min_dist=(0.6 * d).astype(np.float32), desc=s0["desc"][idx], locked=np.ones(npt, np.uint8), is_bad=None)
    last_id = np.full(BOUND, -1, np.int32)
    last_id[idx] = np.arange(npt, dtype=np.int32)
    d_last_id = keep(ctx.to_device(last_id))

    def arm_buffers():
        f = keep(fb.build_device(*cur_img))  # the current frame's buffers; rebuilt in every call
        return dict(f=f, l=f._all[-2], r=f._all[-1], cs=keep(DeviceSlots(ctx, BOUND, state=0)),
                    masg=keep(ctx.empty(BOUND, np.int32)), mrec=keep(ctx.empty(mrec_bytes, np.uint8)),
                    dp=keep(DevicePoints(ctx, pts)), out=keep(LocalFramesOut(ctx, npt, BOUND)))

    def front(b):  # the part both arms share: the builder and the motion stage
        rc = L.lorb_frame_build_dev(fb._p, b["l"].ptr, cols, b["r"].ptr, cols, C.byref(b["f"].out))
        return rc | L.lorb_track_motion_frames_dev(h, C.byref(fps), Tp, pip, C.byref(b["f"].out), nb, C.byref(b["cs"].c),
                                                   C.c_int32(0), Tp, C.byref(fa.out), nb, C.byref(ls.c), None, C.byref(mpar),
                                                   C.byref(opt), b["masg"].ptr, b["mrec"].ptr)

    # arm a
    a = arm_buffers()
    a_mrec, a_masg = np.zeros(mrec_bytes, np.uint8), np.zeros(BOUND, np.int32)
    a_mask, d_mask = np.zeros(max(npt, 1), np.uint8), keep(ctx.empty(max(npt, 1), np.uint8))
    a["dp"].c.in_frame = d_mask.ptr
    a_pose, a_T = np.zeros(6, np.float32), np.zeros(16, np.float32)
    ka = a["f"].keypoints(0)
    a_lrec = keep(ctx.empty(C.sizeof(A.TrackLocalResult), np.uint8))

    def arm_a():
        rc = front(a) | L.lorb_sync(h)
        rc |= L.lorb_memcpy_d2h(h, a_mrec.ctypes.data_as(C.c_void_p), a["mrec"].ptr, C.c_size_t(mrec_bytes))
        rc |= L.lorb_memcpy_d2h(h, a_masg.ctypes.data_as(C.c_void_p), a["masg"].ptr, C.c_size_t(4 * BOUND))
        rec = A.TrackFramesResult.from_buffer(a_mrec)
        ka.n = rec.n_cur
        a_pose[:] = rec.motion.pose[:]  # the rounding of Frame::SetPose
        L.lorb_pose_to_Tcw(A.ptr(a_pose, C.c_float), A.ptr(a_pose[3:], C.c_float), A.ptr(a_T, C.c_float))
        code = a_masg[:rec.n_cur]
        ids = last_id[code[code >= 0]]
        a_mask[:] = 0
        a_mask[ids[ids >= 0]] = 1
        rc |= L.lorb_memcpy_h2d(h, d_mask.ptr, a_mask.ctypes.data_as(C.c_void_p), C.c_size_t(a_mask.nbytes))
        o = a["out"]
        rc |= L.lorb_track_local_dev(h, C.byref(fps), A.ptr(a_T, C.c_float), A.ptr(a_pose, C.c_float), C.byref(ka),
                                     a["cs"].state.ptr, a["cs"].pos.ptr, C.byref(a["dp"].c), C.byref(lpar), C.byref(opt),
                                     o.in_view.ptr, o.track.ptr, o.level.ptr, o.assign.ptr, a_lrec.ptr)
        return rc | L.lorb_sync(h)

    # arm b
    b = arm_buffers()
    b_ids = keep(ctx.to_device(np.full(BOUND, -1, np.int32)))
    d_pose, d_status = (C.c_void_p(v) for v in motion_record_addresses(b["mrec"]))
    src = A.TrackLocalIdSource(b["masg"].ptr.value, b["mrec"].ptr.value, d_last_id.ptr.value, BOUND, 0)

    def arm_b():
        o = b["out"]
        rc = front(b)
        rc |= L.lorb_track_local_frames_dev(h, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b_ids.ptr, d_pose,
                                            d_status, C.byref(src), C.byref(b["dp"].c), C.byref(lpar), C.byref(opt),
                                            o.in_view.ptr, o.track.ptr, o.level.ptr, o.assign.ptr, o.record.ptr)
        return rc | L.lorb_sync(h)

    def verify():
        for f in (arm_a, arm_b):
            assert f() == 0, f.__name__
        ra = A.TrackLocalResult.from_buffer_copy(a_lrec.numpy().tobytes())
        rb = b["out"].result()
        mb = A.TrackFramesResult.from_buffer_copy(b["mrec"].numpy().tobytes())
        n_cur = rb.n_cur
        assert rb.status == 0 and mb.status == 0 and max(n_last, n_cur) <= BOUND and mb.motion.pass_ == 1
        same_T = np.array_equal(a_T, np.array(rb.Tcw_in[:], np.float32))
        fa_, fb_ = ((r.ok, r.nmatches, r.n_in_view, r.n_residuals) for r in (ra, rb.local))
        if same_T:  # the host's Tcw has the device's bits: the same kernels' bodies on the same data
            assert fa_ == fb_ and ra.pose[:] == rb.local.pose[:], (fa_, fb_)
            assert np.array_equal(a["out"].assign.numpy()[:n_cur], b["out"].assign.numpy()[:n_cur])
        strided = npt * BOUND <= 1 << 20
        return dict(n_last=n_last, n_cur=n_cur, bound=BOUND, capacity=fb.capacity, n_points=npt, n_in_frame=rb.n_in_frame,
                    n_held=rb.n_held, motion_nmatches=mb.motion.nmatches_first, local_ok=rb.local.ok,
                    local_nmatches=rb.local.nmatches, local_n_in_view=rb.local.n_in_view,
                    local_n_residuals=rb.local.n_residuals, lm_iterations=rb.local.summary.iterations,
                    host_Tcw_has_device_bits=bool(same_T), arm_a_local=list(fa_),
                    local_path="grid build + " + ("one strided candidate pass" if strided else "count / scan / write"))

    def cleanup():
        for x in held:
            x.free()
        fb.close()

    return dict(a=arm_a, b=arm_b), verify, cleanup, (pi, I, pat, last_id, a_mask, a_pose, a_T, a_mrec, a_masg, src)


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
        time_calls(arms[a], args.warmup)
    samples = {a: [] for a in names}
    for _ in range(args.repeats):
        for a in names:  # interleaved: every round times every arm
            samples[a].append(time_calls(arms[a], args.calls))
    rec = dict(tool="tools/bench_track_frame.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
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
