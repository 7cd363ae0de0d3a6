#!/usr/bin/env python3
"""Per-frame cost of "image pair in -> motion-model pose out" on the GPU: the stereo Frame constructor
followed by VisualOdometry::EstimatePoseMotion (src/visual_odometry.cpp:117-138), the last frame
already built and resident.

Two arms on the same two image pairs, every one through prebuilt ctypes arguments (so Python
marshalling is outside the timed region):
  a  what a caller had to do before lorb_track_motion_frames_dev: lorb_frame_build_dev,
     lorb_memcpy_d2h of the counts, lorb_memcpy_h2d of the has_mp | mp_locked masks (one upload),
     lorb_unproject_stereo_dev of the last frame, lorb_track_motion_dev, lorb_sync
  b  lorb_frame_build_dev, lorb_track_motion_frames_dev with both bounds nfeatures + 25 %, lorb_sync
     (arm b also clears the last frame's slot states first -- one asynchronous lorb_memset_dev -- so
     that UpdateFrame creates every point in every call, as arm a's unprojection of every keypoint does)
Both leave assign and the result record in device memory.  Input: synth.stereo_pair(500, 480, 752) as the
last frame, the same scene 2 pixels further with other pixel noise as the current one, 1000 features, 8
levels; last frame at the identity, predicted pose the identity.

Protocol (tools/bench_frame.py's): warm-up of every arm, then `--repeats` rounds; in every round each arm
runs `--calls` calls back to back, the arms interleaved inside the round.  Reported per arm: median and
min / max over the rounds of the mean time per call.  Gate: b's median below a's median by more than a's
own min-max spread.

  python tools/bench_track_frames.py --out profiles/r12/track_frames.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_track_frames.py --only b --repeats 1 --calls 20
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
from bench_frame import features_per_level, time_calls  # noqa: E402
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd import synth  # noqa: E402
from lorb_slam_amd.frame import DeviceSlots, FrameBuilder  # noqa: E402
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

ROWS, COLS, NFEATURES, N_LEVELS, SEED = 480, 752, 1000, 8, 500


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
    par, opt = A.TrackMotionParams(15.0, 30.0, 20, fps.fx), A.LMOptions.default()
    cols = C.c_int32(COLS)
    rec_bytes = C.sizeof(A.TrackFramesResult)

    # arm a
    fa_cur = keep(fb.build_device(*cur_img))  # the current frame's buffers; rebuilt in every call
    dl, dr = fa_cur._all[-2], fa_cur._all[-1]  # its device images
    a_cnt = np.zeros(2, np.int32)
    mask = np.concatenate([np.ones(n_last, np.uint8), np.zeros(n_last, np.uint8)])  # has_mp | mp_locked after UpdateFrame
    d_mask, a_pos = keep(ctx.empty(2 * n_last, np.uint8)), keep(ctx.empty((n_last, 3), np.float32))
    a_asg, a_rec = keep(ctx.empty(fb.capacity, np.int32)), keep(ctx.empty(rec_bytes, np.uint8))
    lf = A.LastFrameDev(n_last, Tp, d_mask.ptr.value, None, d_mask.ptr.value + n_last, a_pos.ptr, fa.left["desc"].ptr,
                        fa.left["octave"].ptr, fa.left["angle"].ptr)
    ka = fa_cur.keypoints(0)

    def arm_a():
        rc = L.lorb_frame_build_dev(fb._p, dl.ptr, cols, dr.ptr, cols, C.byref(fa_cur.out))
        rc |= L.lorb_memcpy_d2h(h, a_cnt.ctypes.data_as(C.c_void_p), fa_cur.counts.ptr, C.c_size_t(8))
        ka.n = int(a_cnt[0])
        rc |= L.lorb_memcpy_h2d(h, d_mask.ptr, mask.ctypes.data_as(C.c_void_p), C.c_size_t(2 * n_last))
        rc |= L.lorb_unproject_stereo_dev(h, C.byref(fps), Tp, C.c_int32(n_last), fa.left["x"].ptr, fa.left["y"].ptr,
                                          fa.depth.ptr, a_pos.ptr)
        rc |= L.lorb_track_motion_dev(h, C.byref(fps), Tp, pip, C.byref(ka), None, None, C.byref(lf), C.byref(par),
                                      C.byref(opt), a_asg.ptr, a_rec.ptr)
        return rc | L.lorb_sync(h)

    # arm b
    fb_cur = keep(fb.build_device(*cur_img))
    bl, br = fb_cur._all[-2], fb_cur._all[-1]
    bound = NFEATURES + NFEATURES // 4
    ls, cs = keep(DeviceSlots(ctx, bound, state=0)), keep(DeviceSlots(ctx, bound, state=0))
    b_asg, b_rec = keep(ctx.empty(bound, np.int32)), keep(ctx.empty(rec_bytes, np.uint8))
    nb = C.c_int32(bound)

    def arm_b():
        rc = L.lorb_frame_build_dev(fb._p, bl.ptr, cols, br.ptr, cols, C.byref(fb_cur.out))
        rc |= L.lorb_memset_dev(h, ls.state.ptr, C.c_int(0), C.c_size_t(bound))
        rc |= L.lorb_track_motion_frames_dev(h, C.byref(fps), Tp, pip, C.byref(fb_cur.out), nb, C.byref(cs.c), C.c_int32(0),
                                             Tp, C.byref(fa.out), nb, C.byref(ls.c), None, C.byref(par), C.byref(opt),
                                             b_asg.ptr, b_rec.ptr)
        return rc | L.lorb_sync(h)

    def verify():
        for f in (arm_a, arm_b):
            assert f() == 0, f.__name__
        ra = A.TrackMotionResult.from_buffer_copy(a_rec.numpy().tobytes())
        rb = A.TrackFramesResult.from_buffer_copy(b_rec.numpy().tobytes())
        n_cur = int(a_cnt[0])
        assert rb.status == 0 and (rb.n_last, rb.n_cur, rb.n_created) == (n_last, n_cur, n_last), (rb.status, rb.n_last, rb.n_cur)
        assert max(n_last, n_cur) <= bound
        rm = rb.motion  # the same kernels' bodies on the same data: the same bits
        assert ra.pass_ == 1 and (ra.pass_, ra.nmatches_first, ra.nmatches_retry, ra.n_residuals, ra.pose[:]) == \
            (rm.pass_, rm.nmatches_first, rm.nmatches_retry, rm.n_residuals, rm.pose[:])
        assert ra.summary.as_dict() == rm.summary.as_dict()
        assert np.array_equal(a_asg.numpy()[:n_cur], b_asg.numpy()[:n_cur])
        return dict(n_last=n_last, n_cur=n_cur, bound=bound, capacity=fb.capacity, nmatches_first=ra.nmatches_first,
                    n_residuals=ra.n_residuals, lm_iterations=ra.summary.iterations)

    def cleanup():
        for d in held:
            d.free()
        fb.close()

    return dict(a=arm_a, b=arm_b), verify, cleanup, (mask, pi, I, pat)


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
    rec = dict(tool="tools/bench_track_frames.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
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
