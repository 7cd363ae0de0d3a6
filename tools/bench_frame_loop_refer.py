#!/usr/bin/env python3
"""Per-frame cost of having the second motion attempt (VisualOdometry::Run, src/visual_odometry.cpp:50-54) in the
frame loop: lorb_track_motion_refer_pose_dev enqueued behind every frame's motion stage and skipped on the device,
against the two loops there were before it.

Sizes, images, the store and the frame dependency are tools/bench_frame_loop.py's (480 x 752, 1000 features, 8 levels,
bounds 1250, max_local 4096, 4500 points under 12 keyframes; the last frame built once, INITIALIZE-filled and resident
at the identity; frame k + 1 predicts with the mTcc frame k left).  The first attempt passes in every frame, so the
second is never due: what is measured is the price of asking.  The refer frame is the last frame (mReferFrame ==
mPrevFrame after Initialize) with a slot set of its own.  Every call goes through prebuilt ctypes arguments.

  a  the only way to the second attempt before this call, per frame: lorb_frame_build_dev,
     lorb_track_motion_frames_pose_dev, lorb_memcpy_d2h of the motion record (the frame's wait: the host looks at
     status and motion.pass and would issue the pose form on the refer frame), lorb_local_map_update_dev,
     lorb_track_local_frames_dev, lorb_local_map_ids_back_dev, lorb_frame_pose_finish_dev; one lorb_sync after the round.
  b  the six-call loop with no wait (tools/bench_frame_loop.py's arm b): the second attempt is never made.
  c  seven calls, no wait: b with lorb_track_motion_refer_pose_dev behind the motion stage (gids and guard given, so
     lorb_local_map_update_dev gets ids = NULL); one lorb_sync after the round.

Protocol (tools/bench_frame_loop.py's): warm-up of every arm, then `--repeats` rounds; in every round each arm runs
`--calls` frames, the arms interleaved inside the round; every round starts from mTcc = I and ends with a check that
its last frame's status is 0 (outside the timed region).  Reported per arm: median and min / max over the rounds of
the mean time per frame, and whether c's median is below a's by more than a's own min-max spread.

  python tools/bench_frame_loop_refer.py --out profiles/r17/frame_loop_refer.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_frame_loop_refer.py --only c --repeats 1 --calls 20
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
from lorb_slam_amd.frame import (DeviceBlock, DeviceMapStore, DeviceSlots, FrameBuilder, LocalFramesOut, LocalMap,  # noqa: E402
                                 fill_slots, local_map_buffers, local_map_result, model_block, motion_record_addresses,
                                 pose_block, refer_kf_word)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

REFER_KF = 0


def build_arms(ctx):
    L, h = lib(), ctx.handle
    fp = synth.frame_params(width=COLS, height=ROWS)
    fps = A.make_frame_params(fp)
    nd = features_per_level(NFEATURES)
    pat = np.random.default_rng(7).integers(-13, 13, size=1024).astype(np.int32)
    fb = FrameBuilder(ctx, fp, ROWS, COLS, nd, pat)
    last_img = synth.stereo_pair(SEED, ROWS, COLS)
    cur_img = synth.stereo_pair(SEED, ROWS, COLS, shift=2, noise_seed=777)
    fa = fb.build_device(*last_img)  # the last frame, which is also the refer frame: built once, resident
    n_last = int(fa.read_counts()[0])
    held = [fa]

    def keep(d):
        held.append(d)
        return d

    I4 = np.eye(4, dtype=np.float32)
    mpar, lpar, opt = A.TrackMotionParams(15.0, 30.0, 20, fps.fx), A.TrackLocalParams(0.5, 1.0, 20, fps.fx), A.LMOptions.default()
    cols, nb = C.c_int32(COLS), C.c_int32(BOUND)
    mrec_bytes = C.sizeof(A.TrackFramesResult)

    # the last frame's slots (INITIALIZE), the refer frame's own set, the store around the initialised points, the local map
    ls, rs = keep(DeviceSlots(ctx, BOUND, state=0)), keep(DeviceSlots(ctx, BOUND, state=0))
    fill_slots(ctx, fp, I4, fa, ls, A.LORB_SLOTS_INITIALIZE)
    fill_slots(ctx, fp, I4, fa, rs, A.LORB_SLOTS_INITIALIZE)
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
    last_pose, refer_pose = keep(pose_block(ctx, I4)), keep(pose_block(ctx, I4))
    model_I = A.MotionModel()
    model_I.Tcc[:] = [float(v) for v in I4.reshape(16)]

    def arm_buffers():
        f = keep(fb.build_device(*cur_img))  # the current frame's buffers; rebuilt in every frame
        b = dict(f=f, l=f._all[-2], r=f._all[-1], cs=keep(DeviceSlots(ctx, BOUND, state=0)),
                 masg=keep(ctx.empty(BOUND, np.int32)),
                 mrec=keep(ctx.to_device(np.zeros(mrec_bytes, np.uint8))),  # zeroed: verify() compares its bytes, padding too
                 out=keep(LocalFramesOut(ctx, MAX_LOCAL, BOUND)), pose=keep(pose_block(ctx, I4)), model=keep(model_block(ctx, I4)),
                 rrec=keep(DeviceBlock(ctx, A.TrackReferResult)), kf=keep(refer_kf_word(ctx, REFER_KF)))
        b["gid"], b["sid"], b["urec"] = (keep(x) for x in local_map_buffers(ctx, BOUND))
        b["d_pose"], b["d_status"] = (C.c_void_p(v) for v in motion_record_addresses(b["mrec"]))
        b["src"] = A.TrackLocalIdSource(b["masg"].ptr.value, b["mrec"].ptr.value, d_last_gid.ptr.value, BOUND, 0)
        b["d_ustatus"] = C.c_void_p(b["urec"].ptr.value + A.LocalMapResult.status.offset)
        b["d_lstatus"] = C.c_void_p(b["out"].record.ptr.value + A.TrackLocalFramesResult.status.offset)
        b["host_mrec"] = A.TrackFramesResult()
        return b

    def frame(b, mode):
        """One frame of arm `mode`."""
        o = b["out"]
        rc = L.lorb_frame_build_dev(fb._p, b["l"].ptr, cols, b["r"].ptr, cols, C.byref(b["f"].out))
        rc |= L.lorb_track_motion_frames_pose_dev(h, C.byref(fps), b["pose"].ptr, C.byref(b["f"].out), nb, C.byref(b["cs"].c),
                                                  C.c_int32(0), last_pose.ptr, b["model"].ptr, C.byref(fa.out), nb, C.byref(ls.c),
                                                  None, C.byref(mpar), C.byref(opt), b["masg"].ptr, b["mrec"].ptr)
        ids = C.byref(b["src"])
        if mode == "a":  # the frame's wait: the host reads the motion record and decides
            rc |= L.lorb_memcpy_d2h(h, C.byref(b["host_mrec"]), b["mrec"].ptr, C.c_size_t(mrec_bytes))
            assert b["host_mrec"].status != 0 or b["host_mrec"].motion.pass_ != 0, "the bench scene never needs the second attempt"
        elif mode == "c":
            rc |= L.lorb_track_motion_refer_pose_dev(
                h, C.byref(fps), b["pose"].ptr, C.byref(b["f"].out), nb, C.byref(b["cs"].c), C.c_int32(0), refer_pose.ptr,
                b["model"].ptr, C.byref(fa.out), nb, C.byref(rs.c), None, d_last_gid.ptr, nb, d_last_gid.ptr, b["gid"].ptr,
                C.c_int32(REFER_KF), b["kf"].ptr, b["urec"].ptr, C.byref(mpar), C.byref(opt), b["masg"].ptr, b["mrec"].ptr,
                b["rrec"].ptr)
            ids = None  # the gids are in place
        rc |= L.lorb_local_map_update_dev(h, lmap._p, C.byref(store.c), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["gid"].ptr,
                                          b["sid"].ptr, b["d_status"], ids, b["urec"].ptr)
        rc |= L.lorb_track_local_frames_dev(h, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["sid"].ptr, b["d_pose"],
                                            b["d_ustatus"], None, C.byref(lmap.c), C.byref(lpar), C.byref(opt), o.in_view.ptr,
                                            o.track.ptr, o.level.ptr, o.assign.ptr, o.record.ptr)
        rc |= L.lorb_local_map_ids_back_dev(h, lmap._p, C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["sid"].ptr,
                                            b["d_lstatus"], b["gid"].ptr)
        return rc | L.lorb_frame_pose_finish_dev(h, o.record.ptr, last_pose.ptr, b["pose"].ptr, b["model"].ptr)

    bufs = {m: arm_buffers() for m in "abc"}

    def make_round(mode):
        b = bufs[mode]

        def run(n):
            b["model"].upload(model_I)
            t0 = time.perf_counter()
            rc = 0
            for _ in range(n):
                rc |= frame(b, mode)
            rc |= L.lorb_sync(h)  # the round's one wait (arm a: behind its per-frame waits)
            dt = time.perf_counter() - t0
            st = b["out"].result().status
            assert rc == 0 and st == 0, (rc, st)
            return dt / n * 1e6
        return run

    arms = {m: make_round(m) for m in "abc"}

    def verify():
        """The first two frames of a round in every arm: the same codes, counts, pose, gids and blocks, bit for bit
        (the three arms run the same device arithmetic); arm c's refer record says not due."""
        out = {}
        arms["b"](1)  # the first call on the resident last frame creates its points (n_created); every later one finds them
        for n in (1, 2):
            got = {}
            for m in "abc":
                arms[m](n)
                b = bufs[m]
                n_cur = b["out"].result().n_cur
                got[m] = dict(mrec=b["mrec"].numpy(), masg=b["masg"].numpy()[:n_cur], lrec=b["out"].record.numpy(),
                              assign=b["out"].assign.numpy()[:n_cur], gid=b["gid"].numpy()[:n_cur], sid=b["sid"].numpy()[:n_cur],
                              pose=b["pose"].numpy(), model=b["model"].numpy(), urec=b["urec"].numpy())
            for m in "ac":
                for k, v in got["b"].items():
                    assert v.tobytes() == got[m][k].tobytes(), (n, m, k)
            rr = bufs["c"]["rrec"].read()
            mb = A.TrackFramesResult.from_buffer_copy(got["b"]["mrec"].tobytes())
            assert (rr.due, rr.ran, rr.stale) == (0, 0, 0) and mb.status == 0 and mb.motion.pass_ == 1
            assert (rr.first_nmatches_first, rr.first_nmatches_retry) == (mb.motion.nmatches_first, mb.motion.nmatches_retry)
            rb, ub = bufs["b"]["out"].result(), local_map_result(bufs["b"]["urec"])
            assert rb.status == 0 and ub.status == 0
            if n == 2 and ub.refer_kf >= 0:  # the word follows the previous frame's UpdateLocalMap
                assert bufs["c"]["kf"].read().value == ub.refer_kf
            out[f"frame{n}"] = dict(motion_nmatches=mb.motion.nmatches_first, local_ok=rb.local.ok, local_nmatches=rb.local.nmatches,
                                    local_n_in_view=rb.local.n_in_view, local_n_residuals=rb.local.n_residuals,
                                    lm_iterations=rb.local.summary.iterations, n_local=ub.n_local, refer_kf=ub.refer_kf)
        return dict(n_last=n_last, n_cur=n_cur, bound=BOUND, max_local=MAX_LOCAL, store_points=N_POINTS, store_keyframes=N_KF, **out)

    def cleanup():
        for x in held:
            x.free()
        fb.close()

    return arms, verify, cleanup, (pat, model_I)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--only", choices=["a", "b", "c"], help="run one arm only (for a profiler run)")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.calls >= 100 or args.only, "protocol: >= 5 repeats of >= 100 calls"

    ctx = Context(0)
    arms, verify, cleanup, keep = build_arms(ctx)
    info = verify()
    names = [args.only] if args.only else ["a", "b", "c"]
    for a in names:
        arms[a](args.warmup)
    samples = {a: [] for a in names}
    for _ in range(args.repeats):
        for a in names:  # interleaved: every round times every arm
            samples[a].append(arms[a](args.calls))
    rec = dict(tool="tools/bench_frame_loop_refer.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
               unit="us per frame",
               workload="synth.stereo_pair(%d, %d, %d) -> the same, shift 2, noise seed 777; %d features, %d levels" %
               (SEED, ROWS, COLS, NFEATURES, N_LEVELS), **info, arms={})
    for a in names:
        v = samples[a]
        rec["arms"][a] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    if not args.only:
        A_, B_, C_ = (rec["arms"][m] for m in "abc")
        spread_a = A_["max"] - A_["min"]
        rec["comparison"] = dict(c_minus_b=C_["median"] - B_["median"], a_minus_b=A_["median"] - B_["median"],
                                 c_below_a_by=A_["median"] - C_["median"], a_spread=spread_a,
                                 c_below_a_by_more_than_a_spread=A_["median"] - C_["median"] > spread_a)
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
