#!/usr/bin/env python3
"""Per-frame cost of the motion-model tracking chain (VisualOdometry::EstimatePoseMotion) on the GPU.

Three arms on the same frame pair, every one through prebuilt ctypes arguments (so the Python
marshalling of the Context methods is outside the timed region):
  a  today's sequence of host-array calls: lorb_search_by_projection_frame at 15, on a retry pair the
     same at 30 over emptied slots, then lorb_ba_pose_only on residuals gathered beforehand (the
     host-side gather between the calls is NOT timed: the arm is a lower bound of the old path)
  b  lorb_track_motion      (host arrays in, one staging, one fetch)
  c  lorb_track_motion_dev  (inputs resident on the device: enqueue, then one lorb_sync)
Pairs: C1 (synth.two_frames(seed=1): 500 keypoints, 200 shared; the first radius stands) and the
same frames with the prediction shifted by 0.7 along x (13 -> 69 matches: the retry).

Protocol: warm-up of every arm, then `--repeats` rounds; in every round each arm runs `--calls`
calls back to back (host clock around calls that each end in a device wait), the arms interleaved
inside the round.  Reported per arm: median and min / max over the rounds of the mean time per call.
Gate: b's median below a's median by more than a's own min-max spread, and c no slower than b
(c's median <= b's median + b's spread).

  python tools/bench_track_motion.py --out profiles/r07/track_motion.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_track_motion.py --only c --pair c1
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

import lorb_slam_amd.window  # noqa: E402,F401
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd import synth  # noqa: E402
from lorb_slam_amd.runtime import Context, lib  # noqa: E402
from lorb_slam_amd.window import _Staged  # noqa: E402

AA, T0 = [0.01, -0.005, 0.002], [0.05, 0.0, 0.02]


def build_arms(ctx, s, dx):
    """-> (dict arm -> zero-argument callable doing ONE tracked frame, reference result, keep-alive)."""
    L = lib()
    keep = A.KeepAlive()
    fps = A.make_frame_params(s["fp"])
    pi = keep.keep(np.array(AA + [T0[0] + dx, T0[1], T0[2]], np.float32))
    T = keep.keep(A.f32(synth.Tcw_from(AA, [T0[0] + dx, T0[1], T0[2]])).reshape(16))
    nk = len(s["cur_kps"]["x"])
    k, lf = A.make_keypoints(s["cur_kps"], keep), A.make_last_frame(s["last"], keep)
    par = A.TrackMotionParams(15.0, 30.0, 20, fps.fx)
    opt = A.LMOptions.default()
    h, p = ctx.handle, C.c_float

    ref = ctx.track_motion(s["fp"], T, pi, s["cur_kps"], None, None, s["last"], device_resident=False)
    retry = ref["pass_"] != 1

    # arm a: the residuals the old adapter gathers on the host between the calls, prepared once
    asg = ref["assign"]
    idx = np.nonzero(asg >= 0)[0]
    pb = dict(res_off=np.array([0, len(idx)], np.int32), intr=np.array([[fps.fx, fps.fx, fps.cx, fps.cy]], np.float32),
              pose_init=pi[None], pts3d=A.f32(s["last"]["mp_pos"][asg[idx]]),
              obs2d=A.f32(np.stack([s["cur_kps"]["x"][idx], s["cur_kps"]["y"][idx]], 1)))
    batch = A.make_pose_batch(pb, keep)
    zeros = keep.keep(np.zeros(nk, np.uint8))
    a_assign, a_nm = keep.keep(np.empty(nk + 1, np.int32)), C.c_int32(0)
    a_pose, a_sum = keep.keep(np.zeros(6)), A.BASummary()

    def arm_a():
        rc = L.lorb_search_by_projection_frame(h, C.byref(fps), A.ptr(T, p), C.byref(k), A.ptr(zeros, C.c_uint8),
                                               C.byref(lf), C.c_float(15.0), A.ptr(a_assign, C.c_int32), C.byref(a_nm))
        if retry:
            rc |= L.lorb_search_by_projection_frame(h, C.byref(fps), A.ptr(T, p), C.byref(k), A.ptr(zeros, C.c_uint8),
                                                    C.byref(lf), C.c_float(30.0), A.ptr(a_assign, C.c_int32),
                                                    C.byref(a_nm))
        rc |= L.lorb_ba_pose_only(h, C.byref(batch), C.byref(opt), A.ptr(a_pose, C.c_double), None, C.byref(a_sum))
        return rc

    b_assign, b_rec = keep.keep(np.empty(nk + 1, np.int32)), A.TrackMotionResult()

    def arm_b():
        return L.lorb_track_motion(h, C.byref(fps), A.ptr(T, p), A.ptr(pi, p), C.byref(k), None, None, C.byref(lf),
                                   C.byref(par), C.byref(opt), A.ptr(b_assign, C.c_int32), C.byref(b_rec), None)

    st = _Staged(ctx)
    dk, dlf = st.keypoints(s["cur_kps"]), st.last_frame(s["last"], keep)
    d_assign, d_rec = st.empty(nk + 1, np.int32), st.empty(C.sizeof(A.TrackMotionResult), np.uint8)

    def arm_c():
        rc = L.lorb_track_motion_dev(h, C.byref(fps), A.ptr(T, p), A.ptr(pi, p), C.byref(dk), None, None, C.byref(dlf),
                                     C.byref(par), C.byref(opt), d_assign.ptr, d_rec.ptr)
        return rc | L.lorb_sync(h)

    def verify():
        for f in (arm_a, arm_b, arm_c):
            assert f() == 0, f.__name__
        assert np.array_equal(a_assign[:nk], asg) and np.array_equal(b_assign[:nk], asg)
        assert np.array_equal(d_assign.numpy()[:nk], asg)
        rc_ = A.TrackMotionResult.from_buffer_copy(d_rec.numpy().tobytes())
        assert np.array_equal(np.array(b_rec.pose[:]), ref["pose"]) and np.array_equal(np.array(rc_.pose[:]), ref["pose"])
        # arm a solves the same residuals from the same start: the same pose up to the LM's own tolerance
        assert np.allclose(a_pose, ref["pose"], rtol=1e-5, atol=1e-5), (a_pose, ref["pose"])

    return dict(a=arm_a, b=arm_b, c=arm_c), ref, verify, (keep, st)


def time_calls(f, n):
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    return (time.perf_counter() - t0) / n * 1e6  # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--only", choices=["a", "b", "c"], help="run one arm only (for a profiler run)")
    ap.add_argument("--pair", choices=["c1", "retry"], help="run one pair only")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.calls >= 200 or args.only, "protocol: >= 5 repeats of >= 200 calls"

    ctx = Context(0)
    s = synth.two_frames(seed=1)
    pairs = {"c1": 0.0, "retry": 0.7}
    if args.pair:
        pairs = {args.pair: pairs[args.pair]}
    rec = dict(tool="tools/bench_track_motion.py", workload="synth.two_frames(seed=1): 500 keypoints, 200 shared",
               repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup, unit="us per tracked frame",
               pairs={})
    ok = True
    for name, dx in pairs.items():
        arms, ref, verify, keep = build_arms(ctx, s, dx)
        verify()
        names = [args.only] if args.only else ["a", "b", "c"]
        for a in names:
            time_calls(arms[a], args.warmup)
        samples = {a: [] for a in names}
        for _ in range(args.repeats):
            for a in names:  # interleaved: every round times every arm
                samples[a].append(time_calls(arms[a], args.calls))
        out = dict(dx=dx, pass_=ref["pass_"], nmatches_first=ref["nmatches_first"], nmatches_retry=ref["nmatches_retry"],
                   n_residuals=ref["n_residuals"], arms={})
        for a in names:
            v = samples[a]
            out["arms"][a] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
        if not args.only:
            A_, B_, C_ = (out["arms"][x] for x in "abc")
            spread_a, spread_b = A_["max"] - A_["min"], B_["max"] - B_["min"]
            out["gate"] = dict(b_below_a_by=A_["median"] - B_["median"], a_spread=spread_a,
                               b_faster_than_a=A_["median"] - B_["median"] > spread_a,
                               c_minus_b=C_["median"] - B_["median"], b_spread=spread_b,
                               c_no_slower_than_b=C_["median"] <= B_["median"] + spread_b,
                               target_50us_met_by_c=C_["median"] <= 50.0)
            ok = ok and out["gate"]["b_faster_than_a"] and out["gate"]["c_no_slower_than_b"]
        rec["pairs"][name] = out
        keep[1].close()
    if not args.only:
        rec["gate_holds"] = ok
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
