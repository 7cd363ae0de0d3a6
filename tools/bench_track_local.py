#!/usr/bin/env python3
"""Per-frame cost of the local-map tracking chain (VisualOdometry::EstimatePoseLocal after
UpdateLocalMap) on the GPU.

Three arms on the same frame, every one through prebuilt ctypes arguments (so the Python marshalling
of the Context methods is outside the timed region):
  a  today's sequence of host-array calls: lorb_track_local_map, then lorb_ba_pose_only on residuals
     gathered beforehand (the host-side gather between the calls is NOT timed: the arm is a lower
     bound of the old path)
  b  lorb_track_local      (host arrays in, one staging, one completion wait)
  c  lorb_track_local_dev  (inputs resident on the device: enqueue, then one lorb_sync)
Inputs: `live` (synth.local_map_problem(seed=31): 500 keypoints, 2000 local points: the candidate
kernel builds the grid in LDS and writes strided lists: 3 launches) and `large`
(synth.local_map_problem(seed=11): 2000 keypoints, 3000 points: grid launch, count / scan / write,
more than 512 residuals).

Protocol: warm-up of every arm, then `--repeats` rounds; in every round each arm runs `--calls`
calls back to back (host clock around calls that each end in a device wait), the arms interleaved
inside the round.  Reported per arm: median and min / max over the rounds of the mean time per call.
Gate, relative to arm a in the same run: b's median below a's median by more than a's own min-max
spread, and c's median not above b's.

  python tools/bench_track_local.py --out profiles/r08/track_local.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_track_local.py --only c --input live
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

AA, T0 = [0.01, -0.02, 0.005], [0.1, -0.05, 0.2]  # synth.local_map_problem's pose
INPUTS = {"live": dict(seed=31, n_kps=500, n_pts=2000, n_true=300),
          "large": dict(seed=11, n_kps=2000, n_pts=3000, n_true=1200)}


def slot_positions(s, seed):
    """The point each slot would hold: keypoint j back-projected at a depth of its own under the frame's pose."""
    fp, k, T = s["fp"], s["kps"], s["Tcw"].astype(np.float64)
    z = np.random.default_rng(seed + 100).uniform(2, 12, len(k["x"]))
    Xc = np.stack([(k["x"] - fp["cx"]) / fp["fx"] * z, (k["y"] - fp["cy"]) / fp["fy"] * z, z], 1)
    return ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def map_points(pts, conv):
    return A.MapPointsDev(len(pts["max_dist"]), conv(pts["pos"], np.float32), conv(pts["normal"], np.float32),
                          conv(pts["max_dist"], np.float32), conv(pts["min_dist"], np.float32),
                          conv(pts["desc"], np.uint8), conv(pts["locked"], np.uint8), conv(pts["is_bad"], np.uint8),
                          conv(pts["in_frame"], np.uint8))


def build_arms(ctx, s, slot_pos):
    """-> (dict arm -> zero-argument callable doing ONE tracked frame, reference result, verify, keep-alive)."""
    L = lib()
    keep = A.KeepAlive()
    fps = A.make_frame_params(s["fp"])
    pi = keep.keep(np.array(AA + T0, np.float32))
    T = keep.keep(A.f32(s["Tcw"]).reshape(16))
    kps, pts, ss = s["kps"], s["pts"], s["slot_state"]
    nk, npt = len(kps["x"]), len(pts["max_dist"])
    k = A.make_keypoints(kps, keep)
    m = map_points(pts, lambda a, dt: keep.keep(np.ascontiguousarray(a, dt)).ctypes.data)
    hss, hsp = keep.keep(A.u8(ss)), keep.keep(A.f32(slot_pos))
    par = A.TrackLocalParams(0.5, 1.0, 20, fps.fx)
    opt = A.LMOptions.default()
    h, p = ctx.handle, C.c_float

    ref = ctx.track_local(s["fp"], T, pi, kps, ss, slot_pos, pts, device_resident=False)
    assert ref["ok"] == 1, "the benchmark frames pass the gate"

    # arm a: the residuals the old adapter gathers on the host between the calls, prepared once
    asg = ref["assign"]
    idx = np.nonzero((asg >= 0) | ((asg == A.LORB_ASSIGN_UNCHANGED) & (ss != A.LORB_SLOT_EMPTY)))[0]
    X = np.where((asg[idx] >= 0)[:, None], pts["pos"][np.maximum(asg[idx], 0)], slot_pos[idx])
    pb = dict(res_off=np.array([0, len(idx)], np.int32), intr=np.array([[fps.fx, fps.fx, fps.cx, fps.cy]], np.float32),
              pose_init=pi[None], pts3d=A.f32(X), obs2d=A.f32(np.stack([kps["x"][idx], kps["y"][idx]], 1)))
    batch = A.make_pose_batch(pb, keep)
    a_iv, a_tr, a_lv = (keep.keep(np.zeros(npt, np.uint8)), keep.keep(np.zeros((4, npt), np.float32)),
                        keep.keep(np.zeros(npt, np.int32)))
    a_assign, a_nm = keep.keep(np.empty(nk + 1, np.int32)), C.c_int32(0)
    a_pose, a_sum = keep.keep(np.zeros(6)), A.BASummary()

    def arm_a():
        rc = L.lorb_track_local_map(h, C.byref(fps), A.ptr(T, p), C.byref(k), A.ptr(hss, C.c_uint8), C.byref(m),
                                    C.c_float(0.5), C.c_float(1.0), A.ptr(a_iv, C.c_uint8), A.ptr(a_tr, p),
                                    A.ptr(a_lv, C.c_int32), A.ptr(a_assign, C.c_int32), C.byref(a_nm))
        rc |= L.lorb_ba_pose_only(h, C.byref(batch), C.byref(opt), A.ptr(a_pose, C.c_double), None, C.byref(a_sum))
        return rc

    b_iv, b_tr, b_lv = (keep.keep(np.zeros(npt, np.uint8)), keep.keep(np.zeros((4, npt), np.float32)),
                        keep.keep(np.zeros(npt, np.int32)))
    b_assign, b_rec = keep.keep(np.empty(nk + 1, np.int32)), A.TrackLocalResult()

    def arm_b():
        return L.lorb_track_local(h, C.byref(fps), A.ptr(T, p), A.ptr(pi, p), C.byref(k), A.ptr(hss, C.c_uint8),
                                  A.ptr(hsp, p), C.byref(m), C.byref(par), C.byref(opt), A.ptr(b_iv, C.c_uint8),
                                  A.ptr(b_tr, p), A.ptr(b_lv, C.c_int32), A.ptr(b_assign, C.c_int32), C.byref(b_rec), None)

    st = _Staged(ctx)
    dk, dm = st.keypoints(kps), map_points(pts, st.dev)
    dss, dsp = st.dev(ss, np.uint8), st.dev(slot_pos, np.float32)
    d_iv, d_tr, d_lv = st.empty(npt, np.uint8), st.empty((4, npt), np.float32), st.empty(npt, np.int32)
    d_assign, d_rec = st.empty(nk + 1, np.int32), st.empty(C.sizeof(A.TrackLocalResult), np.uint8)

    def arm_c():
        rc = L.lorb_track_local_dev(h, C.byref(fps), A.ptr(T, p), A.ptr(pi, p), C.byref(dk), dss, dsp, C.byref(dm),
                                    C.byref(par), C.byref(opt), d_iv.ptr, d_tr.ptr, d_lv.ptr, d_assign.ptr, d_rec.ptr)
        return rc | L.lorb_sync(h)

    def verify():
        for f in (arm_a, arm_b, arm_c):
            assert f() == 0, f.__name__
        assert np.array_equal(a_assign[:nk], asg) and np.array_equal(b_assign[:nk], asg)
        assert np.array_equal(d_assign.numpy()[:nk], asg)
        assert a_nm.value == ref["nmatches"] and np.array_equal(a_iv, ref["in_view"]) and np.array_equal(b_iv, ref["in_view"])
        rc_ = A.TrackLocalResult.from_buffer_copy(d_rec.numpy().tobytes())
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
    ap.add_argument("--input", choices=list(INPUTS), help="run one input only")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.calls >= 200 or args.only, "protocol: >= 5 repeats of >= 200 calls"

    ctx = Context(0)
    inputs = {args.input: INPUTS[args.input]} if args.input else INPUTS
    rec = dict(tool="tools/bench_track_local.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
               unit="us per tracked frame", inputs={})
    ok = True
    for name, kw in inputs.items():
        s = synth.local_map_problem(**kw)
        arms, ref, verify, keep = build_arms(ctx, s, slot_positions(s, kw["seed"]))
        verify()
        names = [args.only] if args.only else ["a", "b", "c"]
        for a in names:
            time_calls(arms[a], args.warmup)
        samples = {a: [] for a in names}
        for _ in range(args.repeats):
            for a in names:  # interleaved: every round times every arm
                samples[a].append(time_calls(arms[a], args.calls))
        out = dict(workload="synth.local_map_problem(%s)" % ", ".join(f"{k}={v}" for k, v in kw.items()),
                   nmatches=ref["nmatches"], n_in_view=ref["n_in_view"], n_residuals=ref["n_residuals"],
                   iterations=ref["summary"]["iterations"], arms={})
        for a in names:
            v = samples[a]
            out["arms"][a] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
        if not args.only:
            A_, B_, C_ = (out["arms"][x] for x in "abc")
            spread_a = A_["max"] - A_["min"]
            out["gate"] = dict(b_below_a_by=A_["median"] - B_["median"], a_spread=spread_a,
                               b_faster_than_a=A_["median"] - B_["median"] > spread_a,
                               c_minus_b=C_["median"] - B_["median"], c_not_above_b=C_["median"] <= B_["median"])
            ok = ok and out["gate"]["b_faster_than_a"] and out["gate"]["c_not_above_b"]
        rec["inputs"][name] = out
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
