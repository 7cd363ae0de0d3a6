#!/usr/bin/env python3
"""Per-frame cost of the stereo Frame constructor (Frame::Frame(imgLeft, imgRight, camera),
src/frame.cpp:17-63: ORB extraction of both images + ComputeStereoMatches) on the GPU.

Three arms on the same image pair, every one through prebuilt ctypes arguments (so Python marshalling
is outside the timed region):
  a  today's sequence with everything resident on the device: lorb_orb_extract_dev left, then right,
     lorb_memcpy_d2h of the two counts, lorb_compute_stereo_matches_dev, lorb_sync
  b  lorb_frame_build_dev + lorb_sync (images and outputs resident)
  c  lorb_frame_build (host arrays in and out: one staging, one fetch, one wait)
Inputs: synth.stereo_pair(500, 480, 752) with 1000 features and synth.stereo_pair(508, 376, 1241)
with 2000 features, 8 levels each.

Protocol: warm-up of every arm, then `--repeats` rounds; in every round each arm runs `--calls` calls
back to back (host clock around calls that each end in a device wait), the arms interleaved inside
the round.  Reported per arm: median and min / max over the rounds of the mean time per call.
Gate, relative to arm a in the same run: b's median below a's median by more than a's own min-max
spread.

  python tools/bench_frame.py --out profiles/r09/frame.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_frame.py --only b --input 752x480
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
from lorb_slam_amd.frame import SIDE_KEYS, FrameBuilder  # noqa: E402
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

INPUTS = {"752x480": dict(seed=500, rows=480, cols=752, nfeatures=1000),
          "1241x376": dict(seed=508, rows=376, cols=1241, nfeatures=2000)}
N_LEVELS = 8
DT = dict(x=np.float32, y=np.float32, octave=np.int32, size=np.float32, angle=np.float32, response=np.float32)


def features_per_level(nfeatures, scale=1.2, n_levels=N_LEVELS):
    """ORBextractor::ORBextractor, src/ORBextractor.cpp:448-461 (float arithmetic as the reference)."""
    f32 = np.float32
    factor = f32(1.0) / f32(scale)
    per = f32(f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(np.power(np.float64(factor), np.float64(n_levels)))))
    out, s = [], 0
    for _ in range(n_levels - 1):
        v = int(np.rint(per))
        out.append(v)
        s += v
        per = f32(per * factor)
    out.append(max(nfeatures - s, 0))
    return np.array(out, np.int32)


def build_arms(ctx, kw):
    """-> (dict arm -> zero-argument callable doing ONE frame, reference result, verify, cleanup)."""
    L, h = lib(), ctx.handle
    rows, cols = kw["rows"], kw["cols"]
    left, right = synth.stereo_pair(kw["seed"], rows, cols)
    fp = synth.frame_params(width=cols, height=rows)
    fps = A.make_frame_params(fp)
    sf, nd = synth.scale_factors(N_LEVELS), features_per_level(kw["nfeatures"])
    pat = np.random.default_rng(7).integers(-13, 13, size=1024).astype(np.int32)
    fb = FrameBuilder(ctx, fp, rows, cols, nd, pat)
    ref = fb.build(left, right)
    cap, pb = fb.capacity, fb.pyramid_bytes
    held = []

    def dev(a):
        d = ctx.to_device(a)
        held.append(d)
        return d

    def empty(n, dt):
        d = ctx.empty(n, dt)
        held.append(d)
        return d

    dl, dr, dpat = dev(left), dev(right), dev(pat)

    def side():
        s = {k: empty(cap, dt) for k, dt in DT.items()}
        s.update(desc=empty(cap * 32, np.uint8), level_off=empty(N_LEVELS + 1, np.int32), pyramid=empty(pb, np.uint8))
        return s

    # arm a: today's calls
    aL, aR = side(), side()
    a_n = empty(2, np.int32)
    a_ur, a_dp = empty(cap, np.float32), empty(cap, np.float32)
    a_cnt = np.zeros(2, np.int32)
    sfp, ndp = A.ptr(sf, C.c_float), A.ptr(nd, C.c_int32)
    pyrL, pyrR = A.ImagePyramid(), A.ImagePyramid()
    for P, s in ((pyrL, aL), (pyrR, aR)):
        P.n_levels, off = N_LEVELS, 0
        for l in range(N_LEVELS):
            inv = np.float32(1) / sf[l]
            r, c = int(np.rint(np.float32(rows) * inv)), int(np.rint(np.float32(cols) * inv))
            P.offset[l], P.rows[l], P.cols[l], P.step[l] = off, r, c, c
            off += r * c
        P.data = s["pyramid"].ptr.value

    def extract(img, s, dn):
        return L.lorb_orb_extract_dev(h, img.ptr, C.c_int32(rows), C.c_int32(cols), C.c_int32(cols), C.c_int32(N_LEVELS),
                                      sfp, ndp, C.c_int32(20), C.c_int32(7), dpat.ptr, C.c_int32(cap), s["pyramid"].ptr,
                                      C.c_int64(pb), s["x"].ptr, s["y"].ptr, s["octave"].ptr, s["size"].ptr,
                                      s["angle"].ptr, s["response"].ptr, s["desc"].ptr, s["level_off"].ptr, dn)

    dn0, dn1 = C.c_void_p(a_n.ptr.value), C.c_void_p(a_n.ptr.value + 4)
    kL = A.StereoKeys(0, aL["x"].ptr.value, aL["y"].ptr.value, aL["octave"].ptr.value, aL["desc"].ptr.value)
    kR = A.StereoKeys(0, aR["x"].ptr.value, aR["y"].ptr.value, aR["octave"].ptr.value, aR["desc"].ptr.value)

    def arm_a():
        rc = extract(dl, aL, dn0) | extract(dr, aR, dn1)
        rc |= L.lorb_memcpy_d2h(h, a_cnt.ctypes.data_as(C.c_void_p), a_n.ptr, C.c_size_t(8))
        kL.n, kR.n = int(a_cnt[0]), int(a_cnt[1])
        rc |= L.lorb_compute_stereo_matches_dev(h, C.byref(fps), C.byref(kL), C.byref(kR), C.byref(pyrL), C.byref(pyrR),
                                                a_ur.ptr, a_dp.ptr)
        return rc | L.lorb_sync(h)

    # arm b: the builder, resident
    bL, bR = side(), side()
    b_ur, b_dp, b_cnt = empty(cap, np.float32), empty(cap, np.float32), empty(2, np.int32)
    bout = A.FrameOut()
    for s, d in ((bout.left, bL), (bout.right, bR)):
        for k in (*SIDE_KEYS, "level_off", "pyramid"):
            setattr(s, k, d[k].ptr.value)
    bout.u_right, bout.depth, bout.counts = b_ur.ptr.value, b_dp.ptr.value, b_cnt.ptr.value

    def arm_b():
        rc = L.lorb_frame_build_dev(fb._p, dl.ptr, C.c_int32(cols), dr.ptr, C.c_int32(cols), C.byref(bout))
        return rc | L.lorb_sync(h)

    # arm c: host arrays
    cout, chost = A.FrameOut(), {}
    for name, s in (("left", cout.left), ("right", cout.right)):
        hs = {k: np.zeros(cap, dt) for k, dt in DT.items()}
        hs.update(desc=np.zeros((cap, 32), np.uint8), level_off=np.zeros(N_LEVELS + 1, np.int32))
        for k, a in hs.items():
            setattr(s, k, a.ctypes.data)
        chost[name] = hs
    c_ur, c_dp, c_cnt = np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros(2, np.int32)
    cout.u_right, cout.depth, cout.counts = c_ur.ctypes.data, c_dp.ctypes.data, c_cnt.ctypes.data
    lp, rp = left.ctypes.data_as(A.u8p), right.ctypes.data_as(A.u8p)

    def arm_c():
        return L.lorb_frame_build(fb._p, lp, C.c_int32(cols), rp, C.c_int32(cols), C.c_int32(cap), C.byref(cout))

    def verify():
        for f in (arm_a, arm_b, arm_c):
            assert f() == 0, f.__name__
        nl, nr = (int(v) for v in ref["counts"])
        assert nl > 0 and nr > 0 and (ref["depth"] > 0).sum() > 100
        assert list(a_cnt) == [nl, nr] and list(b_cnt.numpy()) == [nl, nr] and list(c_cnt) == [nl, nr]
        for name, n, sa, sb in (("left", nl, aL, bL), ("right", nr, aR, bR)):
            for k in SIDE_KEYS:
                want = ref[name][k].reshape(-1)
                w = 32 if k == "desc" else 1
                assert np.array_equal(sa[k].numpy()[:n * w], want), ("a", name, k)
                assert np.array_equal(sb[k].numpy()[:n * w], want), ("b", name, k)
                assert np.array_equal(chost[name][k].reshape(-1)[:n * w], want), ("c", name, k)
        for ur, dp in ((a_ur.numpy(), a_dp.numpy()), (b_ur.numpy(), b_dp.numpy()), (c_ur, c_dp)):
            assert np.array_equal(ur[:nl], ref["u_right"]) and np.array_equal(dp[:nl], ref["depth"])

    def cleanup():
        for d in held:
            d.free()
        fb.close()

    return dict(a=arm_a, b=arm_b, c=arm_c), ref, verify, cleanup, (left, right, pat, chost)


def time_calls(f, n):
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    return (time.perf_counter() - t0) / n * 1e6  # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--only", choices=["a", "b", "c"], help="run one arm only (for a profiler run)")
    ap.add_argument("--input", choices=list(INPUTS), help="run one input only")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.calls >= 100 or args.only, "protocol: >= 5 repeats of >= 100 calls"

    ctx = Context(0)
    inputs = {args.input: INPUTS[args.input]} if args.input else INPUTS
    rec = dict(tool="tools/bench_frame.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
               unit="us per frame", inputs={})
    ok = True
    for name, kw in inputs.items():
        arms, ref, verify, cleanup, keep = build_arms(ctx, kw)
        verify()
        names = [args.only] if args.only else ["a", "b", "c"]
        for a in names:
            time_calls(arms[a], args.warmup)
        samples = {a: [] for a in names}
        for _ in range(args.repeats):
            for a in names:  # interleaved: every round times every arm
                samples[a].append(time_calls(arms[a], args.calls))
        out = dict(workload="synth.stereo_pair(%d, %d, %d), %d features, %d levels" %
                   (kw["seed"], kw["rows"], kw["cols"], kw["nfeatures"], N_LEVELS),
                   n_left=int(ref["counts"][0]), n_right=int(ref["counts"][1]), depths=int((ref["depth"] > 0).sum()),
                   arms={})
        for a in names:
            v = samples[a]
            out["arms"][a] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
        if not args.only:
            A_, B_ = out["arms"]["a"], out["arms"]["b"]
            spread_a = A_["max"] - A_["min"]
            out["gate"] = dict(b_below_a_by=A_["median"] - B_["median"], a_spread=spread_a,
                               b_faster_than_a=A_["median"] - B_["median"] > spread_a)
            ok = ok and out["gate"]["b_faster_than_a"]
        rec["inputs"][name] = out
        cleanup()
    if not args.only:
        rec["gate_holds"] = ok
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
