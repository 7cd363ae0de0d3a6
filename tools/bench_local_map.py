#!/usr/bin/env python3
"""Per-frame cost of one tracked frame whose local map is the reference's own (UpdateLocalMap,
src/visual_odometry.cpp:234-340, between the two tracking stages): "image pair in -> local-map pose and
global slot ids out", the last frame already built, INITIALIZE-filled and resident.

Two arms on the same two image pairs, every one through prebuilt ctypes arguments (so Python
marshalling is outside the timed region):
  a  the only route before lorb_local_map_update_dev: lorb_frame_build_dev,
     lorb_track_motion_frames_dev, lorb_sync, lorb_memcpy_d2h of the record, of assign and of the slot
     states, then a PRECOMPUTED local table (one block: its n_local rows), slot states and local ids
     uploaded (three lorb_memcpy_h2d) -- the host's UpdateLocalMap itself counts as zero, the floor of any
     host version -- lorb_track_local_frames_dev on that table, lorb_sync
  b  lorb_frame_build_dev, lorb_track_motion_frames_dev, lorb_local_map_update_dev,
     lorb_track_local_frames_dev on the object's table (max_local rows, the rest padding),
     lorb_local_map_ids_back_dev, lorb_sync
Input: synth.stereo_pair(500, 480, 752) as the last frame, the same scene 2 pixels further with other
pixel noise as the current one, 1000 features, 8 levels, bounds 1250, max_local 4096.  The store: 4500
points -- the last frame's initialised points first, the rest copies of them moved by a few centimetres
with random descriptors -- under 12 keyframes: kf0 is the resident last frame, kf k holds the points
[300 (k - 1), 300 (k - 1) + 600), kf5 is bad; observations are the slots' inverse, covisible lists are
ordered by shared points.

Protocol (tools/bench_track_frame.py's): warm-up of every arm, then `--repeats` rounds; in every round
each arm runs `--calls` calls back to back, the arms interleaved inside the round.  Reported per arm:
median and min / max over the rounds of the mean time per call.  Gate: b's median below a's median by
more than a's own min-max spread.

  python tools/bench_local_map.py --out profiles/r15/local_map.json
  rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_local_map.py --only b --repeats 1 --calls 20
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
from lorb_slam_amd.frame import (DeviceMapStore, DeviceSlots, FrameBuilder, LocalFramesOut, LocalMap, fill_slots,  # noqa: E402
                                 local_map_buffers, local_map_result, motion_record_addresses)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

ROWS, COLS, NFEATURES, N_LEVELS, SEED = 480, 752, 1000, 8, 500
BOUND = NFEATURES + NFEATURES // 4
MAX_LOCAL, N_KF, N_POINTS, KF_STEP, KF_WIDTH = 4096, 12, 4500, 300, 600
COLS_ = (("pos", np.float32, 3), ("normal", np.float32, 3), ("max_dist", np.float32, 1), ("min_dist", np.float32, 1),
         ("desc", np.uint8, 32), ("locked", np.uint8, 1), ("is_bad", np.uint8, 1))


def make_store(pts0, last_gid):
    """The store dict of DeviceMapStore around the last frame's points pts0 (global ids 0 .. npt - 1)."""
    rng = np.random.default_rng(11)
    npt, n = len(pts0["pos"]), N_POINTS
    src = rng.integers(0, npt, n - npt)
    jit = rng.normal(scale=0.03, size=(n - npt, 3)).astype(np.float32)
    cat = lambda k, extra: np.concatenate([pts0[k], extra])  # noqa: E731
    s = dict(pos=cat("pos", pts0["pos"][src] + jit), normal=cat("normal", pts0["normal"][src]),
             max_dist=cat("max_dist", pts0["max_dist"][src]), min_dist=cat("min_dist", pts0["min_dist"][src]),
             desc=cat("desc", rng.integers(0, 256, (n - npt, 32), dtype=np.uint8)),
             locked=cat("locked", np.ones(n - npt, np.uint8)), is_bad=np.zeros(n, np.uint8))
    kf_slots = [list(last_gid)] + [list(range(KF_STEP * (k - 1), KF_STEP * (k - 1) + KF_WIDTH)) for k in range(1, N_KF)]
    member = np.zeros((N_KF, n), bool)
    for k, sl in enumerate(kf_slots):
        member[k, [p for p in sl if p >= 0]] = True
    obs = [list(np.nonzero(member[:, p])[0]) for p in range(n)]
    shared = member.astype(np.int32) @ member.astype(np.int32).T
    cov = [[int(j) for j in np.argsort(-shared[k], kind="stable") if j != k and shared[k, j] > 0] for k in range(N_KF)]
    kf_bad = np.zeros(N_KF, np.uint8)
    kf_bad[5] = 1
    return s, obs, kf_bad, kf_slots, cov


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

    # the last frame's slots (INITIALIZE) and the store around its initialised points
    ls = keep(DeviceSlots(ctx, BOUND, state=0))
    fill_slots(ctx, fp, I.reshape(4, 4), fa, ls, A.LORB_SLOTS_INITIALIZE)
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

    def arm_buffers(n_table):
        f = keep(fb.build_device(*cur_img))  # the current frame's buffers; rebuilt in every call
        return dict(f=f, l=f._all[-2], r=f._all[-1], cs=keep(DeviceSlots(ctx, BOUND, state=0)),
                    masg=keep(ctx.empty(BOUND, np.int32)), mrec=keep(ctx.empty(mrec_bytes, np.uint8)),
                    out=keep(LocalFramesOut(ctx, n_table, BOUND)))

    def front(b):  # the part both arms share: the builder and the motion stage
        rc = L.lorb_frame_build_dev(fb._p, b["l"].ptr, cols, b["r"].ptr, cols, C.byref(b["f"].out))
        return rc | L.lorb_track_motion_frames_dev(h, C.byref(fps), Tp, pip, C.byref(b["f"].out), nb, C.byref(b["cs"].c),
                                                   C.c_int32(0), Tp, C.byref(fa.out), nb, C.byref(ls.c), None, C.byref(mpar),
                                                   C.byref(opt), b["masg"].ptr, b["mrec"].ptr)

    # arm b
    b = arm_buffers(MAX_LOCAL)
    b_gid, b_sid, b_urec = (keep(x) for x in local_map_buffers(ctx, BOUND))
    d_pose, d_status = (C.c_void_p(v) for v in motion_record_addresses(b["mrec"]))
    src = A.TrackLocalIdSource(b["masg"].ptr.value, b["mrec"].ptr.value, d_last_gid.ptr.value, BOUND, 0)
    d_ustatus = C.c_void_p(b_urec.ptr.value + A.LocalMapResult.status.offset)
    d_lstatus = C.c_void_p(b["out"].record.ptr.value + A.TrackLocalFramesResult.status.offset)

    def arm_b():
        o = b["out"]
        rc = front(b)
        rc |= L.lorb_local_map_update_dev(h, lmap._p, C.byref(store.c), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b_gid.ptr,
                                          b_sid.ptr, d_status, C.byref(src), b_urec.ptr)
        rc |= L.lorb_track_local_frames_dev(h, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b_sid.ptr, d_pose,
                                            d_ustatus, None, C.byref(lmap.c), C.byref(lpar), C.byref(opt), o.in_view.ptr,
                                            o.track.ptr, o.level.ptr, o.assign.ptr, o.record.ptr)
        rc |= L.lorb_local_map_ids_back_dev(h, lmap._p, C.byref(b["f"].out), nb, C.byref(b["cs"].c), b_sid.ptr, d_lstatus,
                                            b_gid.ptr)
        return rc | L.lorb_sync(h)

    # what arm a uploads is precomputed from one run of arm b's first three calls: the table's n_local
    # rows as ONE block, the slot states after step c and the local ids
    assert front(b) == 0 and L.lorb_local_map_update_dev(h, lmap._p, C.byref(store.c), C.byref(b["f"].out), nb,
                                                          C.byref(b["cs"].c), b_gid.ptr, b_sid.ptr, d_status, C.byref(src),
                                                          b_urec.ptr) == 0
    u = local_map_result(b_urec)
    assert u.status == 0, u.status
    nloc = u.n_local
    t = lmap.numpy()
    parts, off, total = [], {}, 0
    for k, dt, w in COLS_:
        a_ = np.ascontiguousarray(t[k][:nloc]).view(np.uint8).reshape(-1)
        off[k] = total
        parts.append(a_)
        pad = (-len(a_)) % 256
        parts.append(np.zeros(pad, np.uint8))
        total += len(a_) + pad
    h_table = np.concatenate(parts)
    h_state, h_sid = b["cs"].state.numpy()[:BOUND].copy(), b_sid.numpy()[:BOUND].copy()
    d_table = keep(ctx.empty(max(total, 16), np.uint8))
    tb = d_table.ptr.value
    a_pts = A.MapPointsDev(nloc, *(tb + off[k] for k, _, _ in COLS_), None)

    a = arm_buffers(max(nloc, 1))
    a_mrec, a_masg, a_st = np.zeros(mrec_bytes, np.uint8), np.zeros(BOUND, np.int32), np.zeros(BOUND, np.uint8)
    a_sid = keep(ctx.empty(BOUND, np.int32))
    a_pose, a_status = (C.c_void_p(v) for v in motion_record_addresses(a["mrec"]))

    def arm_a():
        o = a["out"]
        rc = front(a) | L.lorb_sync(h)
        rc |= L.lorb_memcpy_d2h(h, a_mrec.ctypes.data_as(C.c_void_p), a["mrec"].ptr, C.c_size_t(mrec_bytes))
        rc |= L.lorb_memcpy_d2h(h, a_masg.ctypes.data_as(C.c_void_p), a["masg"].ptr, C.c_size_t(4 * BOUND))
        rc |= L.lorb_memcpy_d2h(h, a_st.ctypes.data_as(C.c_void_p), a["cs"].state.ptr, C.c_size_t(BOUND))
        # (the host's UpdateLocalMap would run here: counted as zero)
        rc |= L.lorb_memcpy_h2d(h, d_table.ptr, h_table.ctypes.data_as(C.c_void_p), C.c_size_t(h_table.nbytes))
        rc |= L.lorb_memcpy_h2d(h, a["cs"].state.ptr, h_state.ctypes.data_as(C.c_void_p), C.c_size_t(BOUND))
        rc |= L.lorb_memcpy_h2d(h, a_sid.ptr, h_sid.ctypes.data_as(C.c_void_p), C.c_size_t(4 * BOUND))
        rc |= L.lorb_track_local_frames_dev(h, C.byref(fps), C.byref(a["f"].out), nb, C.byref(a["cs"].c), a_sid.ptr, a_pose,
                                            a_status, None, C.byref(a_pts), C.byref(lpar), C.byref(opt), o.in_view.ptr,
                                            o.track.ptr, o.level.ptr, o.assign.ptr, o.record.ptr)
        return rc | L.lorb_sync(h)

    def verify():
        for f in (arm_a, arm_b):
            assert f() == 0, f.__name__
        ra, rb = a["out"].result(), b["out"].result()
        ub = local_map_result(b_urec)
        mb = A.TrackFramesResult.from_buffer_copy(b["mrec"].numpy().tobytes())
        n_cur = rb.n_cur
        assert ra.status == 0 and rb.status == 0 and ub.status == 0 and mb.status == 0 and ub.n_local == nloc
        fa_, fb_ = ((r.local.ok, r.local.nmatches, r.local.n_in_view, r.local.n_residuals) for r in (ra, rb))
        assert fa_ == fb_ and ra.local.pose[:] == rb.local.pose[:], (fa_, fb_)
        assert np.array_equal(a["out"].assign.numpy()[:n_cur], b["out"].assign.numpy()[:n_cur])
        assert np.array_equal(a_sid.numpy()[:n_cur], b_sid.numpy()[:n_cur])
        return dict(n_last=n_last, n_cur=n_cur, bound=BOUND, max_local=MAX_LOCAL, store_points=N_POINTS, store_keyframes=N_KF,
                    n_held=ub.n_held, n_nulled=ub.n_nulled, n_voted=ub.n_voted, n_local_kf=ub.n_local_kf, refer_kf=ub.refer_kf,
                    n_local=ub.n_local, arm_a_table_rows=nloc, arm_a_upload_bytes=int(h_table.nbytes + 5 * BOUND),
                    motion_nmatches=mb.motion.nmatches_first, local_ok=rb.local.ok, local_nmatches=rb.local.nmatches,
                    local_n_in_view=rb.local.n_in_view, local_n_residuals=rb.local.n_residuals,
                    lm_iterations=rb.local.summary.iterations)

    def cleanup():
        for x in held:
            x.free()
        fb.close()

    return dict(a=arm_a, b=arm_b), verify, cleanup, (pi, I, pat, h_table, h_state, h_sid, a_mrec, a_masg, a_st, src, a_pts)


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
    rec = dict(tool="tools/bench_local_map.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
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
