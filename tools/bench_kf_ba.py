#!/usr/bin/env python3
"""What the local bundle adjustment on the keyframe store costs: lorb_kf_store_local_ba_dev behind a forced
insertion against the same window solved by lorb_ba_solver_solve from host arrays.

Scene, sizes and protocol are tools/bench_kf_insert.py's (480 x 752, 1000 features, 8 levels, bounds 1250, 4500
points under 12 keyframes, one of them bad).  The KeyframeStore starts from that store WITH geometry: every initial
keyframe at the identity perturbed by N(0, 1e-3) rad / N(0, 1e-2) m, every slot's keypoint the projection of its
point at the identity plus 0.5 px noise.  Every repetition of every arm starts from the same store state: the store
with the tracked frame (one frame of the seven-call loop) inserted as keyframe 12, made outside the timed region.

  a        ONE store for all repetitions, as a caller has: the forced insertion (LORB_KF_GATE_NONE) is made once,
           untimed; a repetition puts the kf_pose and pos rows back to what the insertion left (untimed), then times
           lorb_kf_store_local_ba_dev and the lorb_sync behind it.  The plan of this camera count is resident.
  a_new    a NEW store per repetition: lorb_kf_store_insert_dev and lorb_kf_store_local_ba_dev on the record's kf and
           status words, enqueued back to back, and the lorb_sync behind them, timed together.  The store owns its
           plans, so this is a store's FIRST local BA: it creates the plan and captures its LM graph.
  a_new_ba the same with the insertion waited for first: the first local BA and its lorb_sync alone.
  a_gather lorb_kf_store_ba_gather_dev alone (it ends with its own wait) on a new store, after a waited insertion.
  b        the window arm a solves, read to the host beforehand (lorb_kf_ba_window_read, untimed), through
           lorb_ba_solver_solve on one solver: what a caller of the parent commit runs once a window is on the host.
           It leaves out the store read and the host gather, so it favours the parent.
  --trace-run: warm-up and `--repeats` rounds of arm a only, for a kernel-trace run of its own
           (rocprofv3 --kernel-trace --stats -- python tools/bench_kf_ba.py --trace-run): the k_kfba_* and
           k_db_result_rows kernels' summed time beside the solve's.

Protocol: warm-up of every arm, then `--repeats` rounds with the arms interleaved inside the round; median and
min / max over the rounds.

  python tools/bench_kf_ba.py --out profiles/r20/kf_ba.json
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

import bench_kf_insert as KI  # noqa: E402
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd.frame import KeyframeStore, keyframe_ba_record, keyframe_ba_result, keyframe_local_ba  # noqa: E402
from lorb_slam_amd.runtime import BASolver, Context, lib  # noqa: E402


def geometry(init, fp):
    """The initial keyframes' geometry: the invariant by construction (the lowest slot that holds the point)."""
    rng = np.random.default_rng(23)
    nk = len(init["kf_bad"])
    pose = np.concatenate([rng.normal(0, 1e-3, (nk, 3)), rng.normal(0, 1e-2, (nk, 3))], 1).astype(np.float32)
    pos = np.asarray(init["pos"], np.float64)
    fx, fy, cx, cy = (float(fp[k]) for k in ("fx", "fy", "cx", "cy"))
    uv, where = [], []
    for row in init["kf_slots"]:
        r = np.asarray(row, np.int64)
        X = pos[np.maximum(r, 0)]
        z = np.where(np.abs(X[:, 2]) > 1e-6, X[:, 2], 1.0)
        u = np.stack([fx * X[:, 0] / z + cx, fy * X[:, 1] / z + cy], 1) + rng.normal(0, 0.5, (len(r), 2))
        u[r < 0] = 0
        uv.append(u.astype(np.float32))
        first = {}
        for j, p in enumerate(row):
            if p >= 0:
                first.setdefault(int(p), j)
        where.append(first)
    return dict(kf_pose=pose, kf_slot_uv=uv, obs_slot=[[where[f][p] for f in o] for p, o in enumerate(init["obs"])])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()

    ctx = Context(0)
    L, h = lib(), ctx.handle
    X = {}
    arms, _, _, base, cleanup = KI.build_arms(ctx, 100, expose=X)
    fp, caps, init, b = X["fp"], X["caps"], X["init"], X["bufs"]["a"]
    geom = geometry(init, fp)
    opt = A.LMOptions.default()
    solver = BASolver(ctx)
    rec = keyframe_ba_record(ctx)
    irec = b["irec"].ptr.value
    d_kf, d_status = irec + A.KfInsertResult.kf.offset, irec + A.KfInsertResult.status.offset
    info = {}

    def fresh():
        """A tracked frame in arm a's buffers and a store in its initial state (untimed)."""
        rc = X["frame"](b, X["lmap_static"], X["static"].c) | L.lorb_sync(h)
        assert rc == 0
        return KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init, geom=geom)

    arms["a"](30)  # the seven-call loop warm: arm a's buffers hold a tracked frame
    steady = fresh()
    assert (X["insert"](b, steady, A.LORB_KF_GATE_NONE) | L.lorb_sync(h)) == 0
    rows = [(steady.geometry["kf_pose"], steady.geometry["kf_pose"].numpy()), (steady.arrays["pos"], steady.arrays["pos"].numpy())]

    def arm_a(keep_window=False):
        for dev, host in rows:  # the state the insertion left
            ctx.check(L.lorb_memcpy_h2d(h, dev.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)), "h2d")
        t0 = time.perf_counter()
        keyframe_local_ba(ctx, steady, fp, d_kf, rec, d_src_status=d_status, opt=opt)
        rc = L.lorb_sync(h)
        dt = time.perf_counter() - t0
        r = keyframe_ba_result(rec)
        assert rc == 0 and r.status == 0 and r.written == 1, (rc, r.status, r.written)
        if keep_window:
            info["window"] = dict(n_poses=r.n_poses, n_fixed=r.n_fixed, n_points=r.n_points, n_obs=r.n_obs, n_cov_bad=r.n_cov_bad,
                                  n_obs_bad_kf=r.n_obs_bad_kf, n_obs_bad_slot=r.n_obs_bad_slot)
        return dt * 1e6

    def arm_a_new():
        store = fresh()
        t0 = time.perf_counter()
        rc = X["insert"](b, store, A.LORB_KF_GATE_NONE)
        keyframe_local_ba(ctx, store, fp, d_kf, rec, d_src_status=d_status, opt=opt)
        rc |= L.lorb_sync(h)
        dt = time.perf_counter() - t0
        r = keyframe_ba_result(rec)
        assert rc == 0 and r.status == 0 and r.written == 1, (rc, r.status, r.written)
        store.free()
        return dt * 1e6

    def arm_a_new_ba():
        store = fresh()
        rc = X["insert"](b, store, A.LORB_KF_GATE_NONE) | L.lorb_sync(h)
        t0 = time.perf_counter()
        keyframe_local_ba(ctx, store, fp, d_kf, rec, d_src_status=d_status, opt=opt)
        rc |= L.lorb_sync(h)
        dt = time.perf_counter() - t0
        r = keyframe_ba_result(rec)
        assert rc == 0 and r.status == 0 and r.written == 1, (rc, r.status, r.written)
        store.free()
        return dt * 1e6

    def arm_a_gather():
        store = fresh()
        rc = X["insert"](b, store, A.LORB_KF_GATE_NONE) | L.lorb_sync(h)
        t0 = time.perf_counter()
        keyframe_local_ba(ctx, store, fp, d_kf, rec, d_src_status=d_status, gather_only=True)
        dt = time.perf_counter() - t0
        assert rc == 0 and keyframe_ba_result(rec).status == 0
        store.free()
        return dt * 1e6

    def host_window():
        store = fresh()
        rc = X["insert"](b, store, A.LORB_KF_GATE_NONE) | L.lorb_sync(h)
        keyframe_local_ba(ctx, store, fp, d_kf, rec, d_src_status=d_status, gather_only=True)
        w = store.ba_window(keyframe_ba_result(rec))
        assert rc == 0
        store.free()
        return w

    def arm_b():
        prep = solver.prepare(host_window())
        L.lorb_sync(h)
        t0 = time.perf_counter()
        _, _, s = solver.solve_prepared(prep, opt)
        dt = time.perf_counter() - t0
        info["solver_summary"] = s
        return dt * 1e6

    if args.trace_run:
        for _ in range(args.warmup + args.repeats):
            arm_a()
        print(json.dumps(dict(tool="tools/bench_kf_ba.py", trace_run=True, solves=args.warmup + args.repeats)))
    else:
        fns = dict(a=arm_a, a_new=arm_a_new, a_new_ba=arm_a_new_ba, a_gather=arm_a_gather, b=arm_b)
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        arm_a(keep_window=True)
        for dev, host in rows:
            ctx.check(L.lorb_memcpy_h2d(h, dev.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)), "h2d")
        info["summary"] = keyframe_local_ba(ctx, steady, fp, d_kf, rec, d_src_status=d_status, opt=opt, summary=True)
        samples = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, f in fns.items():  # interleaved
                samples[k].append(f())
        out = dict(tool="tools/bench_kf_ba.py", repeats=args.repeats, warmup=args.warmup, unit="us per call", **base, state=info, arms={})
        for k, v in samples.items():
            out["arms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
        m = {k: out["arms"][k]["median"] for k in fns}
        out["comparison"] = dict(a_minus_b=m["a"] - m["b"], first_call_minus_steady=m["a_new_ba"] - m["a"],
                                 insertion_in_chain=m["a_new"] - m["a_new_ba"], gather_share_of_a=m["a_gather"] / m["a"])
        print(json.dumps(out))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    steady.free()
    solver.close()
    rec.free()
    cleanup()
    ctx.close()


if __name__ == "__main__":
    main()
