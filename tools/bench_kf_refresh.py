#!/usr/bin/env python3
"""What refreshing the map points of a window costs: lorb_kf_store_refresh_dev with its wait behind the local bundle
adjustment, each of its flags alone, and a whole keyframe step with and without it.

Scene, sizes and protocol are tools/bench_kf_ba.py's (480 x 752, 1000 features, 8 levels, bounds 1250, 4500 points
under 12 keyframes, one of them bad; the KeyframeStore has that tool's geometry).  The appearance of the initial
keyframes: random descriptors, octaves in [0, 8), the centres -R^T t of their pose rows.

  refresh_all   ONE store for all repetitions: the forced insertion is made once; a repetition puts the kf_pose and pos
                rows back, runs lorb_kf_store_local_ba_dev and waits (untimed), then times lorb_kf_store_refresh_dev
                with LORB_KF_REFRESH_ALL and the lorb_sync behind it.
  refresh_centers / refresh_normal_depth / refresh_descriptor   the same with one flag.
  sync_only     the lorb_sync alone on the idle stream: the floor of the arms above.
  step          a NEW store per repetition: insert -> cull (LORB_KF_CULL_REFERENCE) -> local BA -> compact (the gid
                tables of the current and the last frame), enqueued back to back, and the lorb_sync behind them.
  step_refresh  the same with the refresh between the BA and the compaction.

Protocol: warm-up of every arm, then `--repeats` rounds with the arms interleaved inside the round; median and
min / max over the rounds; step_refresh - step is taken round by round.

  python tools/bench_kf_refresh.py --out profiles/r23/kf_refresh.json
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

import bench_kf_ba as KB  # noqa: E402
import bench_kf_insert as KI  # noqa: E402
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd.frame import (KeyframeStore, keyframe_ba_record, keyframe_ba_result, keyframe_compact_record,  # noqa: E402
                                 keyframe_compact_result, keyframe_cull, keyframe_cull_record, keyframe_local_ba,
                                 keyframe_refresh, keyframe_refresh_record, keyframe_refresh_result)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402


def appearance(init, geom):
    """Random descriptors and octaves for every initial keyframe slot; the centre of a pose row is -R^T t."""
    rng = np.random.default_rng(29)
    ns = sum(len(r) for r in init["kf_slots"])
    centers = []
    for p in np.asarray(geom["kf_pose"], np.float32).reshape(-1, 6):
        T = np.zeros(16, np.float32)
        lib().lorb_pose_to_Tcw(p[:3].ctypes.data_as(C.c_void_p), p[3:].ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p))
        T = T.reshape(4, 4).astype(np.float64)
        centers.append(-T[:3, :3].T @ T[:3, 3])
    return dict(kf_slot_desc=rng.integers(0, 256, (ns, 32), dtype=np.uint8), kf_slot_octave=rng.integers(0, 8, ns).astype(np.int32),
                kf_center=np.asarray(centers, np.float32).reshape(-1, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()

    ctx = Context(0)
    L, h = lib(), ctx.handle
    X = {}
    arms, _, _, base, cleanup = KI.build_arms(ctx, 100, expose=X)
    fp, caps, init, b = X["fp"], X["caps"], X["init"], X["bufs"]["a"]
    geom = KB.geometry(init, fp)
    app = appearance(init, geom)
    opt = A.LMOptions.default()
    rec, rrec, crec, mrec = keyframe_ba_record(ctx), keyframe_refresh_record(ctx), keyframe_cull_record(ctx), keyframe_compact_record(ctx)
    irec = b["irec"].ptr.value
    d_kf, d_status = irec + A.KfInsertResult.kf.offset, irec + A.KfInsertResult.status.offset
    info = {}

    def fresh():
        """A tracked frame in arm a's buffers and a store in its initial state, appearance included (untimed)."""
        rc = X["frame"](b, X["lmap_static"], X["static"].c) | L.lorb_sync(h)
        assert rc == 0
        st = KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init, geom=geom)
        st.write_appearance(app)
        return st

    arms["a"](30)  # the seven-call loop warm: arm a's buffers hold a tracked frame
    steady = fresh()
    assert (X["insert"](b, steady, A.LORB_KF_GATE_NONE) | L.lorb_sync(h)) == 0
    rows = [(steady.geometry["kf_pose"], steady.geometry["kf_pose"].numpy()), (steady.arrays["pos"], steady.arrays["pos"].numpy())]
    rows += [(steady.arrays[k], steady.arrays[k].numpy()) for k in ("normal", "max_dist", "min_dist", "desc")]
    rows += [(steady.appearance["kf_center"], steady.appearance["kf_center"].numpy())]

    def arm_refresh(what, key):
        def run():
            for dev, host in rows:  # the state the insertion left
                ctx.check(L.lorb_memcpy_h2d(h, dev.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)), "h2d")
            keyframe_local_ba(ctx, steady, fp, d_kf, rec, d_src_status=d_status, opt=opt)
            rc = L.lorb_sync(h)
            t0 = time.perf_counter()
            keyframe_refresh(ctx, steady, fp, rec, rrec, what=what)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            r, ba = keyframe_refresh_result(rrec), keyframe_ba_result(rec)
            assert rc == 0 and r.status == 0 and ba.written == 1, (rc, r.status, ba.written)
            info[key] = {f: getattr(r, f) for f, _ in A.KfRefreshResult._fields_}
            info["window"] = dict(n_poses=ba.n_poses, n_fixed=ba.n_fixed, n_points=ba.n_points, n_obs=ba.n_obs)
            return dt * 1e6
        return run

    def arm_sync():
        L.lorb_sync(h)
        t0 = time.perf_counter()
        L.lorb_sync(h)
        return (time.perf_counter() - t0) * 1e6

    def tables():
        return [(b["gid"], b["f"].out.counts, KI.BOUND), (X["last_gid"], X["fa"].out.counts, KI.BOUND)]

    def arm_step(refresh):
        def run():
            store = fresh()
            t0 = time.perf_counter()
            rc = X["insert"](b, store, A.LORB_KF_GATE_NONE)
            keyframe_cull(ctx, store, d_kf, crec, d_src_status=d_status, params=A.LORB_KF_CULL_REFERENCE, cur=b["f"], cur_slots=b["cs"],
                          slot_gid=b["gid"], n_max_cur=KI.BOUND)
            keyframe_local_ba(ctx, store, fp, d_kf, rec, d_src_status=d_status, opt=opt)
            if refresh:
                keyframe_refresh(ctx, store, fp, rec, rrec)
            store.compact(mrec, tables=tables(), d_src_status=d_status)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            ba, m = keyframe_ba_result(rec), keyframe_compact_result(mrec)
            assert rc == 0 and ba.status == 0 and ba.written == 1 and m.status == 0, (rc, ba.status, ba.written, m.status)
            if refresh:
                assert keyframe_refresh_result(rrec).status == 0
            store.free()
            return dt * 1e6
        return run

    fns = dict(refresh_all=arm_refresh(A.LORB_KF_REFRESH_ALL, "refresh_all"),
               refresh_centers=arm_refresh(A.LORB_KF_REFRESH_CENTERS, "refresh_centers"),
               refresh_normal_depth=arm_refresh(A.LORB_KF_REFRESH_NORMAL_DEPTH, "refresh_normal_depth"),
               refresh_descriptor=arm_refresh(A.LORB_KF_REFRESH_DESCRIPTOR, "refresh_descriptor"), sync_only=arm_sync,
               step=arm_step(False), step_refresh=arm_step(True))
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    samples = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():  # interleaved
            samples[k].append(f())
    out = dict(tool="tools/bench_kf_refresh.py", repeats=args.repeats, warmup=args.warmup, unit="us per call", **base, state=info, arms={})
    for k, v in samples.items():
        out["arms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    d = [x - y for x, y in zip(samples["step_refresh"], samples["step"])]
    out["comparison"] = dict(step_refresh_minus_step=dict(median=statistics.median(d), min=min(d), max=max(d)),
                             refresh_all_minus_sync=out["arms"]["refresh_all"]["median"] - out["arms"]["sync_only"]["median"])
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for r in (rec, rrec, crec, mrec, steady):
        r.free()
    cleanup()
    ctx.close()


if __name__ == "__main__":
    main()
