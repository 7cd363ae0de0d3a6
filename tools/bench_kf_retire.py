#!/usr/bin/env python3
"""What retiring keyframes costs: one lorb_kf_store_retire_dev with its wait, and the frame loop on a store whose oldest
keyframes are retired against the same loop on the store as it is.

Scene, sizes and protocol are tools/bench_kf_insert.py's (480 x 752, 1000 features, 8 levels, bounds 1250, 4500
points under 12 keyframes, one of them bad); the KeyframeStore has tools/bench_kf_ba.py's geometry, and every keyframe
gets the frame id index + 1 (lorb_kf_store_life_write), because a keyframe with kf_fid 0 is never retired.

  retire_1   a NEW store per repetition (untimed, waited for), then lorb_kf_store_retire_dev for keyframe 0 and the
             lorb_sync behind it, timed together.
  retire_8   the same for keyframes 0 .. 7.
  loop7      the seven-call loop on a KeyframeStore view with tight counts, no insertion (tools/bench_kf_insert.py's arm
             d): the arm WITHOUT the call, the comparison.
  loop7_retired4  the same loop on a store whose keyframes 0 .. 3 were retired (untimed) before the loop starts.

Protocol: warm-up of every arm, then `--repeats` rounds with the arms interleaved inside the round; the loop arms run
`--calls` frames per round and report the mean per frame; median and min / max over the rounds.

  python tools/bench_kf_retire.py --out profiles/r25/kf_retire.json
"""
import argparse
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
from lorb_slam_amd.frame import (KeyframeStore, keyframe_retire, keyframe_retire_record, keyframe_retire_result,  # noqa: E402
                                 local_map_result)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()

    ctx = Context(0)
    L, h = lib(), ctx.handle
    X = {}
    arms, _, _, base, cleanup = KI.build_arms(ctx, 100, expose=X)
    fp, caps, init = X["fp"], X["caps"], X["init"]
    geom = KB.geometry(init, fp)
    n_kf = len(init["kf_bad"])
    d_list = ctx.to_device(np.arange(8, dtype=np.int32))
    d_n = {n: ctx.to_device(np.array([n], np.int32)) for n in (1, 4, 8)}
    rrec = keyframe_retire_record(ctx)
    info = {}

    def fresh():
        store = KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init, geom=geom)
        store.write_life(dict(kf_fid=np.arange(1, n_kf + 1, dtype=np.int32)))
        return store

    def arm_retire(n):
        def run():
            store = fresh()
            rc = L.lorb_sync(h)
            t0 = time.perf_counter()
            keyframe_retire(ctx, store, d_list, d_n[n], rrec, n_max_list=8)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            r = keyframe_retire_result(rrec)
            assert rc == 0 and r.status == 0, (rc, r.status)
            info["retire_%d" % n] = {f: getattr(r, f) for f, _ in A.KfRetireResult._fields_}
            store.free()
            return dt * 1e6
        return run

    def arm_loop(retired):
        def run(n=args.calls):
            store = fresh()
            if retired:
                keyframe_retire(ctx, store, d_list, d_n[retired], rrec, n_max_list=8)
            store.counts()  # waits; tight bounds
            view, lmap = store.view(), X["lmap_grow"]
            bb = X["bufs"]["d"]
            bb["model"].upload(X["model_I"])
            L.lorb_sync(h)
            t0 = time.perf_counter()
            rc = 0
            for _ in range(n):
                rc |= X["frame"](bb, lmap, view, None)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            st = bb["out"].result().status
            assert rc == 0 and st == 0, (rc, st)
            u = local_map_result(bb["urec"])
            info["loop7_retired%d" % retired] = dict(n_local_kf=u.n_local_kf, n_local=u.n_local)
            store.free()
            return dt / n * 1e6
        return run

    arms["a"](30)  # the seven-call loop warm
    fns = dict(retire_1=arm_retire(1), retire_8=arm_retire(8), loop7=arm_loop(0), loop7_retired4=arm_loop(4))
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    samples = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():  # interleaved
            samples[k].append(f())
    out = dict(tool="tools/bench_kf_retire.py", repeats=args.repeats, warmup=args.warmup, calls_per_repeat=args.calls,
               unit="us per frame (loop arms), us per call with its wait (the others)", **base, state=info, arms={})
    for k, v in samples.items():
        out["arms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    m = {k: out["arms"][k]["median"] for k in fns}
    out["comparison"] = dict(loop_retired4_minus_loop=m["loop7_retired4"] - m["loop7"],
                             loop7_spread=out["arms"]["loop7"]["max"] - out["arms"]["loop7"]["min"],
                             retire_8_minus_1=m["retire_8"] - m["retire_1"])
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for r in (rrec, d_list, *d_n.values()):
        r.free()
    cleanup()
    ctx.close()


if __name__ == "__main__":
    main()
