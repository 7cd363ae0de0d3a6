#!/usr/bin/env python3
"""What the points' life and the map-point culling cost: one lorb_kf_store_cull_dev with its wait, and the frame loop
with lorb_kf_store_observe_dev in it against the same loop without.

Scene, sizes and protocol are tools/bench_kf_insert.py's (480 x 752, 1000 features, 8 levels, bounds 1250, 4500
points under 12 keyframes, one of them bad); the KeyframeStore has tools/bench_kf_ba.py's geometry.

  loop7      the seven-call loop on a KeyframeStore view with tight counts, no insertion (tools/bench_kf_insert.py's
             arm d): the parent commit's loop.
  loop8      the same with lorb_kf_store_observe_dev (LORB_KF_FOUND_NEVER, the reference) enqueued behind
             lorb_track_local_frames_dev and in front of lorb_local_map_ids_back_dev: eight calls per frame.
  loop8_slots  loop8 under LORB_KF_FOUND_SLOTS.
  cull_none  a NEW store per repetition with the tracked frame inserted as keyframe 12 (untimed, waited for), then
             lorb_kf_store_cull_dev under LORB_KF_CULL_REFERENCE with the frame group and the lorb_sync behind it, timed
             together.  The points that insertion created are zero frames old: nobody is culled, the two kernels behind
             the verdicts return at once.
  cull_created  the same under {0.25, 0, 2, 3}: every point the insertion created has one observation and is culled,
             its keyframe slot and its frame slot are erased and the observation CSR is rebuilt.
  insert_cull_ba  insertion, cull (reference parameters) and local BA on the record words, enqueued back to back on
             a new store, and the lorb_sync behind them; insert_ba is the same without the cull (tools/bench_kf_ba.py's
             a_new).

Protocol: warm-up of every arm, then `--repeats` rounds with the arms interleaved inside the round; the loop arms run
`--calls` frames per round and report the mean per frame; median and min / max over the rounds.

  python tools/bench_kf_cull.py --out profiles/r21/kf_cull.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_kf_ba as KB  # noqa: E402
import bench_kf_insert as KI  # noqa: E402
from lorb_slam_amd import _abi as A  # noqa: E402
from lorb_slam_amd.frame import (KeyframeStore, keyframe_ba_record, keyframe_ba_result, keyframe_cull, keyframe_cull_record,  # noqa: E402
                                 keyframe_cull_result, keyframe_local_ba, keyframe_observe_record, keyframe_observe_result)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

CULL_CREATED = (0.25, 0, 2, 3)


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
    fp, caps, init, b = X["fp"], X["caps"], X["init"], X["bufs"]["a"]
    geom = KB.geometry(init, fp)
    opt = A.LMOptions.default()
    crec, brec, orec = keyframe_cull_record(ctx), keyframe_ba_record(ctx), keyframe_observe_record(ctx)
    irec = b["irec"].ptr.value
    d_kf, d_status = irec + A.KfInsertResult.kf.offset, irec + A.KfInsertResult.status.offset
    nb = C.c_int32(KI.BOUND)
    info = {}

    def fresh():
        """A tracked frame in arm a's buffers and a store in its initial state (untimed)."""
        rc = X["frame"](b, X["lmap_static"], X["static"].c) | L.lorb_sync(h)
        assert rc == 0
        return KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init, geom=geom)

    def cull(store, params):
        keyframe_cull(ctx, store, d_kf, crec, d_src_status=d_status, params=params, cur=b["f"], cur_slots=b["cs"], slot_gid=b["gid"],
                      n_max_cur=KI.BOUND)

    def arm_cull(params, key):
        def run():
            store = fresh()
            rc = X["insert"](b, store, A.LORB_KF_GATE_NONE) | L.lorb_sync(h)
            t0 = time.perf_counter()
            cull(store, params)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            r = keyframe_cull_result(crec)
            assert rc == 0 and r.status == 0, (rc, r.status)
            info[key] = {f: getattr(r, f) for f, _ in A.KfCullResult._fields_}
            store.free()
            return dt * 1e6
        return run

    def arm_chain(with_cull):
        def run():
            store = fresh()
            t0 = time.perf_counter()
            rc = X["insert"](b, store, A.LORB_KF_GATE_NONE)
            if with_cull:
                cull(store, A.LORB_KF_CULL_REFERENCE)
            keyframe_local_ba(ctx, store, fp, d_kf, brec, d_src_status=d_status, opt=opt)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            r = keyframe_ba_result(brec)
            assert rc == 0 and r.status == 0 and r.written == 1, (rc, r.status, r.written)
            store.free()
            return dt * 1e6
        return run

    def arm_loop(rule):
        def run(n=args.calls):
            store = KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init, geom=geom)
            store.counts()  # tight bounds
            view, lmap = store.view(), X["lmap_grow"]
            fid = [0]

            def observe(bb, lm):
                fid[0] += 1
                return L.lorb_kf_store_observe_dev(h, store._p, C.c_int32(fid[0]), C.byref(bb["f"].out), nb, C.byref(bb["cs"].c),
                                                   bb["gid"].ptr, bb["sid"].ptr, C.byref(lm.view), bb["urec"].ptr, bb["out"].in_view.ptr,
                                                   bb["d_lstatus"], C.c_int32(rule), orec.ptr)

            bb = X["bufs"]["d"]
            bb["model"].upload(X["model_I"])
            L.lorb_sync(h)
            t0 = time.perf_counter()
            rc = 0
            for _ in range(n):
                rc |= X["frame"](bb, lmap, view, None if rule is None else observe)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            st = bb["out"].result().status
            assert rc == 0 and st == 0, (rc, st)
            if rule is not None:
                r = keyframe_observe_result(orec)
                assert r.status == 0
                info["observe_%d" % rule] = dict(n_held=r.n_held, n_in_view=r.n_in_view, n_found=r.n_found)
            store.free()
            return dt / n * 1e6
        return run

    arms["a"](30)  # the seven-call loop warm: arm a's buffers hold a tracked frame
    fns = dict(loop7=arm_loop(None), loop8=arm_loop(A.LORB_KF_FOUND_NEVER), loop8_slots=arm_loop(A.LORB_KF_FOUND_SLOTS),
               cull_none=arm_cull(A.LORB_KF_CULL_REFERENCE, "cull_none"), cull_created=arm_cull(CULL_CREATED, "cull_created"),
               insert_ba=arm_chain(False), insert_cull_ba=arm_chain(True))
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    samples = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():  # interleaved
            samples[k].append(f())
    out = dict(tool="tools/bench_kf_cull.py", repeats=args.repeats, warmup=args.warmup, calls_per_repeat=args.calls,
               unit="us per frame (loop arms), us per call (the others)", **base, state=info, arms={})
    for k, v in samples.items():
        out["arms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    m = {k: out["arms"][k]["median"] for k in fns}
    out["comparison"] = dict(observe_per_frame=m["loop8"] - m["loop7"], observe_slots_per_frame=m["loop8_slots"] - m["loop7"],
                             loop7_spread=out["arms"]["loop7"]["max"] - out["arms"]["loop7"]["min"],
                             cull_in_chain=m["insert_cull_ba"] - m["insert_ba"])
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for r in (crec, brec, orec):
        r.free()
    cleanup()
    ctx.close()


if __name__ == "__main__":
    main()
