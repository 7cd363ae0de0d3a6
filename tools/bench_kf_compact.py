#!/usr/bin/env python3
"""What reclaiming dead point rows costs, and what carrying them costs: one lorb_kf_store_compact_dev with its wait, and
the frame loop and one insertion on a store with 0, 10 and 100 times as many dead rows as live ones against the same
store compacted.

Scene, sizes and protocol are tools/bench_kf_cull.py's (480 x 752, 1000 features, 8 levels, bounds 1250, 4500 points
under 12 keyframes, one of them bad; the KeyframeStore has tools/bench_kf_ba.py's geometry).

  compact_created  a NEW store per repetition with the tracked frame inserted as keyframe 12 and culled under
             {0.25, 0, 2, 3} (untimed, waited for): every point the insertion created is culled.  Then
             lorb_kf_store_compact_dev with the gid tables of the current and of the last frame, d_map and the lorb_sync
             behind it, timed together.  The culled points are dropped.
  compact_none  the same behind a cull under LORB_KF_CULL_REFERENCE: nobody is culled, the call has nothing to drop and
             its last two kernels return at once.
  loop8_dead{0,10,100}  the eight-call frame loop (tools/bench_kf_cull.py's loop8, lorb_kf_store_observe_dev under
             LORB_KF_FOUND_NEVER) on a store whose 4500 live points are followed by 0, 10 or 100 times as many dead rows
             (bad, unobserved, in no keyframe row -- what lorb_kf_store_cull_dev leaves), the host's bounds tight
             (lorb_kf_store_counts): every kernel that walks the points bound walks the dead rows.
  loop8_dead{10,100}_compacted  the same store after one compaction and lorb_kf_store_counts.
  insert_dead{0,10,100}, insert_dead{10,100}_compacted  one LORB_KF_GATE_NONE insertion of the tracked frame and the
             wait behind it on those stores (each arm's store takes one keyframe per round).

Protocol: warm-up of every arm, then `--repeats` rounds with the arms interleaved inside the round; the loop arms run
`--calls` frames per round and report the mean per frame; median and min / max over the rounds.

  python tools/bench_kf_compact.py --out profiles/r22/kf_compact.json
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
from lorb_slam_amd.frame import (KeyframeStore, LocalMap, keyframe_compact_record, keyframe_compact_result, keyframe_cull,  # noqa: E402
                                 keyframe_cull_record, keyframe_cull_result, keyframe_observe_record)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

CULL_CREATED = (0.25, 0, 2, 3)


def with_dead_rows(init, geom, factor):
    """The initial store with factor * n_points dead rows behind its live ones."""
    n = len(init["pos"])
    d = factor * n
    out = dict(init)
    for k in ("pos", "normal", "max_dist", "min_dist", "desc", "locked"):
        a = np.asarray(init[k])
        out[k] = np.concatenate([a, np.zeros((d,) + a.shape[1:], a.dtype)])
    bad = np.zeros(n, np.uint8) if init.get("is_bad") is None else np.asarray(init["is_bad"], np.uint8)
    out["is_bad"] = np.concatenate([bad, np.ones(d, np.uint8)])
    out["obs"] = list(init["obs"]) + [[] for _ in range(d)]
    return out, dict(geom, obs_slot=list(geom["obs_slot"]) + [[] for _ in range(d)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--factors", default="0,10,100", help="dead rows per live row of the stores, 0 first (default 0,10,100)")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    FACTORS = tuple(int(v) for v in args.factors.split(","))
    assert FACTORS[0] == 0, "the first store is the one without dead rows"

    ctx = Context(0)
    L, h = lib(), ctx.handle
    X = {}
    arms, _, _, base, cleanup = KI.build_arms(ctx, 100, expose=X)
    fp, caps, init, b = X["fp"], X["caps"], X["init"], X["bufs"]["a"]
    geom = KB.geometry(init, fp)
    n_live = len(init["pos"])
    rounds = args.warmup + args.repeats
    crec, orec, mrec = keyframe_cull_record(ctx), keyframe_observe_record(ctx), keyframe_compact_record(ctx)
    irec = b["irec"].ptr.value
    d_kf, d_status = irec + A.KfInsertResult.kf.offset, irec + A.KfInsertResult.status.offset
    nb = C.c_int32(KI.BOUND)
    info = {}

    def tables(bb):
        return [(bb["gid"], bb["f"].out.counts, KI.BOUND), (X["last_gid"], X["fa"].out.counts, KI.BOUND)]

    def store_with(factor):
        s, g = with_dead_rows(init, geom, factor)
        P = len(s["pos"])
        st = KeyframeStore(ctx, caps["max_kf"] + rounds, P + (rounds + 2) * KI.BOUND, caps["max_obs"] + rounds * KI.BOUND,
                           caps["max_kf_slots"] + rounds * KI.BOUND, init=s, geom=g)
        st.counts()  # tight bounds
        return st

    def fresh():
        """A tracked frame in arm a's buffers and a store in its initial state (untimed)."""
        rc = X["frame"](b, X["lmap_static"], X["static"].c) | L.lorb_sync(h)
        assert rc == 0
        return KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init, geom=geom)

    dmap = ctx.to_device(np.zeros(caps["max_points"], np.int32))

    def arm_compact(params, key):
        def run():
            store = fresh()
            rc = X["insert"](b, store, A.LORB_KF_GATE_NONE)
            keyframe_cull(ctx, store, d_kf, crec, d_src_status=d_status, params=params, cur=b["f"], cur_slots=b["cs"], slot_gid=b["gid"],
                          n_max_cur=KI.BOUND)
            rc |= L.lorb_sync(h)
            t0 = time.perf_counter()
            store.compact(mrec, tables=tables(b), d_src_status=d_status, d_map=dmap)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            r, c = keyframe_compact_result(mrec), keyframe_cull_result(crec)
            assert rc == 0 and r.status == 0 and c.status == 0, (rc, r.status, c.status)
            assert r.n_dropped >= c.n_culled_ratio + c.n_culled_obs, (r.n_dropped, c.n_culled_ratio, c.n_culled_obs)
            info[key] = {f: getattr(r, f) for f, _ in A.KfCompactResult._fields_}
            store.free()
            return dt * 1e6
        return run

    arms["a"](30)  # the loop warm: arm a's buffers hold a tracked frame
    # the stores that carry dead rows, and their compacted twins: made once, outside the rounds
    stores, lmaps = {}, {}
    big = ctx.to_device(np.zeros((1 + max(FACTORS)) * n_live + (rounds + 2) * KI.BOUND, np.int32))
    for f in FACTORS:
        stores["dead%d" % f] = store_with(f)
        if f:
            st = stores["dead%d_compacted" % f] = store_with(f)
            st.compact(mrec, tables=tables(b), d_map=big)
            assert L.lorb_sync(h) == 0
            r = keyframe_compact_result(mrec)
            assert r.status == 0 and r.n_dropped >= f * n_live and r.n_points <= n_live, (r.status, r.n_dropped, r.n_points)
            st.counts()
    for k, st in stores.items():
        lmaps[k] = LocalMap(ctx, KI.MAX_LOCAL, st.caps.max_kf, st.caps.max_points)
        info["store_" + k] = st.counts()

    def arm_loop(key):
        store, lmap = stores[key], lmaps[key]
        fid = [0]

        def observe(bb, lm):
            fid[0] += 1
            return L.lorb_kf_store_observe_dev(h, store._p, C.c_int32(fid[0]), C.byref(bb["f"].out), nb, C.byref(bb["cs"].c),
                                               bb["gid"].ptr, bb["sid"].ptr, C.byref(lm.view), bb["urec"].ptr, bb["out"].in_view.ptr,
                                               bb["d_lstatus"], C.c_int32(A.LORB_KF_FOUND_NEVER), orec.ptr)

        def run(n=args.calls):
            view = store.view()
            bb = X["bufs"]["d"]
            bb["model"].upload(X["model_I"])
            L.lorb_sync(h)
            t0 = time.perf_counter()
            rc = 0
            for _ in range(n):
                rc |= X["frame"](bb, lmap, view, observe)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            st = bb["out"].result().status
            assert rc == 0 and st == 0, (rc, st)
            return dt / n * 1e6
        return run

    def arm_insert(key):
        store = stores[key]

        def run():
            rc = X["frame"](b, X["lmap_static"], X["static"].c) | L.lorb_sync(h)  # a tracked frame, untimed
            t0 = time.perf_counter()
            rc |= X["insert"](b, store, A.LORB_KF_GATE_NONE)
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            rec = b["irec"].read()
            assert rc == 0 and rec.status == 0 and rec.inserted == 1, (rc, rec.status, rec.inserted)
            store.counts()  # tight bounds again (untimed)
            return dt * 1e6
        return run

    fns = dict(compact_created=arm_compact(CULL_CREATED, "compact_created"), compact_none=arm_compact(A.LORB_KF_CULL_REFERENCE, "compact_none"))
    for k in stores:
        fns["loop8_" + k] = arm_loop(k)
    for k in stores:  # the loops first: an insertion grows its store
        fns["insert_" + k] = arm_insert(k)
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    samples = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():  # interleaved
            samples[k].append(f())
    out = dict(tool="tools/bench_kf_compact.py", repeats=args.repeats, warmup=args.warmup, calls_per_repeat=args.calls,
               unit="us per frame (loop arms), us per call (the others)", live_points=n_live, **base, state=info, arms={})
    for k, v in samples.items():
        out["arms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    # the arms of one round run back to back, so the difference is taken round by round: median [min, max]
    def paired(a, b):
        d = [x - y for x, y in zip(samples[a], samples[b])]
        return dict(median=statistics.median(d), min=min(d), max=max(d))

    out["comparison"] = {}
    for what in ("loop8", "insert"):
        for f in FACTORS:
            if f:
                out["comparison"]["%s_dead%d_minus_dead0" % (what, f)] = paired("%s_dead%d" % (what, f), "%s_dead0" % what)
                out["comparison"]["%s_dead%d_compacted_minus_dead0" % (what, f)] = paired("%s_dead%d_compacted" % (what, f), "%s_dead0" % what)
        out["comparison"]["%s_dead0_spread" % what] = out["arms"]["%s_dead0" % what]["max"] - out["arms"]["%s_dead0" % what]["min"]
    out["comparison"]["compact_created_minus_none"] = paired("compact_created", "compact_none")
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for r in (crec, orec, mrec, dmap, big, *lmaps.values(), *stores.values()):
        r.free()
    cleanup()
    ctx.close()


if __name__ == "__main__":
    main()
