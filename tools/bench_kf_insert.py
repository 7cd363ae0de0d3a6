#!/usr/bin/env python3
"""What lorb_kf_store_insert_dev costs: one insertion, the frame loop with an insertion enqueued every tenth frame
against the same loop on a static store, and lorb_local_map_update_dev on the store's bounds against tightened counts.

Scene, sizes and protocol are tools/bench_frame_loop_refer.py's (480 x 752, 1000 features, 8 levels, bounds 1250,
max_local 4096, 4500 points under 12 keyframes; the last frame built once, INITIALIZE-filled and resident at the
identity; frame k + 1 predicts with the mTcc frame k left; the seven-call frame of its arm c).  The KeyframeStore
starts from that store (weight maps: the shared-point counts) with room for the round's insertions; every round of
every arm that inserts starts from a fresh store, made outside the timed region.

  a  the seven-call loop on the static DeviceMapStore: the parent commit's loop.
  b  the same loop on the KeyframeStore's view (taken every frame, no wait) with lorb_kf_store_insert_dev enqueued
     behind every tenth frame's lorb_frame_pose_finish_dev, LORB_KF_GATE_RATIO: the device decides.
  c  b with LORB_KF_GATE_NONE: every tenth frame IS inserted, the store grows through the round.
  d  the loop on a KeyframeStore view whose counts are tight (lorb_kf_store_counts), no insertion.
  e  the loop on a view whose bounds carry INSERTS_PER_ROUND insertions that did not happen (enqueued before the
     round; status 1 on the device), none in the round: e - d is what the bounds cost lorb_local_map_update_dev per frame.
  one insertion: a tracked frame (one frame of arm a, untimed), then ONE LORB_KF_GATE_NONE insertion of it and the
     lorb_sync behind it, timed together; the median of INSERTS_PER_ROUND of them into one growing store.

Protocol: warm-up of every arm, then `--repeats` rounds; in every round each arm runs `--calls` frames, the arms
interleaved inside the round; every round ends with a check of its last frame's status (outside the timed region).
Reported per arm: median and min / max over the rounds of the mean time per frame.

  python tools/bench_kf_insert.py --out profiles/r19/kf_insert.json
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
from lorb_slam_amd.frame import (DeviceBlock, DeviceMapStore, DeviceSlots, FrameBuilder, KeyframeStore, LocalFramesOut,  # noqa: E402
                                 LocalMap, fill_slots, local_map_buffers, local_map_result, model_block,
                                 motion_record_addresses, pose_block, refer_kf_word)
from lorb_slam_amd.runtime import Context, lib  # noqa: E402

REFER_KF = 0
EVERY = 10


def build_arms(ctx, calls, expose=None):
    """expose: a dict that receives the scene's parts (tools/bench_kf_ba.py builds its arms from them)."""
    L, h = lib(), ctx.handle
    inserts = max(calls // EVERY, 1)  # INSERTS_PER_ROUND
    fp = synth.frame_params(width=COLS, height=ROWS)
    fps = A.make_frame_params(fp)
    nd = features_per_level(NFEATURES)
    pat = np.random.default_rng(7).integers(-13, 13, size=1024).astype(np.int32)
    fb = FrameBuilder(ctx, fp, ROWS, COLS, nd, pat)
    last_img = synth.stereo_pair(SEED, ROWS, COLS)
    cur_img = synth.stereo_pair(SEED, ROWS, COLS, shift=2, noise_seed=777)
    fa = fb.build_device(*last_img)
    n_last = int(fa.read_counts()[0])
    held = [fa]

    def keep(d):
        held.append(d)
        return d

    I4 = np.eye(4, dtype=np.float32)
    mpar, lpar, opt = A.TrackMotionParams(15.0, 30.0, 20, fps.fx), A.TrackLocalParams(0.5, 1.0, 20, fps.fx), A.LMOptions.default()
    cols, nb = C.c_int32(COLS), C.c_int32(BOUND)
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
    pts, obs, kf_bad, kf_slots, cov = make_store(pts0, last_gid[:n_last])
    static = keep(DeviceMapStore(ctx, pts, obs, kf_bad, kf_slots, cov))
    # the same store as a KeyframeStore: the weight maps are the shared-point counts the lists were ordered by
    member = np.zeros((N_KF, N_POINTS), np.int32)
    for k, sl in enumerate(kf_slots):
        member[k, [p for p in sl if p >= 0]] = 1
    shared = member @ member.T
    conn = [{int(j): int(shared[k, j]) for j in range(N_KF) if j != k and shared[k, j] > 0} for k in range(N_KF)]
    init = dict(pts, obs=obs, kf_bad=kf_bad, kf_slots=kf_slots, cov=cov, conn=conn)
    caps = dict(max_kf=N_KF + inserts + 4, max_points=N_POINTS + (inserts + 1) * BOUND,
                max_obs=sum(len(o) for o in obs) + (inserts + 1) * BOUND, max_kf_slots=sum(len(s) for s in kf_slots) + (inserts + 1) * BOUND)

    def new_store():
        return KeyframeStore(ctx, caps["max_kf"], caps["max_points"], caps["max_obs"], caps["max_kf_slots"], init=init)

    lmap_static = keep(LocalMap(ctx, MAX_LOCAL, N_KF, N_POINTS))
    lmap_grow = keep(LocalMap(ctx, MAX_LOCAL, caps["max_kf"], caps["max_points"]))
    last_pose, refer_pose = keep(pose_block(ctx, I4)), keep(pose_block(ctx, I4))
    model_I = A.MotionModel()
    model_I.Tcc[:] = [float(v) for v in I4.reshape(16)]
    bad_pose = keep(DeviceBlock(ctx, A.FramePose))  # sentinel bytes: status != 0

    def arm_buffers():
        f = keep(fb.build_device(*cur_img))
        b = dict(f=f, l=f._all[-2], r=f._all[-1], cs=keep(DeviceSlots(ctx, BOUND, state=0)), masg=keep(ctx.empty(BOUND, np.int32)),
                 mrec=keep(ctx.to_device(np.zeros(C.sizeof(A.TrackFramesResult), np.uint8))),
                 out=keep(LocalFramesOut(ctx, MAX_LOCAL, BOUND)), pose=keep(pose_block(ctx, I4)), model=keep(model_block(ctx, I4)),
                 rrec=keep(DeviceBlock(ctx, A.TrackReferResult)), kf=keep(refer_kf_word(ctx, REFER_KF)),
                 irec=keep(DeviceBlock(ctx, A.KfInsertResult)))
        b["gid"], b["sid"], b["urec"] = (keep(x) for x in local_map_buffers(ctx, BOUND))
        b["d_pose"], b["d_status"] = (C.c_void_p(v) for v in motion_record_addresses(b["mrec"]))
        b["d_ustatus"] = C.c_void_p(b["urec"].ptr.value + A.LocalMapResult.status.offset)
        b["d_lstatus"] = C.c_void_p(b["out"].record.ptr.value + A.TrackLocalFramesResult.status.offset)
        return b

    def insert(b, store, gate):
        return L.lorb_kf_store_insert_dev(h, store._p, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["gid"].ptr,
                                          b["pose"].ptr, b["d_lstatus"], C.c_int32(gate), b["kf"].ptr, b["urec"].ptr, b["irec"].ptr)

    def frame(b, lmap, view, between=None):
        """One frame: tools/bench_frame_loop_refer.py's arm c on the given store view.  between: a call enqueued behind
        the local stage and in front of the ids' way back (tools/bench_kf_cull.py: lorb_kf_store_observe_dev)."""
        o = b["out"]
        rc = L.lorb_frame_build_dev(fb._p, b["l"].ptr, cols, b["r"].ptr, cols, C.byref(b["f"].out))
        rc |= L.lorb_track_motion_frames_pose_dev(h, C.byref(fps), b["pose"].ptr, C.byref(b["f"].out), nb, C.byref(b["cs"].c),
                                                  C.c_int32(0), last_pose.ptr, b["model"].ptr, C.byref(fa.out), nb, C.byref(ls.c),
                                                  None, C.byref(mpar), C.byref(opt), b["masg"].ptr, b["mrec"].ptr)
        rc |= L.lorb_track_motion_refer_pose_dev(
            h, C.byref(fps), b["pose"].ptr, C.byref(b["f"].out), nb, C.byref(b["cs"].c), C.c_int32(0), refer_pose.ptr,
            b["model"].ptr, C.byref(fa.out), nb, C.byref(rs.c), None, d_last_gid.ptr, nb, d_last_gid.ptr, b["gid"].ptr,
            C.c_int32(REFER_KF), b["kf"].ptr, b["urec"].ptr, C.byref(mpar), C.byref(opt), b["masg"].ptr, b["mrec"].ptr, b["rrec"].ptr)
        rc |= L.lorb_local_map_update_dev(h, lmap._p, C.byref(view), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["gid"].ptr,
                                          b["sid"].ptr, b["d_status"], None, b["urec"].ptr)
        rc |= L.lorb_track_local_frames_dev(h, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["sid"].ptr, b["d_pose"],
                                            b["d_ustatus"], None, C.byref(lmap.c), C.byref(lpar), C.byref(opt), o.in_view.ptr,
                                            o.track.ptr, o.level.ptr, o.assign.ptr, o.record.ptr)
        if between is not None:
            rc |= between(b, lmap)
        rc |= L.lorb_local_map_ids_back_dev(h, lmap._p, C.byref(b["f"].out), nb, C.byref(b["cs"].c), b["sid"].ptr, b["d_lstatus"],
                                            b["gid"].ptr)
        return rc | L.lorb_frame_pose_finish_dev(h, o.record.ptr, last_pose.ptr, b["pose"].ptr, b["model"].ptr)

    bufs = {m: arm_buffers() for m in "abcde"}
    info = {}

    def make_round(mode):
        b = bufs[mode]
        gate = A.LORB_KF_GATE_NONE if mode == "c" else A.LORB_KF_GATE_RATIO

        def run(n):
            store = None if mode == "a" else new_store()
            if mode == "e":  # bounds inflated by insertions that end at status 1 on the device (the pose block's status)
                for _ in range(inserts):
                    rc = L.lorb_kf_store_insert_dev(h, store._p, C.byref(fps), C.byref(b["f"].out), nb, C.byref(b["cs"].c),
                                                    b["gid"].ptr, bad_pose.ptr, None, C.c_int32(gate), None, None, b["irec"].ptr)
                    assert rc == 0
            lmap = lmap_static if mode == "a" else lmap_grow
            view = static.c if mode == "a" else store.view()
            b["model"].upload(model_I)
            L.lorb_sync(h)
            t0 = time.perf_counter()
            rc, n_ins = 0, 0
            for k in range(n):
                if mode in "bc":
                    view = store.view()
                rc |= frame(b, lmap, view)
                if mode in "bc" and k % EVERY == EVERY - 1 and n_ins < inserts:
                    rc |= insert(b, store, gate)
                    n_ins += 1
            rc |= L.lorb_sync(h)
            dt = time.perf_counter() - t0
            st, up = b["out"].result().status, local_map_result(b["urec"])
            # arm c's store grows past what max_local holds of it (every inserted keyframe sees the tracked points, so
            # all of them are local): from then on UpdateLocalMap reports status 2 and the local stage does not run
            assert rc == 0 and (st == 0 or mode == "c"), (rc, st)
            info[mode] = dict(last_frame_status=st, last_update_status=up.status, last_n_local=up.n_local, last_n_local_kf=up.n_local_kf)
            if store is not None:
                v = store.view()
                rec = b["irec"].read()
                info[mode].update(view_points=v.points.n, view_kf=v.n_kf, **store.counts())
                if mode in "bce":
                    info[mode]["last_insert"] = dict(status=rec.status, inserted=rec.inserted, n_map=rec.n_map, n_cur=rec.n_cur)
                store.free()
            return dt / n * 1e6
        return run

    arms = {m: make_round(m) for m in "abcde"}

    def one_insertion(n):
        """min(n, INSERTS_PER_ROUND) times: one frame of arm a (untimed: it leaves a tracked frame's slots and gids),
        then ONE LORB_KF_GATE_NONE insertion of that frame and the wait for it, timed together -> the median, us."""
        b = bufs["a"]
        store = new_store()
        t = []
        for _ in range(min(n, inserts)):
            rc = frame(b, lmap_static, static.c) | L.lorb_sync(h)
            t0 = time.perf_counter()
            rc |= insert(b, store, A.LORB_KF_GATE_NONE)
            rc |= L.lorb_sync(h)
            t.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0
        rec = b["irec"].read()
        assert rec.status == 0 and rec.inserted == 1, (rec.status, rec.inserted)
        info["one_insertion"] = dict(insertions=len(t), n_cur=rec.n_cur, n_map=rec.n_map, n_observed=rec.n_observed,
                                     n_adopted=rec.n_adopted, n_created=rec.n_created, n_connected=rec.n_connected, **store.counts())
        store.free()
        return statistics.median(t)

    def cleanup():
        for x in held:
            x.free()
        fb.close()

    if expose is not None:
        expose.update(fp=fp, fps=fps, init=init, caps=caps, bufs=bufs, frame=frame, insert=insert, static=static,
                      lmap_static=lmap_static, lmap_grow=lmap_grow, model_I=model_I, keep=keep, opt=opt, fa=fa, last_gid=d_last_gid)
    base = dict(n_last=n_last, bound=BOUND, max_local=MAX_LOCAL, store_points=N_POINTS, store_keyframes=N_KF, caps=caps,
                inserts_per_round=inserts, every=EVERY)
    return arms, one_insertion, info, base, cleanup


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.calls >= 100, "protocol: >= 5 repeats of >= 100 calls"

    ctx = Context(0)
    arms, one_insertion, info, base, cleanup = build_arms(ctx, args.calls)
    names = list("abcde")
    arms["a"](args.warmup)  # arm a's slots are the tracked frame one_insertion inserts
    one_insertion(args.calls)
    for a in names:
        arms[a](args.warmup)
    samples = {a: [] for a in names}
    single = []
    for _ in range(args.repeats):
        for a in names:  # interleaved: every round times every arm
            samples[a].append(arms[a](args.calls))
        single.append(one_insertion(args.calls))
    rec = dict(tool="tools/bench_kf_insert.py", repeats=args.repeats, calls_per_repeat=args.calls, warmup=args.warmup,
               unit="us per frame (arms), us per insertion (one_insertion)",
               workload="synth.stereo_pair(%d, %d, %d) -> the same, shift 2, noise seed 777; %d features, %d levels" %
               (SEED, ROWS, COLS, NFEATURES, N_LEVELS), **base, state=info, arms={})
    for a in names:
        v = samples[a]
        rec["arms"][a] = dict(median=statistics.median(v), min=min(v), max=max(v), samples=v)
    rec["one_insertion"] = dict(median=statistics.median(single), min=min(single), max=max(single), samples=single)
    m = {a: rec["arms"][a]["median"] for a in names}
    rec["comparison"] = dict(b_minus_a=m["b"] - m["a"], c_minus_a=m["c"] - m["a"], d_minus_a=m["d"] - m["a"], e_minus_d=m["e"] - m["d"],
                             e_minus_d_percent_of_frame=100.0 * (m["e"] - m["d"]) / m["d"],
                             a_spread=rec["arms"]["a"]["max"] - rec["arms"]["a"]["min"])
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
