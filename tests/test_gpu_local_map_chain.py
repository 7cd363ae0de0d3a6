"""GPU: one tracked frame with the reference's own local map as five enqueued calls and ONE wait --
lorb_frame_build_dev (the builder fixture's frames), lorb_track_motion_frames_dev,
lorb_local_map_update_dev, lorb_track_local_frames_dev, lorb_local_map_ids_back_dev -- against the two-wait
composition in which the host waits after the motion stage, runs the restatement of UpdateLocalMap
(tests/local_map_ref.py), uploads the slot states, the local ids and the local table, and calls
lorb_track_local_frames_dev on them.  Bit for bit: slots, both id arrays, assign, the tracking fields and
the record.

The scene is tests/test_gpu_track_local_frames.py's (case "320x256", dx = 0.1, frame A INITIALIZE-filled).
The store holds A's initialised points behind 40 inert ones (so global and local indices differ) under
five keyframes: kf0 (the resident last frame) and kf1 are voted, kf2 has the most votes but is bad, kf3
comes in through the expansion (kf0's covisibles: kf2 bad, kf1 listed, kf3), kf4 never becomes local.  The
points k % 5 == 0 sit only in kf2 and kf4: slots that hold them are held but not local.  The points
k % 7 == 3 are bad: slots that hold them are emptied."""
import ctypes as C

import numpy as np
import pytest

import local_map_ref as R
import lorb_slam_amd.window as W
import test_gpu_track_frames as TR
import test_gpu_track_local_frames as TLF
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceMapStore, DevicePoints, LocalFramesOut, LocalMap, enqueue_track_motion_frames,
                                 fill_slots, local_map_buffers, local_map_ids_back, local_map_result, local_map_update,
                                 motion_record_addresses, track_local_frames)
from lorb_slam_amd.runtime import lib
from test_gpu_track_frames import builders  # noqa: F401 -- the module-scoped builder fixture

pytestmark = pytest.mark.gpu

G, SENT, FILL, I4 = W.ORB_GUARD, W.ORB_SENTINEL, TR.FILL, TR.I4
EMPTY = A.LORB_SLOT_EMPTY
N_EXTRA, TH = 40, 2.0


def build_store(S):
    """(store dict, the last frame's global slot ids)."""
    pts = S["pts"]
    n0 = len(pts["pos"])
    n = N_EXTRA + n0
    k = np.arange(n0)
    g = k + N_EXTRA
    cat = lambda a, b: np.concatenate([a, b])  # noqa: E731
    store = dict(n_points=n,
                 pos=cat(np.tile(np.array([[0.5, -0.5, -6.0]], np.float32), (N_EXTRA, 1)), pts["pos"]),
                 normal=cat(np.tile(np.array([[0, 0, -1]], np.float32), (N_EXTRA, 1)), pts["normal"]),
                 max_dist=cat(np.full(N_EXTRA, 12, np.float32), pts["max_dist"]),
                 min_dist=cat(np.full(N_EXTRA, 2, np.float32), pts["min_dist"]),
                 desc=cat(np.full((N_EXTRA, 32), 0x5a, np.uint8), pts["desc"]),
                 locked=cat(np.zeros(N_EXTRA, np.uint8), pts["locked"]),
                 is_bad=cat(np.zeros(N_EXTRA, np.uint8), (k % 7 == 3).astype(np.uint8)),
                 kf_bad=np.array([0, 0, 1, 0, 0], np.uint8))
    store["obs"] = [[3] if e < 20 else [4] for e in range(N_EXTRA)] + [[0] + ([1] if i % 2 == 0 else []) + [2] for i in k]
    store["kf_slots"] = [list(g[k % 5 != 0]) + [-1, -1],
                         [-1] + list(g[(k % 2 == 0) & (k % 5 != 0)]) + list(range(10)),
                         list(g),
                         list(range(10, 20)) + list(g[k % 10 == 6]),
                         list(range(20, 40)) + list(g[k % 5 == 0])]
    store["cov"] = [[2, 1, 3], [0], [], [0, 1], []]
    last_gid = np.where(S["last_id"] >= 0, S["last_id"] + N_EXTRA, -1).astype(np.int32)
    return store, last_gid


def h2d(ctx, dev, host):
    host = np.ascontiguousarray(host)
    ctx.check(lib().lorb_memcpy_h2d(ctx.handle, dev.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)), "h2d")


def test_chain_equals_host_composition(ctx, builders):
    S = TLF.scene()
    fp, n_cur = S["fp"], S["n_cur"]
    nc, nl = n_cur + 1, S["n_last"] + 1
    store, last_gid = build_store(S)
    max_local = store["n_points"] - 3
    pi, T = TR.prediction(TLF.DX)
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        dstore = DeviceMapStore(ctx, store, store["obs"], store["kf_bad"], store["kf_slots"], store["cov"])
        lmap = LocalMap(ctx, max_local, 8, store["n_points"] + 5)
        dlast = ctx.to_device(TR.guarded(last_gid, nl))
        bt.held += [dstore, lmap, dlast]

        def motion():
            """Fresh slot sets, the motion stage enqueued: (cur slots, assign, record)."""
            ls = bt.slots(nl, TR.entry_slots(nl))
            fill_slots(ctx, fp, I4, bt.fa, ls, A.LORB_SLOTS_INITIALIZE)
            cs = bt.slots(nc, TR.entry_slots(nc))
            masg = ctx.to_device(np.full(nc + G, FILL, np.int32))
            mrec = ctx.to_device(np.full(C.sizeof(A.TrackFramesResult), SENT, np.uint8))
            bt.held += [masg, mrec]
            enqueue_track_motion_frames(ctx, fp, T, pi, bt.fb, cs, I4, bt.fa, ls, masg, mrec)
            return cs, masg, mrec

        def outputs(out, cs, sid):
            return dict(rec=out.record.numpy(), assign=out.assign.numpy(), in_view=out.in_view.numpy(), track=out.track.numpy(),
                        level=out.level.numpy(), slots=cs.numpy(), sid=sid.numpy())

        # the chain: five enqueued calls (the frames were built by the fixture), one wait
        cs, masg, mrec = motion()
        d_pose, d_mstatus = motion_record_addresses(mrec)
        gid, sid, urec = local_map_buffers(ctx, nc, None, FILL)
        out = LocalFramesOut(ctx, lmap.n, nc, FILL)
        bt.held += [gid, sid, urec, out]
        ids = A.TrackLocalIdSource(masg.ptr.value, mrec.ptr.value, dlast.ptr.value, nl, 0)
        d_ustatus = local_map_update(ctx, lmap, dstore, bt.fb, cs, gid, sid, urec, n_max_cur=nc, d_src_status=d_mstatus,
                                     id_source=ids)
        track_local_frames(ctx, fp, bt.fb, cs, sid, d_pose, lmap, out=out, n_max_cur=nc, d_src_status=d_ustatus, th=TH)
        local_map_ids_back(ctx, lmap, bt.fb, cs, sid, gid, n_max_cur=nc,
                           d_local_status=out.record.ptr.value + A.TrackLocalFramesResult.status.offset)
        a = outputs(out, cs, sid)  # the first fetch is the wait
        a.update(gid=gid.numpy(), urec=local_map_result(urec), lmap=lmap.numpy(), mrec=mrec.numpy(), masg=masg.numpy())

        # the composition: wait, host UpdateLocalMap, upload, local stage, wait, host ids_back
        cs2, masg2, mrec2 = motion()
        ctx.sync()
        m_asg, m_rec = masg2.numpy(), A.TrackFramesResult.from_buffer_copy(mrec2.numpy().tobytes())
        assert TLF.same(mrec2.numpy(), a["mrec"]) and np.array_equal(m_asg, a["masg"]) and m_rec.status == 0
        st0 = cs2.state.numpy()
        ref = R.update_local_map(store, st0[:n_cur], np.full(n_cur, FILL, np.int32), n_cur, max_local,
                                 dict(assign=m_asg, pass_=m_rec.motion.pass_, given=0, last_gid=last_gid))
        assert ref["status"] == 0 and ref["local_kf"] == [0, 1, 3] and ref["refer_kf"] == 0 and ref["n_nulled"] >= 1
        nloc = ref["n_local"]
        assert 20 < nloc < max_local
        st0[:n_cur] = ref["state"]
        h2d(ctx, cs2.state, st0)
        sid2 = ctx.to_device(np.concatenate([ref["slot_id"], np.full(nc + G - n_cur, FILL, np.int32)]))
        table = dict(is_bad=np.ones(max_local, np.uint8))
        for k in R.COLS:
            table[k] = np.zeros((max_local,) + store[k].shape[1:], store[k].dtype)  # as lorb_local_map_create leaves them
            table[k][:nloc] = ref["rows"][k]
        table["is_bad"][:nloc] = 0
        dp = DevicePoints(ctx, table)
        out2 = LocalFramesOut(ctx, dp.n, nc, FILL)
        bt.held += [sid2, dp, out2]
        d_pose2, d_mstatus2 = motion_record_addresses(mrec2)
        track_local_frames(ctx, fp, bt.fb, cs2, sid2, d_pose2, dp, out=out2, n_max_cur=nc, d_src_status=d_mstatus2, th=TH)
        b = outputs(out2, cs2, sid2)
        gid2 = R.ids_back(b["slots"]["state"][:n_cur], b["sid"][:n_cur], ref["gid"], ref["l2g"])

    # the update stage against the restatement
    u = a["urec"]
    assert (u.status, u.n_cur, u.n_held, u.n_nulled, u.n_voted, u.n_local_kf, u.refer_kf, u.n_local) == \
        (0, n_cur, ref["n_held"], ref["n_nulled"], ref["n_voted"], 3, 0, nloc)
    assert list(a["lmap"]["l2g"][:nloc]) == ref["l2g"] and np.array_equal(a["lmap"]["g2l"][:store["n_points"]], ref["g2l"])
    for k in (*R.COLS, "is_bad"):
        assert TLF.same(a["lmap"][k], table[k]), k
    # the chain against the composition, bit for bit
    for k in ("state", "pos", "desc"):
        assert TLF.same(a["slots"][k], b["slots"][k]), k
    assert np.array_equal(a["sid"], b["sid"])
    assert np.array_equal(a["gid"][:n_cur], gid2) and (a["gid"][n_cur:] == FILL).all()
    assert np.array_equal(a["assign"], b["assign"]) and np.array_equal(a["in_view"], b["in_view"])
    iv = a["in_view"][:max_local] == 1
    assert TLF.same(a["track"][:4 * max_local].reshape(4, max_local)[:, iv], b["track"][:4 * max_local].reshape(4, max_local)[:, iv])
    assert np.array_equal(a["level"][:max_local][iv], b["level"][:max_local][iv])
    assert TLF.same(a["rec"], b["rec"])
    # the scene exercises what it is meant to
    rec = A.TrackLocalFramesResult.from_buffer_copy(a["rec"].tobytes()[:C.sizeof(A.TrackLocalFramesResult)])
    held, sidn = a["slots"]["state"][:n_cur] != EMPTY, a["sid"][:n_cur]
    assert rec.status == 0 and rec.local.nmatches > 0 and (a["assign"][:n_cur] >= 0).sum() > 0
    assert (held & (sidn < 0) & (gid2 >= 0)).sum() >= 1       # held points outside the local map kept their gid
    assert (held & (sidn >= 0)).sum() >= 20 and (gid2[held & (sidn >= 0)] == np.array(ref["l2g"])[sidn[held & (sidn >= 0)]]).all()
    assert not a["in_view"][nloc:max_local].any()             # the padding rows are never in view
