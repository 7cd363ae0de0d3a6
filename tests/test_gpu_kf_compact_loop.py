"""GPU: a compaction between two WHOLE tracked frames is invisible up to the index map.

Built frames: tests/test_gpu_track_refer.py's whole loop (TLF.scene(): image B tracked against A, then A against B;
frame 1's first motion attempt fails, so its second attempt runs on the refer frame and takes its gids from
d_refer_slot_gid) on a KeyframeStore made from tests/test_gpu_local_map_chain.py's map, with a consistent geometry
and five dead rows among its first points.  Per frame all of: motion, refer, UpdateLocalMap, the local stage,
observe, ids back, pose finish -- then the frame becomes a keyframe: insert -> cull -> local BA.  Between K2's local BA
and frame 2's motion stage:
  [compact, with the gid tables of frame 1 (it becomes d_last), of the refer frame and of frame 0]
so lorb_track_motion_refer_pose_dev reads rewritten tables as d_last_slot_gid / d_refer_slot_gid, and
lorb_local_map_update_dev, the local stage and lorb_local_map_ids_back_dev run on a compacted store.

Arms: with and without the compaction; a wait after every call, and none until the end.  With and without waits the
runs are equal byte for byte.  With and without the compaction they are equal once the indices of the run without
are sent through d_map (points made afterwards numbered from the new count): every record, assignment, pose and model
block and slot set of every frame as bytes, every gid table and l2g through the map, g2l row for row, K3's BA window,
and every store, geometry and life array.  lorb_kf_insert_result.n_points of K3 is smaller by the rows dropped."""
import ctypes as C

import numpy as np
import pytest

import kf_cull_cases as CC
import kf_store_ref as R
import test_gpu_kf_compact_chain as CHN
import test_gpu_kf_cull as CU
import test_gpu_kf_store as KS
import test_gpu_local_map_chain as LMC
import test_gpu_track_frames as TR
import test_gpu_track_local_frames as TLF
import test_gpu_track_refer as TRF
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (KeyframeStore, LocalMap, _sentinel, keyframe_ba_record, keyframe_ba_result, keyframe_compact_record,
                                 keyframe_compact_result, keyframe_cull, keyframe_cull_record, keyframe_cull_result, keyframe_insert,
                                 keyframe_insert_result, keyframe_local_ba, keyframe_observe, keyframe_observe_record,
                                 keyframe_observe_result, local_map_ids_back, local_map_result, local_map_update, model_block,
                                 motion_record_addresses, track_local_frames)
from test_gpu_track_frames import builders  # noqa: F401 -- the module-scoped builder fixture

pytestmark = pytest.mark.gpu

G, FILL = KS.G, KS.FILL
raw, through, fields = KS.raw, CHN.through, CHN.fields
DEAD = (1, 3, 5, 12, 25)          # points of the map no frame holds: bad, unobserved, in no keyframe row
CULL_CREATED = (0.25, 0, 2, 3)    # every point an insertion creates has one observation: culled at once


def loop_store(S):
    """LMC.build_store's map as a KeyframeStore init with a geometry that reprojects its points at the identity pose,
    DEAD made what lorb_kf_store_cull_dev leaves behind."""
    s, last_gid = LMC.build_store(S)
    s["obs"] = [list(o) for o in s["obs"]]
    s["kf_slots"] = [[int(p) for p in row] for row in s["kf_slots"]]
    held = set(int(g) for g in last_gid if g >= 0)
    assert not held & set(DEAD)
    for p in DEAD:
        s["is_bad"][p] = 1
        s["obs"][p] = []
    s["kf_slots"] = [[-1 if p in DEAD else p for p in row] for row in s["kf_slots"]]
    s["conn"] = [{} for _ in s["kf_bad"]]
    g = CC.geometry_for(s, seed=5)
    fp = S["fp"]
    fx, fy, cx, cy = (float(fp[k]) for k in ("fx", "fy", "cx", "cy"))
    pos = np.asarray(s["pos"], np.float64)
    uv = []
    for row in s["kf_slots"]:
        r = np.asarray(row, np.int64)
        X = pos[np.maximum(r, 0)]
        z = np.where(np.abs(X[:, 2]) > 1e-6, X[:, 2], 1.0)
        u = np.stack([fx * X[:, 0] / z + cx, fy * X[:, 1] / z + cy], 1)
        u[r < 0] = 0
        uv.append(u.astype(np.float32))
    g["kf_slot_uv"], g["kf_pose"] = uv, [np.zeros(6, np.float32) for _ in uv]
    return s, g, last_gid


class Arm(TRF.ReferLoop):
    """TRF.ReferLoop on a KeyframeStore, the refer frame's gids real store indices, and the keyframe step's objects."""

    def __init__(self, ctx, bt, S, compact, wait):
        super().__init__(ctx, bt, S)
        self.compact_it, self.wait = compact, wait
        s, g, last_gid = loop_store(S)
        cn, N = R.counts(s), self.N
        self.store = self.dstore = KeyframeStore(ctx, cn["n_kf"] + 4, cn["n_points"] + 3 * N, cn["n_obs"] + 4 * N,
                                                 cn["n_kf_slots"] + 3 * N, init=s, geom=g)
        self.store.fill(cn)
        self.store.fill_geometry(cn)
        self.store.fill_life(cn)
        self.P0 = cn["n_points"]
        self.lmap = LocalMap(ctx, self.store.caps.max_points, self.store.caps.max_kf, self.store.caps.max_points)
        self.lmap.fill()
        self.refer_gid_h = np.asarray(last_gid, np.int32).copy()   # the refer frame is image A as well: the store's own indices
        self.refer_gid = ctx.to_device(TR.guarded(self.refer_gid_h, N))
        self.irec = [_sentinel(ctx, KS.REC + G, np.uint8) for _ in range(2)]
        self.crec, self.brec = [keyframe_cull_record(ctx) for _ in range(2)], [keyframe_ba_record(ctx) for _ in range(2)]
        self.orec = [keyframe_observe_record(ctx) for _ in range(2)]
        self.mrec = keyframe_compact_record(ctx)
        self.dmap = ctx.to_device(np.full(self.store.caps.max_points + G, FILL, np.int32))
        self.m1, self.m2 = model_block(ctx, TRF.shift(TRF.DX)), model_block(ctx, TRF.shift(TRF.DX))
        bt.held += [self.store, self.lmap, self.refer_gid, self.mrec, self.dmap, self.m1, self.m2, *self.irec, *self.crec, *self.brec,
                    *self.orec]

    def sync(self):
        if self.wait:
            self.ctx.sync()

    def frame(self, k, img, cur, last_img, last, model, prev_update):
        """All seven calls of one tracked frame, then the frame as a keyframe: insert -> cull -> local BA."""
        ctx, N, fp = self.ctx, self.N, self.fp
        self.motion(img, cur, last_img, last, model)
        self.sync()
        self.refer(img, cur, last, model, prev_update)
        self.sync()
        d_pose, d_mstatus = motion_record_addresses(cur.mrec)
        d_ustatus = local_map_update(ctx, self.lmap, self.store, img, cur.slots, cur.gid, cur.sid, cur.urec, n_max_cur=N,
                                     d_src_status=d_mstatus)
        self.sync()
        track_local_frames(ctx, fp, img, cur.slots, cur.sid, d_pose, self.lmap, out=cur.out, n_max_cur=N, d_src_status=d_ustatus,
                           th=TRF.TH, min_matches=TRF.LOCAL_MIN)
        self.sync()
        d_lstatus = cur.out.record.ptr.value + A.TrackLocalFramesResult.status.offset
        keyframe_observe(ctx, self.store, 30 + k, img, cur.slots, cur.gid, cur.sid, self.lmap, cur.urec, cur.out.in_view,
                         self.orec[k - 1], n_max_cur=N, d_local_status=d_lstatus)
        self.sync()
        local_map_ids_back(ctx, self.lmap, img, cur.slots, cur.sid, cur.gid, n_max_cur=N, d_local_status=d_lstatus)
        self.sync()
        self.finish(cur, last)
        self.sync()
        irec = self.irec[k - 1]
        keyframe_insert(ctx, self.store, fp, img, cur.slots, cur.gid, cur.pose, irec, n_max_cur=N, d_src_status=d_lstatus,
                        gate=R.GATE_NONE, refer_kf=self.kf, update_record=cur.urec)
        self.sync()
        d_kf, d_st = irec.ptr.value + A.KfInsertResult.kf.offset, irec.ptr.value + A.KfInsertResult.status.offset
        keyframe_cull(ctx, self.store, d_kf, self.crec[k - 1], d_src_status=d_st, params=CULL_CREATED, cur=img, cur_slots=cur.slots,
                      slot_gid=cur.gid, n_max_cur=N)
        self.sync()
        keyframe_local_ba(ctx, self.store, fp, d_kf, self.brec[k - 1], d_src_status=d_st)
        self.sync()
        return d_st

    def run(self):
        ctx, bt, S = self.ctx, self.bt, self.S
        fr = self.fr = [self.first(), self.new(), self.new()]
        img = {0: bt.fa}
        for k, c in ((1, S["cb"]), (2, S["ca"])):
            img[k] = bt.b.build_device(c["left"], c["right"])
            bt.held.append(img[k])
        d_st = self.frame(1, img[1], fr[1], img[0], fr[0], self.m1, self.no_update)
        if self.compact_it:
            N = self.N
            self.store.compact(self.mrec, tables=[(fr[1].gid, img[1].out.counts, N), (self.refer_gid, bt.fa.out.counts, N),
                                                  (fr[0].gid, bt.fa.out.counts, N)], d_src_status=d_st, d_map=self.dmap)
            self.sync()
        self.frame(2, img[2], fr[2], img[1], fr[1], self.m2, fr[1].urec)
        ctx.sync()

    def read(self):
        st = self.store
        out = dict(counts=st.counts(), arrays=CU.all_arrays(st), store=st.read(), frames=[f.read() for f in self.fr],
                   objects=self.objects(), refer_gid=self.refer_gid.numpy(), rrec=[r.numpy() for r in self.rrecs], lmap=self.lmap.numpy(),
                   dmap=self.dmap.numpy())
        out["rec"] = dict(compact=keyframe_compact_result(self.mrec))
        for k in (1, 2):
            out["rec"].update({"insert%d" % (k + 1): keyframe_insert_result(self.irec[k - 1]), "cull%d" % (k + 1): keyframe_cull_result(self.crec[k - 1]),
                               "ba%d" % (k + 1): keyframe_ba_result(self.brec[k - 1]), "observe%d" % k: keyframe_observe_result(self.orec[k - 1]),
                               "update%d" % k: local_map_result(self.fr[k].urec)})
        out["window"] = st.ba_window(out["rec"]["ba3"]) if out["rec"]["ba3"].status == 0 else None
        # the shape CHN.same_up_to_the_map takes: frame 2 is "the next frame"
        f2 = out["frames"][2]
        out.update(slots={k[6:]: v for k, v in f2.items() if k.startswith("slots_")}, gid=f2["gid"], seen_gid=out["refer_gid"], sid=f2["sid"],
                   pose3=f2["pose"])
        out["rec"].update(update=out["rec"]["update2"], observe=out["rec"]["observe2"])
        return out


def same_bytes(a, b, what):
    CHN.same_bytes(a, b, what)
    for fa, fb in zip(a["frames"], b["frames"]):
        for k in fa:
            assert np.array_equal(raw(fa[k]), raw(fb[k])), (what, k)
    for k in a["objects"]:
        assert np.array_equal(raw(a["objects"][k]), raw(b["objects"][k])), (what, k)
    for x, y in zip(a["rrec"], b["rrec"]):
        assert np.array_equal(x, y), what
    assert bytes(a["rec"]["observe1"]) == bytes(b["rec"]["observe1"]) and bytes(a["rec"]["update1"]) == bytes(b["rec"]["update1"])


def test_two_whole_frames_with_and_without_a_compaction(ctx, builders):
    S = TLF.scene()
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        out, P0 = {}, None
        for key in ((True, False), (True, True), (False, False), (False, True)):
            arm = Arm(ctx, bt, S, *key)
            arm.run()
            out[key] = arm.read()
            P0 = arm.P0
    a, b = out[True, False], out[False, False]
    # non-vacuity: both frames tracked and became keyframes; the second attempt of frame 1 ran on the refer frame; points
    # were created and culled; the dead rows of the map and the culled points went, so every index above the first moved
    c = a["rec"]["compact"]
    i2, i3 = a["rec"]["insert2"], a["rec"]["insert3"]
    assert TRF.refer_record(dict(rrec=a["rrec"][0]))[:3] == (1, 1, 0)
    for k in (1, 2):
        f = a["frames"][k]
        mrec = A.TrackFramesResult.from_buffer_copy(f["mrec"].tobytes()[:TRF.MREC])
        lrec = A.TrackLocalFramesResult.from_buffer_copy(f["lrec"].tobytes()[:C.sizeof(A.TrackLocalFramesResult)])
        assert mrec.status == 0 and mrec.motion.pass_ != 0 and lrec.status == 0, (k, mrec.status, mrec.motion.pass_, lrec.status)
    assert i2.status == 0 and i2.inserted == 1 and i2.n_created > 0 and i2.n_observed > 0
    culled = a["rec"]["cull2"].n_culled_obs + a["rec"]["cull2"].n_culled_ratio
    assert culled >= i2.n_created
    assert c.status == 0 and c.n_points_before == i2.n_points and c.n_dropped == len(DEAD) + culled
    assert c.n_gids_mapped > 0 and c.n_kf_slots_mapped > 0
    dmap = a["dmap"]
    assert all(dmap[p] == -1 for p in DEAD) and dmap[0] == 0 and dmap[P0 - 1] == P0 - 1 - len(DEAD)
    assert i3.status == 0 and i3.inserted == 1 and i3.n_observed > 0
    assert b["rec"]["compact"].status == KS.SENT_I32                      # never called
    same_bytes(out[True, False], out[True, True], "with, no wait / waits")
    same_bytes(out[False, False], out[False, True], "without, no wait / waits")
    for a, b in ((out[True, False], out[False, False]), (out[True, True], out[False, True])):
        CHN.same_up_to_the_map(a, b)
        m = CHN.full_map(a, b)
        # every frame: the gids through the map, everything else as bytes
        for k, (fa, fb) in enumerate(zip(a["frames"], b["frames"])):
            for key in fa:
                if key == "gid":
                    assert np.array_equal(fa[key], through(m, fb[key])), (k, key)
                elif key == "urec":
                    assert fields(A.LocalMapResult.from_buffer_copy(fa[key].tobytes()[:C.sizeof(A.LocalMapResult)])) == \
                        fields(A.LocalMapResult.from_buffer_copy(fb[key].tobytes()[:C.sizeof(A.LocalMapResult)])), k
                else:
                    assert np.array_equal(raw(fa[key]), raw(fb[key])), (k, key)
        assert np.array_equal(a["refer_gid"], through(m, b["refer_gid"])) and not np.array_equal(a["refer_gid"], b["refer_gid"])
        for key in a["objects"]:
            assert np.array_equal(raw(a["objects"][key]), raw(b["objects"][key])), key
        for x, y in zip(a["rrec"], b["rrec"]):
            assert np.array_equal(x, y)
        for key in ("observe1", "update1"):
            assert bytes(a["rec"][key]) == bytes(b["rec"][key]), key
