"""GPU: in the chain a compaction is invisible up to the index map.

The scene and the first steps are tests/test_gpu_kf_cull.py's chain: K1 creates twelve points, two frames see some of
them, then observe -> insert -> cull -> local BA for K2, where six points are culled by the observation rule and two by
the ratio.  It goes on:
  [compact, with the gid tables of the current frame (K2's, the one that becomes the last frame) and of the frame the
   tracker still keeps from before (frames 21 / 22, which hold c0 and c1 -- culled, so the table HOLDS them)]
  the next frame, id 25, on the last frame's slots and gids as the motion stage hands them on: UpdateLocalMap,
  observe, ids back
  K3 = that frame: insert -> cull -> local BA.
This scene has no images; the stages that need a built frame (motion, refer, the local stage, pose finish) run behind
a compaction in tests/test_gpu_kf_compact_loop.py, on built frames, with all seven calls of a frame.

Arms: with and without the compaction; with a wait after every call, and with none until the end.  Everything the
runs leave is equal once the indices of the run WITHOUT are sent through d_map (points made after the compaction
are numbered from the new count): records, slots, gids, local ids, the local map, the BA window, and every store,
geometry and life array -- rows float for float as bytes, indices through the map.  The one result that depends on a
point's absolute index is a count: lorb_kf_insert_result.n_points, which is smaller by the rows dropped.

A separate case gives the store one point row too few for K3 without the compaction: status 2 there, inserted with
it."""
import ctypes as C

import numpy as np
import pytest

import kf_ba_cases as BC
import kf_cull_cases as CC
import kf_store_cases as KC
import kf_store_ref as R
import test_gpu_kf_ba as KB
import test_gpu_kf_cull as CU
import test_gpu_kf_store as KS
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, KeyframeStore, LocalMap, _sentinel, keyframe_ba_record, keyframe_ba_result,
                                 keyframe_compact_record, keyframe_compact_result, keyframe_cull, keyframe_cull_record,
                                 keyframe_cull_result, keyframe_insert, keyframe_insert_result, keyframe_local_ba, keyframe_observe,
                                 keyframe_observe_record, keyframe_observe_result, local_map_buffers, local_map_ids_back,
                                 local_map_result, local_map_update)

pytestmark = pytest.mark.gpu

G, FILL = KS.G, KS.FILL
raw = KS.raw
POSE6_K3 = np.array([0.03, -0.02, 0.01, 0.25, -0.15, 1.4], np.float32)
MAX_LOCAL = 1024


def k3_case(k2):
    """The frame after K2: K2's keypoints moved a little, depth on the two slots K2's cull emptied (they create)."""
    n = k2["n_cur"]
    k3 = dict(k2, frame={k: v.copy() for k, v in k2["frame"].items()})
    k3["frame"]["x"] = (k3["frame"]["x"] + np.float32(1.5)).astype(np.float32)
    k3["frame"]["depth"][n - 6:n - 4] = [2.5, 3.5]
    return k3


class Arm(CU.ChainArm):
    """CU.ChainArm with the objects of the steps behind K2's local BA."""

    def __init__(self, ctx, sc, compact, wait, max_points=None):
        super().__init__(ctx, sc)
        self.compact_it, self.wait = compact, wait
        # the scene's capacities end with K2: a store with room for K3's observations and slots (max_points: the
        # scene's, or the given one), and the set-up once more on it
        n3 = self.k2["n_max_cur"] + 20
        c = self.k2["caps"]
        self.caps = dict(c, max_obs=c["max_obs"] + n3, max_kf_slots=c["max_kf_slots"] + n3,
                         max_points=c["max_points"] if max_points is None else max_points)
        self.store.free()
        s, c = sc["store"], self.caps
        self.store = KeyframeStore(ctx, c["max_kf"], c["max_points"], c["max_obs"], c["max_kf_slots"], init=s, geom=sc["geom"])
        cn = R.counts(s)
        self.store.fill(cn)
        self.store.fill_geometry(cn)
        self.store.fill_life(cn)
        for a in self.s1.values():
            a.free()
        self.s1 = self.step(self.k1, KB.POSE6)
        self.no.observe(ctx, self.store, 20)
        self.insert(self.s1, self.k1)
        for fid in (21, 22):
            d = self.seen_dev
            keyframe_observe(ctx, self.store, fid, d["frame"], d["slots"], d["gid"], d["lid"], self.view, d["update"], d["in_view"],
                             self.orec, n_max_cur=self.seen["n_max_cur"])
        ctx.sync()
        assert keyframe_insert_result(self.s1["rec"]).n_created == CC.N_CREATED
        self.finish_init()

    def finish_init(self):
        ctx = self.ctx
        self.k3 = k3_case(self.k2)
        nmax = self.k3["n_max_cur"]
        caps = self.caps
        self.frame3 = KS.Frame(ctx, self.k3)
        self.pose3 = DeviceBlock(ctx, A.FramePose, KB.pose_value(self.k3["pose"], POSE6_K3))
        self.irec3 = _sentinel(ctx, KS.REC + G, np.uint8)
        self.crec3, self.brec3, self.orec3 = keyframe_cull_record(ctx), keyframe_ba_record(ctx), keyframe_observe_record(ctx)
        self.mrec = keyframe_compact_record(ctx)
        self.dmap = ctx.to_device(np.full(caps["max_points"] + G, FILL, np.int32))
        unused, self.sid, self.urec = local_map_buffers(ctx, nmax, None, FILL)
        unused.free()
        self.lmap = LocalMap(ctx, MAX_LOCAL, caps["max_kf"], caps["max_points"])
        self.lmap.fill()
        self.in_view = ctx.to_device((np.arange(MAX_LOCAL) % 3 != 0).astype(np.uint8))

    def sync(self):
        if self.wait:
            self.ctx.sync()

    def run(self, upto_insert=False):
        ctx, s2, k3 = self.ctx, self.s2, self.k3
        nmax = k3["n_max_cur"]
        for call in (self.observe_k2, self.insert_k2, self.cull, self.local_ba):
            call()
            self.sync()
        irec2 = s2["rec"].ptr.value
        if self.compact_it:
            d = self.seen_dev
            self.store.compact(self.mrec, tables=[(s2["gid"], s2["frame"].out.counts, self.k2["n_max_cur"]),
                                                  (d["gid"], d["frame"].out.counts, self.seen["n_max_cur"])],
                               d_src_status=irec2 + A.KfInsertResult.status.offset, d_map=self.dmap)
            self.sync()
        # frame 25 on the last frame's slots and gids
        local_map_update(ctx, self.lmap, self.store, self.frame3, s2["slots"], s2["gid"], self.sid, self.urec, n_max_cur=nmax)
        self.sync()
        keyframe_observe(ctx, self.store, 25, self.frame3, s2["slots"], s2["gid"], self.sid, self.lmap, self.urec, self.in_view,
                         self.orec3, n_max_cur=nmax)
        self.sync()
        local_map_ids_back(ctx, self.lmap, self.frame3, s2["slots"], self.sid, s2["gid"], n_max_cur=nmax)
        self.sync()
        # K3
        keyframe_insert(ctx, self.store, k3["fp"], self.frame3, s2["slots"], s2["gid"], self.pose3, self.irec3, n_max_cur=nmax,
                        gate=R.GATE_NONE)
        self.sync()
        if upto_insert:
            ctx.sync()
            return
        ir = self.irec3.ptr.value
        d_kf, d_st = ir + A.KfInsertResult.kf.offset, ir + A.KfInsertResult.status.offset
        keyframe_cull(ctx, self.store, d_kf, self.crec3, d_src_status=d_st, params=CC.CHAIN_PARAMS, cur=self.frame3, cur_slots=s2["slots"],
                      slot_gid=s2["gid"], n_max_cur=nmax)
        self.sync()
        keyframe_local_ba(ctx, self.store, self.sc["fp"], d_kf, self.brec3, d_src_status=d_st)
        ctx.sync()

    def read(self):
        """Everything the run left (waits)."""
        st = self.store
        out = dict(counts=st.counts(), arrays=CU.all_arrays(st), store=st.read(), slots=self.s2["slots"].numpy(),
                   gid=self.s2["gid"].numpy(), seen_gid=self.seen_dev["gid"].numpy(), sid=self.sid.numpy(), lmap=self.lmap.numpy(),
                   dmap=self.dmap.numpy(), pose3=self.pose3.numpy())
        out["rec"] = dict(insert2=keyframe_insert_result(self.s2["rec"]), cull2=keyframe_cull_result(self.crec),
                          ba2=keyframe_ba_result(self.brec), update=local_map_result(self.urec),
                          observe=keyframe_observe_result(self.orec3), insert3=keyframe_insert_result(self.irec3),
                          cull3=keyframe_cull_result(self.crec3), ba3=keyframe_ba_result(self.brec3),
                          compact=keyframe_compact_result(self.mrec))
        out["window"] = st.ba_window(out["rec"]["ba3"]) if out["rec"]["ba3"].status == 0 else None
        return out

    def free(self):
        for a in (self.frame3, self.pose3, self.irec3, self.crec3, self.brec3, self.orec3, self.mrec, self.dmap, self.sid, self.urec,
                  self.lmap, self.in_view):
            a.free()
        super().free()


def fields(rec, but=()):
    return {f: getattr(rec, f) for f, _ in rec._fields_ if f not in but}


def same_bytes(a, b, what=""):
    """Two runs of the same arm: every array, table and record byte for byte."""
    for k in a["arrays"]:
        assert np.array_equal(raw(a["arrays"][k]), raw(b["arrays"][k])), (what, k)
    for k in ("gid", "seen_gid", "sid", "dmap", "pose3"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in a["slots"]:
        assert np.array_equal(raw(a["slots"][k]), raw(b["slots"][k])), (what, k)
    for k in a["lmap"]:
        assert np.array_equal(raw(a["lmap"][k]), raw(b["lmap"][k])), (what, k)
    for k in a["rec"]:
        assert bytes(a["rec"][k]) == bytes(b["rec"][k]), (what, k)
    assert a["counts"] == b["counts"]


def full_map(with_, without):
    """old -> new over every point the run WITHOUT the compaction ends with: d_map below the count at the compaction,
    the points made afterwards numbered from the new count."""
    c = with_["rec"]["compact"]
    P_old, P_new, P_b = c.n_points_before, c.n_points, without["counts"]["n_points"]
    assert P_old == without["rec"]["insert2"].n_points == with_["rec"]["insert2"].n_points and P_new == P_old - c.n_dropped
    m = np.concatenate([with_["dmap"][:P_old], P_new + np.arange(P_b - P_old)]).astype(np.int32)
    assert (with_["dmap"][P_old:] == FILL).all()
    return m


def through(m, idx):
    """Index array `idx` of the run without, sent through the map (-1 and indices outside stay)."""
    idx = np.asarray(idx)
    out = idx.copy()
    ok = (idx >= 0) & (idx < len(m))
    out[ok] = m[idx[ok]]
    return out


def same_up_to_the_map(a, b):
    """a: the run with the compaction, b: the run without."""
    m = full_map(a, b)
    keep = m >= 0
    ca, cb = a["counts"], b["counts"]
    n_drop = a["rec"]["compact"].n_dropped
    assert n_drop > 0 and ca["n_points"] == cb["n_points"] - n_drop == int(keep.sum())
    assert {k: v for k, v in ca.items() if k != "n_points"} == {k: v for k, v in cb.items() if k != "n_points"}
    Pa, Pb = ca["n_points"], cb["n_points"]
    A_, B_ = a["arrays"], b["arrays"]
    # the rows, float for float as bytes; a dropped point is bad, unobserved and in no row
    for k in ("pos", "normal", "max_dist", "min_dist", "desc", "locked", "is_bad", "life_visible", "life_found", "life_first_fid",
              "life_recent"):
        assert np.array_equal(raw(A_[k][:Pa]), raw(B_[k][:Pb][keep])), k
    assert a["store"]["obs"] == [o for p, o in enumerate(b["store"]["obs"]) if keep[p]]
    assert all(b["store"]["is_bad"][p] and not b["store"]["obs"][p] for p in np.nonzero(~keep)[0])
    no = ca["n_obs"]
    for k in ("obs_kf", "obs_slot"):
        assert np.array_equal(A_[k][:no], B_[k][:no]), k
    # the indices through the map
    ns = ca["n_kf_slots"]
    assert np.array_equal(A_["kf_slot_point"][:ns], through(m, B_["kf_slot_point"][:ns]))
    assert not set(int(g) for g in B_["kf_slot_point"][:ns] if g >= 0) & set(int(p) for p in np.nonzero(~keep)[0])
    # what has no point index in it
    nk = ca["n_kf"]
    for k, n in (("kf_bad", nk), ("kf_slot_off", nk + 1), ("cov_off", nk + 1), ("cov_kf", ca["n_cov"]), ("kf_pose", nk), ("kf_slot_uv", ns),
                 ("life_kf_fid", nk), ("life_frame_word", 1)):
        assert np.array_equal(raw(A_[k][:n]), raw(B_[k][:n])), k
    assert a["store"]["conn"] == b["store"]["conn"]
    # the tracker's objects
    for k in a["slots"]:
        assert np.array_equal(raw(a["slots"][k]), raw(b["slots"][k])), k
    assert np.array_equal(a["gid"], through(m, b["gid"])) and np.array_equal(a["seen_gid"], through(m, b["seen_gid"]))
    assert np.array_equal(a["sid"], b["sid"]) and np.array_equal(a["pose3"], b["pose3"])
    # the local map of frame 25: the table in ascending point order, which the map preserves
    ua, ub = a["rec"]["update"], b["rec"]["update"]
    assert fields(ua) == fields(ub) and ua.status == 0 and ua.n_local > 0
    la, lb = a["lmap"], b["lmap"]
    nl = ua.n_local
    assert np.array_equal(la["l2g"][:nl], through(m, lb["l2g"][:nl])) and (through(m, lb["l2g"][:nl]) >= 0).all()
    assert np.array_equal(la["g2l"][:Pa], lb["g2l"][:Pb][keep]) and (lb["g2l"][:Pb][~keep] == -1).all()
    for k in la:
        if k not in ("l2g", "g2l"):
            assert np.array_equal(raw(la[k]), raw(lb[k])), k
    # the records: equal, but for the one count that is a point index
    ra, rb = a["rec"], b["rec"]
    for k in ("insert2", "cull2", "ba2", "observe", "cull3", "ba3"):
        assert bytes(ra[k]) == bytes(rb[k]), k
    assert fields(ra["insert3"], but=("n_points",)) == fields(rb["insert3"], but=("n_points",))
    assert ra["insert3"].n_points == rb["insert3"].n_points - n_drop == Pa
    assert ra["insert3"].status == 0 and ra["insert3"].inserted == 1 and ra["insert3"].n_created >= 2
    assert ra["cull3"].status == 0 and ra["ba3"].status == 0 and ra["ba3"].written == 1
    # K3's window
    wa, wb = a["window"], b["window"]
    assert np.array_equal(wa["l2g"], through(m, wb["l2g"]))
    for k in wa:
        if k not in ("l2g", "intr"):
            assert np.array_equal(raw(np.asarray(wa[k])), raw(np.asarray(wb[k]))), k


def test_compaction_is_invisible_up_to_the_map(ctx):
    sc = BC.chain_scene()
    arms = {(c, w): Arm(ctx, sc, c, w) for c in (True, False) for w in (True, False)}
    try:
        out = {}
        for key, arm in arms.items():
            arm.run()
            out[key] = arm.read()
        # non-vacuity: eight points were culled at K2; c0 and c1 are still in the kept frame's table, so six go
        c = out[True, False]["rec"]["compact"]
        created = arms[True, False].created
        assert c.status == 0 and c.n_dropped == 6 and c.n_bad_kept >= 2 and c.n_gids_mapped > 0 and c.n_kf_slots_mapped > 0
        dmap = out[True, False]["dmap"]
        assert all(dmap[p] == -1 for p in created[6:]) and all(dmap[p] >= 0 for p in created[:6])
        assert (dmap[:created[6]] == np.arange(created[6])).all() and (dmap[created[-1] + 1:c.n_points_before] >= created[6]).all()
        assert out[False, False]["rec"]["compact"].status == KS.SENT_I32          # never called
        assert out[True, False]["rec"]["insert3"].n_created == 2
        same_bytes(out[True, False], out[True, True], "with, no wait / waits")
        same_bytes(out[False, False], out[False, True], "without, no wait / waits")
        same_up_to_the_map(out[True, False], out[False, False])
        same_up_to_the_map(out[True, True], out[False, True])
    finally:
        for arm in arms.values():
            arm.free()


def test_reclaimed_rows_are_usable_at_once(ctx):
    """K3 makes two points.  With max_points = the count after K2 + 1, the insertion answers status 2 without the
    compaction; behind it the six reclaimed rows are there and the same call inserts."""
    sc = BC.chain_scene()
    P2 = sc["store"]["n_points"] + CC.N_CREATED + sum(1 for st in sc["case"]["slots"]["state"] if st == KC.FREE)
    arms = {c: Arm(ctx, sc, c, False, max_points=P2 + 1) for c in (False, True)}
    try:
        got = {}
        for c, arm in arms.items():
            arm.run(upto_insert=True)
            got[c] = (keyframe_insert_result(arm.s2["rec"]), keyframe_insert_result(arm.irec3), arm.store.counts())
        for c in got:
            assert got[c][0].status == 0 and got[c][0].inserted == 1 and got[c][0].n_points == P2
        without, with_ = got[False][1], got[True][1]
        assert without.status == 2 and without.inserted == 0 and without.n_created == 2 and got[False][2]["n_points"] == P2
        assert with_.status == 0 and with_.inserted == 1 and with_.n_created == 2 and with_.n_points == P2 - 6 + 2
        assert got[True][2]["n_points"] == P2 - 4 and got[True][2]["n_kf"] == got[False][2]["n_kf"] + 1
    finally:
        for arm in arms.values():
            arm.free()
