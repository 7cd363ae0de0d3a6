"""GPU: lorb_kf_store_refresh_dev in the mapper step, on tests/kf_ba_cases.py's chain_scene().

1. Forced insertion -> gather -> refresh: K's appearance rows are the frame's; every CREATED and every adopted point
   keeps normal, max_dist and min_dist bit for bit (one observation, the inputs of the insertion's new_point), a created
   one its descriptor too, an adopted one takes K's; every held point equals the restatement over its grown list.
2. Insertion -> lorb_kf_store_local_ba_dev -> refresh with all flags, nothing between the calls: n_centers is the
   window's poses; centres of fixed and outside keyframes keep their bits; every moved centre lies within
   2^-20 max(1, |t|_inf) of oracle.inv4_f32(oracle.pose_to_Tcw(kf_pose)); the points are bit-exact against the
   restatement fed with the centres read back; the next lorb_local_map_update_dev carries the refreshed rows.
3. A written-back rvec of exactly 0: the centre has the oracle's bits (Rodrigues' identity branch, no trig).
4. A refused insertion: the BA record says 1, the refresh writes its status and nothing else."""
import copy
import ctypes as C

import numpy as np
import pytest

import kf_ba_cases as BC
import kf_ba_ref as B
import kf_refresh_cases as RC
import kf_refresh_ref as RR
import kf_store_ref as R
import oracle as O
import test_gpu_kf_ba as TB
import test_gpu_kf_refresh as TR
import test_gpu_kf_store as KS
import test_gpu_kf_store_chain as CH
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import LocalMap, keyframe_ba_result, keyframe_insert_result, keyframe_local_ba, keyframe_refresh

pytestmark = pytest.mark.gpu

raw, sentinel, SENT_I32 = KS.raw, KS.sentinel, KS.SENT_I32
COLS = TR.COLS
N_CREATED = 12
CENTER_BOUND = 2.0 ** -20   # rotation entries within 2^-23 of the host's (tests/test_gpu_track_local_frames.py's bound):
                            # 3 * 2^-23 * |t|_inf from them, plus the LU's own roundings


def scene():
    """chain_scene() with the last N_CREATED of K's own slots EMPTY with a depth instead of FREE with a position: the
    insertion creates those points by unprojection and adopts the others."""
    sc = BC.chain_scene()
    c = sc["case"]
    n = c["n_cur"]
    c["slots"]["state"][n - N_CREATED:n] = KS.KC.EMPTY
    c["frame"]["depth"][n - N_CREATED:n] = np.linspace(4.0, 15.0, N_CREATED).astype(np.float32)
    sc["app"] = RC.appearance_for(sc["store"], sc["geom"], seed=77)
    return sc


class Arm(TB.ChainArm):
    def __init__(self, ctx, sc):
        super().__init__(ctx, sc)
        cn = R.counts(sc["store"])
        self.store.fill_life(cn)
        self.store.fill_appearance(cn)
        self.store.write_appearance(RR.flat_appearance(sc["app"]))
        self.rf_rec = TR.keyframe_refresh_record(ctx)

    def gather(self):
        rec = self.rig.rec.ptr.value
        keyframe_local_ba(self.ctx, self.store, self.sc["fp"], rec + A.KfInsertResult.kf.offset, self.ba_rec,
                          d_src_status=rec + A.KfInsertResult.status.offset, gather_only=True)

    def refresh(self, what=RR.ALL):
        keyframe_refresh(self.ctx, self.store, self.sc["fp"], self.ba_rec, self.rf_rec, what=what)

    def result(self):
        b = self.rf_rec.numpy()
        assert sentinel(b[TR.REC:])
        return A.KfRefreshResult.from_buffer_copy(b.tobytes()[:TR.REC])

    def free(self):
        self.rf_rec.free()
        super().free()


def restated_insertion(sc):
    """The store, geometry and appearance after the forced insertion, restated."""
    c = sc["case"]
    ref = KS.reference(c)
    assert ref["inserted"]
    g = B.insert_geometry(sc["geom"], ref, c["frame"], sc["pose6"], c["n_cur"])
    app = RR.insert_appearance(sc["app"], ref, c["frame"], c["pose"], c["n_cur"])
    return ref, g, app


def test_insertion_gather_refresh(ctx):
    sc = scene()
    c = sc["case"]
    arm = Arm(ctx, sc)
    try:
        arm.insert()     # nothing between the three calls
        arm.gather()
        arm.refresh()
        ins = keyframe_insert_result(arm.rig.rec)
        assert ins.inserted == 1 and ins.n_created == N_CREATED and ins.n_adopted == 40 - N_CREATED
        ref, g, app = restated_insertion(sc)
        s, K, n = ref["store"], ref["kf"], c["n_cur"]
        cn = R.counts(s)
        # K's appearance rows are the frame's; nothing past the new counts
        got_app, flat = arm.store.read_appearance(), RR.flat_appearance(app)
        for k in flat:
            assert got_app[k].shape == flat[k].shape and np.array_equal(raw(got_app[k]), raw(flat[k])), k
        assert np.array_equal(got_app["kf_slot_desc"][-n:], c["frame"]["desc"][:n])
        for k, v in arm.store.appearance.items():
            assert sentinel(v.numpy()[cn["n_kf"] if k == "kf_center" else cn["n_kf_slots"]:]), k
        ba, rec = keyframe_ba_result(arm.ba_rec), arm.result()
        assert ba.status == 0 and ba.written == 0
        win = arm.store.ba_window(ba)
        r = RR.refresh(s, g, app, dict(kf=K, local_kf=win["local_kf"], l2g=win["l2g"]), got_app["kf_center"], sc["fp"])
        TR.same_record(rec, r["rec"])
        assert rec.n_centers == 0 and rec.n_refreshed == rec.n_points == ba.n_points
        got = arm.store.read()
        TB.same_geometry(arm.store, g)
        for k in COLS:                                               # every point, held ones over their grown lists
            assert np.array_equal(raw(got[k]), raw(np.asarray(r[k], got[k].dtype))), k
        for k in ("pos", "locked", "is_bad"):
            assert np.array_equal(raw(got[k]), raw(np.asarray(s[k], got[k].dtype))), k
        assert got["obs"] == [[int(v) for v in o] for o in s["obs"]]
        # the fixed point: one observation, the same inputs as new_point
        row = s["kf_slots"][K]
        new = [(j, p) for j, p in enumerate(row) if s["obs"][p] == [K]]
        assert len(new) == 40
        for j, p in new:
            created = j >= n - N_CREATED
            for k in ("normal", "max_dist", "min_dist") + (("desc",) if created else ()):
                assert np.array_equal(raw(got[k][p]), raw(np.asarray(s[k])[p])), (k, p)
            assert np.array_equal(got["desc"][p], c["frame"]["desc"][j])          # K's descriptor, adopted or created
        assert any(not np.array_equal(s["desc"][p], c["frame"]["desc"][j]) for j, p in new if j < n - N_CREATED)
        held = [p for p in win["l2g"] if len(s["obs"][p]) > 1]
        assert len(held) > 100 and any(not np.array_equal(raw(got["normal"][p]), raw(s["normal"][p])) for p in held)
    finally:
        arm.free()


def test_insertion_local_ba_refresh(ctx):
    sc = scene()
    arm = Arm(ctx, sc)
    try:
        arm.insert()     # nothing between the three calls
        arm.local_ba()
        arm.refresh()
        ba, rec = keyframe_ba_result(arm.ba_rec), arm.result()
        assert ba.status == 0 and ba.written == 1
        ref, g, app = restated_insertion(sc)
        s, K = ref["store"], ref["kf"]
        win = arm.store.ba_window(ba)
        got, geo, got_app = arm.store.read(), arm.store.read_geometry(), arm.store.read_appearance()
        assert rec.n_centers == ba.n_poses == len(win["local_kf"]) and rec.status == 0
        # the centres: outside the window the bits stay; inside, the host's value within the bound
        before = RR.flat_appearance(app)["kf_center"]
        local = [int(f) for f in win["local_kf"]]
        others = [f for f in range(len(before)) if f not in local]
        assert len(others) >= 2 and set(int(f) for f in win["fixed_kf"]) <= set(others)
        assert np.array_equal(raw(got_app["kf_center"][others]), raw(before[others]))
        host = RR.centers(geo["kf_pose"], local, before, O.pose_to_Tcw, O.inv4_f32)
        worst = 0.0
        for f in local:
            t = float(np.abs(geo["kf_pose"][f, 3:]).max())
            dev = float(np.abs(got_app["kf_center"][f].astype(np.float64) - host[f].astype(np.float64)).max())
            worst = max(worst, dev / max(1.0, t))
            assert dev <= CENTER_BOUND * max(1.0, t), (f, dev, t)
        print(f"refreshed centres: largest deviation from the host's {worst:.3e} max(1, |t|_inf) (bound {CENTER_BOUND:.3e})")
        assert not np.array_equal(raw(got_app["kf_center"][local]), raw(before[local]))
        # the points: the restatement on the refined positions and the centres read back
        s2 = dict(s, pos=got["pos"])
        assert not np.array_equal(raw(got["pos"]), raw(np.asarray(s["pos"], np.float32)))
        r = RR.refresh(s2, g, app, dict(kf=K, local_kf=win["local_kf"], l2g=win["l2g"]), got_app["kf_center"], sc["fp"], written=1)
        TR.same_record(rec, r["rec"])
        for k in COLS:
            assert np.array_equal(raw(got[k]), raw(np.asarray(r[k], got[k].dtype))), k
        for k in ("kf_slot_desc", "kf_slot_octave"):
            assert np.array_equal(raw(got_app[k]), raw(RR.flat_appearance(app)[k])), k
        # the next frame's UpdateLocalMap gathers the refreshed rows
        gids = [int(p) for p in win["l2g"][[0, 1, 2, -3, -2, -1]]]
        probe = CH.Probe(ctx, gids)
        probe.lmap.free()
        caps = sc["case"]["caps"]
        probe.lmap = LocalMap(ctx, 512, caps["max_kf"], caps["max_points"])
        probe.lmap.fill()
        try:
            probe.update(arm.store)
            table = probe.read()
        finally:
            probe.free()
        n_local = A.LocalMapResult.from_buffer_copy(table["rec"].tobytes()[:C.sizeof(A.LocalMapResult)]).n_local
        assert n_local >= len(gids)
        for p in gids:
            at = int(np.nonzero(table["l2g"][:n_local] == p)[0][0])
            for k in COLS + ("pos",):
                assert np.array_equal(raw(table[k][at]), raw(got[k][p])), (k, p)
    finally:
        arm.free()


def test_zero_rotation_centre_has_the_oracles_bits(ctx):
    """kf 3 of the hand case with rvec = 0 and a hand-made BA record that says written = 1: pose_to_Tcw takes its
    identity branch, so the centre is the host's bit for bit; the other local keyframes within the bound; keyframes
    outside the window are not touched."""
    c = copy.deepcopy(RC.hand_case())
    c["geom"]["kf_pose"][3][:3] = 0
    c["geom"]["kf_pose"][3][3:] = (0.3, -1.7, 2.9)
    rig = TR.RefreshRig(ctx, c)
    try:
        ba = rig.gather()
        assert ba.status == 0 and ba.written == 0
        fake = A.KfBaResult.from_buffer_copy(bytes(ba))
        fake.written = 1
        h = np.full(C.sizeof(fake) + KS.G, KS.SENT, np.uint8)
        h[:C.sizeof(fake)] = np.frombuffer(bytes(fake), np.uint8)
        d = ctx.to_device(h)
        try:
            rig.refresh(RR.CENTERS, ba_record=d)
            rec = rig.result()
        finally:
            d.free()
        TR.same_record(rec, dict(status=0, kf=5, n_points=4, n_refreshed=4, n_bad=0, n_empty=0, n_obs_bad_slot=0, n_desc_changed=0,
                                 n_centers=3))
        got = rig.store.read_appearance()["kf_center"]
        pose = np.asarray(c["geom"]["kf_pose"], np.float32).reshape(-1, 6)
        host = RR.centers(pose, [5, 3, 1], c["app"]["kf_center"], O.pose_to_Tcw, O.inv4_f32)
        assert np.array_equal(raw(got[3]), raw(host[3])) and np.array_equal(host[3], -pose[3, 3:])
        for f in (5, 1):
            assert np.abs(got[f].astype(np.float64) - host[f]).max() <= CENTER_BOUND * max(1.0, float(np.abs(pose[f, 3:]).max())), f
        assert np.array_equal(raw(got[[0, 2, 4]]), raw(c["app"]["kf_center"][[0, 2, 4]]))
        s = rig.store.read()
        for k in COLS:                                               # CENTERS alone: no point column moves
            assert np.array_equal(raw(s[k]), raw(np.asarray(c["store"][k], s[k].dtype))), k
    finally:
        rig.free()


def test_refused_insertion(ctx):
    """Under the ratio gate the scene's frame is refused: the BA record says 1, the refresh stores its status and
    nothing else."""
    sc = scene()
    arm = Arm(ctx, sc)
    try:
        before = TR.everything(arm.store)
        arm.rig.insert(gate=R.GATE_RATIO)
        arm.local_ba()
        arm.refresh()
        assert keyframe_insert_result(arm.rig.rec).inserted == 0 and keyframe_ba_result(arm.ba_rec).status == 1
        TR.same_record(arm.result(), dict(status=1))
        after = TR.everything(arm.store)
        for k in before:
            assert np.array_equal(raw(after[k]), raw(before[k])), k
    finally:
        arm.free()
