"""GPU: the growing store in the chain.

1. From an empty store a LORB_KF_GATE_NONE insertion and three gated ones (the second of them refused) are enqueued
   with no wait between them -- hand-made slot sets stand in for tracked frames -- and after the one wait the
   records, slots, gids, counts and every array of the store equal the restatement applied four times.
2. Behind each insertion lorb_local_map_update_dev runs on the store's VIEW, taken before the wait: its counts are
   the host's bounds, which exceed the truth from the first insertion on (and by a whole keyframe after the refused
   one).  Everything it leaves equals, byte for byte, the same call on a DeviceMapStore uploaded from the
   restatement's exact store; and again after lorb_kf_store_counts has tightened the bounds.
3. The next frame's lorb_track_motion_refer_pose_dev step b leaves K in the reference-frame word after an
   insertion, and UpdateLocalMap's choice after a refused one."""
import ctypes as C

import numpy as np
import pytest

import kf_store_cases as KC
import kf_store_ref as R
import test_gpu_kf_store as KS
import test_gpu_local_map as LM
import test_gpu_track_frames as TR
import test_gpu_track_local_frames as TLF
import test_gpu_track_refer as TRF
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, DeviceMapStore, DeviceSlots, KeyframeStore, LocalMap, _sentinel, keyframe_insert,
                                 keyframe_insert_result, local_map_buffers, local_map_update)
from test_gpu_track_frames import builders  # noqa: F401 -- the module-scoped builder fixture

pytestmark = pytest.mark.gpu

G, SENT, FILL, REC = KS.G, KS.SENT, KS.FILL, KS.REC
LOCKED = KC.LOCKED
CAPS, N_MAX = KC.CHAIN_CAPS, KC.CHAIN_N_MAX
MAX_LOCAL = 64
CHOICE = 1       # the keyframe this frame's UpdateLocalMap chose as mReferFrame
frames, restate = KC.chain_frames, KC.chain_restate   # checked by hand in tests/test_kf_store_ref.py


class Step:
    """One frame's device objects for the insertion, and one probe's for the local-map update behind it."""

    def __init__(self, ctx, c, probe_gid):
        self.ctx, self.c = ctx, c
        n = c["n_cur"]
        self.frame = KS.Frame(ctx, c)
        self.slots = DeviceSlots(ctx, N_MAX, state=c["slots"]["state"], pos=c["slots"]["pos"], desc=c["slots"]["desc"])
        g = np.full(N_MAX + G, FILL, np.int32)
        g[:n] = c["gid"]
        self.gid = ctx.to_device(g)
        self.pose = DeviceBlock(ctx, A.FramePose, KS.pose_value(c["pose"]))
        self.rec = _sentinel(ctx, REC + G, np.uint8)
        self.probe = Probe(ctx, probe_gid)

    def free(self):
        for a in (self.frame, self.slots, self.gid, self.pose, self.rec, self.probe):
            a.free()


class Probe:
    """A frame whose slots hold the given store points, a local map of its own filled with sentinel bytes, and the
    buffers of one lorb_local_map_update_dev call."""

    def __init__(self, ctx, gids):
        self.ctx, self.n = ctx, len(gids)
        self.nc = self.n + 1
        self.frame = LM.Counts(ctx, self.n)
        self.slots = DeviceSlots(ctx, self.nc, state=[LOCKED] * self.n)
        self.gid, self.sid, self.rec = local_map_buffers(ctx, self.nc, gids, FILL)
        self.lmap = LocalMap(ctx, MAX_LOCAL, CAPS["max_kf"], CAPS["max_points"])
        self.lmap.fill()

    def update(self, store):
        local_map_update(self.ctx, self.lmap, store, self.frame, self.slots, self.gid, self.sid, self.rec, n_max_cur=self.nc)

    def read(self):
        r = dict(rec=self.rec.numpy(), gid=self.gid.numpy(), sid=self.sid.numpy())
        r.update({"slot_" + k: v for k, v in self.slots.numpy().items()})
        r.update(self.lmap.numpy())
        return r

    def free(self):
        for a in (self.frame, self.slots, self.gid, self.sid, self.rec, self.lmap):
            a.free()


def probe_gids(s):
    """Three of the oldest and three of the newest points of a store."""
    n = s["n_points"]
    return [0, 1, 2, n - 3, n - 2, n - 1]


def exact_update(ctx, s, gids):
    """The same update on a DeviceMapStore uploaded from the restatement's exact store."""
    dms = DeviceMapStore(ctx, s, s["obs"], s["kf_bad"], s["kf_slots"], s["cov"])
    p = Probe(ctx, gids)
    try:
        p.update(dms)
        return p.read()
    finally:
        p.free()
        dms.free()


def assert_same_update(got, want, s, bounds):
    """Byte for byte.  Under bounds kf_votes and g2l are compared up to the true counts: the entries between truth
    and bound are below the counts that call was given (0 and -1 there), on an exact store they are past them."""
    c = R.counts(s)
    for k in want:
        a, b = got[k], want[k]
        if bounds and k in ("kf_votes", "g2l"):
            m = c["n_kf"] if k == "kf_votes" else c["n_points"]
            a, b = a[:m], b[:m]
        assert np.array_equal(KS.raw(a), KS.raw(b)), k
    rec = A.LocalMapResult.from_buffer_copy(got["rec"].tobytes()[:C.sizeof(A.LocalMapResult)])
    assert rec.status == 0 and rec.n_held == 6 and rec.n_local > 0 and rec.n_local_kf > 0


def test_four_insertions_and_the_view_with_one_wait(ctx):
    fs = frames()
    refs = restate(fs)
    store = KeyframeStore(ctx, **CAPS)
    store.fill(R.counts(R.empty_store()))
    steps = [Step(ctx, c, probe_gids(r["store"])) for c, r in zip(fs, refs)]
    try:
        views = []
        for st in steps:  # eight calls, no wait
            keyframe_insert(ctx, store, st.c["fp"], st.frame, st.slots, st.gid, st.pose, st.rec, n_max_cur=N_MAX, gate=st.c["gate"])
            v = store.view()
            views.append((v.n_kf, v.points.n, v.n_obs, v.n_kf_slots, v.n_cov))
            st.probe.update(store)
        ctx.sync()  # the one wait
        # the bounds the views carried: a keyframe and N_MAX points / slots per enqueued insertion, the capacities
        assert views == [(k + 1, min(N_MAX * (k + 1), CAPS["max_points"]), CAPS["max_obs"], min(N_MAX * (k + 1), CAPS["max_kf_slots"]),
                          CAPS["max_kf"] ** 2) for k in range(4)]
        for st, ref in zip(steps, refs):
            n = st.c["n_cur"]
            rec = keyframe_insert_result(st.rec)
            for f in R.FIELDS:
                assert getattr(rec, f) == ref["rec"].get(f, KS.SENT_I32), f
            sl, gid = st.slots.numpy(), st.gid.numpy()
            assert np.array_equal(sl["state"][:n], ref["state"]) and KS.sentinel(sl["state"][n:])
            assert np.array_equal(KS.raw(sl["pos"][:n]), KS.raw(ref["pos"])) and KS.sentinel(sl["pos"][n:])
            assert np.array_equal(sl["desc"][:n], ref["desc"]) and KS.sentinel(sl["desc"][n:])
            assert np.array_equal(gid[:n], ref["gid"]) and (gid[n:] == FILL).all()
            # the update behind this insertion, on bounds
            assert_same_update(st.probe.read(), exact_update(ctx, ref["store"], probe_gids(ref["store"])), ref["store"], bounds=True)
        final = refs[-1]["store"]
        cn = R.counts(final)
        assert store.view().n_kf == 4                       # still the bound: the refused insertion counted
        assert store.counts() == cn and store.view().n_kf == 3 and store.view().points.n == cn["n_points"]
        KS.same_store(store.read(), final)
        past = dict(obs_off=cn["n_points"] + 1, obs_kf=cn["n_obs"], kf_slot_off=cn["n_kf"] + 1, kf_slot_point=cn["n_kf_slots"],
                    cov_off=cn["n_kf"] + 1, cov_kf=cn["n_cov"], kf_bad=cn["n_kf"])
        for k, arr in store.arrays.items():
            tail = arr.numpy()[past.get(k, cn["n_points"]):]
            assert (tail == 1).all() if k in ("is_bad", "kf_bad") else KS.sentinel(tail), k
        # once more with the bounds tightened: now the whole arrays agree
        v = store.view()
        assert (v.n_kf, v.points.n, v.n_obs, v.n_kf_slots, v.n_cov) == tuple(cn[k] for k in ("n_kf", "n_points", "n_obs", "n_kf_slots", "n_cov"))
        p = Probe(ctx, probe_gids(final))
        try:
            p.update(store)
            assert_same_update(p.read(), exact_update(ctx, final, probe_gids(final)), final, bounds=False)
        finally:
            p.free()
    finally:
        for st in steps:
            st.free()
        store.free()


@pytest.mark.parametrize("name,inserted", [("two_slots", True), ("gate_8_of_20", False)])
def test_the_refer_word_behind_an_insertion(ctx, builders, name, inserted):
    """This frame's UpdateLocalMap record names keyframe CHOICE; the insertion behind it stores K in the word AND
    in that record, so that the next frame's step b (which re-applies the record to the word) leaves K there; a
    refused insertion leaves both alone and step b stores CHOICE."""
    S = TLF.scene()
    with TR.Built(ctx, builders, S["ca"], S["cb"]) as bt:
        nxt = TRF.Rig(ctx, bt, S, x_last=0.0, prev_kf=CHOICE, prev_status=0)
        ks = KS.Rig(ctx, KC.all_cases()[name], word=nxt.kf, update=nxt.upd)
        try:
            ks.insert()
            nxt.first()  # the next frame: its first attempt passes, the second is not due; step b runs all the same
            nxt.refer()
            after = nxt.read()
            rec = keyframe_insert_result(ks.rec)
        finally:
            ks.free()
    word = int(after["kf"][:4].view(np.int32)[0])
    upd = A.LocalMapResult.from_buffer_copy(after["upd"].tobytes()[:C.sizeof(A.LocalMapResult)])
    assert TRF.refer_record(after)[:3] == (0, 0, 0) and upd.status == 0
    if inserted:
        assert rec.inserted == 1 and rec.kf == 2 and word == 2 and upd.refer_kf == 2
    else:
        assert rec.inserted == 0 and word == CHOICE and upd.refer_kf == CHOICE
    assert (after["kf"][4:] == SENT).all() and (after["upd"][C.sizeof(A.LocalMapResult):] == SENT).all()
