"""GPU: lorb_kf_store_refresh_dev behind a bare lorb_kf_store_ba_gather_dev (written = 0: no centre moves), and the
store's appearance (lorb_kf_store_appear_write / _read / _view; lorb_slam_amd.frame.KeyframeStore.write_appearance /
keyframe_refresh).  Everything is bit-exact against the restatement tests/kf_refresh_ref.py given the centres the store
reports: the record, the four refreshed columns; every other array of read(), read_geometry(), read_life() and the
appearance keeps its bytes, as do the sentinel bytes past the true counts of every array; the BA's scratch is at rest
(a second gather gives the same window)."""
import copy
import ctypes as C

import numpy as np
import pytest

import kf_ba_cases as BC
import kf_refresh_cases as RC
import kf_refresh_ref as RR
import kf_store_ref as R
import test_gpu_kf_ba as TB
import test_gpu_kf_store as KS
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import keyframe_compact_record, keyframe_refresh, keyframe_refresh_record
from lorb_slam_amd.runtime import LorbError, lib

pytestmark = pytest.mark.gpu

G, SENT, SENT_I32 = KS.G, KS.SENT, KS.SENT_I32
REC = C.sizeof(A.KfRefreshResult)
raw, sentinel = KS.raw, KS.sentinel
CASES = RC.all_cases()
COLS = ("normal", "max_dist", "min_dist", "desc")


def everything(store):
    """Every array of the store over its whole capacity: the view's, the geometry's, the life's, the appearance's."""
    a = TB.arrays_of(store)
    a.update({"life_" + k: v.numpy() for k, v in store.life.items()})
    a.update({k: v.numpy() for k, v in store.appearance.items()})
    return a


class RefreshRig(TB.BaRig):
    """TB.BaRig with the case's appearance written and sentinel bytes behind the true counts of the new arrays and of
    the life arrays too."""

    def __init__(self, ctx, case, appearance=True, **kw):
        super().__init__(ctx, case, **kw)
        self.store.fill_life(self.cn)
        self.store.fill_appearance(self.cn)
        if appearance:
            self.store.write_appearance(RR.flat_appearance(case["app"]))
        self.rrec = keyframe_refresh_record(ctx)

    def gather(self):
        self.run(gather_only=True)
        return self.record()

    def refresh(self, what=RR.ALL, ba_record=None):
        self.ctx.check(lib().lorb_memset_dev(self.ctx.handle, self.rrec.ptr, C.c_int(SENT), C.c_size_t(REC)), "memset")
        keyframe_refresh(self.ctx, self.store, self.fp, ba_record if ba_record is not None else self.rec, self.rrec, what=what)

    def result(self):
        b = self.rrec.numpy()
        assert sentinel(b[REC:])
        return A.KfRefreshResult.from_buffer_copy(b.tobytes()[:REC])

    def free(self):
        self.rrec.free()
        super().free()


def same_record(rec, want):
    for f in RR.FIELDS:
        assert getattr(rec, f) == want.get(f, SENT_I32), (f, getattr(rec, f), want.get(f))


def refresh_and_compare(rig, what=RR.ALL):
    """One gather and one refresh; -> (record, restatement).  The restatement is fed the centres the store reports."""
    c = rig.case
    ba = rig.gather()
    assert ba.status == 0
    win0 = rig.store.ba_window(ba)
    before = everything(rig.store)
    rig.refresh(what)
    rec = rig.result()
    after = everything(rig.store)
    np_ = rig.cn["n_points"]
    store = dict(c["store"], **{k: before[k][:np_] for k in COLS})   # a second call starts from the first one's rows
    ref = RR.refresh(store, c["geom"], c["app"], dict(kf=c["kf"], local_kf=win0["local_kf"], l2g=win0["l2g"]),
                     after["kf_center"][:rig.cn["n_kf"]], rig.fp, what=what)
    same_record(rec, ref["rec"])
    for k in COLS:
        assert np.array_equal(raw(after[k][:np_]), raw(np.asarray(ref[k], after[k].dtype))), k
    for k in after:                                                  # everything else, and every tail past a count
        if k in COLS:
            assert np.array_equal(raw(after[k][np_:]), raw(before[k][np_:])), k
        else:
            assert np.array_equal(raw(after[k]), raw(before[k])), k
    for k in COLS + ("kf_slot_desc", "kf_slot_octave", "kf_center"):
        past = np_ if k in COLS else rig.cn["n_kf"] if k == "kf_center" else rig.cn["n_kf_slots"]
        assert sentinel(after[k][past:]), k
    # the BA's scratch is at rest: a second gather gives the same window
    ba2 = rig.gather()
    assert bytes(ba2) == bytes(ba)
    TB.same_window(rig.store.ba_window(ba2), win0)
    return rec, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_refresh(ctx, name):
    rig = RefreshRig(ctx, CASES[name])
    try:
        rec, ref = refresh_and_compare(rig)
        assert rec.status == 0 and rec.n_centers == 0 and rec.n_refreshed > 0
        c = rig.case
        if name == "hand":
            same_record(rec, c["want"]["rec"])
            assert ref["chosen"] == c["want"]["chosen"]
            got = rig.store.read()
            for i, g in enumerate(c["want"]["l2g"]):
                assert np.array_equal(raw(got["normal"][g]), raw(np.array(c["want"]["normal"][i], np.float32))), g
                assert np.array_equal(got["desc"][g], RC.low_bits(c["want"]["took"][i])), g
        if name == "identical":                                      # the first wins; the count is bits, not choices
            p0 = RC.p0_of(c)
            i0 = [int(v) for v in rig.store.ba_window(rig.record())["l2g"]].index(p0)
            assert ref["chosen"][i0] == 0
            d = c["app"]["kf_slot_desc"][c["store"]["obs"][p0][0]][c["geom"]["obs_slot"][p0][0]]
            assert RR.hamming(c["store"]["desc"][p0], d) > 1 and rec.n_desc_changed >= RR.hamming(c["store"]["desc"][p0], d)
        if name == "equal_medians":
            i0 = [int(v) for v in rig.store.ba_window(rig.record())["l2g"]].index(RC.p0_of(c))
            assert ref["chosen"][i0] == 0
        if name == "all_bad":                                        # the descriptor stays, the normal moves
            own = [p for p in c["store"]["kf_slots"][c["kf"]] if c["store"]["obs"][p] == [c["kf"]]]
            got = rig.store.read()
            assert len(own) == 2
            for p in own:
                assert np.array_equal(got["desc"][p], c["store"]["desc"][p])
                assert not np.array_equal(raw(got["normal"][p]), raw(c["store"]["normal"][p]))
        # a second refresh on the refreshed rows: the same rows again, no bit of a descriptor changes
        rec2, _ = refresh_and_compare(rig)
        assert rec2.n_desc_changed == 0 and rec2.n_refreshed == rec.n_refreshed
    finally:
        rig.free()


@pytest.mark.parametrize("what", [RR.NORMAL_DEPTH, RR.DESCRIPTOR, RR.CENTERS, RR.CENTERS | RR.DESCRIPTOR])
def test_each_flag_alone(ctx, what):
    """The columns of the other half stay byte for byte (refresh_and_compare's restatement leaves them); CENTERS
    alone, behind a gather, writes the record and nothing else."""
    rig = RefreshRig(ctx, CASES["random_a"])
    try:
        s = rig.store.read()
        rec, _ = refresh_and_compare(rig, what)
        got = rig.store.read()
        moved = {k: not np.array_equal(raw(got[k]), raw(s[k])) for k in COLS}
        assert moved["desc"] == bool(what & RR.DESCRIPTOR)
        assert moved["normal"] == moved["max_dist"] == moved["min_dist"] == bool(what & RR.NORMAL_DEPTH)
        assert rec.n_centers == 0
    finally:
        rig.free()


def test_bad_points_and_damaged_observations(ctx):
    """A window point that went bad after the gather is skipped and counted; an observation whose slot lies outside
    its keyframe's row is skipped in both halves and counted; a point left without any counts as empty."""
    c = copy.deepcopy(CASES["hand"])
    rig = RefreshRig(ctx, c)
    try:
        ba = rig.gather()
        win = rig.store.ba_window(ba)
        before = everything(rig.store)
        # p2 goes bad; p7's observation in kf3 (obs index 8 of the store, TB's geometry test) names slot 99; p0's only one too
        off = rig.store.read()["csr"]["obs_off"]
        is_bad, slot = before["is_bad"].copy(), before["obs_slot"].copy()
        is_bad[2] = 1
        slot[off[7] + 1] = 99
        slot[off[0]] = 99
        for arr, v in ((rig.store.arrays["is_bad"], is_bad), (rig.store.geometry["obs_slot"], slot)):
            rig.ctx.check(lib().lorb_memcpy_h2d(rig.ctx.handle, arr.ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes)), "h2d")
        c["store"]["is_bad"][2] = 1
        c["geom"]["obs_slot"][7][1] = 99
        c["geom"]["obs_slot"][0][0] = 99
        rig.refresh()
        rec = rig.result()
        after = everything(rig.store)
        ref = RR.refresh(c["store"], c["geom"], c["app"], dict(kf=5, local_kf=win["local_kf"], l2g=win["l2g"]),
                         after["kf_center"][:6], rig.fp)
        same_record(rec, ref["rec"])
        assert (rec.n_bad, rec.n_empty, rec.n_obs_bad_slot, rec.n_refreshed) == (1, 1, 2, 2)
        for k in COLS:
            assert np.array_equal(raw(after[k][:10]), raw(np.asarray(ref[k], after[k].dtype))), k
        for p in (2, 0):
            for k in COLS:
                assert np.array_equal(raw(after[k][p]), raw(before[k][p])), (k, p)
    finally:
        rig.free()


def test_statuses_write_nothing(ctx):
    """A BA record with status 1 (a no-op gather) or 3 (no points): status = 1 and not a byte written, in the store
    or in the rest of the record; LORB_OK both times.  Then a good call on the same store."""
    rig = RefreshRig(ctx, CASES["hand"])
    try:
        assert rig.gather().status == 0
        before = everything(rig.store)
        for status in (1, 3):
            fake = A.KfBaResult(status, 5, 3, 2, 4, 9, 0, 0, 0, 1)
            h = np.full(C.sizeof(fake) + G, SENT, np.uint8)
            h[:C.sizeof(fake)] = np.frombuffer(bytes(fake), np.uint8)
            d = rig.ctx.to_device(h)
            try:
                rig.refresh(ba_record=d)
                same_record(rig.result(), dict(status=1))
                assert np.array_equal(d.numpy(), h)
            finally:
                d.free()
            after = everything(rig.store)
            for k in before:
                assert np.array_equal(raw(after[k]), raw(before[k])), k
        rig.set(-1)                                                  # the gather itself refuses: its record says 1
        rig.run(gather_only=True)
        assert rig.record().status == 1
        rig.refresh()
        same_record(rig.result(), dict(status=1))
        after = everything(rig.store)
        for k in before:
            assert np.array_equal(raw(after[k]), raw(before[k])), k
        rig.set(5)
        rec, _ = refresh_and_compare(rig)
        assert rec.status == 0 and rec.n_refreshed == 4
    finally:
        rig.free()


def test_invalid_calls(ctx):
    """LORB_E_INVALID before anything is enqueued: a store without appearance, what = 0 or an unknown bit, n_levels out
    of range, no window yet, and after a compaction ("no current window")."""
    rig = RefreshRig(ctx, CASES["hand"], appearance=False)
    try:
        assert rig.gather().status == 0
        before = everything(rig.store)
        with pytest.raises(LorbError, match="rc=-1.*appearance"):
            rig.refresh()
        rig.store.write_appearance(dict(kf_center=RR.flat_appearance(rig.case["app"])["kf_center"]))   # in part: still none
        with pytest.raises(LorbError, match="rc=-1.*appearance"):
            rig.refresh()
        assert sentinel(rig.rrec.numpy())
        rig.store.write_appearance(RR.flat_appearance(rig.case["app"]))
        for what in (0, 8, 15):
            with pytest.raises(LorbError, match="rc=-1.*flags"):
                rig.refresh(what)
        fp = rig.fp
        for n in (0, A.LORB_MAX_LEVELS + 1):
            rig.fp = dict(fp, n_levels=n)
            with pytest.raises(LorbError, match="rc=-1.*n_levels"):
                rig.refresh()
        rig.fp = fp
        assert sentinel(rig.rrec.numpy())
        crec = keyframe_compact_record(ctx)
        try:
            rig.store.compact(crec)
            with pytest.raises(LorbError, match="rc=-1.*no current window"):
                rig.refresh()
        finally:
            crec.free()
        assert sentinel(rig.rrec.numpy())
        after = everything(rig.store)
        for k in COLS:
            assert np.array_equal(raw(after[k]), raw(before[k])), k
        rec, _ = refresh_and_compare(rig)                            # a gather makes the window current again
        assert rec.status == 0
    finally:
        rig.free()
    rig = RefreshRig(ctx, CASES["hand"])
    try:
        with pytest.raises(LorbError, match="rc=-1.*no current window"):   # nothing gathered yet
            rig.refresh()
    finally:
        rig.free()


def test_appearance_write_and_read(ctx):
    """write -> read returns the rows; the counts must equal the true ones; an octave outside [0, LORB_MAX_LEVELS)
    names its entry; nothing past the counts is written; a store created empty is complete."""
    c = CASES["hand"]
    rig = RefreshRig(ctx, c, appearance=False)
    try:
        flat = RR.flat_appearance(c["app"])
        cn = rig.cn
        for kw in (dict(n_kf=cn["n_kf"] + 1), dict(n_kf_slots=cn["n_kf_slots"] - 1)):
            with pytest.raises(LorbError, match="rc=-1.*counts"):
                rig.store.write_appearance({}, **kw)
        for bad in (A.LORB_MAX_LEVELS, -1):
            o = flat["kf_slot_octave"].copy()
            o[4] = bad
            with pytest.raises(LorbError, match=rf"rc=-1.*kf_slot_octave\[4\] = {bad} "):
                rig.store.write_appearance(dict(flat, kf_slot_octave=o))
        for k, v in rig.store.appearance.items():
            assert sentinel(v.numpy()[cn["n_kf"] if k == "kf_center" else cn["n_kf_slots"]:]), k
        rig.store.write_appearance(flat)
        got = rig.store.read_appearance()
        for k in flat:
            assert got[k].shape == flat[k].shape and np.array_equal(raw(got[k]), raw(flat[k])), k
        for k, v in rig.store.appearance.items():
            assert sentinel(v.numpy()[cn["n_kf"] if k == "kf_center" else cn["n_kf_slots"]:]), k
        small = A.KfStoreAppearHost(cn["n_kf"] - 1, cn["n_kf_slots"])
        keep = np.zeros((cn["n_kf"], 3), np.float32)
        small.kf_center = keep.ctypes.data
        with pytest.raises(LorbError, match="rc=-1.*smaller"):
            ctx.check(lib().lorb_kf_store_appear_read(rig.store._p, C.byref(small)), "lorb_kf_store_appear_read")
    finally:
        rig.free()
