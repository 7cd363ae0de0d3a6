"""GPU: the keyframe insertion on the device (lorb_kf_store_*; lorb_slam_amd.frame.KeyframeStore / keyframe_insert)
on the hand-built and generated cases of tests/kf_store_cases.py, bit for bit against the restatement
tests/kf_store_ref.py -- the record, the slots (state, pos, desc), the gids, the true counts and every array of
lorb_kf_store_read, the weight map included -- with every byte past a count keeping what it held before the call:
sentinel bytes are written beforehand past every count in the slots, the gids and every array of the store
(KeyframeStore.fill; is_bad / kf_bad hold 1 there, the inert rows)."""
import ctypes as C

import numpy as np
import pytest

import kf_store_cases as KC
import kf_store_ref as R
import lorb_slam_amd.window as W
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, DeviceSlots, KeyframeStore, _guarded, _sentinel, keyframe_insert,
                                 keyframe_insert_result, refer_kf_word)
from lorb_slam_amd.runtime import LorbError, lib

pytestmark = pytest.mark.gpu

G, SENT, FILL = W.ORB_GUARD, W.ORB_SENTINEL, -77
SENT_I32 = int(np.full(4, SENT, np.uint8).view(np.int32)[0])
REC = C.sizeof(A.KfInsertResult)
CASES = KC.all_cases()
# the implementation's constants (lorb_kfstore.hip): kWalk, kTile, kCountWin; a wavefront; kSortMax is the largest max_kf
WALK, TILE, WINDOW, WAVE, SORT_MAX = 1024, 1024, 1024, 64, 4096
SIZES = KC.size_cases(WALK, TILE, WINDOW, WAVE)
NO_KF = -5


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def sentinel(a):
    return (raw(a) == SENT).all()


class Frame:
    """What the insertion reads of a lorb_frame_out: counts[0], the left x, y, octave, desc and the depth, each of
    n_max entries with a guard band."""

    def __init__(self, ctx, c):
        self.ctx, nc, f = ctx, c["n_max_cur"], c["frame"]

        def pad(a, dt, w=1):
            h = np.zeros((nc, w) if w > 1 else nc, dt)
            h[:len(a)] = a
            return _guarded(ctx, h, dt, w)

        self.arrays = dict(x=pad(f["x"], np.float32), y=pad(f["y"], np.float32), octave=pad(f["octave"], np.int32),
                           desc=pad(f["desc"], np.uint8, 32), depth=pad(f["depth"], np.float32),
                           counts=ctx.to_device(np.array([c["n_cur"], 0] + [FILL] * G, np.int32)))
        self.out = A.FrameOut()
        for k in ("x", "y", "octave", "desc"):
            setattr(self.out.left, k, self.arrays[k].ptr.value)
        self.out.depth, self.out.counts = self.arrays["depth"].ptr.value, self.arrays["counts"].ptr.value

    def set(self, n):
        v = np.array([n], np.int32)
        self.ctx.check(lib().lorb_memcpy_h2d(self.ctx.handle, self.arrays["counts"].ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(4)),
                       "h2d")

    def free(self):
        for a in self.arrays.values():
            a.free()


def pose_value(pose):
    p = A.FramePose()
    p.Twc[:] = [float(v) for v in np.asarray(pose["Twc"], np.float32).reshape(16)]
    p.status = int(pose["status"])
    return p


class Rig:
    """One case's device objects, sentinel bytes behind every count."""

    def __init__(self, ctx, c, word=None, update=None):
        self.ctx, self.c = ctx, c
        s, n, self.nc = c["store"], c["n_cur"], c["n_max_cur"]
        k = c["caps"]
        self.store = KeyframeStore(ctx, k["max_kf"], k["max_points"], k["max_obs"], k["max_kf_slots"],
                                   init=s if len(s["kf_bad"]) or s["n_points"] else None)
        self.frame = Frame(ctx, c)
        self.slots = DeviceSlots(ctx, self.nc, state=c["slots"]["state"], pos=c["slots"]["pos"], desc=c["slots"]["desc"])
        g = np.full(self.nc + G, FILL, np.int32)
        g[:n] = c["gid"]
        self.gid = ctx.to_device(g)
        self.pose = DeviceBlock(ctx, A.FramePose, pose_value(c["pose"]))
        self.rec = _sentinel(ctx, REC + G, np.uint8)
        self.own = [] if word is not None else [refer_kf_word(ctx, NO_KF), _sentinel(ctx, C.sizeof(A.LocalMapResult) + G, np.uint8)]
        self.word, self.update = (word, update) if word is not None else self.own
        self.store.fill(R.counts(s))

    def snapshot(self):
        return {k: a.numpy() for k, a in self.store.arrays.items()}

    def insert(self, d_src_status=None, gate=None):
        self.ctx.check(lib().lorb_memset_dev(self.ctx.handle, self.rec.ptr, C.c_int(SENT), C.c_size_t(REC)), "memset")
        self.before = dict(slots=self.slots.numpy(), gid=self.gid.numpy(), store=self.snapshot())
        keyframe_insert(self.ctx, self.store, self.c["fp"], self.frame, self.slots, self.gid, self.pose, self.rec, n_max_cur=self.nc,
                        d_src_status=d_src_status, gate=self.c["gate"] if gate is None else gate, refer_kf=self.word,
                        update_record=self.update)

    def read(self):
        return dict(rec_bytes=self.rec.numpy(), slots=self.slots.numpy(), gid=self.gid.numpy(), counts=self.store.counts(),
                    store=self.store.read(), arrays=self.snapshot(), word=int(self.word.numpy()[:4].view(np.int32)[0]),
                    update=self.update.numpy())

    def free(self):
        for a in (self.frame, self.slots, self.gid, self.pose, self.rec, self.store, *self.own):
            a.free()


def same_store(got, s):
    """Everything lorb_kf_store_read returned against a restatement's store."""
    assert {k: got[k] for k in KeyframeStore.COUNTS} == R.counts(s)
    for k in R.COLS:
        assert np.array_equal(raw(got[k]), raw(np.asarray(s[k], got[k].dtype))), k
    assert np.array_equal(got["kf_bad"], s["kf_bad"])
    for k in ("obs", "kf_slots", "cov"):
        assert got[k] == [[int(v) for v in row] for row in s[k]], k
    assert got["conn"] == [{int(f): int(w) for f, w in c.items()} for c in s["conn"]]
    for k in ("obs_off", "kf_slot_off", "cov_off", "conn_off"):
        assert got["csr"][k][0] == 0, k


def check(rig, r, ref):
    c = rig.c
    n = c["n_cur"]
    # the record: the fields the call writes, the others and the guard band untouched
    rec = A.KfInsertResult.from_buffer_copy(r["rec_bytes"].tobytes()[:REC])
    for f in R.FIELDS:
        assert getattr(rec, f) == ref["rec"].get(f, SENT_I32), (f, getattr(rec, f), ref["rec"].get(f))
    assert sentinel(r["rec_bytes"][REC:])
    # the slots and the gids
    sl = r["slots"]
    assert np.array_equal(sl["state"][:n], ref["state"][:n]) and sentinel(sl["state"][n:])
    assert np.array_equal(raw(sl["pos"][:n]), raw(ref["pos"][:n])) and sentinel(sl["pos"][n:])
    assert np.array_equal(sl["desc"][:n], ref["desc"][:n]) and sentinel(sl["desc"][n:])
    assert np.array_equal(r["gid"][:n], ref["gid"][:n]) and (r["gid"][n:] == FILL).all()
    # the store: the true counts, every array of read, and the bytes past every count
    s = ref["store"]
    cn = R.counts(s)
    assert r["counts"] == cn
    same_store(r["store"], s)
    a = r["arrays"]
    past = dict(obs_off=cn["n_points"] + 1, obs_kf=cn["n_obs"], kf_slot_off=cn["n_kf"] + 1, kf_slot_point=cn["n_kf_slots"],
                cov_off=cn["n_kf"] + 1, cov_kf=cn["n_cov"], kf_bad=cn["n_kf"])
    for k, v in a.items():
        tail = v[past.get(k, cn["n_points"]):]
        assert (tail == 1).all() if k in ("is_bad", "kf_bad") else sentinel(tail), k
    # mReferFrame: the word and this frame's local-map record take K on insertion only
    up = A.LocalMapResult.from_buffer_copy(r["update"].tobytes()[:C.sizeof(A.LocalMapResult)])
    if ref["inserted"]:
        assert r["word"] == ref["kf"] and up.refer_kf == ref["kf"]
    else:
        assert r["word"] == NO_KF and up.refer_kf == SENT_I32
        for k in a:  # nothing of the store moved
            assert np.array_equal(raw(a[k]), raw(rig.before["store"][k])), k
        assert all(np.array_equal(raw(sl[k]), raw(rig.before["slots"][k])) for k in sl)
        assert np.array_equal(r["gid"], rig.before["gid"])
    up.refer_kf = SENT_I32
    assert sentinel(np.frombuffer(bytes(up), np.uint8)) and sentinel(r["update"][C.sizeof(A.LocalMapResult):])


def reference(c, **kw):
    a = dict(pose=c["pose"], n_cur=c["n_cur"], gate=c["gate"], src_status=0)
    a.update(kw)
    return R.insert_keyframe(c["store"], c["caps"], c["fp"], c["frame"], a["pose"], c["slots"], c["gid"], a["n_cur"], c["n_max_cur"],
                             a["gate"], src_status=a["src_status"])


def run_case(ctx, c):
    rig = Rig(ctx, c)
    try:
        rig.insert()
        r = rig.read()
        ref = reference(c)
        check(rig, r, ref)
        return r, ref
    finally:
        rig.free()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(ctx, name):
    r, ref = run_case(ctx, CASES[name])
    rec = A.KfInsertResult.from_buffer_copy(r["rec_bytes"].tobytes()[:REC])
    for k, want in CASES[name]["want"].items():  # the hand answers, once more on the device's side
        n = CASES[name]["n_cur"]
        if k in R.FIELDS:
            got = getattr(rec, k)
        else:
            st = r["store"]
            got = dict(gid=list(r["gid"][:n]), state=list(r["slots"]["state"][:n]), row=st["kf_slots"][-1] if ref["inserted"] else None,
                       obs=st["obs"], cov=st["cov"], conn=st["conn"], locked=list(st["locked"][CASES[name]["store"]["n_points"]:]))[k]
        assert got == want, (name, k, got, want)


@pytest.mark.parametrize("name", sorted(SIZES))
def test_sizes_that_cross_the_kernels_limits(ctx, name):
    """n_cur = kWalk + 6; n_points = 2 kTile + 3 with owners on both sides of both borders; n_kf = kCountWin + 1 with
    observers in both windows, a neighbour row of a wavefront + 7 keys and one of kCountWin + 1 keys (more than one
    key per thread of k_kf_order)."""
    c = SIZES[name]
    assert dict(walk_plus=c["n_cur"] == WALK + 6, two_tiles=c["store"]["n_points"] == 2 * TILE + 3,
                window_plus=len(c["store"]["kf_bad"]) == WINDOW + 1 <= SORT_MAX)[name]
    r, ref = run_case(ctx, c)
    assert ref["inserted"]
    if name == "window_plus":
        assert len(r["store"]["cov"][3]) == WAVE + 7 and len(r["store"]["cov"][WINDOW]) == WINDOW + 1


@pytest.mark.parametrize("fail", ["count_above", "count_negative", "src_status", "pose_status"])
def test_status_1(ctx, fail):
    """A failing input stores status = 1 and nothing else; the next call on the same objects is correct."""
    c = CASES["two_slots"]
    rig = Rig(ctx, c)
    dstat = ctx.to_device(np.array([3 if fail == "src_status" else 0], np.int32))
    try:
        if fail.startswith("count"):
            rig.frame.set(rig.nc + 1 if fail == "count_above" else -1)
        if fail == "pose_status":
            rig.pose.upload(pose_value(dict(c["pose"], status=1)))
        rig.insert(d_src_status=dstat.ptr.value)
        check(rig, rig.read(), reference(c, src_status=1))
        rig.frame.set(c["n_cur"])
        rig.pose.upload(pose_value(c["pose"]))
        ctx.check(lib().lorb_memset_dev(ctx.handle, dstat.ptr, C.c_int(0), C.c_size_t(4)), "memset")
        rig.insert(d_src_status=dstat.ptr.value)
        check(rig, rig.read(), reference(c))
    finally:
        dstat.free()
        rig.free()


def test_refused_then_forced(ctx):
    """The refused gate leaves everything but three fields of the record; LORB_KF_GATE_NONE on the same objects then
    inserts the same frame."""
    c = CASES["gate_8_of_20"]
    rig = Rig(ctx, c)
    try:
        rig.insert()
        check(rig, rig.read(), reference(c))
        rig.insert(gate=A.LORB_KF_GATE_NONE)
        ref = reference(c, gate=R.GATE_NONE)
        assert ref["inserted"]
        check(rig, rig.read(), ref)
    finally:
        rig.free()


def test_two_stores_on_one_context(ctx):
    """Two stores interleaved on one context, each with its own scratch: neither disturbs the other."""
    a, b = Rig(ctx, CASES["weights_2_3_3"]), Rig(ctx, CASES["gid_outside"])
    try:
        a.insert()
        b.insert()
        ra, rb = a.read(), b.read()
        check(a, ra, reference(a.c))
        check(b, rb, reference(b.c))
    finally:
        a.free()
        b.free()


def test_errors(ctx):
    c = CASES["two_slots"]
    rig = Rig(ctx, c)
    other = KeyframeStore(ctx, 2, 2, 2, 2)
    try:
        def call(match, **kw):
            a = dict(store=rig.store, n_max_cur=rig.nc, gate=A.LORB_KF_GATE_RATIO, fp=c["fp"])
            a.update(kw)
            with pytest.raises(LorbError, match=match):
                keyframe_insert(ctx, a["store"], a["fp"], rig.frame, rig.slots, rig.gid, rig.pose, rig.rec, n_max_cur=a["n_max_cur"],
                                gate=a["gate"])

        call("positive", n_max_cur=0)
        call("positive", n_max_cur=-1)
        call("max_kf_slots", store=other)  # a bound of 10 against 2 slots
        call("unknown gate", gate=2)
        call("n_levels", fp=dict(c["fp"], n_levels=0))
        call("n_levels", fp=dict(c["fp"], n_levels=17))
        keep = rig.frame.out.depth
        rig.frame.out.depth = None
        call("null array")
        rig.frame.out.depth = keep
        for caps in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0)):
            with pytest.raises(LorbError, match="positive"):
                KeyframeStore(ctx, *caps)
        with pytest.raises(LorbError, match="LDS"):
            KeyframeStore(ctx, SORT_MAX + 1, 4, 4, 4)
        s = c["store"]
        with pytest.raises(LorbError, match="capacity"):
            KeyframeStore(ctx, 1, 8, 8, 8, init=s)  # two keyframes
        with pytest.raises(LorbError, match="outside the store"):
            KeyframeStore(ctx, 4, 8, 8, 8, init=dict(s, obs=[[0], [1], [0, 2]]))
        with pytest.raises(LorbError, match="ascending"):
            bad = dict(s, conn=[{1: 1}, {0: 1}])
            h, keep = KeyframeStore._host(bad)
            keep["conn_kf"][:] = [1, 1]  # valid indices; make the second row's not ascend: one row of two equal keys
            keep["conn_off"][:] = [0, 2, 2]
            out = C.c_void_p()
            caps = A.KfStoreCaps(4, 8, 8, 8)
            ctx.check(lib().lorb_kf_store_create(ctx.handle, C.byref(caps), C.byref(h), C.byref(out)), "lorb_kf_store_create")
        rig.insert()  # the next call is fine
        check(rig, rig.read(), reference(c))
    finally:
        other.free()
        rig.free()
