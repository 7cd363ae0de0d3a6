"""GPU: UpdateLocalMap on the device (lorb_local_map_update_dev, lorb_local_map_ids_back_dev;
lorb_slam_amd.frame.local_map_update / local_map_ids_back) on hand-built stores (tests/local_map_cases.py),
bit for bit against the restatement tests/local_map_ref.py -- slots, gids, local ids, votes, keyframe
list, refer_kf, l2g, g2l, table rows and record -- with every byte past a count keeping what it held
before the call.  The object's own arrays are filled with sentinel bytes before each call (LocalMap.fill)
and are made larger than the store's counts, so writes past n_kf, n_points and n_local would show."""
import ctypes as C

import numpy as np
import pytest

import local_map_cases as LC
import local_map_ref as R
import lorb_slam_amd.window as W
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceMapStore, DeviceSlots, LocalMap, local_map_buffers, local_map_ids_back,
                                 local_map_result, local_map_update)
from lorb_slam_amd.runtime import LorbError, lib

pytestmark = pytest.mark.gpu

G, SENT, FILL = W.ORB_GUARD, W.ORB_SENTINEL, -77
SENT_I32 = int(np.full(4, SENT, np.uint8).view(np.int32)[0])
REC = C.sizeof(A.LocalMapResult)
CASES = LC.all_cases()
FIELDS = ("status", "n_cur", "n_held", "n_nulled", "n_voted", "n_local_kf", "refer_kf", "n_local")


class Counts:
    """A frame of which only counts[0] exists: all the local-map calls read of a lorb_frame_out."""

    def __init__(self, ctx, n_cur):
        self.ctx = ctx
        self.counts = ctx.to_device(np.array([n_cur, 0] + [FILL] * G, np.int32))
        self.out = A.FrameOut()
        self.out.counts = self.counts.ptr.value

    def set(self, n):
        v = np.array([n], np.int32)
        self.ctx.check(lib().lorb_memcpy_h2d(self.ctx.handle, self.counts.ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(4)), "h2d")

    def free(self):
        self.counts.free()


class Rig:
    """One case's device objects.  The capacities exceed the store's counts by a few entries."""

    def __init__(self, ctx, c, lmap=None):
        self.ctx, self.c = ctx, c
        s, n = c["store"], c["n_cur"]
        self.nc = n + 1
        self.store = DeviceMapStore(ctx, s, s["obs"], s["kf_bad"], s["kf_slots"], s["cov"])
        self.lmap = lmap or LocalMap(ctx, c["max_local"], len(s["kf_bad"]) + 3, s["n_points"] + 5)
        self.own = lmap is None
        self.frame = Counts(ctx, n)
        self.slots = DeviceSlots(ctx, self.nc, state=c["state"])
        self.gid, self.sid, self.rec = local_map_buffers(ctx, self.nc, c["gid"], FILL)
        self.extra = []
        self.ids = None
        if c["ids"] is not None:
            i = c["ids"]
            mrec = A.TrackFramesResult()
            mrec.motion.pass_ = i["pass_"]
            self.extra = [ctx.to_device(np.concatenate([i["assign"], np.full(G + 1, FILL, np.int32)])),
                          ctx.to_device(np.frombuffer(bytes(mrec), np.uint8)), ctx.to_device(i["last_gid"])]
            self.ids = A.TrackLocalIdSource(self.extra[0].ptr.value, self.extra[1].ptr.value, self.extra[2].ptr.value,
                                            len(i["last_gid"]), i["given"])

    def update(self, d_src_status=None, fill=True):
        if fill:
            self.lmap.fill()
        self.before = dict(slots=self.slots.numpy())
        return local_map_update(self.ctx, self.lmap, self.store, self.frame, self.slots, self.gid, self.sid, self.rec,
                                n_max_cur=self.nc, d_src_status=d_src_status, id_source=self.ids)

    def read(self):
        r = dict(rec=local_map_result(self.rec), rec_bytes=self.rec.numpy(), slots=self.slots.numpy(), gid=self.gid.numpy(),
                 sid=self.sid.numpy())
        r.update(self.lmap.numpy())
        return r

    def free(self):
        for a in (self.store, self.frame, self.slots, self.gid, self.sid, self.rec, *self.extra):
            a.free()
        if self.own:
            self.lmap.free()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def sentinel(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SENT).all()


def check(rig, r, ref=None):
    """Everything the call left against the restatement, and the bytes past every count."""
    c = rig.c
    s, n = c["store"], c["n_cur"]
    ref = ref or R.update_local_map(s, c["state"], c["gid"], n, rig.lmap.max_local, c["ids"])
    rec = r["rec"]
    want = dict(ref, n_local_kf=len(ref["local_kf"]))
    assert [getattr(rec, f) for f in FIELDS] == [want[f] for f in FIELDS], [(f, getattr(rec, f), want[f]) for f in FIELDS]
    assert (r["rec_bytes"][REC:] == SENT).all()
    # the slots: states, and nothing else of them
    assert np.array_equal(r["slots"]["state"][:n], ref["state"]) and sentinel(r["slots"]["state"][n:])
    assert all(np.array_equal(r["slots"][k].view(np.uint8), rig.before["slots"][k].view(np.uint8)) for k in ("pos", "desc"))
    assert np.array_equal(r["gid"][:n], ref["gid"]) and (r["gid"][n:] == FILL).all()
    nkf, npt, nl = len(s["kf_bad"]), s["n_points"], ref["n_local"]
    assert np.array_equal(r["kf_votes"][:nkf], ref["votes"]) and sentinel(r["kf_votes"][nkf:])
    nlk = len(ref["local_kf"])
    assert list(r["local_kf"][:nlk]) == ref["local_kf"] and sentinel(r["local_kf"][nlk:])
    assert np.array_equal(r["g2l"][:npt], ref["g2l"]) and sentinel(r["g2l"][npt:])
    cols = [k for k in R.COLS]
    if ref["status"] == 0:
        assert np.array_equal(r["sid"][:n], ref["slot_id"]) and (r["sid"][n:] == FILL).all()
        assert list(r["l2g"][:nl]) == ref["l2g"] and sentinel(r["l2g"][nl:])
        assert (r["is_bad"][:nl] == 0).all() and (r["is_bad"][nl:] == 1).all()
        for k in cols:
            assert nl == 0 or np.array_equal(raw(r[k][:nl]), raw(ref["rows"][k])), k
            assert sentinel(r[k][nl:]), k
    else:
        assert (r["sid"] == FILL).all() and sentinel(r["l2g"]) and (r["is_bad"] == 1).all()
        assert all(sentinel(r[k]) for k in cols)
    return ref


def run_case(ctx, name):
    rig = Rig(ctx, CASES[name])
    try:
        rig.update()
        r = rig.read()
        ref = check(rig, r)
        for k, want in CASES[name]["want"].items():  # the hand answers, once more on the device's side
            got = dict(status=r["rec"].status, votes=r["kf_votes"][:len(ref["votes"])], local_kf=r["local_kf"][:len(ref["local_kf"])],
                       refer_kf=r["rec"].refer_kf, n_voted=r["rec"].n_voted, n_held=r["rec"].n_held, n_nulled=r["rec"].n_nulled,
                       n_local=r["rec"].n_local, l2g=r["l2g"][:ref["n_local"]] if ref["status"] == 0 else [],
                       slot_id=r["sid"][:rig.c["n_cur"]], state=r["slots"]["state"][:rig.c["n_cur"]],
                       gid=r["gid"][:rig.c["n_cur"]])[k]
            assert np.array_equal(np.asarray(got), np.asarray(want)), (name, k)
        return r
    finally:
        rig.free()


# 1 - 4, 6, 7, 9 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in sorted(CASES) if not k.startswith("compact_")])
def test_case(ctx, name):
    run_case(ctx, name)


# 5 -- compaction across tile boundaries -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["all", "none", "alternating"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3 * 1024 + 1])
def test_compaction(ctx, n, mode):
    run_case(ctx, f"compact_{n}_{mode}")


# 6 -- overflow keeps c and d ----------------------------------------------------------------------------------
def test_overflow_keeps_votes_and_list(ctx):
    a, b = run_case(ctx, "exact_fit"), run_case(ctx, "overflow")
    assert (a["rec"].status, b["rec"].status, b["rec"].n_local) == (0, 2, 3)
    for k in ("kf_votes", "local_kf", "gid"):
        assert np.array_equal(a[k][:3], b[k][:3]), k
    assert np.array_equal(a["slots"]["state"], b["slots"]["state"])


# 8 -- status 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fail", ["count_above", "count_negative", "src_status"])
def test_status(ctx, fail):
    """A failing input stores status = 1 and nothing else; the next call on the same objects is correct."""
    rig = Rig(ctx, CASES["bad_point"])
    dstat = ctx.to_device(np.array([3 if fail == "src_status" else 0], np.int32))
    try:
        if fail != "src_status":
            rig.frame.set(rig.nc + 1 if fail == "count_above" else -1)
        rig.update(d_src_status=dstat.ptr.value)
        r = rig.read()
        assert r["rec"].status == 1
        rec = A.LocalMapResult.from_buffer_copy(r["rec_bytes"].tobytes()[:REC])
        rec.status = SENT_I32
        assert sentinel(np.frombuffer(bytes(rec), np.uint8)) and sentinel(r["rec_bytes"][REC:])
        assert all(np.array_equal(r["slots"][k].view(np.uint8), rig.before["slots"][k].view(np.uint8)) for k in r["slots"])
        assert np.array_equal(r["gid"][:rig.c["n_cur"]], rig.c["gid"]) and (r["gid"][rig.c["n_cur"]:] == FILL).all()
        assert (r["sid"] == FILL).all() and (r["is_bad"] == 1).all()
        for k in ("l2g", "g2l", "kf_votes", "local_kf", *R.COLS):
            assert sentinel(r[k]), k
        rig.frame.set(rig.c["n_cur"])
        ctx.check(lib().lorb_memset_dev(ctx.handle, dstat.ptr, C.c_int(0), C.c_size_t(4)), "memset")
        rig.update(d_src_status=dstat.ptr.value)
        check(rig, rig.read())
    finally:
        dstat.free()
        rig.free()


# 9 -- the id source against gids passed directly ------------------------------------------------------------------
def test_ids_given_equals_direct(ctx):
    a, b = run_case(ctx, "ids_given"), run_case(ctx, "ids_direct")
    for k in a:
        if k == "slots":
            assert all(np.array_equal(a[k][q].view(np.uint8), b[k][q].view(np.uint8)) for q in a[k])
        elif k != "rec":
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


# 10 -- ids_back -------------------------------------------------------------------------------------------------
def test_ids_back(ctx):
    """After an update the local stage is played by hand: slot 3 (a created point) is matched to local row 2,
    slot 5 (a held point whose gid lay outside the store) stays; slot 1 was emptied by step c; slot 4 holds a
    local point; slot 5 is given a gid the local map does not name and keeps it."""
    rig = Rig(ctx, CASES["bad_point"])
    dstat = ctx.to_device(np.array([0], np.int32))
    try:
        rig.update()
        r = rig.read()
        ref = check(rig, r)
        n = rig.c["n_cur"]
        sid = r["sid"].copy()
        sid[3] = 2  # the local stage matched slot 3 to local row 2 (global point 3)
        gid = r["gid"].copy()
        gid[5] = 11  # a held point outside the local map (any gid the table does not name)
        for dev, host in ((rig.sid, sid), (rig.gid, gid)):
            ctx.check(lib().lorb_memcpy_h2d(ctx.handle, dev.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)), "h2d")
        state = r["slots"]["state"][:n]
        want = R.ids_back(state, sid[:n], gid[:n], ref["l2g"])
        assert list(want) == [0, -1, -1, 3, 2, 11]  # by hand: l2g = [0, 2, 3]
        # a non-zero status writes nothing
        ctx.check(lib().lorb_memset_dev(ctx.handle, dstat.ptr, C.c_int(1), C.c_size_t(4)), "memset")
        local_map_ids_back(ctx, rig.lmap, rig.frame, rig.slots, rig.sid, rig.gid, n_max_cur=rig.nc, d_local_status=dstat.ptr.value)
        assert np.array_equal(rig.gid.numpy(), gid)
        ctx.check(lib().lorb_memset_dev(ctx.handle, dstat.ptr, C.c_int(0), C.c_size_t(4)), "memset")
        local_map_ids_back(ctx, rig.lmap, rig.frame, rig.slots, rig.sid, rig.gid, n_max_cur=rig.nc, d_local_status=dstat.ptr.value)
        got = rig.gid.numpy()
        assert np.array_equal(got[:n], want) and (got[n:] == FILL).all()
        assert np.array_equal(rig.sid.numpy(), sid)
        # a count out of range writes nothing either
        rig.frame.set(rig.nc + 1)
        ctx.check(lib().lorb_memcpy_h2d(ctx.handle, rig.gid.ptr, gid.ctypes.data_as(C.c_void_p), C.c_size_t(gid.nbytes)), "h2d")
        local_map_ids_back(ctx, rig.lmap, rig.frame, rig.slots, rig.sid, rig.gid, n_max_cur=rig.nc)
        assert np.array_equal(rig.gid.numpy(), gid)
    finally:
        dstat.free()
        rig.free()


# 11 -- two objects on one context, and the context's other chains in between ------------------------------------------
def test_two_objects_and_context_reuse(ctx):
    import test_gpu_track_local as TL
    a, b = Rig(ctx, CASES["votes"]), Rig(ctx, CASES["grow_9_to_11"])
    try:
        a.update()
        b.update()
        a.update(fill=False)  # a second call on the same object: counters and flags are cleared inside the call
        ra, rb = a.read(), b.read()
        check(a, ra)
        check(b, rb)
        s = TL.problem(33, 300, 400, 58)
        want = TL.expected(s, 0.0)
        TL.check(TL.run(ctx, s, 0.0), want)
        b.update()
        TL.check(TL.run(ctx, s, 0.0), want)
        check(b, b.read())
        # one object, two stores in turn: what the first call flagged and voted does not leak into the second
        c = Rig(ctx, CASES["dedupe"], lmap=LocalMap(ctx, 8, 8, 16))
        d = Rig(ctx, CASES["bad_point"], lmap=c.lmap)
        try:
            c.update()
            check(c, c.read())
            d.update()
            check(d, d.read())
        finally:
            c.free()
            d.free()
            c.lmap.free()
    finally:
        a.free()
        b.free()


# 12 -- errors with a live context name the cause ----------------------------------------------------------------
def test_errors(ctx):
    rig = Rig(ctx, CASES["votes"])
    other = LocalMap(ctx, 2, 2, 2)
    try:
        def call(match, **kw):
            a = dict(lmap=rig.lmap, store=rig.store, n_max_cur=rig.nc)
            a.update(kw)
            with pytest.raises(LorbError, match=match):
                local_map_update(ctx, a["lmap"], a["store"], rig.frame, rig.slots, rig.gid, rig.sid, rig.rec,
                                 n_max_cur=a["n_max_cur"], id_source=rig.ids)

        call("positive", n_max_cur=0)
        call("positive", n_max_cur=-1)
        call("8M", n_max_cur=(8 << 20) // rig.lmap.max_local + 1)
        call("max_points", lmap=other)  # 6 points against a capacity of 2
        sc = rig.store.c
        for field, match in (("n_obs", "negative"), ("n_kf_slots", "negative"), ("n_cov", "negative")):
            keep = getattr(sc, field)
            setattr(sc, field, -1)
            call(match)
            setattr(sc, field, keep)
        sc.n_kf = rig.lmap.max_kf + 1
        call("max_kf")
        sc.n_kf = 5
        sc.points.in_frame = rig.gid.ptr.value
        call("in_frame")
        sc.points.in_frame = None
        desc = sc.points.desc
        sc.points.desc = desc + 4
        call("16-byte")
        sc.points.desc = None
        call("null array")
        sc.points.desc = desc
        for caps in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
            with pytest.raises(LorbError, match="positive"):
                LocalMap(ctx, *caps)
        with pytest.raises(LorbError, match="positive"):
            local_map_ids_back(ctx, rig.lmap, rig.frame, rig.slots, rig.sid, rig.gid, n_max_cur=0)
        rig.update()  # the next call is fine
        check(rig, rig.read())
    finally:
        other.free()
        rig.free()
