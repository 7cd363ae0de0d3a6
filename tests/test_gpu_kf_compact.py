"""GPU: lorb_kf_store_compact_dev (lorb_slam_amd.frame.KeyframeStore.compact), bit for bit against the restatement
tests/kf_compact_ref.py.

Every store, geometry and life array over its WHOLE capacity (integers equal, floats as bytes, sentinel bytes written
past every count beforehand), the gid tables with their guard bands, d_map and the record are compared with what
kf_compact_ref.compact_arrays makes of the same arrays read before the call: what the call must write, and every byte it
must leave alone.

Sizes (the workgroup tile is 1024 points): 1023 / 1024 / 1025 / 2049 points; dropped points on both sides of a tile
edge and straddling it; the first and the last point; every point; none; a keyframe row of more than 1025 slots and a
gid table of 1025 entries; a table holding one point twice; table entries that are -1, outside the store, or past the
count; zero tables; the same table named twice.
Behaviour: a bad point kept by a keyframe slot only, by a table only, by an observation only; each status-1 path
against sentinels everywhere; a refused call followed by a good one; two compactions in a row; the words at rest
between calls, by behaviour: an insertion, a cull and a BA gather enqueued straight behind a compaction equal the
restatement's."""
import ctypes as C

import numpy as np
import pytest

import kf_ba_ref as B
import kf_compact_ref as M
import kf_cull_cases as CC
import kf_cull_ref as L
import kf_store_cases as KC
import kf_store_ref as R
import test_gpu_kf_ba as KB
import test_gpu_kf_cull as CU
import test_gpu_kf_store as KS
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import (DeviceBlock, DeviceSlots, KeyframeStore, _sentinel, keyframe_ba_result, keyframe_compact_record,
                                 keyframe_cull, keyframe_cull_record, keyframe_cull_result, keyframe_insert, keyframe_insert_result,
                                 keyframe_ba_record, keyframe_local_ba)
from lorb_slam_amd.runtime import Context, LorbError, lib

pytestmark = pytest.mark.gpu

G, SENT, FILL, SENT_I32 = KS.G, KS.SENT, KS.FILL, KS.SENT_I32
raw, sentinel, all_arrays, h2d, memset = KS.raw, KS.sentinel, CU.all_arrays, CU.h2d, CU.memset
REC = C.sizeof(A.KfCompactResult)
TILE = 1024  # points per tile of the compaction's kernels (kT in lorb_kfcompact.hip)
COUNTS = ("n_points", "n_obs", "n_kf_slots")


# -- the cases -------------------------------------------------------------------------------------------------------
def kill(s, geom, points, keep_slot=(), keep_obs=()):
    """What lorb_kf_store_cull_dev leaves of a culled point: bad, out of every keyframe row, no observation.
    keep_slot: the rows go on naming it; keep_obs: it stays observed, its slots emptied (a store without geometry)."""
    for p in points:
        s["is_bad"][p] = 1
        for f, j in zip(s["obs"][p], geom["obs_slot"][p]):
            if p not in keep_slot:
                s["kf_slots"][f][j] = -1
        if p not in keep_obs:
            s["obs"][p], geom["obs_slot"][p] = [], []


def table(rng, P, count, n_max, hold=(), twice=None, past=(), avoid=()):
    """A gid table: `count` examined entries -- the points of `hold`, `twice` two times, -1, indices outside the store,
    random points but those of `avoid` -- and entries past the count that name the points of `past` (then FILL)."""
    g = np.full(n_max + G, FILL, np.int32)
    body = list(hold) + ([twice, twice] if twice is not None else []) + [-1, P, P + 4, -1]
    pool = np.setdiff1d(np.arange(P), np.asarray(list(avoid), np.int64))
    body += [int(v) for v in rng.choice(pool, max(count - len(body), 0))]
    body = [body[i] for i in rng.permutation(len(body))][:count]
    g[:len(body)] = body
    g[count:count + len(past)] = list(past)[:n_max - count]
    return dict(gid=g, n_max=n_max, count=count)


def generated(n_points, n_kf, seed, drop=(), keep_slot=(), keep_obs=(), table_hold=(), tables=1, table_count=40, alive=False,
              everyone=False, geom=True):
    rng = np.random.default_rng(12000 + seed)
    c = CC.generated(n_points, n_kf, seed)
    s, g = c["store"], c["geom"]
    if alive:                                            # nothing to drop: every bad point is still observed
        for p in range(n_points):
            if not s["obs"][p]:
                s["is_bad"][p] = 0
    def observed(p):                                     # the next point that is alive and observed: a hold to take away
        while s["is_bad"][p] or not s["obs"][p]:
            p += 1
        return p

    keep_slot, keep_obs, table_hold = ([observed(p) for p in v] for v in (keep_slot, keep_obs, table_hold))
    drop = range(n_points) if everyone else sorted(set(drop) | set(keep_slot) | set(keep_obs) | set(table_hold))
    kill(s, g, drop, keep_slot, keep_obs)
    P = n_points
    past = [p for p in drop if p not in keep_slot and p not in keep_obs and p not in table_hold][:3]
    tabs = []
    if tables and not everyone:
        live = [p for p in range(P) if not s["is_bad"][p]]
        avoid = set(drop) - set(table_hold)
        tabs.append(table(rng, P, table_count, table_count + 5, hold=table_hold, twice=live[len(live) // 2], past=past, avoid=avoid))
        for i in range(1, tables):
            tabs.append(table(rng, P, 7 + i, 12 + i, past=past[:1], avoid=avoid))
    elif tables:
        tabs.append(dict(gid=np.array([-1, P, -1] + [FILL] * G, np.int32), n_max=3, count=3))
    return dict(store=s, geom=g if geom else None, obs_slot=g["obs_slot"], life=c["life"], tables=tabs, drop=list(drop),
                keep_slot=list(keep_slot), keep_obs=list(keep_obs), table_hold=list(table_hold))


def cases():
    c = {}
    for n in (1023, 1024, 1025):                         # the first and the last point; both sides of the tile edge
        edge = [p for p in (TILE - 2, TILE - 1, TILE) if p < n]
        c[f"points_{n}"] = generated(n, 6, seed=n, drop=sorted(set([0, 1, 5, n // 2, n - 1] + edge)))
    # a run of dropped points straddling the first tile edge, single ones on either side of the second, the last
    c["points_2049_straddle"] = generated(2 * TILE + 1, 2, seed=7, drop=list(range(TILE - 5, TILE + 6)) + [2 * TILE - 1, 2 * TILE],
                                          table_count=TILE + 1, tables=2)
    c["points_2049_left_of_edge"] = generated(2 * TILE + 1, 3, seed=8, drop=[0, TILE - 1, 2 * TILE - 1])
    c["points_2049_right_of_edge"] = generated(2 * TILE + 1, 3, seed=9, drop=[TILE, 2 * TILE], tables=3)
    c["every_point"] = generated(1030, 4, seed=10, everyone=True)
    c["none"] = generated(1100, 5, seed=11, alive=True)
    c["zero_tables"] = generated(300, 4, seed=12, drop=[0, 7, 150, 299], tables=0)
    c["eight_tables"] = generated(500, 4, seed=13, drop=[3, 250, 499], tables=8, table_count=20)
    c["kept_by_slot_only"] = generated(200, 4, seed=14, drop=[4, 5, 6, 120], keep_slot=[5, 120])
    c["kept_by_table_only"] = generated(200, 4, seed=15, drop=[4, 5, 6, 120], table_hold=[5, 120])
    c["kept_by_observation_only"] = generated(200, 4, seed=16, drop=[4, 5, 6, 120], keep_obs=[5, 120], geom=False)
    return c


CASES = cases()


# -- the rig ---------------------------------------------------------------------------------------------------------
class Rig:
    """A store (with geometry unless the case has none) and life a few rows larger than its counts, sentinel bytes
    behind every count; the tables with a guard band and their count words; the source status word; d_map; the record."""

    def __init__(self, ctx, case, slack=5, d_map=True):
        self.ctx, self.case = ctx, case
        s = case["store"]
        cn = self.cn = R.counts(s)
        self.store = KeyframeStore(ctx, cn["n_kf"] + slack, cn["n_points"] + slack, cn["n_obs"] + slack, cn["n_kf_slots"] + slack,
                                   init=s, geom=case["geom"])
        self.store.fill(cn)
        self.store.fill_geometry(cn)
        self.store.fill_life(cn)
        self.store.write_life(case["life"])
        CU.set_frame_word(ctx, self.store, case["life"]["frame_word"])
        self.gids = [ctx.to_device(t["gid"]) for t in case["tables"]]
        self.words = ctx.to_device(np.array([0] + [t["count"] for t in case["tables"]] + [FILL] * G, np.int32))
        self.map = ctx.to_device(np.full(cn["n_points"] + slack + G, FILL, np.int32)) if d_map else None
        self.rec = keyframe_compact_record(ctx)

    def set(self, src_status=0, counts=None):
        h2d(self.ctx, self.words, [src_status] + [t["count"] for t in self.case["tables"]] if counts is None else [src_status] + list(counts))

    def tables(self):
        w = self.words.ptr.value
        return [(g, w + 4 * (i + 1), t["n_max"]) for i, (g, t) in enumerate(zip(self.gids, self.case["tables"]))]

    def run(self, status_word=True, tables=None):
        memset(self.ctx, self.rec, REC)
        self.store.compact(self.rec, tables=self.tables() if tables is None else tables,
                           d_src_status=self.words.ptr.value if status_word else None, d_map=self.map)
        b = self.rec.numpy()
        assert sentinel(b[REC:])
        return A.KfCompactResult.from_buffer_copy(b.tobytes()[:REC])

    def snapshot(self):
        """Everything the call may touch, as it stands (waits)."""
        n = self.store.counts()
        return dict(arrays=all_arrays(self.store), counts=n, tables=[g.numpy() for g in self.gids],
                    map=None if self.map is None else self.map.numpy(), words=self.words.numpy())

    def free(self):
        for a in (self.store, self.words, self.rec, self.map, *self.gids):
            if a is not None:
                a.free()


def restate(case, before, src_status=0, counts=None):
    tabs = [dict(gid=g, n_max=t["n_max"], count=t["count"] if counts is None else counts[i])
            for i, (g, t) in enumerate(zip(before["tables"], case["tables"]))]
    return M.compact_arrays(before["arrays"], before["counts"], tabs, src_status=src_status, d_map=before["map"])


def check(rig, rec, ref, before):
    """The device after a call against the restatement of the state before it: every array over its whole capacity,
    the tables and d_map with their guard bands, the counts, the record (fields the call does not write keep the
    sentinel)."""
    CU.same_record(rec, ref["rec"], M.FIELDS)
    after = rig.snapshot()
    for k, v in ref["arrays"].items():
        assert np.array_equal(raw(after["arrays"][k]), raw(v)), k
    for i, t in enumerate(ref["tables"]):
        assert np.array_equal(after["tables"][i], t["gid"]), i
    if ref["d_map"] is not None:
        assert np.array_equal(after["map"], ref["d_map"])
    assert after["counts"] == dict(before["counts"], n_points=ref["n_points"])
    assert np.array_equal(after["words"], before["words"])
    return after


# -- 2. against the restatement ----------------------------------------------------------------------------------------
def case_is_what_its_name_says(name, case, ref, P):
    m, r = ref["d_map"][:P], ref["rec"]
    dropped = set(int(p) for p in np.nonzero(m < 0)[0])
    assert r["status"] == 0 and r["n_points_before"] == P == case["store"]["n_points"]
    held = set(case["keep_slot"]) | set(case["keep_obs"]) | set(case["table_hold"])
    assert set(case["drop"]) - held <= dropped and not dropped & held
    for t in case["tables"]:                              # entries past the count name dropped points and stay
        n = t["count"]
        assert all(int(g) in dropped or g == FILL for g in t["gid"][n:]) and (name in ("every_point", "none") or t["gid"][n] != FILL)
    if name.startswith("points_"):
        assert P == int(name.split("_")[1]) and r["n_bad_kept"] > 0 and r["n_gids_mapped"] > 0 and r["n_kf_slots_mapped"] > 0
        assert any(case["store"]["is_bad"][g] == 0 and list(t["gid"][:t["count"]]).count(g) >= 2 for t in case["tables"]
                   for g in t["gid"][:t["count"]] if 0 <= g < P)                           # a table holds one point twice
    if name in ("points_1023", "points_1024", "points_1025"):
        assert {0, P - 1} <= dropped
    if name == "points_2049_straddle":
        assert set(range(TILE - 5, TILE + 6)) | {2 * TILE - 1, 2 * TILE} <= dropped
        assert max(len(row) for row in case["store"]["kf_slots"]) >= TILE + 1 and case["tables"][0]["count"] == TILE + 1
    if name == "points_2049_left_of_edge":
        assert {TILE - 1, 2 * TILE - 1} <= dropped and not {TILE, 2 * TILE} & dropped
    if name == "points_2049_right_of_edge":
        assert {TILE, 2 * TILE} <= dropped and not {TILE - 1, 2 * TILE - 1} & dropped
    if name == "every_point":
        assert r["n_points"] == 0 and r["n_dropped"] == P and ref["arrays"]["obs_off"][0] == 0
    if name == "none":
        assert r["n_dropped"] == 0 and r["n_bad_kept"] > 0 and list(m) == list(range(P))
    if name.startswith("kept_by"):
        assert len(held) == 2 and {4, 6} <= dropped and all(m[p] >= 0 and case["store"]["is_bad"][p] for p in held)
        named = {int(g) for t in case["tables"] for g in t["gid"][:t["count"]]}
        for p in held:                                    # the one hold, and no other
            assert bool(case["store"]["obs"][p]) == (name == "kept_by_observation_only")
            assert any(p in row for row in case["store"]["kf_slots"]) == (name == "kept_by_slot_only")
            assert (p in named) == (name == "kept_by_table_only")
    if name == "eight_tables":
        assert len(case["tables"]) == 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_compact(ctx, name):
    case = CASES[name]
    rig = Rig(ctx, case)
    try:
        before = rig.snapshot()
        P = before["counts"]["n_points"]
        ref = restate(case, before)
        r = ref["rec"]
        case_is_what_its_name_says(name, case, ref, P)
        rec = rig.run()
        mid = check(rig, rec, ref, before)
        if r["n_dropped"] == 0:                           # not a byte of the store or of a table changes
            for k in mid["arrays"]:
                assert np.array_equal(raw(mid["arrays"][k]), raw(before["arrays"][k])), k
            for a, b in zip(mid["tables"], before["tables"]):
                assert np.array_equal(a, b)
        if case["geom"] is not None and r["n_points"]:    # the invariant on what the device holds
            st, dg = rig.store.read(), rig.store.read_geometry()
            off, o = st["csr"]["kf_slot_off"], 0
            for p, obs in enumerate(st["obs"]):
                for f in obs:
                    assert st["csr"]["kf_slot_point"][off[f] + dg["obs_slot"][o]] == p, (p, f)
                    o += 1
        # a second compaction drops nothing: the holds are back at rest, the store stands
        ref2 = restate(case, mid)
        assert ref2["rec"]["n_dropped"] == 0 and ref2["rec"]["n_bad_kept"] == r["n_bad_kept"]
        rec = rig.run(status_word=False)
        last = check(rig, rec, ref2, mid)
        for k in last["arrays"]:
            assert np.array_equal(raw(last["arrays"][k]), raw(mid["arrays"][k])), k
    finally:
        rig.free()


def test_the_same_table_named_twice_is_mapped_once(ctx):
    case = CASES["kept_by_table_only"]
    rig = Rig(ctx, case)
    try:
        before = rig.snapshot()
        ref = restate(case, before)
        assert ref["rec"]["n_dropped"] > 0 and ref["rec"]["n_gids_mapped"] > 0
        rec = rig.run(tables=rig.tables() * 2)
        check(rig, rec, ref, before)
    finally:
        rig.free()


@pytest.mark.parametrize("fail", ["src_status", "count_negative", "count_above", "second_table_above"])
def test_refused_call_then_a_good_one(ctx, fail):
    """Status 1 stores the status and nothing else -- sentinels everywhere stay, d_map included; the good call behind
    it equals the good call alone."""
    case = CASES["eight_tables"]
    rig = Rig(ctx, case)
    try:
        good = [t["count"] for t in case["tables"]]
        bad = list(good)
        if fail == "count_negative":
            bad[0] = -1
        elif fail == "count_above":
            bad[0] = case["tables"][0]["n_max"] + 1
        elif fail == "second_table_above":
            bad[7] = case["tables"][7]["n_max"] + 1
        src = 2 if fail == "src_status" else 0
        rig.set(src, bad)
        before = rig.snapshot()
        ref = restate(case, before, src_status=src, counts=bad)
        assert ref["rec"] == dict(status=1)
        rec = rig.run()
        after = check(rig, rec, ref, before)
        for k in after["arrays"]:
            assert np.array_equal(raw(after["arrays"][k]), raw(before["arrays"][k])), k
        assert (after["map"] == FILL).all()
        rig.set(0, good)
        before = rig.snapshot()
        ref = restate(case, before)
        assert ref["rec"]["status"] == 0 and ref["rec"]["n_dropped"] >= 3
        check(rig, rig.run(status_word=fail != "src_status"), ref, before)
    finally:
        rig.free()


def test_compact_errors(ctx):
    """LORB_E_INVALID before anything is enqueued; the next call is fine."""
    case = CASES["zero_tables"]
    rig = Rig(ctx, case)
    gid, cnt = ctx.to_device(np.zeros(8, np.int32)), ctx.to_device(np.array([4], np.int32))
    try:
        before = rig.snapshot()
        with pytest.raises(LorbError, match="gid tables"):
            rig.store.compact(rig.rec, tables=[(gid, cnt)] * 9)
        with pytest.raises(LorbError, match="positive"):
            rig.store.compact(rig.rec, tables=[(gid, cnt, 0)])
        with pytest.raises(LorbError, match="another bound or count"):
            rig.store.compact(rig.rec, tables=[(gid, cnt, 8), (gid, cnt, 6)])
        with pytest.raises(LorbError, match="null array"):
            rig.store.compact(rig.rec, tables=[(gid, 0)])
        # the null arguments and the table count, with a live context, straight through the C entry point
        f, h, st, rec = lib().lorb_kf_store_compact_dev, ctx.handle, rig.store._p, rig.rec.ptr
        tab = (A.KfGidTable * 8)(*[A.KfGidTable(gid.ptr.value, 8, cnt.ptr.value)] * 8)
        two = C.c_int32(2)
        assert f(h, None, None, tab, two, None, rec) == -1                          # no store
        assert f(h, st, None, tab, two, None, None) == -1                           # no record
        assert f(h, st, None, None, two, None, rec) == -1                           # tables promised, none given
        assert f(h, st, None, tab, C.c_int32(-1), None, rec) == -1 and f(h, st, None, tab, C.c_int32(9), None, rec) == -1
        for field in ("d_gid", "d_count"):
            bad = (A.KfGidTable * 2)(A.KfGidTable(gid.ptr.value, 8, cnt.ptr.value), A.KfGidTable(gid.ptr.value + 4, 4, cnt.ptr.value))
            setattr(bad[1], field, None)
            assert f(h, st, None, bad, two, None, rec) == -1, field
        c2 = Context(0)
        theirs = KeyframeStore(c2, 2, 8, 8, 8)
        try:                                             # a store of another context, through this one
            rc = lib().lorb_kf_store_compact_dev(ctx.handle, theirs._p, None, None, C.c_int32(0), None, rig.rec.ptr)
            with pytest.raises(LorbError, match="another context"):
                ctx.check(rc, "lorb_kf_store_compact_dev")
        finally:
            theirs.free()
            c2.close()
        ref = restate(case, before)
        assert ref["rec"]["n_dropped"] >= 4
        check(rig, rig.run(), ref, before)
    finally:
        for a in (rig, gid, cnt):
            a.free()


# -- the words at rest, by behaviour: an insertion, a cull and a BA gather straight behind a compaction ----------------
def behind_a_compaction_restated():
    """The restatements in the order of test_insert_cull_gather_behind_a_compaction."""
    case = CC.hand_case()
    f = case["frame"]
    n, nmax = f["n_cur"], f["n_max_cur"]
    c1 = L.cull(case["store"], case["obs_slot"], case["life"], case["kf"], case["params"], frame=f)
    tab = dict(gid=np.concatenate([c1["gid"], np.full(nmax - n + G, FILL, np.int32)]), n_max=nmax, count=n)
    cm = M.compact_store(c1["store"], c1["obs_slot"], c1["life"], [tab])
    assert cm["dropped"] == [1, 2] and cm["rec"]["n_bad_kept"] == 1 and list(cm["map"]) == [0, -1, -1, 1, 2, 3, 4]   # p0: bad, held
    s1, geom1 = cm["store"], dict(case["geom"], obs_slot=cm["obs_slot"])
    gid1 = cm["tables"][0]["gid"][:n]
    # the frame becomes keyframe 4: slots as the cull left them; depth on the two slots it emptied
    k = KC.case(s1, list(c1["state"]), list(gid1), {}, depth=[3.0 if st == R.EMPTY else KC.NO for st in c1["state"]], gate=R.GATE_NONE,
                seed=91, slack=6)
    k["n_max_cur"] = nmax
    ins = R.insert_keyframe(s1, k["caps"], k["fp"], k["frame"], k["pose"], k["slots"], k["gid"], n, nmax, R.GATE_NONE)
    assert ins["inserted"] and ins["rec"]["n_created"] == 2 and ins["rec"]["n_observed"] >= 1
    life1 = dict(cm["life"], frame_word=7)
    life2 = L.insert_life(life1, s1, k["frame"], k["slots"], k["gid"], ins)
    geom2 = B.insert_geometry(geom1, ins, k["frame"], KB.POSE6, n)
    c2 = L.cull(ins["store"], geom2["obs_slot"], life2, ins["kf"], (0.25, 0, 2, 3),
                frame=dict(n_cur=n, n_max_cur=nmax, state=ins["state"], gid=ins["gid"]))
    assert len(c2["culled"]) >= 2                             # the created points have one observation
    geom3 = dict(geom2, obs_slot=c2["obs_slot"])
    want = B.gather(c2["store"], geom3, ins["kf"])
    assert want["rec"]["status"] == 0 and want["rec"]["n_points"] > 0
    return dict(case=case, f=f, n=n, nmax=nmax, c1=c1, cm=cm, k=k, ins=ins, c2=c2, geom3=geom3, want=want)


def test_insert_cull_gather_behind_a_compaction(ctx):
    """The hand case of the cull: cull (p1 and p2 go bad), compact with the tracker's frame as the one table, then --
    nothing waited for in between -- the frame inserted as keyframe 4, culled, and its window gathered.  Everything
    equals the restatements applied in the same order: the insertion's owner words, the BA's first positions, the
    cull's marks and the compaction's holds were at rest."""
    r = behind_a_compaction_restated()
    case, f, n, nmax, c1, cm, k, ins, c2, geom3, want = (r[x] for x in ("case", "f", "n", "nmax", "c1", "cm", "k", "ins", "c2", "geom3", "want"))
    caps = k["caps"]
    cn = R.counts(case["store"])
    store = KeyframeStore(ctx, caps["max_kf"], caps["max_points"] + 4, caps["max_obs"] + 8, caps["max_kf_slots"], init=case["store"],
                          geom=case["geom"])
    store.fill(cn)
    store.fill_geometry(cn)
    store.fill_life(cn)
    store.write_life(case["life"])
    CU.set_frame_word(ctx, store, 7)
    frame = KS.Frame(ctx, k)
    slots = DeviceSlots(ctx, nmax, state=f["state"], pos=k["slots"]["pos"], desc=k["slots"]["desc"])
    g = np.full(nmax + G, FILL, np.int32)
    g[:n] = f["gid"]
    gid = ctx.to_device(g)
    pose = DeviceBlock(ctx, A.FramePose, KB.pose_value(k["pose"], KB.POSE6))
    words = ctx.to_device(np.array([case["kf"], 0], np.int32))
    irec, crec, crec2, brec, mrec = (_sentinel(ctx, KS.REC + G, np.uint8), keyframe_cull_record(ctx), keyframe_cull_record(ctx),
                                     keyframe_ba_record(ctx), keyframe_compact_record(ctx))
    dmap = ctx.to_device(np.full(caps["max_points"] + 4, FILL, np.int32))
    try:
        d, ir = words.ptr.value, irec.ptr.value
        keyframe_cull(ctx, store, d, crec, d_src_status=d + 4, params=case["params"], cur=frame, cur_slots=slots, slot_gid=gid, n_max_cur=nmax)
        store.compact(mrec, tables=[(gid, frame.out.counts, nmax)], d_src_status=d + 4, d_map=dmap)
        keyframe_insert(ctx, store, k["fp"], frame, slots, gid, pose, irec, n_max_cur=nmax, gate=R.GATE_NONE)
        keyframe_cull(ctx, store, ir + A.KfInsertResult.kf.offset, crec2, d_src_status=ir + A.KfInsertResult.status.offset,
                      params=(0.25, 0, 2, 3), cur=frame, cur_slots=slots, slot_gid=gid, n_max_cur=nmax)
        keyframe_local_ba(ctx, store, k["fp"], ir + A.KfInsertResult.kf.offset, brec, d_src_status=ir + A.KfInsertResult.status.offset,
                          gather_only=True)
        ctx.sync()
        CU.same_record(keyframe_cull_result(crec), c1["rec"], L.CULL_FIELDS)
        CU.same_record(A.KfCompactResult.from_buffer_copy(mrec.numpy().tobytes()[:REC]), cm["rec"], M.FIELDS)
        assert list(dmap.numpy()[:7]) == list(cm["map"]) and (dmap.numpy()[7:] == FILL).all()
        rec = keyframe_insert_result(irec)
        for fld in R.FIELDS:
            assert getattr(rec, fld) == ins["rec"].get(fld, SENT_I32), fld
        CU.same_record(keyframe_cull_result(crec2), c2["rec"], L.CULL_FIELDS)
        s = c2["store"]
        KS.same_store(store.read(), s)
        KB.same_geometry(store, geom3)
        CU.same_life(store, c2["life"], R.counts(s))
        B.check_invariant(s, geom3)
        got_g, got_s = gid.numpy(), slots.numpy()
        assert np.array_equal(got_g[:n], c2["gid"]) and (got_g[n:] == FILL).all() and np.array_equal(got_s["state"][:n], c2["state"])
        ra = keyframe_ba_result(brec)
        assert ra.status == 0 and ra.kf == ins["kf"]
        win = store.ba_window(ra)
        for key in KB.WINDOW_INT:
            assert np.array_equal(win[key], want[key]), key
        for key in KB.WINDOW_FLOAT:
            assert np.array_equal(raw(win[key]), raw(np.asarray(want[key], np.float32))), key
    finally:
        for a in (store, frame, slots, gid, pose, words, irec, crec, crec2, brec, mrec, dmap):
            a.free()
