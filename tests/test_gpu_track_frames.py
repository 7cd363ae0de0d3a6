"""GPU parity of the device slots (lorb_frame_slots_fill_dev) and of motion tracking straight from two
device-built frames (lorb_track_motion_frames_dev; lorb_slam_amd.frame.fill_slots / track_motion_frames)
against the oracle alone: O.orb_extract / O.compute_stereo_matches build the frames, O.unproject_stereo
the created points, O.search_by_projection_frame at 15 and 30 the matches, O.ba_pose_only the pose; the
slot expectations are numpy over the oracle's assign.  assign, pass, both match counts, n_residuals,
n_last, n_cur, n_created and both slot sets -- guard bands included -- must be bit-equal, the pose
within the motion chain's tolerances.  The frames are A = case(name) and B = case(name, 2, 777) of
tests/test_gpu_frame.py (every band 2 pixels further, other pixel noise); the last frame sits at the
identity and the predicted pose is the identity moved by dx along x.  Every case first asserts, from
the oracle alone, the property that makes it that case."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import lorb_slam_amd.window as W
import test_gpu_frame as TF
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import DeviceSlots, FrameBuilder, fill_slots, track_motion_frames
from lorb_slam_amd.runtime import LorbError, lib
from test_gpu_track_motion import close, summaries_agree

pytestmark = pytest.mark.gpu

UNCHANGED, NULL = A.LORB_ASSIGN_UNCHANGED, A.LORB_ASSIGN_NULL
EMPTY, FREE, LOCKED = A.LORB_SLOT_EMPTY, A.LORB_SLOT_FREE, A.LORB_SLOT_LOCKED
UPDATE, INIT = A.LORB_SLOTS_UPDATE_FRAME, A.LORB_SLOTS_INITIALIZE
G, SENT = W.ORB_GUARD, W.ORB_SENTINEL
FILL = -77  # what assign holds before the call
I4 = np.eye(4, dtype=np.float32)

# name -> (n_left of A, of B), keypoints of A with depth >= 0 -- the figures the shapes were chosen by
SHAPES = {"160x120": ((111, 111), 39), "376x240": ((271, 270), 125), "320x256": ((495, 500), 254)}
DX_PASS0 = 0.5  # 160x120: both radii find <= 20 (asserted below)
# (name, dx) -> the oracle's (matches at 15, at 30 or -1, pass); all last slots EMPTY on entry
CASES = {("160x120", 0.0): (39, -1, 1), ("160x120", 0.2): (12, 28, 2), ("160x120", DX_PASS0): None,
         ("376x240", 0.2): (33, -1, 1), ("320x256", 0.1): (211, -1, 1)}
RETRY_FIGURES = {("376x240", 0.2): 96, ("320x256", 0.1): 242}  # what a4 at 30 finds where pass 1 stood


def frames(name):
    return TF.case(name), TF.case(name, 2, 777)


def prediction(dx):
    """(pose_init, cur_Tcw): the identity moved by dx along x."""
    T = I4.copy()
    T[0, 3] = dx
    return np.array([0, 0, 0, dx, 0, 0], np.float32), T


def guarded(a, n_max, width=None):
    """a (n entries) as the first entries of an n_max + G array of sentinel bytes."""
    shape = (n_max + G,) if width is None else (n_max + G, width)
    out = np.full(int(np.prod(shape)) * np.dtype(a.dtype).itemsize, SENT, np.uint8).view(a.dtype).reshape(shape)
    out[:len(a)] = a
    return out


def entry_slots(n_max, state=None, pos=None, desc=None):
    """Host image of a DeviceSlots as the call finds it."""
    s = dict(state=np.full(n_max + G, SENT, np.uint8), pos=guarded(np.zeros((0, 3), np.float32), n_max, 3),
             desc=np.full((n_max + G, 32), SENT, np.uint8))
    for k, v in (("state", state), ("pos", pos), ("desc", desc)):
        if v is not None:
            s[k][:len(v)] = v
    return s


def filled(fp, Tcw, o, slots, mode):
    """lorb_frame_slots_fill_dev in numpy over the oracle's frame o: (slots after, n_created)."""
    n = int(o["counts"][0])
    unp = O.unproject_stereo(fp, Tcw, o["left"]["x"], o["left"]["y"], o["depth"])
    out = {k: v.copy() for k, v in slots.items()}
    if mode == UPDATE:
        m = slots["state"][:n] == EMPTY
        out["state"][:n][m] = FREE
    else:
        m = o["depth"] >= 0
        out["state"][:n] = np.where(m, LOCKED, EMPTY)
    out["pos"][:n][m] = unp[m]
    out["desc"][:n][m] = o["left"]["desc"][m]
    return out, int(m.sum())


def compose(fp, pi, T, kps, ss, slot_pos, last, min_matches=20):
    """The reference's three calls composed from the oracle (tests/test_gpu_track_motion.py::expected
    with the pose given)."""
    n = len(kps["x"])
    a1, n1 = O.search_by_projection_frame(fp, T, kps, ss, last, 15.0)
    if n1 <= min_matches:
        a, n2 = O.search_by_projection_frame(fp, T, kps, np.zeros(n, np.uint8), last, 30.0)
        pass_ = 2 if n2 > min_matches else 0
        has = a >= 0
    else:
        a, n2, pass_ = a1, -1, 1
        has = (a >= 0) | ((a == UNCHANGED) & (ss != EMPTY))
    idx = np.nonzero(has)[0]
    pts = np.zeros((len(idx), 3), np.float32)
    m = a[idx] >= 0
    pts[m] = last["mp_pos"][a[idx][m]]
    if (~m).any():
        pts[~m] = slot_pos[idx[~m]]
    obs = np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(np.float32).reshape(-1, 2)
    e = dict(assign=a, pass_=pass_, nmatches_first=n1, nmatches_retry=n2, n_residuals=len(idx))
    if pass_:
        pb = dict(res_off=np.array([0, len(idx)], np.int32),
                  intr=np.array([[fp["fx"], fp["fx"], fp["cx"], fp["cy"]]], np.float32),  # the PoseCost quirk
                  pose_init=pi[None], pts3d=pts, obs2d=obs)
        po, To, so = O.ba_pose_only(pb)
        e.update(pose=po[0], Tcw=To[0], summary=so[0])
    else:
        e.update(pose=pi.astype(np.float64), Tcw=O.pose_to_Tcw(pi[:3], pi[3:]), summary=A.BASummary().as_dict())
    return e


def expected(oa, ob, fp, dx, last_entry, cur_entry, given=False, outlier=None):
    """What lorb_track_motion_frames_dev must leave: the record's fields, assign, and both slot sets as
    whole guarded arrays.  last_entry / cur_entry: entry_slots() images."""
    n_last, n_cur = int(oa["counts"][0]), int(ob["counts"][0])
    pi, T = prediction(dx)
    last_after, n_created = filled(fp, I4, oa, last_entry, UPDATE)
    st = last_after["state"][:n_last]
    last = dict(Tcw=I4, has_mp=(st != EMPTY).astype(np.uint8), outlier=outlier, mp_locked=(st == LOCKED).astype(np.uint8),
                mp_pos=last_after["pos"][:n_last].copy(), mp_desc=last_after["desc"][:n_last].copy(),
                octave=oa["left"]["octave"], angle=oa["left"]["angle"])
    kps = dict({k: ob["left"][k] for k in ("x", "y", "octave", "angle", "desc")}, u_right=ob["u_right"])
    ss = cur_entry["state"][:n_cur].copy() if given else np.zeros(n_cur, np.uint8)
    if n_cur == 0 or n_last == 0:  # nothing to match: both passes find 0 (the oracle is not asked about empty frames)
        e = dict(assign=np.full(n_cur, UNCHANGED, np.int32), pass_=0, nmatches_first=0, nmatches_retry=0, n_residuals=0,
                 pose=pi.astype(np.float64), Tcw=O.pose_to_Tcw(pi[:3], pi[3:]), summary=A.BASummary().as_dict())
    else:
        e = compose(fp, pi, T, kps, ss, cur_entry["pos"][:n_cur], last)
    a = e["assign"]
    cur_after = {k: v.copy() for k, v in cur_entry.items()}
    hit = a >= 0
    keep = (a == UNCHANGED) & (e["pass_"] == 1) & given
    cs = cur_after["state"][:n_cur]
    cs[~hit & ~keep] = EMPTY
    cs[hit] = st[a[hit]]
    cur_after["pos"][:n_cur][hit] = last["mp_pos"][a[hit]]
    cur_after["desc"][:n_cur][hit] = last["mp_desc"][a[hit]]
    e.update(n_last=n_last, n_cur=n_cur, n_created=n_created, status=0, last_slots=last_after, cur_slots=cur_after,
             last=last, kps=kps)
    return e


@functools.lru_cache(maxsize=None)
def plain(name, dx):
    """Case a's expectation: all last slots EMPTY on entry, current slots not given.  Independent of the
    bounds but for the guard arrays' lengths, which check() cuts to."""
    ca, cb = frames(name)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    return expected(ca["o"], cb["o"], ca["fp"], dx, entry_slots(n_last, state=np.zeros(n_last, np.uint8)), entry_slots(n_cur))


def shape_guard(name):
    ca, cb = frames(name)
    (na, nb), nd = SHAPES[name]
    assert (int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])) == (na, nb)
    assert int((ca["o"]["depth"] >= 0).sum()) == nd == int((ca["o"]["depth"] > 0).sum())


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def check_slots(got, want, n_max, what):
    """Whole guarded arrays, byte for byte; `want` may have been made for a larger bound."""
    for k in ("state", "pos", "desc"):
        g, w = got[k], want[k]
        assert len(g) == n_max + G, (what, k)
        n = len(w) - G  # the entries `want` was made for: everything past them is sentinel in both
        assert same_bytes(g[:min(n, n_max)], w[:min(n, n_max)]), (what, k)
        assert (np.ascontiguousarray(g[min(n, n_max):]).view(np.uint8) == SENT).all(), (what, k, "guard")


def check(r, e, n_max_cur, n_max_last):
    assert r["status"] == 0
    n_cur = e["n_cur"]
    assert (r["n_last"], r["n_cur"], r["n_created"]) == (e["n_last"], n_cur, e["n_created"])
    assert len(r["assign"]) == n_max_cur + G and np.array_equal(r["assign"][:n_cur], e["assign"])
    assert (r["assign"][n_cur:] == FILL).all()
    assert (r["pass_"], r["nmatches_first"], r["nmatches_retry"], r["n_residuals"]) == \
        (e["pass_"], e["nmatches_first"], e["nmatches_retry"], e["n_residuals"])
    check_slots(r["last_slots"], e["last_slots"], n_max_last, "last")
    check_slots(r["cur_slots"], e["cur_slots"], n_max_cur, "cur")
    if e["pass_"] == 0:
        assert np.array_equal(r["pose"], e["pose"])  # pose_init widened, bit for bit
        assert r["summary"] == A.BASummary().as_dict()
    assert close(r["pose"], e["pose"]), np.abs(r["pose"] - e["pose"]).max()
    summaries_agree(r["summary"], e["summary"])
    assert np.allclose(r["Tcw"], e["Tcw"], rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def builders(ctx):
    made = {}

    def get(rows, cols, L, nf):
        key = (rows, cols, L, nf)
        if key not in made:
            fp, _, nd = TF.geometry(rows, cols, L, nf)
            made[key] = FrameBuilder(ctx, fp, rows, cols, nd, TF.pattern())
        return made[key]

    yield get
    for b in made.values():
        b.close()


class Built:
    """Frames A and B of a shape on the device plus slot sets; everything is freed on exit."""

    def __init__(self, ctx, builders, ca, cb):
        self.ctx, self.b = ctx, builders(*ca["geom"])
        self.ca, self.cb, self.held = ca, cb, []

    def __enter__(self):
        self.fa = self.b.build_device(self.ca["left"], self.ca["right"])
        self.held.append(self.fa)
        self.fb = self.b.build_device(self.cb["left"], self.cb["right"])
        self.held.append(self.fb)
        return self

    def slots(self, n_max, entry):
        s = DeviceSlots(self.ctx, n_max, entry["state"][:n_max], entry["pos"][:n_max], entry["desc"][:n_max])
        self.held.append(s)
        return s

    def __exit__(self, *exc):
        for h in self.held:
            h.free()


def run(ctx, bt, fp, dx, last_slots, cur_slots, **kw):
    pi, T = prediction(dx)
    return track_motion_frames(ctx, fp, T, pi, bt.fb, cur_slots, I4, bt.fa, last_slots, assign_fill=FILL, **kw)


# a -- each shape at its dx values, bounds = the builder's capacity (where 8M allows) and tight -------------
@pytest.mark.parametrize("bounds", ["capacity", "tight"])
@pytest.mark.parametrize("name,dx", list(CASES))
def test_shapes(ctx, builders, name, dx, bounds):
    shape_guard(name)
    ca, cb = frames(name)
    e = plain(name, dx)
    fig = (e["nmatches_first"], e["nmatches_retry"], e["pass_"])
    if CASES[(name, dx)] is None:
        assert e["pass_"] == 0 and e["nmatches_first"] <= 20 and e["nmatches_retry"] <= 20
    else:
        assert fig == CASES[(name, dx)]
    if (name, dx) in RETRY_FIGURES:
        assert O.search_by_projection_frame(ca["fp"], prediction(dx)[1], e["kps"], None, e["last"], 30.0)[1] == \
            RETRY_FIGURES[(name, dx)]
    if name != "160x120":  # rotation null-outs: NULL codes, which empty their slots
        assert (e["assign"] == NULL).sum() >= 5
    if name == "160x120":  # 72 created points at the origin: z = 0 under the identity, 1 / z infinite, u NaN
        assert e["n_created"] == 111 and int((~e["last"]["mp_pos"].any(1)).sum()) == 72
    n_last, n_cur = e["n_last"], e["n_cur"]
    with Built(ctx, builders, ca, cb) as bt:
        cap = bt.b.capacity
        if bounds == "capacity":
            assert cap * cap <= 8 << 20 and cap > max(n_last, n_cur) + 1
            nl = nc = cap
        else:
            nl = nc = max(n_last, n_cur) + 1
        ls = bt.slots(nl, entry_slots(nl, state=np.zeros(n_last, np.uint8)))
        cs = bt.slots(nc, entry_slots(nc))
        check(run(ctx, bt, ca["fp"], dx, ls, cs), e, nc, nl)


def test_bound_layouts():
    """The two bounds of test_shapes take different paths: the tight bounds the one-pass strided
    candidate layout with the grid in LDS, the capacity of the two larger shapes the count / scan / write
    passes with the grid kernel (past 1M entries and past 1024 keypoints)."""
    for name, ((na, nb), _) in SHAPES.items():
        ca, _ = frames(name)
        cap = W.orb_extract_capacity(*ca["left"].shape, ca["nd"], ca["sf"])[0]
        tight = max(na, nb) + 1
        assert tight * tight <= 1 << 20 and tight <= 1024
        if name != "160x120":
            assert 1 << 20 < cap * cap <= 8 << 20 and cap > 1024
        else:
            assert cap * cap <= 1 << 20 and cap <= 1024


# the fill alone, both modes ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["160x120", "376x240"])
def test_fill_alone(ctx, builders, name):
    """INITIALIZE on sentinel-filled slots, then UPDATE_FRAME on what it left: LOCKED slots stay, EMPTY
    ones become FREE points at the origin.  Positions are O.unproject_stereo's bits under a pose that is
    not the identity."""
    shape_guard(name)
    ca, cb = frames(name)
    o, fp = ca["o"], ca["fp"]
    T = np.array(O.pose_to_Tcw(np.array([0.02, -0.01, 0.005], np.float32), np.array([0.3, -0.1, 0.2], np.float32)))
    n = int(o["counts"][0])
    nd = SHAPES[name][1]
    with Built(ctx, builders, ca, cb) as bt:
        for n_max in (n, bt.b.capacity):
            e0 = entry_slots(n_max)
            s = bt.slots(n_max, e0)
            e1, made1 = filled(fp, T, o, e0, INIT)
            assert made1 == nd and set(np.unique(e1["state"][:n])) == {EMPTY, LOCKED}
            assert fill_slots(ctx, fp, T, bt.fa, s, INIT) == made1
            check_slots(s.numpy(), e1, n_max, "initialize")
            e2, made2 = filled(fp, T, o, e1, UPDATE)
            assert made2 == n - nd and not e2["pos"][:n][e1["state"][:n] == EMPTY].any()
            assert fill_slots(ctx, fp, T, bt.fa, s, UPDATE) == made2
            check_slots(s.numpy(), e2, n_max, "update_frame")
            assert fill_slots(ctx, fp, T, bt.fa, s, UPDATE) == 0  # nothing left to create
            check_slots(s.numpy(), e2, n_max, "update_frame again")
        short = bt.slots(n - 1, entry_slots(n - 1))  # a bound below the count: nothing is written
        assert fill_slots(ctx, fp, T, bt.fa, short, INIT) == -1
        check_slots(short.numpy(), entry_slots(n - 1), n - 1, "bound below the count")
        with pytest.raises(LorbError):
            fill_slots(ctx, fp, T, bt.fa, s, 2)


# b -- last slots pre-filled by INITIALIZE: LOCKED points in a4, LOCKED states in the current slots ------
@pytest.mark.parametrize("name,dx", [("320x256", 0.1), ("160x120", 0.2)])
def test_initialized_last_frame(ctx, builders, name, dx):
    ca, cb = frames(name)
    fp, oa = ca["fp"], ca["o"]
    n_last, n_cur = int(oa["counts"][0]), int(cb["o"]["counts"][0])
    nl, nc = n_last + 1, n_cur + 3
    init, _ = filled(fp, I4, oa, entry_slots(nl), INIT)
    e = expected(oa, cb["o"], fp, dx, init, entry_slots(nc))
    assert e["n_created"] == n_last - SHAPES[name][1]
    a, st = e["assign"], e["last_slots"]["state"][:n_last]
    assert (st[a[a >= 0]] == LOCKED).sum() >= 10  # LOCKED points matched ...
    assert (e["cur_slots"]["state"][:n_cur] == LOCKED).sum() >= 10  # ... and their state carried over
    # the occupancy rule is at work: with every point unlocked the codes differ
    assert not np.array_equal(a, plain(name, dx)["assign"])
    with Built(ctx, builders, ca, cb) as bt:
        ls, cs = bt.slots(nl, entry_slots(nl)), bt.slots(nc, entry_slots(nc))
        assert fill_slots(ctx, fp, I4, bt.fa, ls, INIT) == SHAPES[name][1]
        check(run(ctx, bt, fp, dx, ls, cs), e, nc, nl)


# c -- current slots given: UNCHANGED keeps them and they enter the residuals -----------------------------
def given_slots(name, dx):
    ca, cb = frames(name)
    n_cur = int(cb["o"]["counts"][0])
    a = plain(name, dx)["assign"]
    rng = np.random.default_rng(5)
    state = np.zeros(n_cur, np.uint8)
    hit, miss = np.nonzero(a >= 0)[0], np.nonzero(a == UNCHANGED)[0]
    state[hit[::5]] = LOCKED   # a4 must pass these by
    state[hit[1::5]] = FREE    # and may overwrite these
    state[miss[::4]] = FREE    # these stay and are residuals
    state[miss[1::4]] = LOCKED
    k = cb["o"]["left"]
    z = rng.uniform(2, 12, n_cur)
    pos = np.stack([(k["x"] - ca["fp"]["cx"]) / ca["fp"]["fx"] * z, (k["y"] - ca["fp"]["cy"]) / ca["fp"]["fy"] * z, z], 1)
    desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    return state, pos.astype(np.float32), desc


def test_current_slots_given(ctx, builders):
    name, dx = "320x256", 0.1
    ca, cb = frames(name)
    fp = ca["fp"]
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    state, pos, desc = given_slots(name, dx)
    nl, nc = n_last + 1, n_cur + 1
    last0 = entry_slots(nl, state=np.zeros(n_last, np.uint8))
    cur0 = entry_slots(nc, state, pos, desc)
    e = expected(ca["o"], cb["o"], fp, dx, last0, cur0, given=True)
    a = e["assign"]
    kept = (a == UNCHANGED) & (state != EMPTY)
    assert e["pass_"] == 1 and kept.sum() >= 20 and e["n_residuals"] == (a >= 0).sum() + kept.sum()
    assert ((a >= 0) & (state == FREE)).sum() >= 1 and not ((a >= 0) & (state == LOCKED)).any()
    assert same_bytes(e["cur_slots"]["pos"][:n_cur][kept], pos[kept])
    nulled = (a == NULL) & (state != EMPTY)  # a rotation null-out empties a given slot
    assert nulled.sum() >= 1 and (e["cur_slots"]["state"][:n_cur][nulled] == EMPTY).all()
    # not given, the same arrays are ignored: the plain expectation's codes, every other slot EMPTY
    e0 = expected(ca["o"], cb["o"], fp, dx, last0, cur0, given=False)
    assert np.array_equal(e0["assign"], plain(name, dx)["assign"]) and not np.array_equal(e0["assign"], a)
    with Built(ctx, builders, ca, cb) as bt:
        check(run(ctx, bt, fp, dx, bt.slots(nl, last0), bt.slots(nc, cur0), cur_slots_given=True), e, nc, nl)
        check(run(ctx, bt, fp, dx, bt.slots(nl, last0), bt.slots(nc, cur0)), e0, nc, nl)
    # the retry empties given slots too (src/visual_odometry.cpp:128)
    name, dx = "160x120", 0.2
    ca, cb = frames(name)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    state, pos, desc = given_slots(name, dx)
    last0, cur0 = entry_slots(n_last + 1, state=np.zeros(n_last, np.uint8)), entry_slots(n_cur + 1, state, pos, desc)
    e = expected(ca["o"], cb["o"], ca["fp"], dx, last0, cur0, given=True)
    assert e["pass_"] == 2 and e["n_residuals"] == (e["assign"] >= 0).sum()
    assert (e["cur_slots"]["state"][:n_cur][e["assign"] < 0] == EMPTY).all() and (state[e["assign"] < 0] != EMPTY).any()
    with Built(ctx, builders, ca, cb) as bt:
        check(run(ctx, bt, ca["fp"], dx, bt.slots(n_last + 1, last0), bt.slots(n_cur + 1, cur0), cur_slots_given=True), e,
              n_cur + 1, n_last + 1)


def test_last_outliers(ctx, builders):
    """d_last_outlier removes last-frame points from the search (Frame::mvbOutlier)."""
    name, dx = "376x240", 0.2
    ca, cb = frames(name)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    a = plain(name, dx)["assign"]
    out = np.zeros(n_last, np.uint8)
    out[a[a >= 0][::3]] = 1
    last0, cur0 = entry_slots(n_last, state=np.zeros(n_last, np.uint8)), entry_slots(n_cur)
    e = expected(ca["o"], cb["o"], ca["fp"], dx, last0, cur0, outlier=out)
    assert not np.array_equal(e["assign"], a) and not np.isin(e["assign"], np.nonzero(out)[0]).any()
    with Built(ctx, builders, ca, cb) as bt:
        check(run(ctx, bt, ca["fp"], dx, bt.slots(n_last, last0), bt.slots(n_cur, cur0), last_outlier=out), e, n_cur, n_last)


# e -- a bound below a count: status 1, nothing else written ---------------------------------------------
@pytest.mark.parametrize("short", ["cur", "last"])
def test_bound_below_count(ctx, builders, short):
    name, dx = "376x240", 0.2
    ca, cb = frames(name)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    nl, nc = (n_last, n_cur - 1) if short == "cur" else (n_last - 1, n_cur)
    last0 = entry_slots(nl, state=np.zeros(nl, np.uint8))
    cur0 = entry_slots(nc)
    with Built(ctx, builders, ca, cb) as bt:
        r = run(ctx, bt, ca["fp"], dx, bt.slots(nl, last0), bt.slots(nc, cur0))
        assert r["status"] == 1
        rec = A.TrackFramesResult.from_buffer_copy(r["record_bytes"].tobytes())
        rec.status = int.from_bytes(bytes([SENT] * 4), "little", signed=True)
        assert (np.frombuffer(bytes(rec), np.uint8) == SENT).all()  # the rest of the record is as it was
        assert (r["assign"] == FILL).all()
        check_slots(r["last_slots"], last0, nl, "last")
        check_slots(r["cur_slots"], cur0, nc, "cur")
        # the context is fine afterwards
        ls, cs = bt.slots(n_last, entry_slots(n_last, state=np.zeros(n_last, np.uint8))), bt.slots(n_cur, entry_slots(n_cur))
        check(run(ctx, bt, ca["fp"], dx, ls, cs), plain(name, dx), n_cur, n_last)


# f -- a blank current image, a blank last image ----------------------------------------------------------
@pytest.mark.parametrize("blank", ["cur", "last"])
def test_blank_frames(ctx, builders, blank):
    geom = (256, 320, 8, 500)
    full, none = TF.case("320x256"), TF.blank_case(*geom, "left")
    assert int(none["o"]["counts"][0]) == 0 and int(full["o"]["counts"][0]) == 495
    ca, cb = (full, none) if blank == "cur" else (none, full)
    ca = dict(ca, geom=geom)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    nl, nc = n_last + 2, n_cur + 2
    last0, cur0 = entry_slots(nl, state=np.zeros(n_last, np.uint8)), entry_slots(nc)
    e = expected(ca["o"], cb["o"], full["fp"], 0.1, last0, cur0)
    assert e["n_created"] == n_last and e["pass_"] == 0 and len(e["assign"]) == n_cur
    with Built(ctx, builders, ca, cb) as bt:
        check(run(ctx, bt, full["fp"], 0.1, bt.slots(nl, last0), bt.slots(nc, cur0)), e, nc, nl)


# g -- the chain into lorb_track_local_dev ----------------------------------------------------------------
def local_points(init, n_last, a):
    """A's initialised points as the local map: plausible normals and distance bounds, the points the
    motion stage put into the current frame flagged in_frame."""
    idx = np.nonzero(init["state"][:n_last] == LOCKED)[0]
    pos = init["pos"][:n_last][idx]
    d = np.linalg.norm(pos.astype(np.float64), axis=1)
    ok = d > 0
    idx, pos, d = idx[ok], pos[ok], d[ok]
    in_frame = np.isin(idx, a[a >= 0]).astype(np.uint8)
    return dict(pos=pos.copy(), normal=(pos / d[:, None]).astype(np.float32), max_dist=(1.6 * d).astype(np.float32),
                min_dist=(0.6 * d).astype(np.float32), desc=init["desc"][:n_last][idx].copy(),
                locked=np.ones(len(idx), np.uint8), is_bad=None, in_frame=in_frame)


def stage2(fp, kps, ss, sp, pts, pi2, T2, th):
    """EstimatePoseLocal after UpdateLocalMap composed from the oracle."""
    fr, a2, nm = O.track_local_map(fp, T2, kps, ss, pts, 0.5, th)
    idx = np.nonzero((a2 >= 0) | ((a2 == UNCHANGED) & (ss != EMPTY)))[0]
    X = np.where((a2[idx] >= 0)[:, None], pts["pos"][np.maximum(a2[idx], 0)], sp[idx]).astype(np.float32)
    obs = np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(np.float32)
    e = dict(assign=a2, in_view=fr["in_view"], counts=(int(nm > 20), nm, int(fr["in_view"].sum()), len(idx)))
    if nm > 20:
        po, _, so = O.ba_pose_only(dict(res_off=np.array([0, len(idx)], np.int32), pose_init=pi2[None], pts3d=X, obs2d=obs,
                                        intr=np.array([[fp["fx"], fp["fx"], fp["cx"], fp["cy"]]], np.float32)))
        e.update(pose=po[0], summary=so[0])
    return e


def test_chain_into_track_local(ctx, builders):
    """Build A and B, INITIALIZE-fill A, the new call, the record fetched once, then
    lorb_track_local_dev with kps.n = n_cur and the returned current slots as d_slot_state / d_slot_pos
    over A's initialised points: equal to O.track_local_map + O.ba_pose_only on the oracle's frames.
    At th = 1 the search finds 19 (the gate fails), at th = 2 it finds 22 and the pose is optimised."""
    name, dx = "320x256", 0.1
    ca, cb = frames(name)
    fp, oa, ob = ca["fp"], ca["o"], cb["o"]
    n_last, n_cur = int(oa["counts"][0]), int(ob["counts"][0])
    nl, nc = n_last + 1, n_cur + 1
    init, _ = filled(fp, I4, oa, entry_slots(nl), INIT)
    e = expected(oa, ob, fp, dx, init, entry_slots(nc))
    assert e["pass_"] == 1
    pts = local_points(init, n_last, e["assign"])
    # stage 2 starts from the pose stage 1 found, rounded as Frame::SetPose rounds it.  (The oracle's
    # pose: the device's may differ in the last bits, and the pose is a host value of the call either way.)
    pi2 = e["pose"].astype(np.float32)
    T2 = np.array(O.pose_to_Tcw(pi2[:3], pi2[3:]))
    ss, sp = e["cur_slots"]["state"][:n_cur].copy(), e["cur_slots"]["pos"][:n_cur].copy()
    want = {th: stage2(fp, e["kps"], ss, sp, pts, pi2, T2, th) for th in (1.0, 2.0)}
    assert pts["in_frame"].sum() >= 20 and (ss == LOCKED).sum() >= 20
    assert want[1.0]["counts"][:2] == (0, 19) and want[2.0]["counts"][:2] == (1, 22)
    with Built(ctx, builders, ca, cb) as bt:
        ls, cs = bt.slots(nl, entry_slots(nl)), bt.slots(nc, entry_slots(nc))
        fill_slots(ctx, fp, I4, bt.fa, ls, INIT)
        r = run(ctx, bt, fp, dx, ls, cs)
        check(r, e, nc, nl)
        held = [ctx.to_device(pts[k]) for k in ("pos", "normal", "max_dist", "min_dist", "desc", "locked", "in_frame")]
        npt = len(pts["pos"])
        m = A.MapPointsDev(npt, held[0].ptr, held[1].ptr, held[2].ptr, held[3].ptr, held[4].ptr, held[5].ptr, None, held[6].ptr)
        iv, tr, lv = ctx.empty(npt, np.uint8), ctx.empty((4, npt), np.float32), ctx.empty(npt, np.int32)
        asg, drec = ctx.empty(n_cur, np.int32), ctx.empty(C.sizeof(A.TrackLocalResult), np.uint8)
        held += [iv, tr, lv, asg, drec]
        try:
            fps, opt = A.make_frame_params(fp), A.LMOptions.default()
            k, T16 = bt.fb.keypoints(r["n_cur"]), A.f32(T2).reshape(16)
            for th, w in want.items():
                par = A.TrackLocalParams(0.5, th, 20, fp["fx"])
                ctx.check(lib().lorb_track_local_dev(ctx.handle, C.byref(fps), A.ptr(T16, C.c_float), A.ptr(pi2, C.c_float),
                                                     C.byref(k), cs.state.ptr, cs.pos.ptr, C.byref(m), C.byref(par),
                                                     C.byref(opt), iv.ptr, tr.ptr, lv.ptr, asg.ptr, drec.ptr),
                          "lorb_track_local_dev")
                rec = A.TrackLocalResult.from_buffer_copy(drec.numpy().tobytes())
                assert np.array_equal(asg.numpy(), w["assign"]) and np.array_equal(iv.numpy(), w["in_view"]), th
                assert (rec.ok, rec.nmatches, rec.n_in_view, rec.n_residuals) == w["counts"], th
                if rec.ok:
                    assert close(np.array(rec.pose[:]), w["pose"])
                    summaries_agree(rec.summary.as_dict(), w["summary"])
                else:
                    assert np.array_equal(np.array(rec.pose[:]), pi2.astype(np.float64))
        finally:
            for h in held:
                h.free()


# h -- scratch reuse: the existing chains on the same context afterwards ----------------------------------
def test_context_reuse(ctx, builders):
    import test_gpu_track_motion as TM
    name, dx = "376x240", 0.2
    ca, cb = frames(name)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    s = TM.frames(500, 200, 1)
    with Built(ctx, builders, ca, cb) as bt:
        cap = bt.b.capacity
        for nl, nc in ((cap, cap), (n_last + 1, n_cur + 1)):
            ls = bt.slots(nl, entry_slots(nl, state=np.zeros(n_last, np.uint8)))
            check(run(ctx, bt, ca["fp"], dx, ls, bt.slots(nc, entry_slots(nc))), plain(name, dx), nc, nl)
            for d in (0.0, 0.7):
                TM.check(TM.run(ctx, s, d, None, None), TM.expected(s, d, None, None))
            a_g, n_g = ctx.search_by_projection_frame_dev(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], 15.0)
            a_o, n_o = O.search_by_projection_frame(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], 15.0)
            assert n_g == n_o and np.array_equal(a_g, a_o)


def test_errors(ctx, builders):
    """With a live context: bounds whose product passes 8M, non-positive bounds and null arrays are
    LORB_E_INVALID before anything is enqueued; the next call is fine."""
    name, dx = "160x120", 0.0
    ca, cb = frames(name)
    n_last, n_cur = int(ca["o"]["counts"][0]), int(cb["o"]["counts"][0])
    with Built(ctx, builders, ca, cb) as bt:
        ls = bt.slots(n_last, entry_slots(n_last, state=np.zeros(n_last, np.uint8)))
        cs = bt.slots(n_cur, entry_slots(n_cur))
        for nl, nc in ((4097, 2048), (2048, 4097), (2897, 2897), (0, n_cur), (n_last, 0), (-1, n_cur)):
            with pytest.raises(LorbError):
                run(ctx, bt, ca["fp"], dx, ls, cs, n_max_last=nl, n_max_cur=nc)
        saved = cs.c.pos
        cs.c.pos = None
        with pytest.raises(LorbError):
            run(ctx, bt, ca["fp"], dx, ls, cs)
        cs.c.pos = saved
        check(run(ctx, bt, ca["fp"], dx, ls, cs), plain(name, dx), n_cur, n_last)
