"""Hand-built problems for the windowed matchers of lorb_window.hip: a4 = SearchByProjection(Frame,
Frame), a5 = SearchByProjection(Frame, set<MapPoint>).  Pure numpy; shared by
test_oracle_window_cases.py (CPU: oracle == pyref, claims, hand-derived answers) and
test_gpu_window_edges.py (GPU == oracle).

A case is a dict:
  kind    "a4" | "a5"
  args    the call's inputs: a4 (fp, cur_Tcw, cur_kps, slot_state, last, th), a5 (fp, kps, slot_state, pts, th)
  claims  {text: bool}: what makes the case what it says it is, computed here with numpy alone
  dist    [(query, keypoint, distance)]: descriptor distances the case was built to have
  expect  None or (assign, nmatches): the answer derived by hand

Descriptors are a base XOR a chosen bit set, so every distance that matters is known.  The frame of
every semantic case has negative fractional min_x / min_y and fractional max_x / max_y, as undistorted
image bounds are.  All poses are pure translations along z (R = I), so a last-frame point's projection
is X / Z scaled; `proj` restates the float arithmetic to place keypoints exactly on a window's edge.

SEMANTIC cases are small (pure Python can follow); PATH cases straddle these constants of
lorb_window.hip (if one changes, re-derive the shapes -- test_oracle_window_cases.py checks the sizes
against the values restated below):
  kRegCand = 8        candidates of a query held in registers by the resolver (np <= 1024)
  kStageKps = 1024    keypoints up to which the candidate kernel builds the grid in its own LDS
  kRegQueries = 1024  queries up to which the resolver preloads (`regc`)
  kCandStrided = 2^20 nq * nk up to which one strided candidate pass is used
  kGridLds = 6144     keypoints up to which the grid build keeps the cell lists in LDS
  kCandBound = 8*2^20 nq * nk past which the candidate total is read back
  kResolveLds = 30720 words: 4 nk + 2 nq <= it -> LDS mode 2, else nq + nk <= it -> mode 1, else 0
"""
import functools

import numpy as np

from lorb_slam_amd import synth

f32 = np.float32
UNCHANGED, NULL = -1, -2
EMPTY, FREE, LOCKED = 0, 1, 2
K_REG_CAND, K_STAGE_KPS, K_REG_QUERIES = 8, 1024, 1024
K_CAND_STRIDED, K_GRID_LDS, K_CAND_BOUND, K_RESOLVE_LDS = 1 << 20, 6144, 8 << 20, 30720


def resolve_lds_mode(nq, nk):
    return 2 if 4 * nk + 2 * nq <= K_RESOLVE_LDS else 1 if nq + nk <= K_RESOLVE_LDS else 0


# ------------------------------------------------------------------------------------------ helpers
def frame(min_x=-17.3, min_y=-11.6, max_x=770.4, max_y=492.7):
    fp = dict(synth.frame_params())
    fp.update(min_x=f32(min_x), min_y=f32(min_y), max_x=f32(max_x), max_y=f32(max_y))
    fp["grid_w_inv"] = f32(f32(64) / (fp["max_x"] - fp["min_x"]))
    fp["grid_h_inv"] = f32(f32(48) / (fp["max_y"] - fp["min_y"]))
    return fp


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def _rha(v):  # round half away from zero
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def cell_of(fp, x, y):
    """(column, row) of a keypoint, or None if it falls outside the 64 x 48 grid"""
    c = _rha(f32(f32(x) - fp["min_x"]) * fp["grid_w_inv"])
    r = _rha(f32(f32(y) - fp["min_y"]) * fp["grid_h_inv"])
    return (c, r) if 0 <= c < 64 and 0 <= r < 48 else None


def hist_bin(last_angle, cur_angle):
    rot = f32(f32(last_angle) - f32(cur_angle))
    if rot < 0:
        rot = f32(rot + f32(360))
    b = _rha(f32(rot * f32(f32(30) / f32(360))))
    return 0 if b == 30 else b


def base(k):
    return np.random.default_rng(7000 + k).integers(0, 256, 32, dtype=np.uint8)


def flip(d, bits):
    out = np.array(d, np.uint8).copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def near(d, n, lo=0):
    """d with bits lo .. lo + n - 1 flipped: at distance n from d"""
    return flip(d, range(lo, lo + n))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def pose(tz):
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = f32(tz)
    return T


def proj(fp, T, X):
    """a4's projection of world point X under the pure translation T, in the reference's float
    arithmetic (products accumulated in double, one cast): (u, v, invzc)"""
    X = np.asarray(X, np.float32)
    c = [f32(float(X[i]) + float(T[i, 3])) for i in range(3)]
    invz = f32(1.0 / float(c[2]))
    u = f32(f32(f32(fp["fx"] * c[0]) * invz) + fp["cx"])
    v = f32(f32(f32(fp["fy"] * c[1]) * invz) + fp["cy"])
    return u, v, invz


def world_at(fp, T, u, v, z):
    """a world point that projects close to (u, v) at depth z under T"""
    return np.array([(u - float(fp["cx"])) / float(fp["fx"]) * z - float(T[0, 3]),
                     (v - float(fp["cy"])) / float(fp["fy"]) * z - float(T[1, 3]), z - float(T[2, 3])], np.float32)


def motion(fp, T_cur, T_last):
    """(forward, backward) of src/matcher.cpp:77-87 for pure translations"""
    twc = f32(-float(T_cur[2, 3]))
    tlc = f32(float(twc) + float(T_last[2, 3]))
    return bool(tlc > fp["b"]), bool(f32(-tlc) > fp["b"])


def site(k, pitch=40, per_row=17):
    return 40.0 + pitch * (k % per_row), 40.0 + pitch * (k // per_row)


class Kps:
    def __init__(self):
        self.x, self.y, self.o, self.a, self.ur, self.d, self.s = [], [], [], [], [], [], []

    def add(self, x, y, desc, octave=0, angle=0.0, uR=-1.0, state=EMPTY):
        for lst, v in zip((self.x, self.y, self.o, self.a, self.ur, self.d, self.s), (x, y, octave, angle, uR, desc, state)):
            lst.append(v)
        return len(self.x) - 1

    def build(self):
        kps = dict(x=np.array(self.x, np.float32), y=np.array(self.y, np.float32), octave=np.array(self.o, np.int32),
                   angle=np.array(self.a, np.float32), u_right=np.array(self.ur, np.float32),
                   desc=np.array(self.d, np.uint8).reshape(-1, 32))
        return kps, np.array(self.s, np.uint8)


class A4:
    """one a4 call under construction: last-frame points in call order, current keypoints"""

    def __init__(self, fp=None, tz=0.0, th=15.0):
        self.fp, self.T, self.TL, self.th = fp or frame(), pose(tz), pose(0.0), th
        self.k = Kps()
        self.X, self.o, self.a, self.d, self.lk, self.hm, self.ol = [], [], [], [], [], [], []
        self.dist, self.claims = [], {}

    def pt(self, u, v, desc, octave=0, angle=0.0, locked=1, z=4.0, X=None, has_mp=1, outlier=0):
        X = world_at(self.fp, self.T, u, v, z) if X is None else np.asarray(X, np.float32)
        for lst, val in zip((self.X, self.o, self.a, self.d, self.lk, self.hm, self.ol),
                            (X, octave, angle, desc, locked, has_mp, outlier)):
            lst.append(val)
        return (len(self.X) - 1,) + proj(self.fp, self.T, X)

    def kp(self, *a, **kw):
        return self.k.add(*a, **kw)

    def pair(self, s, b, dist=10, rot=0.0, octave=0, locked=1, cur_angle=0.0):
        """an isolated match at lattice site s: one point, one keypoint `dist` bits away, their angles
        `rot` apart; -> (point, slot)"""
        x, y = site(s)
        q, u, v, _ = self.pt(x, y, base(b), octave=octave, angle=rot, locked=locked)
        j = self.kp(x, y, near(base(b), dist), octave=octave, angle=cur_angle)
        self.dist.append((q, j, dist))
        return q, j

    def case(self, expect=None, slot_state=True):
        kps, st = self.k.build()
        last = dict(Tcw=self.TL, has_mp=np.array(self.hm, np.uint8), outlier=np.array(self.ol, np.uint8),
                    mp_locked=np.array(self.lk, np.uint8), mp_pos=np.array(self.X, np.float32).reshape(-1, 3),
                    mp_desc=np.array(self.d, np.uint8).reshape(-1, 32), octave=np.array(self.o, np.int32),
                    angle=np.array(self.a, np.float32))
        return dict(kind="a4", args=(self.fp, self.T, kps, st if slot_state else None, last, self.th),
                    claims=self.claims, dist=self.dist, expect=_expect(expect, len(st)),
                    qdesc=last["mp_desc"], kdesc=kps["desc"])


class A5:
    def __init__(self, fp=None, th=1.0):
        self.fp, self.th = fp or frame(), th
        self.k = Kps()
        self.p = {k: [] for k in ("track_in_view", "is_bad", "locked", "proj_x", "proj_y", "proj_xr", "pred_level",
                                  "view_cos", "desc")}
        self.dist, self.claims = [], {}

    def pt(self, x, y, desc, level=0, vc=0.9, locked=1, xr=0.0, in_view=1, bad=0):
        for k, v in zip(self.p, (in_view, bad, locked, x, y, xr, level, vc, desc)):
            self.p[k].append(v)
        return len(self.p["proj_x"]) - 1

    def kp(self, *a, **kw):
        return self.k.add(*a, **kw)

    def case(self, expect=None, slot_state=True):
        kps, st = self.k.build()
        dt = dict(track_in_view=np.uint8, is_bad=np.uint8, locked=np.uint8, proj_x=np.float32, proj_y=np.float32,
                  proj_xr=np.float32, pred_level=np.int32, view_cos=np.float32, desc=np.uint8)
        pts = {k: np.array(v, dt[k]) for k, v in self.p.items()}
        pts["desc"] = pts["desc"].reshape(-1, 32)
        return dict(kind="a5", args=(self.fp, kps, st if slot_state else None, pts, self.th), claims=self.claims,
                    dist=self.dist, expect=_expect(expect, len(st)), qdesc=pts["desc"], kdesc=kps["desc"])


def _expect(e, nk):
    if e is None:
        return None
    slots, nm = e
    a = np.full(nk, UNCHANGED, np.int32)
    for j, v in slots.items():
        a[j] = v
    return a, nm


# ---------------------------------------------------------------------------------- semantic cases
def tie_first_wins():
    """Equal best distances: the first candidate in GetFeaturesInArea order wins -- insertion order
    inside a cell, column before row across cells -- which is not the lowest keypoint index."""
    c = A4()
    fp = c.fp
    cw, ch = 1.0 / float(fp["grid_w_inv"]), 1.0 / float(fp["grid_h_inv"])
    xb = float(fp["min_x"]) + 20.5 * cw   # between columns 20 and 21
    yb = float(fp["min_y"]) + 30.5 * ch   # between rows 30 and 31
    xc0, yc0 = float(fp["min_x"]) + 40 * cw, float(fp["min_y"]) + 10 * ch  # the middle of cell (40, 10)
    pad = [c.kp(700.0, 20.0 + 5 * i, base(900 + i)) for i in range(3)]  # indices 0..2, matched by nobody
    q0, *_ = c.pt(xb, 100.0, base(0))
    q1, *_ = c.pt(300.0, yb, base(1))
    q2, *_ = c.pt(xc0, yc0, base(2))
    # across columns: the right-hand keypoint gets the lower index, the left-hand column is walked first
    r0 = c.kp(xb + 4, 100.0, near(base(0), 20, 0))
    l0 = c.kp(xb - 4, 100.0, near(base(0), 20, 40))
    # across rows of one column: the lower row is walked first
    b1 = c.kp(300.0, yb + 4, near(base(1), 20, 0))
    t1 = c.kp(300.0, yb - 4, near(base(1), 20, 40))
    # inside one cell: insertion (index) order
    a2 = c.kp(xc0 - 2, yc0, near(base(2), 20, 0))
    b2 = c.kp(xc0 + 2, yc0, near(base(2), 20, 40))
    # diagonal: (column 51, row 30) against (column 50, row 31) -- column-major order takes the latter
    xd = float(fp["min_x"]) + 50.5 * cw
    q3, *_ = c.pt(xd, yb, base(3))
    ur3 = c.kp(xd + 4, yb - 4, near(base(3), 20, 0))
    ll3 = c.kp(xd - 4, yb + 4, near(base(3), 20, 40))
    c.dist += [(q0, r0, 20), (q0, l0, 20), (q1, b1, 20), (q1, t1, 20), (q2, a2, 20), (q2, b2, 20), (q3, ur3, 20),
               (q3, ll3, 20)]
    cl = c.claims
    cl["diagonal cells"] = cell_of(fp, xd + 4, yb - 4) == (51, 30) and cell_of(fp, xd - 4, yb + 4) == (50, 31)
    cl["columns differ, rows equal"] = cell_of(fp, xb - 4, 100.0) == (20, cell_of(fp, xb + 4, 100.0)[1]) and \
        cell_of(fp, xb + 4, 100.0)[0] == 21
    cl["rows differ, columns equal"] = cell_of(fp, 300.0, yb - 4)[1] == 30 and cell_of(fp, 300.0, yb + 4)[1] == 31 and \
        cell_of(fp, 300.0, yb - 4)[0] == cell_of(fp, 300.0, yb + 4)[0]
    cl["one cell"] = cell_of(fp, xc0 - 2, yc0) == cell_of(fp, xc0 + 2, yc0) == (40, 10)
    cl["first in order has the higher index"] = l0 > r0 and t1 > b1 and a2 < b2 and ll3 > ur3 and len(pad) == 3
    return c.case(({l0: q0, t1: q1, a2: q2, ll3: q3}, 4))


def tie_first_wins_a5():
    """a5: a tie of the best across two levels keeps the first (across columns: the left one); a tie
    of the second best keeps the first second's level, which decides whether the ratio test applies."""
    c = A5()
    fp = c.fp
    cw = 1.0 / float(fp["grid_w_inv"])
    xb = float(fp["min_x"]) + 20.5 * cw
    p0 = c.pt(xb, 100.0, base(0), level=1)
    r0 = c.kp(xb + 2, 100.0, near(base(0), 20, 0), octave=1)
    l0 = c.kp(xb - 2, 100.0, near(base(0), 20, 40), octave=0)
    # best 10 at level 1; seconds tie at 12: level 1 first (10 > 9.6 rejects), level 0 first (accepts)
    exp = {l0: p0}
    for k, first_level in enumerate((1, 0)):
        x, y = site(40 + 2 * k)
        b = base(1 + k)
        p = c.pt(x, y, b, level=1)
        best = c.kp(x, y, near(b, 10), octave=1)
        s1 = c.kp(x + 1, y, near(b, 12, 50), octave=first_level)
        s2 = c.kp(x + 2, y, near(b, 12, 100), octave=1 - first_level)
        c.dist += [(p, best, 10), (p, s1, 12), (p, s2, 12)]
        if first_level == 0:
            exp[best] = p
    c.dist += [(p0, r0, 20), (p0, l0, 20)]
    c.claims["left column first, higher index"] = cell_of(fp, xb - 2, 100.0)[0] == 20 and cell_of(fp, xb + 2, 100.0)[0] == 21 and l0 > r0
    c.claims["10 / 12 fails the ratio"] = 10 > 0.8 * 12
    return c.case((exp, 2))


def th_high():
    """bestDist 100 is accepted, 101 is not, and candidates at 256 never become a best."""
    c = A4()
    q0, j0 = c.pair(0, 0, dist=100)
    q1, j1 = c.pair(1, 1, dist=101)
    x, y = site(2)
    q2, *_ = c.pt(x, y, base(2))
    j2 = c.kp(x, y, np.bitwise_not(base(2)))
    c.dist.append((q2, j2, 256))
    return c.case(({j0: q0}, 1))


def slot_states(with_state=True):
    """Pre-call LOCKED slots are never candidates, occupied-but-FREE slots are; with no slot array
    every slot is EMPTY."""
    c = A4()
    x, y = site(0)
    q0, *_ = c.pt(x, y, base(0))
    lk = c.kp(x - 3, y, near(base(0), 5), state=LOCKED)
    em = c.kp(x + 3, y, near(base(0), 30, 50))
    x, y = site(1)
    q1, *_ = c.pt(x, y, base(1))
    fr = c.kp(x - 3, y, near(base(1), 5), state=FREE)
    e1 = c.kp(x + 3, y, near(base(1), 30, 50))
    c.dist += [(q0, lk, 5), (q0, em, 30), (q1, fr, 5), (q1, e1, 30)]
    if with_state:
        return c.case(({em: q0, fr: q1}, 2))
    return c.case(({lk: q0, fr: q1}, 2), slot_state=False)


def double_accept(loser=None):
    """An unlocked earlier point and a later point accept one slot: the later index stays and both
    count.  loser = 0 / 1: that one of the two falls in a histogram bin that loses (11 matches in bin
    0 against 1): the slot becomes NULL and the count drops by exactly one."""
    c = A4()
    x, y = site(0)
    q0, *_ = c.pt(x, y, base(0), locked=0, angle=60.0 if loser == 0 else 0.0)
    for _ in range(130):  # points without a map point: the two writers are far apart in the call
        c.pt(x, y, base(0), has_mp=0)
    q1, *_ = c.pt(x + 1, y, near(base(0), 3, 200), locked=1, angle=60.0 if loser == 1 else 0.0)
    s = c.kp(x, y, near(base(0), 8))
    c.dist += [(q0, s, 8), (q1, s, 11)]
    exp = {}
    for i in range(10):
        q, j = c.pair(1 + i, 10 + i)
        exp[j] = q
    c.claims["bins"] = (hist_bin(60.0, 0.0), hist_bin(0.0, 0.0)) == (5, 0)
    c.claims["writers more than a wavefront apart"] = q1 - q0 > 64
    if loser is None:
        exp[s] = q1
        return c.case((exp, 12))
    # 11 in bin 0, 1 in bin 5: 1 < 0.1f * 11 drops bin 5
    exp[s] = NULL
    return c.case((exp, 11))


def claims_in_call_a4():
    """A locked earlier point takes the later point's best slot: the later point takes its second."""
    c = A4()
    x, y = site(0)
    q0, *_ = c.pt(x, y, base(0), locked=1)
    q1, *_ = c.pt(x, y, base(0), locked=1)
    s = c.kp(x - 2, y, near(base(0), 5))
    t = c.kp(x + 2, y, near(base(0), 20, 100))
    # the same with an unlocked first point: both take the best, the later index stays
    x, y = site(1)
    q2, *_ = c.pt(x, y, base(1), locked=0)
    q3, *_ = c.pt(x, y, base(1), locked=1)
    s2 = c.kp(x - 2, y, near(base(1), 5))
    t2 = c.kp(x + 2, y, near(base(1), 20, 100))
    c.dist += [(q0, s, 5), (q1, s, 5), (q1, t, 20), (q2, s2, 5), (q3, s2, 5), (q3, t2, 20)]
    return c.case(({s: q0, t: q1, s2: q3}, 4))


def claims_in_call_a5():
    """The slot an earlier locked point takes was the later point's SECOND best at the best's level:
    with the claim the ratio test has no second and accepts (40 against 256); where the earlier point
    is unlocked the second stays and 40 > 0.8 * 45 rejects."""
    c = A5()
    exp, nm = {}, 0
    for k, locked in enumerate((1, 0)):
        x, y = site(k)
        b0 = base(10 * k)
        b1 = near(b0, 50)                       # the later point's descriptor
        p0 = c.pt(x, y, b0, locked=locked)
        p1 = c.pt(x, y, b1, locked=1)
        s = c.kp(x - 1, y, near(b0, 5))         # 5 from p0, 45 from p1
        b = c.kp(x + 1, y, near(b1, 40, 100))   # 40 from p1, 90 from p0
        c.dist += [(p0, s, 5), (p1, s, 45), (p1, b, 40), (p0, b, 90)]
        exp[s] = p0
        nm += 1
        if locked:
            exp[b] = p1
            nm += 1
    c.claims["ratio rejects 40 / 45"] = 40 > 0.8 * 45
    return c.case((exp, nm))


RATIO_PAIRS = [(4, 5), (40, 50), (80, 100), (100, 125), (41, 50)]


def ratio_edge():
    """a5's ratio test at 0.8 * bestDist2 exactly, its same-level condition, a locked second best."""
    c = A5()
    exp, nm, k = {}, 0, 0
    for second in ("same", "other_level", "locked"):
        for d1, d2 in RATIO_PAIRS:
            x, y = site(k)
            b = base(k)
            p = c.pt(x, y, b, level=1)
            j1 = c.kp(x - 1, y, near(b, d1), octave=1)
            j2 = c.kp(x + 1, y, near(b, d2, 128), octave=0 if second == "other_level" else 1,
                      state=LOCKED if second == "locked" else EMPTY)
            c.dist += [(p, j1, d1), (p, j2, d2)]
            if second != "same" or not d1 > 0.8 * d2:
                exp[j1] = p
                nm += 1
            k += 1
    c.claims["4k / 5k pairs sit on the edge"] = all(not d1 > 0.8 * d2 and d1 * 5 == d2 * 4 for d1, d2 in RATIO_PAIRS[:4])
    c.claims["41 / 50 is past it"] = 41 > 0.8 * 50
    c.claims["one rejection"] = nm == 14
    return c.case((exp, nm))


def radius_edge_a4():
    """|dx| == r is outside the window (strict <) and one float below is inside; the stereo check keeps
    |ur - uR| == radius and drops one ulp more; uR <= 0 skips it; a projection at u == max_x is kept and
    one float above is dropped; a point behind the camera is skipped."""
    fp = frame()
    T = pose(0.0)
    r = f32(15.0)
    # the frame's right bound is set to the exact projection of point qm, so u == max_x
    Xm = world_at(fp, T, 770.4, 300.0, 4.0)
    um, vm, _ = proj(fp, T, Xm)
    Xa = Xm.copy()
    while proj(fp, T, Xa)[0] <= um:
        Xa[0] = up(Xa[0])
    ua = proj(fp, T, Xa)[0]
    fp = frame(max_x=um)
    c = A4(fp)
    cl, exp = c.claims, {}
    # window edge in x and y
    x, y = site(0)
    q0, u, v, _ = c.pt(x, y, base(0))
    on = c.kp(f32(u + r), v, near(base(0), 3))
    inn = c.kp(down(f32(u + r)), v, near(base(0), 30, 50))
    cl["dx == r and one float below"] = f32(f32(u + r) - u) == r and abs(f32(down(f32(u + r)) - u)) < r
    x, y = site(2)
    q1, u, v, _ = c.pt(x, y, base(1))
    on_y = c.kp(u, f32(v - r), near(base(1), 3))
    in_y = c.kp(u, up(f32(v - r)), near(base(1), 30, 50))
    cl["dy == -r and one float above"] = abs(f32(f32(v - r) - v)) == r and abs(f32(up(f32(v - r)) - v)) < r
    exp.update({inn: q0, in_y: q1})
    # stereo
    x, y = site(4)
    q2, u, v, iz = c.pt(x, y, base(2))
    ur = f32(u - f32(fp["bf"] * iz))
    keep = c.kp(u - 2, v, near(base(2), 30, 50), uR=f32(ur - r))
    drop = c.kp(u + 2, v, near(base(2), 3), uR=down(f32(ur - r)))
    cl["stereo error == radius kept, above dropped"] = abs(f32(ur - f32(ur - r))) == r and abs(f32(ur - down(f32(ur - r)))) > r
    x, y = site(6)
    q3, u, v, iz = c.pt(x, y, base(3))
    zero = c.kp(u - 2, v, near(base(3), 3), uR=0.0)
    c.kp(u + 2, v, near(base(3), 30, 50), uR=-1.0)
    exp.update({keep: q2, zero: q3})
    # image bound
    qm, u, v, _ = c.pt(0, 0, base(4), X=Xm)
    km = c.kp(um - 9, vm, near(base(4), 3))
    qa, u2, _, _ = c.pt(0, 0, base(5), X=Xa)
    c.kp(um - 9, vm + 40, near(base(5), 3))
    cl["u == max_x and one float above"] = u == fp["max_x"] and u2 == ua == up(fp["max_x"])
    cl["bound keypoints are in column 63"] = cell_of(fp, um - 9, vm)[0] == 63
    exp[km] = qm
    # behind the camera: the keypoint sits where the point would project
    Xb = np.array([0.5, 0.3, -4.0], np.float32)
    qb, ub, vb, izb = c.pt(0, 0, base(6), X=Xb)
    c.kp(ub, vb, base(6))
    cl["behind the camera, projection inside the image"] = izb < 0 and fp["min_x"] < ub < fp["max_x"] and fp["min_y"] < vb < fp["max_y"]
    c.dist += [(q0, on, 3), (q0, inn, 30), (q1, on_y, 3), (q2, drop, 3), (q2, keep, 30), (q3, zero, 3)]
    return c.case((exp, 5))


def radius_edge_a5(th=1.0):
    """RadiusByViewingCos at float32(0.998) (2.5: the float is above the double 0.998) and one float
    below (4.0); th == 1 leaves r alone, th = 3 scales it (7.5 / 12)."""
    c = A5(th=th)
    exp, nm = {}, 0
    for k, vc in enumerate((f32(0.998), down(f32(0.998)))):
        x, y = site(k)
        p = c.pt(x, y, base(k), vc=vc)
        nr = c.kp(x + 3, y, near(base(k), 30))
        far = c.kp(x - 10, y, near(base(k), 10, 100))
        c.dist += [(p, nr, 30), (p, far, 10)]
        r = (2.5 if float(vc) > 0.998 else 4.0) * (1.0 if th == 1.0 else th)
        if r > 10:
            exp[far] = p
            nm += 1
        elif r > 3:
            exp[nr] = p
            nm += 1
    c.claims["float32(0.998) is above 0.998"] = float(f32(0.998)) > 0.998 >= float(down(f32(0.998)))
    c.claims["matches"] = nm == (1 if th == 1.0 else 2)
    # |dx| == r exactly at level 2: r = 4 * 1.44
    r = f32(f32(4.0) * c.fp["scale_factors"][2]) if th == 1.0 else f32(f32(f32(4.0) * f32(th)) * c.fp["scale_factors"][2])
    x, y = 0.0, 200.0  # r has more digits than floats near a lattice site carry: project at x = 0
    p = c.pt(f32(x), y, base(9), level=2)
    c.kp(f32(f32(x) + r), y, near(base(9), 3), octave=2)
    inn = c.kp(down(f32(f32(x) + r)), y, near(base(9), 40, 50), octave=1)
    c.claims["dx == r"] = f32(f32(f32(x) + r) - f32(x)) == r
    exp[inn] = p
    return c.case((exp, nm + 1))


LEVEL_MODES = ("neither", "forward", "backward", "at_b_forward", "past_b_forward", "at_b_backward", "past_b_backward")
_OFFS = [(-3, -3), (-1, -3), (1, -3), (3, -3), (-3, 3), (-1, 3), (1, 3), (3, 3)]


def _allowed(mode, o):
    if mode == "forward":
        return range(o, 8)
    if mode == "backward":
        return range(0, o + 1)
    return range(max(o - 1, 0), min(o + 1, 7) + 1)


def levels_a4(mode):
    """The level window of a4 in its three motion modes, at last octaves 0, 1 and 7 with a candidate
    at every octave 0..7.  Per octave two points: one whose distances fall with the octave (the highest
    allowed octave wins) and one whose distances rise (the lowest wins).  Forward at octave 0 applies
    no level filter at all.  The camera moves +-0.3 m, exactly b, or one float past b along z."""
    b = frame()["b"]
    tz = {"neither": 0.0, "forward": -0.3, "backward": 0.3, "at_b_forward": -b, "past_b_forward": -up(b),
          "at_b_backward": b, "past_b_backward": up(b)}[mode]
    c = A4(tz=tz)
    fwd, bwd = motion(c.fp, c.T, c.TL)
    want = {"neither": (False, False), "forward": (True, False), "backward": (False, True),
            "at_b_forward": (False, False), "past_b_forward": (True, False), "at_b_backward": (False, False),
            "past_b_backward": (False, True)}[mode]
    c.claims["motion mode"] = (fwd, bwd) == want
    m = "forward" if fwd else "backward" if bwd else "neither"
    exp = {}
    for ci, o in enumerate((0, 1, 7)):
        for ri, rising in enumerate((False, True)):
            x, y = 130.0 + 200 * ci, 130.0 + 210 * ri
            bs = base(10 * ci + ri)
            q, *_ = c.pt(x, y, bs, octave=o)
            slots = []
            for k, (dx, dy) in enumerate(_OFFS):
                d = 12 + 4 * k if rising else 40 - 4 * k
                slots.append(c.kp(x + dx, y + dy, near(bs, d), octave=k))
                c.dist.append((q, slots[-1], d))
            al = _allowed(m, o)
            exp[slots[min(al) if rising else max(al)]] = q
    c.claims["forward at octave 0 takes octave 7"] = m != "forward" or list(_allowed(m, 0)) == list(range(8))
    return c.case((exp, 6))


def levels_a5():
    """a5's level window [L - 1, L] at predicted levels 0 and 7, candidates at every octave."""
    c = A5()
    exp = {}
    for ci, L in enumerate((0, 7)):
        for ri, rising in enumerate((False, True)):
            x, y = 130.0 + 200 * ci, 130.0 + 210 * ri
            bs = base(10 * ci + ri)
            p = c.pt(x, y, bs, level=L)
            slots = []
            for k, (dx, dy) in enumerate(_OFFS):
                d = 12 + 4 * k if rising else 40 - 4 * k
                slots.append(c.kp(x + dx, y + dy, near(bs, d), octave=k))
                c.dist.append((p, slots[-1], d))
            al = range(max(L - 1, 0), L + 1)
            exp[slots[min(al) if rising else max(al)]] = p
    return c.case((exp, 4))


HISTOGRAMS = {
    # name: ([(rot degrees, count)], bins kept)
    "10_1_1": ([(60.0, 10), (84.0, 1), (108.0, 1)], {5, 7, 9}),
    "11_1": ([(60.0, 11), (84.0, 1)], {5}),
    "20_2_1": ([(60.0, 20), (84.0, 2), (108.0, 1)], {5, 7}),
    "four_equal": ([(108.0, 3), (48.0, 3), (240.0, 3), (24.0, 3)], {2, 4, 9}),
    "one_bin": ([(60.0, 4)], {5}),
    "two_bins": ([(60.0, 4), (300.0, 1)], {5, 25}),
    "tie_second": ([(60.0, 5), (120.0, 2), (24.0, 2), (240.0, 2)], {5, 2, 10}),
    "negative_rot": ([(-60.0, 11), (60.0, 1)], {25}),  # rot < 0 gains 360: bin 25, not bin 5
}


def histogram(name):
    """Accepted matches in prescribed rotation bins (one isolated match each): the 10 % rule of
    ComputeThreeMaxima at equality (0.1f * 10 == 1), ties between bins, fewer than three bins."""
    spec, kept = HISTOGRAMS[name]
    c = A4()
    exp, nm, s, counts = {}, 0, 0, {}
    for rot, n in spec:
        la, ca = (rot, 0.0) if rot >= 0 else (10.0, 10.0 - rot)
        b = hist_bin(la, ca)
        counts[b] = counts.get(b, 0) + n
        for _ in range(n):
            q, j = c.pair(s, s, rot=la, cur_angle=ca, locked=s % 2)
            exp[j] = q if b in kept else NULL
            nm += b in kept
            s += 1
    c.claims["bins"] = counts == {int(rot % 360 // 12): n for rot, n in spec}
    c.claims["0.1f * 10 == 1"] = f32(0.1) * f32(10) == f32(1) and f32(1) < f32(0.1) * f32(11)
    return c.case((exp, nm))


def histogram_rounding():
    """rot * factor at x.5 rounds up (6 deg -> bin 1, 18 deg -> bin 2), one float below rounds down.
    Bin 1 holds 30 + 2, bin 0 three (0 deg, just below 6 deg, a tiny negative rot), bin 2 one: both
    minor bins are under 3.2 and lose, so every rounding decision shows in a slot."""
    c = A4()
    exp, nm, s = {}, 0, 0
    items = [(12.0, 0.0)] * 30 + [(6.0, 0.0), (down(6.0), 0.0), (0.0, 0.0), (10.0, up(10.0)), (18.0, 0.0), (down(18.0), 0.0)]
    bins = []
    for la, ca in items:
        x, y = site(s)
        q, *_ = c.pt(x, y, base(s), angle=la, locked=s % 2)
        j = c.kp(x, y, near(base(s), 10), angle=ca)
        c.dist.append((q, j, 10))
        b = hist_bin(la, ca)
        bins.append(b)
        exp[j] = q if b == 1 else NULL
        nm += b == 1
        s += 1
    c.claims["bins of the six probes"] = bins[30:] == [1, 0, 0, 0, 2, 1]
    c.claims["x.5 products"] = f32(f32(6) * f32(f32(30) / f32(360))) == f32(0.5) and f32(f32(18) * f32(f32(30) / f32(360))) == f32(1.5)
    c.claims["tiny negative rot wraps to 360"] = f32(f32(f32(10) - up(10.0)) + f32(360)) == f32(360)
    return c.case((exp, nm))


def histogram_wrap():
    """Five matches at rot 0 and five at a tiny negative rot (360 -> bin 30 -> bin 0) make bin 0 hold
    10; bins 5, 7, 9 hold one each: 5 and 7 stay (10 / 1 / 1), 9 is the fourth.  Were the negative rots
    binned anywhere else, bins 7 and 9 would both lose."""
    c = A4()
    exp, nm, s = {}, 0, 0
    items = [(0.0, 0.0)] * 5 + [(10.0, up(10.0))] * 5 + [(60.0, 0.0), (84.0, 0.0), (108.0, 0.0)]
    for la, ca in items:
        x, y = site(s)
        q, *_ = c.pt(x, y, base(s), angle=la)
        j = c.kp(x, y, near(base(s), 10), angle=ca)
        c.dist.append((q, j, 10))
        b = hist_bin(la, ca)
        exp[j] = q if b in (0, 5, 7) else NULL
        nm += b in (0, 5, 7)
        s += 1
    c.claims["ten in bin 0"] = [hist_bin(la, ca) for la, ca in items] == [0] * 10 + [5, 7, 9]
    return c.case((exp, nm))


def grid_edges_a4():
    """Keypoints within half a cell of max_x / max_y round to column 64 / row 48: outside the grid and
    never matched although inside the window.  Keypoints in column 0 / 63 and row 0 / 47, with windows
    clipped on each of the four sides."""
    c = A4()
    fp = c.fp
    mx, my, nx, ny = (float(fp[k]) for k in ("max_x", "max_y", "min_x", "min_y"))
    exp, cl = {}, c.claims
    # right: the closer keypoint is out of the grid
    q, u, v, _ = c.pt(mx - 8, 200.0, base(0))
    out = c.kp(mx - 3, 200.0, near(base(0), 2))
    inn = c.kp(mx - 9, 200.0, near(base(0), 30, 50))
    cl["right: out of grid / column 63"] = cell_of(fp, mx - 3, 200.0) is None and cell_of(fp, mx - 9, 200.0)[0] == 63
    exp[inn] = q
    c.dist += [(q, out, 2), (q, inn, 30)]
    # bottom
    q, u, v, _ = c.pt(300.0, my - 7, base(1))
    out = c.kp(300.0, my - 2, near(base(1), 2))
    inn = c.kp(300.0, my - 8, near(base(1), 30, 50))
    cl["bottom: out of grid / row 47"] = cell_of(fp, 300.0, my - 2) is None and cell_of(fp, 300.0, my - 8)[1] == 47
    exp[inn] = q
    c.dist += [(q, out, 2), (q, inn, 30)]
    # left and top: column 0 / row 0 (keypoints may lie left of min_x + half a cell: they round to 0)
    q, u, v, _ = c.pt(nx + 3, 100.0, base(2))
    j = c.kp(nx + 1, 100.0, near(base(2), 7))
    cl["left: column 0"] = cell_of(fp, nx + 1, 100.0)[0] == 0
    exp[j] = q
    c.dist.append((q, j, 7))
    q, u, v, _ = c.pt(500.0, ny + 3, base(3))
    j = c.kp(500.0, ny + 1, near(base(3), 7))
    cl["top: row 0"] = cell_of(fp, 500.0, ny + 1)[1] == 0
    exp[j] = q
    c.dist.append((q, j, 7))
    # the corner cell (63, 47)
    q, u, v, _ = c.pt(mx - 8, my - 7, base(4))
    j = c.kp(mx - 10, my - 9, near(base(4), 7))
    cl["corner cell"] = cell_of(fp, mx - 10, my - 9) == (63, 47)
    exp[j] = q
    c.dist.append((q, j, 7))
    return c.case((exp, 5))


def grid_edges_a5():
    """a5 takes projections as given: windows clipped on the four sides and windows wholly outside the
    image (an empty area) beside keypoints in the border cells."""
    c = A5()
    fp = c.fp
    mx, my, nx, ny = (float(fp[k]) for k in ("max_x", "max_y", "min_x", "min_y"))
    exp = {}
    spots = [(nx + 1, 100.0, nx - 1, 100.0), (mx - 8, 150.0, mx - 6, 150.0), (200.0, ny + 1, 200.0, ny - 1),
             (250.0, my - 8, 250.0, my - 6)]
    for k, (kx, ky, px, py) in enumerate(spots):   # clipped windows that still reach their keypoint
        p = c.pt(px, py, base(k))
        j = c.kp(kx, ky, near(base(k), 9))
        exp[j] = p
        c.dist.append((p, j, 9))
    for k, (px, py) in enumerate([(mx + 100, 150.0), (nx - 100, 100.0), (200.0, ny - 100), (250.0, my + 100)]):
        c.pt(px, py, base(k))                      # the same descriptors, far outside
    c.claims["border cells"] = [cell_of(fp, s[0], s[1]) for s in spots] == [
        (0, cell_of(fp, 0, 100.0)[1]), (63, cell_of(fp, 0, 150.0)[1]), (cell_of(fp, 200.0, 0)[0], 0), (cell_of(fp, 250.0, 0)[0], 47)]
    return c.case((exp, 4))


def grid_big_window():
    """a4 at th 30, octave 7: radius 107.5, a window of about 18 x 21 cells -- more than 64, so the
    walk takes several 64-cell batches; the best candidate lies in the last column."""
    c = A4(th=30.0)
    fp = c.fp
    q, u, v, _ = c.pt(400.0, 250.0, base(0), octave=7)
    rng = np.random.default_rng(5)
    for k in range(40):
        dx, dy = rng.uniform(-100, 100, 2)
        j = c.kp(400.0 + dx, 250.0 + dy, near(base(0), 40 + k, 10), octave=6 + k % 2)
        c.dist.append((q, j, 40 + k))
    best = c.kp(400.0 + 104, 250.0 + 101, near(base(0), 12), octave=7)
    c.kp(400.0 + 108, 250.0, near(base(0), 3), octave=7)   # just outside the window
    c.dist.append((q, best, 12))
    r = float(f32(30.0) * fp["scale_factors"][7])
    ncell = (int(np.ceil((400 + r + 17.3) * fp["grid_w_inv"])) - int(np.floor((400 - r + 17.3) * fp["grid_w_inv"])) + 1) * \
        (int(np.ceil((250 + r + 11.6) * fp["grid_h_inv"])) - int(np.floor((250 - r + 11.6) * fp["grid_h_inv"])) + 1)
    c.claims["more than 64 cells"] = ncell > 64
    c.claims["radius"] = 104 < r < 108
    return c.case(({best: q}, 1))


def grid_crowded_cell():
    """One cell holding 70 keypoints: a 64-cell batch carries more than 64 entries, and the best is
    entry 68.  The query has more than kRegCand candidates with the best in the global tail."""
    c = A4()
    fp = c.fp
    cw, ch = 1.0 / float(fp["grid_w_inv"]), 1.0 / float(fp["grid_h_inv"])
    x0, y0 = float(fp["min_x"]) + 30 * cw, float(fp["min_y"]) + 20 * ch
    q, u, v, _ = c.pt(x0, y0, base(0))
    cells = set()
    for k in range(70):
        x, y = x0 - 4 + 8 * (k % 10) / 9.0, y0 - 3.5 + 7 * (k // 10) / 6.0
        d = 8 if k == 68 else 30 + k % 20
        j = c.kp(x, y, near(base(0), d, k), octave=k % 2)
        c.dist.append((q, j, d))
        cells.add(cell_of(fp, x, y))
    c.claims["one cell"] = cells == {(30, 20)}
    return c.case(({68: q}, 1))


def cluster(kind, nk):
    """nk keypoints in one window and five queries on it (nk = 1, 7, 8, 9: the register preload of
    the resolver clamps to the stride nk < kRegCand, fills exactly, and spills one candidate to the
    global tail; 20, 70: a long tail).  The keypoints are a base with 40 seeded bits flipped (about 70
    bits from each other); query i is 10 + i bits from its target: the last candidate, the first, the
    last again (claimed by then, so it falls back on the rest), a middle one; the fifth is inactive."""
    c = A4() if kind == "a4" else A5(th=3.0)
    x, y = site(20)
    rng = np.random.default_rng(nk)
    kd = [flip(base(3), rng.choice(200, size=40, replace=False)) for _ in range(nk)]
    targets = [nk - 1, 0, nk - 1, nk // 2, 0]
    qs = []
    for i, t in enumerate(targets):
        d = near(kd[t], 10 + i, 200 + 10 * i)
        if kind == "a4":
            qs.append(c.pt(x, y, d, locked=1, has_mp=int(i != 4))[0])
        else:
            qs.append(c.pt(x, y, d, level=1, locked=1, in_view=int(i != 4)))
    for j in range(nk):
        c.kp(x - 6 + 12.0 * (j % 10) / 9.0, y - 4 + (j // 10), kd[j], octave=j % 2)
    for i, t in enumerate(targets):
        c.dist.append((qs[i], t, 10 + i))
    c.claims["the rest stay under TH_HIGH"] = all(hamming(kd[0], k) <= 90 for k in kd)
    c.claims["window holds every keypoint"] = nk <= 70
    return c.case(None)


def chain_depth(kind, n, locked=True):
    """A dependency chain: keypoints 3 px apart on rows of 200, point k projected midway between slots
    k - 1 and k, 5 bits from slot k - 1 and 9 from slot k.  All points locked: point k finds slot k - 1
    taken by point k - 1 and takes slot k, so assign == arange(n) after a chain of depth n (n <= 200;
    longer chains break at the row starts).  All unlocked: every point keeps its first choice and the
    last writer stays."""
    c = A4(th=4.0) if kind == "a4" else A5()
    A = [list(range(0, 7)), list(range(7, 14)), list(range(14, 21))]
    b = base(0)
    S = [flip(b, A[k % 3]) for k in range(n)]
    pos = [(20.0 + 3.0 * (k % 200), 30.0 + 20.0 * (k // 200)) for k in range(n)]
    for k in range(n):
        pd = flip(flip(b, A[(k - 1) % 3]), A[k % 3][:5])
        x, y = pos[k][0] - 1.5, pos[k][1]
        c.pt(x, y, pd, locked=int(locked))
        if k % 200:
            c.dist.append((k, k - 1, 5))
        c.dist.append((k, k, 9))
    for k in range(n):
        c.kp(pos[k][0], pos[k][1], S[k])
    if locked:
        exp = {k: k for k in range(n)}
    else:
        exp = {k: k + 1 for k in range(n - 1) if (k + 1) % 200}
    c.claims["rows of 200"] = n <= 200 or n > K_REG_QUERIES
    return c.case((exp, n))


def two_frames_300():
    s = synth.two_frames(seed=1, n_kps=300, n_shared=150, prefilled=30)
    return dict(kind="a4", args=(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], s["last"], 15.0), claims={},
                dist=[], expect=None, qdesc=s["last"]["mp_desc"], kdesc=s["cur_kps"]["desc"])


SEMANTIC = {
    "tie_first_wins": tie_first_wins,
    "tie_first_wins_a5": tie_first_wins_a5,
    "th_high": th_high,
    "slot_states": slot_states,
    "slot_states_none": functools.partial(slot_states, False),
    "double_accept": double_accept,
    "double_accept_first_loses": functools.partial(double_accept, 0),
    "double_accept_second_loses": functools.partial(double_accept, 1),
    "claims_in_call_a4": claims_in_call_a4,
    "claims_in_call_a5": claims_in_call_a5,
    "ratio_edge": ratio_edge,
    "radius_edge_a4": radius_edge_a4,
    "radius_edge_a5_th1": functools.partial(radius_edge_a5, 1.0),
    "radius_edge_a5_th3": functools.partial(radius_edge_a5, 3.0),
    "levels_a5": levels_a5,
    "histogram_rounding": histogram_rounding,
    "histogram_wrap": histogram_wrap,
    "grid_edges_a4": grid_edges_a4,
    "grid_edges_a5": grid_edges_a5,
    "grid_big_window": grid_big_window,
    "grid_crowded_cell": grid_crowded_cell,
    "chain_a5_200": functools.partial(chain_depth, "a5", 200),
    "chain_a4_200": functools.partial(chain_depth, "a4", 200),
    "chain_a5_1100": functools.partial(chain_depth, "a5", 1100),
    "chain_a4_1100": functools.partial(chain_depth, "a4", 1100),
    "chain_a5_200_unlocked": functools.partial(chain_depth, "a5", 200, False),
    "chain_a4_200_unlocked": functools.partial(chain_depth, "a4", 200, False),
    "chain_a5_1100_unlocked": functools.partial(chain_depth, "a5", 1100, False),
    "chain_a4_1100_unlocked": functools.partial(chain_depth, "a4", 1100, False),
    "two_frames_300": two_frames_300,
}
SEMANTIC.update({"levels_a4_" + m: functools.partial(levels_a4, m) for m in LEVEL_MODES})
SEMANTIC.update({"histogram_" + h: functools.partial(histogram, h) for h in HISTOGRAMS})
# stride < kRegCand (1, 7), == (8), one candidate in the global tail (9), a long tail (20, 70)
SEMANTIC.update({"cluster_%s_%d" % (k, n): functools.partial(cluster, k, n) for k in ("a4", "a5") for n in (1, 7, 8, 9, 20, 70)})


# -------------------------------------------------------------------------------------- path cases
# (nq, nk): what the row straddles
PATH_SHAPES = {
    "stage_at": (100, 1024),       # nk == kStageKps: the candidate kernel builds the grid in LDS
    "stage_over": (100, 1025),     # nk > kStageKps: a grid built by a launch of its own
    "regc_at": (1024, 300),        # nq == kRegQueries: the resolver preloads its candidates
    "regc_over": (1025, 300),      # nq > kRegQueries: no preload, queries strided over the workgroup
    "strided_at": (1024, 1024),    # nq nk == kCandStrided: one strided pass
    "strided_over": (1025, 1024),  # nq nk > kCandStrided: count / scan / write
    "grid_global": (100, 6200),    # nk > kGridLds: the grid build's cell lists in global memory
    "resolve_mode1": (3000, 6200),   # 4 nk + 2 nq = 30800 > kResolveLds >= nq + nk: LDS mode 1
    "resolve_mode0": (24600, 6200),  # nq + nk = 30800 > kResolveLds: mode 0; nq nk > kCandBound: total read back
}
PATH_LIVE = 300  # live queries of the largest row


def _scatter(rng, n, live):
    """indices of the `live` live queries among n, in order"""
    return np.sort(rng.choice(n, size=live, replace=False))


def path_a4(name):
    nq, nk = PATH_SHAPES[name]
    live = min(nq, PATH_LIVE if nq > 3000 else nq)
    s = synth.two_frames(seed=40 + len(name), n_kps=nk, n_shared=min(nk // 2, max(live * 2 // 3, 1)), locked_frac=0.6,
                         prefilled=nk // 20)
    L = s["last"]
    rng = np.random.default_rng(nq + nk)
    src = np.concatenate([np.nonzero(L["has_mp"])[0], np.nonzero(L["has_mp"] == 0)[0]])[:live]  # map points first
    src = np.sort(src) if len(src) == live else np.resize(src, live)
    where = _scatter(rng, nq, live)
    rows = np.zeros(nq, np.int64)
    rows[where] = src
    last = {k: (v if k == "Tcw" else np.ascontiguousarray(v[rows])) for k, v in L.items()}
    dead = np.ones(nq, bool)
    dead[where] = False
    last["has_mp"] = np.where(dead, 0, last["has_mp"]).astype(np.uint8)
    return dict(kind="a4", args=(s["fp"], s["cur_Tcw"], s["cur_kps"], s["slot_state"], last, 15.0), claims={}, dist=[],
                expect=None, shape=(nq, nk))


def path_a5(name):
    nq, nk = PATH_SHAPES[name]
    live = min(nq, PATH_LIVE if nq > 3000 else nq)
    pr = synth.local_points_problem(seed=60 + len(name), n_kps=nk, n_pts=live, n_true=min(live, nk) * 2 // 3,
                                    slot_prefill=nk // 20)
    rng = np.random.default_rng(nq + nk + 1)
    where = _scatter(rng, nq, live)
    pts = {}
    for k, v in pr["pts"].items():
        a = np.zeros((nq,) + v.shape[1:], v.dtype)
        a[where] = v
        pts[k] = a
    return dict(kind="a5", args=(pr["fp"], pr["kps"], pr["slot_state"], pts, 1.0), claims={}, dist=[], expect=None,
                shape=(nq, nk))


def path_local_map(name):
    """track_local_map inputs (the fused frustum + candidate kernel) at a row's shape"""
    nq, nk = PATH_SHAPES[name]
    pr = synth.local_map_problem(seed=80 + len(name), n_kps=nk, n_pts=nq, n_true=min(1200, nq // 2, nk // 2),
                                 n_in_frame=min(150, nq // 4))
    if nq > 3000:  # all but PATH_LIVE points already matched in the frame: they are skipped
        rng = np.random.default_rng(nq)
        inf = np.ones(nq, np.uint8)
        inf[_scatter(rng, nq, PATH_LIVE)] = 0
        pr["pts"]["in_frame"] = inf
    return pr


PATH = {}
for _n in PATH_SHAPES:
    PATH["a4_" + _n] = functools.partial(path_a4, _n)
    PATH["a5_" + _n] = functools.partial(path_a5, _n)


@functools.lru_cache(maxsize=None)
def get(name):
    """the case, built once per process (treat it as read-only)"""
    return (SEMANTIC.get(name) or PATH[name])()
