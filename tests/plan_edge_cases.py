"""Hand-built local-BA windows that reach the data-dependent branches of the plan builders
(lorb_ba_build.hip): long point runs at chosen wave / workgroup positions (k_db_sorted's run scan and
its 16-observation loops, k_db_segsort's insertion sort), runs of unobserved points (the point-offset
fill, the global-atomic bit path past kDbWords words), a point with up to kGB - 1 observations (the
group size bound S = kGB - maxk down to 1: empty interior groups), more than 512 point groups (partial
runs without LORB_SG_F), the camera counts around the fused covisibility tables' limits, an idle
camera, a split covisibility graph and a one-camera plan.  Pure numpy; the properties each case
claims are asserted in test_plan_edge_cases.py (CPU), the solves in test_gpu_plan_edges.py.

Geometry (test_gpu_solver.wide_window's): optimised camera i at (0.1 i, 0, 0), fixed camera j at
(-0.1 (j + 1), 0, 0), no rotation; points at depth 4 .. 20, so every point is in front of every
camera; 0.5 px observation noise; initial values perturbed as wide_window perturbs them."""
import functools

import numpy as np

INTR = (435.2, 435.2, 367.5, 252.2)
WAVE, BLOCK = 64, 256  # k_db_sorted: one thread per slot, 64-slot waves, 256-slot workgroups
K_GB = 256             # observations a point group holds (lorb_ba_dev.h)


def window(seed, n_opt, n_fixed, points, gaps=None, tail=0):
    """The window dict lorb_ba_local / or_ba_local take.  points: for each observed point the list of
    frames that see it (>= 0: optimised camera, -1 - j: fixed camera j), kept in that order;
    gaps: {index into points: unobserved points inserted before it}; tail: unobserved points after
    the last one.  Observations are sorted by point."""
    rng = np.random.default_rng(seed)
    gaps = gaps or {}
    fx, fy, cx, cy = INTR
    cam_x = lambda f: 0.1 * f if f >= 0 else -0.1 * (-f)  # frame -1 - j -> -0.1 (j + 1)
    pts, obs_p, obs_f = [], [], []
    free = lambda: [rng.uniform(-6, 0.1 * n_opt + 6), rng.uniform(-3, 3), rng.uniform(4, 20)]
    for i, fr in enumerate(points):
        for _ in range(gaps.get(i, 0)):
            pts.append(free())
        fr = [int(f) for f in fr]
        assert all(-n_fixed <= f < n_opt for f in fr), (i, fr)
        x0 = float(np.mean([cam_x(f) for f in fr]))
        obs_p += [len(pts)] * len(fr)
        obs_f += fr
        pts.append([x0 + rng.uniform(-2, 2), rng.uniform(-3, 3), rng.uniform(4, 20)])
    for _ in range(tail):
        pts.append(free())
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    obs_p = np.asarray(obs_p, np.int32); obs_f = np.asarray(obs_f, np.int32)
    cam = np.where(obs_f >= 0, 0.1 * obs_f, -0.1 * (-obs_f.astype(np.float64)))
    Xc = pts[obs_p].copy()
    Xc[:, 0] -= cam
    uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1) + rng.normal(0, 0.5, (len(obs_p), 2))
    poses = np.zeros((n_opt, 6)); poses[:, 3] = -0.1 * np.arange(n_opt)
    fixed = np.zeros((n_fixed, 6)); fixed[:, 3] = 0.1 * (np.arange(n_fixed) + 1)
    pose_init = poses.copy()
    pose_init[:, :3] += rng.normal(0, 2e-3, (n_opt, 3))
    pose_init[:, 3:] += rng.normal(0, 2e-2, (n_opt, 3))
    return dict(pose_init=pose_init.astype(np.float32), fixed_pose=fixed.astype(np.float32).reshape(-1, 6),
                point_init=(pts + rng.normal(0, 5e-2, pts.shape)).astype(np.float32), obs_point=obs_p, obs_frame=obs_f,
                obs_uv=uv.astype(np.float32), intr=tuple(np.float32(v) for v in INTR))


def frames(rng, n_opt, n_fixed, k_opt, k_fixed, shuffle=True):
    """k_opt consecutive optimised cameras and k_fixed consecutive fixed ones, in a drawn order"""
    a = int(rng.integers(0, n_opt - k_opt + 1))
    fr = list(range(a, a + k_opt))
    if k_fixed:
        b = int(rng.integers(0, n_fixed - k_fixed + 1))
        fr += [-1 - j for j in range(b, b + k_fixed)]
    if shuffle:
        fr = [fr[i] for i in rng.permutation(len(fr))]
    return fr


def filler_lengths(rng, total):
    """run lengths of 3 .. 9 that sum to total (0, or >= 3)"""
    assert total == 0 or total >= 3, total
    out = []
    while total:
        ok = [k for k in range(3, 10) if total - k == 0 or total - k >= 3]
        out.append(int(rng.choice(ok)))
        total -= out[-1]
    return out


def run_starts(obs_point):
    """(first slot, length, point) of every point's run in point-sorted slots"""
    op = np.asarray(obs_point)
    s = np.flatnonzero(np.r_[True, op[1:] != op[:-1]])
    return s, np.diff(np.r_[s, len(op)]), op[s]


# ---- case 1: run lengths -----------------------------------------------------------------
N_OPT1, N_FIX1 = 50, 40
# the named runs: length and first slot.  lane = slot % 64, workgroup = slot // 256; the tail is what
# of the run lies past the wave of its first slot (k_db_sorted scans it in batches of 8).
RUNS1 = dict(
    lane0=(65, 64),      # starts at lane 0, covers wave 1 and one slot more (tail 1)
    late=(17, 189),      # starts at lane 61, ends in the next wave (tail 14)
    border=(90, 230),    # crosses the workgroup border at 256 and covers wave 4 whole
    tail64=(72, 376),    # starts at lane 56; tail 64: eight full batches, then an empty one
    tail8=(33, 487),     # starts at lane 39; tail 8: one full batch; crosses the border at 512
    wave=(64, 576),      # exactly one wave: no boundary above lane 0 in the ballot, tail 0
    to_end=(63, 705),    # starts at lane 1 and ends with its wave (tail 0 from inside a wave)
)
SHORT1 = (2, 15, 16, 18)  # around the 16-observation forms of the duplicate / covisibility loops


def _long_frames(rng, n, n_opt=N_OPT1, n_fixed=N_FIX1):
    if n == 2:  # two optimised cameras (a fixed one would leave a single optimised camera)
        return frames(rng, n_opt, n_fixed, 2, 0)
    k_opt = n_opt if n >= n_opt + n_fixed else min(n - 1, n_opt - 5)
    return frames(rng, n_opt, n_fixed, k_opt, n - k_opt)


def run_length_points(seed=101, extra_fillers=190):
    """case 1's point list and {name: index into it} of the named runs"""
    rng = np.random.default_rng(seed)
    pts, named, pos = [], {}, 0

    def fill(to):
        nonlocal pos
        for k in filler_lengths(rng, to - pos):
            pts.append(frames(rng, N_OPT1, N_FIX1, k - 1, 1)); pos += k

    def put(n, name=None):
        nonlocal pos
        if name:
            named[name] = len(pts)
        pts.append(_long_frames(rng, n)); pos += n
    order = sorted(RUNS1.items(), key=lambda kv: kv[1][1])
    shorts = list(SHORT1)
    for name, (n, at) in order:
        # the short runs go where the gap before a named run leaves room for them and a filler
        while shorts and at - pos - shorts[0] >= 3 and name != "lane0":
            put(shorts.pop(0))
        fill(at)
        put(n, name)
    for n in shorts:
        put(n)
    for _ in range(extra_fillers):
        k = int(rng.integers(3, 10))
        pts.append(frames(rng, N_OPT1, N_FIX1, k - 1, 1)); pos += k
    return pts, named


@functools.lru_cache(maxsize=None)
def run_lengths():
    pts, named = run_length_points()
    return window(201, N_OPT1, N_FIX1, pts), named


# ---- case 2: gaps ------------------------------------------------------------------------
def gap_plan(mult64):
    """case 1's points with unobserved points among them: 5 before point 0; 300 in a row in front of
    a run that starts inside a 256-slot block (the block's later points then lie more than kDbWords = 4
    point words past its first); exactly 64 in a row; 700 at the end; and a few more before another
    point, which bring n_points to a multiple of 64 (mult64) or away from one.
    Returns (points, names, gaps, tail)."""
    pts, named = run_length_points()
    starts = np.cumsum([0] + [len(f) for f in pts])[:-1]
    mid = int(np.flatnonzero((starts % BLOCK >= 60) & (starts % BLOCK <= 120) & (starts > 1024))[0])
    g = {0: 5, mid: 300, named["tail64"]: 64}
    n = len(pts) + 5 + 300 + 64 + 700
    pad = (-n) % 64 or 64
    if not mult64:
        pad = pad - 1 if pad > 1 else 7
    g[named["wave"]] = pad
    return pts, dict(named, mid=mid), g, 700


@functools.lru_cache(maxsize=None)
def gaps(mult64=False):
    pts, named, g, tail = gap_plan(mult64)
    return window(201, N_OPT1, N_FIX1, pts, gaps=g, tail=tail), dict(named, gaps=g, tail=tail)


@functools.lru_cache(maxsize=None)
def gaps_128(seed=251):
    """the same kinds of gaps at 128 cameras, where k_db_sorted's covisibility tables are not fused: only
    there do the covisibility counts come from the camera x point bits (k_db_cov), so only there does a
    bit lost on the global-atomic path change the plan.  128 fixed cameras, 600 points with 4 consecutive
    optimised cameras and a fixed one."""
    rng = np.random.default_rng(seed)
    pts = [frames(rng, 128, 128, 4, 1) for _ in range(600)]
    mid = next(i for i in range(210, 600) if 60 <= (5 * i) % BLOCK <= 120)
    g = {0: 5, mid: 300, 400: 64, 500: 7}
    return window(seed, 128, 128, pts, gaps=g, tail=700), dict(mid=mid, gaps=g, tail=700)


# ---- case 3: one point with up to kGB - 1 observations -----------------------------------
N_OPT3, N_FIX3 = 16, 239


@functools.lru_cache(maxsize=None)
def maxk(n, seed=301):
    """one point seen by n frames (all 16 optimised cameras and n - 16 fixed ones), 60 points with 4
    consecutive optimised cameras and a fixed one, and a point seen by 20 fixed cameras and the two
    optimised cameras farthest apart.  S = kGB - n."""
    rng = np.random.default_rng(seed)
    pts = [frames(rng, N_OPT3, N_FIX3, 4, 1) for _ in range(60)]
    big = [int(f) for f in rng.permutation(list(range(N_OPT3)) + [-1 - j for j in range(n - N_OPT3)])]
    far = [0] + [-1 - j for j in range(100, 120)] + [N_OPT3 - 1]
    pts.insert(30, big)
    pts.insert(46, far)
    return window(seed + n, N_OPT3, N_FIX3, pts), dict(big=30, far=46)


# ---- case 4: more than 512 point groups --------------------------------------------------
N_OPT4, N_FIX4 = 20, 230


@functools.lru_cache(maxsize=None)
def partial_runs(seed=401):
    """one point seen by all 250 frames (S = 6) and 620 points with 4 consecutive optimised cameras and
    a fixed one: K + P = 3971, 662 point groups, sg_factor 2 without LORB_SG_F"""
    rng = np.random.default_rng(seed)
    pts = [frames(rng, N_OPT4, N_FIX4, 4, 1) for _ in range(620)]
    pts.insert(310, [int(f) for f in rng.permutation(list(range(N_OPT4)) + [-1 - j for j in range(N_FIX4)])])
    return window(seed, N_OPT4, N_FIX4, pts), dict(big=310)


def layout(w):
    """db_layout's counts of a window: (S, point groups, groups per partial run, partial runs)"""
    K, P = len(w["obs_point"]), len(w["point_init"])
    mk = int(np.bincount(w["obs_point"], minlength=P).max())
    S = K_GB - mk
    G = (K + P - 1) // S + 1
    SF = (G + 479) // 480 if G > 512 else 1
    return S, G, SF, (G + SF - 1) // SF


# ---- case 5: the camera counts around the fused covisibility tables' limits --------------
@functools.lru_cache(maxsize=None)
def fuse(n_kf):
    """synth.ba_window at n_kf keyframes, slots stable-sorted by point.  k_db_sorted's covisibility
    tables (4 (C^2 + C) bytes) are fused while they fit 64 KB: up to 127 cameras; with the camera x
    point bit words in front of them (32 C bytes) the kernel's dynamic LDS passes 64 KB at 124."""
    from lorb_slam_amd import synth
    # 0.02 px noise: at synth's 0.5 px this long thin chain (3 - 4 cameras per point, 80 fixed observations)
    # does not meet the function tolerance within 10 iterations under Ceres-default options; at 0.02 px the
    # oracle stops on it after 9
    w = synth.ba_window(seed=1, n_kf=n_kf, n_pts=600, obs_lens=(3, 4), n_fixed=2, fixed_obs_per_kf=40, noise_px=0.02)
    o = np.argsort(w["obs_point"], kind="stable")
    return dict(w, obs_point=w["obs_point"][o], obs_frame=w["obs_frame"][o], obs_uv=w["obs_uv"][o]), {}


# ---- case 6: idle camera, split graph, one camera ----------------------------------------
@functools.lru_cache(maxsize=None)
def idle_and_split(seed=601):
    """12 cameras: camera 5 sees nothing, cameras 0 .. 4 and 6 .. 11 share no point"""
    rng = np.random.default_rng(seed)
    pts = []
    for i in range(90):
        lo, n = (0, 5) if i % 2 == 0 else (6, 6)
        k = int(rng.integers(2, 5))
        a = lo + int(rng.integers(0, n - k + 1))
        pts.append([int(f) for f in rng.permutation(list(range(a, a + k)) + [-1 - int(rng.integers(0, 2))])])
    return window(seed, 12, 2, pts), dict(idle=5)


@functools.lru_cache(maxsize=None)
def one_camera(seed=611):
    """a single optimised camera; every point is seen by it and by two of three fixed cameras"""
    rng = np.random.default_rng(seed)
    pts = [[0] + [-1 - int(j) for j in rng.choice(3, 2, replace=False)] for _ in range(60)]
    return window(seed, 1, 3, pts), {}


CASES = {
    "run_lengths": run_lengths,
    "gaps": gaps,
    "gaps_mult64": lambda: gaps(True),
    "gaps_128": gaps_128,
    "maxk_255": lambda: maxk(255),
    "maxk_254": lambda: maxk(254),
    "maxk_128": lambda: maxk(128),
    "partial_runs": partial_runs,
    "fuse_123": lambda: fuse(123),
    "fuse_124": lambda: fuse(124),
    "fuse_127": lambda: fuse(127),
    "idle_and_split": idle_and_split,
    "one_camera": one_camera,
}


def case(name):
    """(window, names) of a case; the window is shared between tests: do not write into it"""
    return CASES[name]()


# ---- duplicates in a long run, limits ----------------------------------------------------
def dup_window(start, i, j, seed=701):
    """(clean, dup): a window of case 1's shape whose 72-observation run begins at slot `start`; in dup
    the observation at position j of that run (a fixed camera's) is one more of the optimised camera
    at position i"""
    rng = np.random.default_rng(seed)
    pts = [frames(rng, N_OPT1, N_FIX1, k - 1, 1) for k in filler_lengths(rng, start)]
    at = len(pts)
    run = frames(rng, N_OPT1, N_FIX1, 45, 27, shuffle=False)
    fix, opt = [f for f in run if f < 0], [f for f in run if f >= 0]
    run = [None] * 72
    run[j] = fix.pop()
    rest = [f for f in rng.permutation(opt + fix)]
    k = [q for q in range(72) if q != j]
    for q, f in zip(k, rest):
        run[q] = int(f)
    if run[i] < 0:  # position i holds an optimised camera
        q = next(q for q in range(72) if run[q] >= 0 and q != j)
        run[i], run[q] = run[q], run[i]
    pts.append(run)
    pts += [frames(rng, N_OPT1, N_FIX1, int(k) - 1, 1) for k in rng.integers(3, 10, 120)]
    clean = window(seed + start, N_OPT1, N_FIX1, pts)
    s, n, _ = run_starts(clean["obs_point"])
    assert s[at] == start and n[at] == 72
    dup = dict(clean, obs_frame=clean["obs_frame"].copy())
    assert dup["obs_frame"][start + j] < 0 <= dup["obs_frame"][start + i]
    dup["obs_frame"][start + j] = dup["obs_frame"][start + i]
    return clean, dup


def with_fixed_capacity(w, n_fixed):
    """w with unreferenced fixed poses appended up to n_fixed rows"""
    fp = np.zeros((n_fixed, 6), np.float32)
    fp[:, 3] = 0.1 * (np.arange(n_fixed) + 1)
    fp[:len(w["fixed_pose"])] = w["fixed_pose"]
    return dict(w, fixed_pose=fp)


def wide_point_window(n_opt, n_fixed, big, seed=801, n_fill=600):
    """n_fill points with 4 consecutive optimised cameras and a fixed one, and in their middle one point
    seen by the frames `big`"""
    rng = np.random.default_rng(seed)
    pts = [frames(rng, n_opt, n_fixed, 4, 1) for _ in range(n_fill)]
    pts.insert(n_fill // 2, [int(f) for f in big])
    return window(seed, n_opt, n_fixed, pts), n_fill // 2


# the 72-observation run's first slot and the positions of the two copies in it
DUPS = {"beyond_16": (10, 20, 40), "two_waves": (100, 5, 60), "two_blocks": (230, 5, 60)}


@functools.lru_cache(maxsize=None)
def dup_case(name):
    return dup_window(*DUPS[name])


N_FIX_LIMIT = K_GB - N_OPT1  # fixed poses for which case 1's 50 cameras give a point kGB observations


@functools.lru_cache(maxsize=None)
def device_limit():
    """(good, bad) of one shape (50 optimised, 206 fixed): case 1 with unreferenced fixed poses appended, and
    case 1's points plus one seen by all 256 frames (one more than a device plan's point group takes)"""
    pts, _ = run_length_points()
    big = list(range(N_OPT1)) + [-1 - j for j in range(N_FIX_LIMIT)]
    bad = window(202, N_OPT1, N_FIX_LIMIT, pts + [big])
    return with_fixed_capacity(run_lengths()[0], N_FIX_LIMIT), bad


@functools.lru_cache(maxsize=None)
def host_limit(n_obs):
    """128 optimised cameras and n_obs - 128 fixed ones, one point seen by all of them"""
    nf = n_obs - 128
    return wide_point_window(128, nf, list(range(128)) + [-1 - j for j in range(nf)], seed=800 + n_obs)


@functools.lru_cache(maxsize=None)
def host_span_127():
    """128 optimised cameras, one point seen by cameras 0 and 127 (and a fixed one); 128 fixed cameras, whose
    long baselines to the optimised ones hold the points' depths"""
    return wide_point_window(128, 128, [0, 127, -1], seed=1)


@functools.lru_cache(maxsize=None)
def short_runs(seed=901):
    """case 1's shape with runs of 3 .. 9 only (S = kGB - 9): a rebuild from or to case 1 changes S"""
    rng = np.random.default_rng(seed)
    return window(seed, N_OPT1, N_FIX1, [frames(rng, N_OPT1, N_FIX1, int(k) - 1, 1) for k in rng.integers(3, 10, 260)])
