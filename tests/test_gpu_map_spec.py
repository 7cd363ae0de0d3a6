"""GPU: the LocalMapping step's speculative plan build against the same chain with
LORB_NO_SPEC=1 (the build that waits for its readback before the gather and the solve).

A step that speculates enqueues the gather and the LM solve on the previous step's plan structure and
verifies afterwards; whatever happens -- the assumption holds, the adjacency pattern changed, a
buffer has to grow -- the map and the LM trace after every step are the serial build's, bit for bit.
The counters (lorb_map_counts' last two words) are checked against a prediction made on the CPU from
the reference chain's observation lists: a step after the first always speculates, and it falls back
exactly when the window's adjacency pattern differs from the previous step's (or, in the growth test,
when the pattern is constant and a buffer is too small)."""
import numpy as np
import pytest

from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth
from lorb_slam_amd.runtime import LocalMap

pytestmark = pytest.mark.gpu
OPT10 = A.LMOptions.default(max_num_iterations=10, function_tolerance=0.0, gradient_tolerance=0.0,
                            parameter_tolerance=0.0)
ARRAYS = ("point", "point_desc", "obs_point", "obs_kf", "obs_uv", "obs_frame", "pose", "fixed_pose", "match_train")
COUNTS = ("t0", "points", "observations", "keypoints", "new_points", "new_observations", "matches")
# two-sided Cholesky with the folded tail / k_ba_chol_w
SHAPES = {"kf24": dict(seed=9, n_kf=24, n_fixed=3, n_new=90, obs_lens=(4, 5), n_kps=800),
          "kf12": dict(seed=9, n_kf=12, n_fixed=3, n_new=60, obs_lens=(4, 5), n_kps=600)}
_cache = {}


def sequence(shape, steps):
    key = (shape, steps)
    if key not in _cache:
        _cache[key] = synth.mapping_sequence(steps=steps, **SHAPES[shape])
    return _cache[key]


def run(ctx, monkeypatch, seq, n, spec, spoil_at=(), overlap=False, init=None):
    """n steps of a new map; returns the state (lorb_map_read + LM trace) after every step.  overlap:
    the keyframes resident beforehand, the steps back to back with no sync, one state at the end."""
    if spec:
        monkeypatch.delenv("LORB_NO_SPEC", raising=False)
    else:
        monkeypatch.setenv("LORB_NO_SPEC", "1")
    monkeypatch.delenv("LORB_SPEC_SPOIL", raising=False)
    fp = A.make_frame_params(synth.frame_params())
    M = LocalMap(ctx, init or seq["init"])
    dev = []
    try:
        if overlap:
            dev = [(k["pose"], k["Tcw"], len(k["x"]), ctx.to_device(A.u8(k["desc"])), ctx.to_device(A.f32(k["x"])),
                    ctx.to_device(A.f32(k["y"])), ctx.to_device(A.f32(k["depth"]))) for k in seq["steps"][:n]]
            ctx.sync()
            M.set_overlap(True)
            for k in dev:
                M.step_dev(fp, *k, OPT10)
            return [dict(M.read(), trace=M.trace())]
        out = []
        for i in range(n):
            if i in spoil_at:  # the switch that spoils the kept adjacency before this step's build
                monkeypatch.setenv("LORB_SPEC_SPOIL", "1")
            M.step(fp, seq["steps"][i], OPT10)
            monkeypatch.delenv("LORB_SPEC_SPOIL", raising=False)
            out.append(dict(M.read(), trace=M.trace()))
        return out
    finally:
        M.close()
        for k in dev:
            for a in k[3:]:
                a.free()
        monkeypatch.delenv("LORB_NO_SPEC", raising=False)


def same_bits(a, b, label):
    for k in COUNTS:
        assert a[k] == b[k], (label, k, a[k], b[k])
    for k in ARRAYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (label, k)
    assert a["summary"] == b["summary"], (label, a["summary"], b["summary"])
    assert a["trace"] == b["trace"], label


def adjacency(g, W):
    """the window's camera adjacency pattern as the plan build sees it: cameras that share a point,
    the diagonal set for a camera with an observation"""
    B = np.zeros((max(g["points"], 1), W), np.int32)
    m = g["obs_frame"] >= 0
    B[g["obs_point"][m], g["obs_frame"][m]] = 1
    return (B.T @ B) > 0


def predicted_fallbacks(ref, W, forced=()):
    """per step, the fallbacks so far: a step after the first falls back when its pattern differs from
    the previous step's, or when the switch spoiled the kept pattern"""
    adj = [adjacency(g, W) for g in ref]
    out, n = [], 0
    for i in range(len(ref)):
        if i > 0 and (i in forced or not np.array_equal(adj[i], adj[i - 1])):
            n += 1
        out.append(n)
    return out


def check_chain(got, ref, W, forced=()):
    fb = predicted_fallbacks(ref, W, forced)
    for i, (a, b) in enumerate(zip(got, ref)):
        same_bits(a, b, f"step {i}")
        assert b["speculated_builds"] == 0 and b["spec_fallbacks"] == 0
        assert a["speculated_builds"] == i, (i, a["speculated_builds"])  # every step after the first
        assert a["spec_fallbacks"] == fb[i], (i, a["spec_fallbacks"], fb)
    return fb


@pytest.mark.parametrize("shape", ["kf24", "kf12"])
def test_spec_hit_path(ctx, monkeypatch, shape):
    """4 steps of a stationary stream: the window's pattern is the same at every step (checked here
    from the reference chain's observation lists), so every step after the first speculates and none
    falls back; every array and the LM trace equal the LORB_NO_SPEC=1 chain's after every step"""
    seq = sequence(shape, 4)
    W = SHAPES[shape]["n_kf"]
    ref = run(ctx, monkeypatch, seq, 4, spec=False)
    adj = [adjacency(g, W) for g in ref]
    assert all(np.array_equal(adj[0], a) for a in adj[1:]), "the sequence's pattern changes: pick another seed"
    got = run(ctx, monkeypatch, seq, 4, spec=True)
    fb = check_chain(got, ref, W)
    assert fb[-1] == 0 and got[-1]["speculated_builds"] == 3


def test_spec_miss_changed_pattern(ctx, monkeypatch):
    """a keyframe without keypoints (no observation: its camera leaves the pattern; the crossCheck
    would tie random descriptors to some point, so an empty keyframe it is) enters at step 2.  That
    step's assumption fails on the device (the speculative solve runs on an empty plan) and on the
    host, which builds and solves again; the changed row then slides through the window, so the steps
    after it fall back as well -- as predicted from the reference chain's patterns -- and every step
    equals the LORB_NO_SPEC=1 chain bit for bit"""
    base = sequence("kf12", 5)
    k = base["steps"][2]
    steps = list(base["steps"])
    steps[2] = dict(k, x=k["x"][:0], y=k["y"][:0], desc=k["desc"][:0], depth=k["depth"][:0])
    seq = dict(base, steps=steps)
    ref = run(ctx, monkeypatch, seq, 5, spec=False)
    assert ref[2]["matches"] == 0 and ref[2]["new_points"] == 0
    got = run(ctx, monkeypatch, seq, 5, spec=True)
    fb = check_chain(got, ref, 12)
    assert fb[1] == 0 and fb[2] == 1 and fb[-1] >= 1, fb


@pytest.mark.parametrize("shape", ["kf24", "kf12"])
def test_spec_miss_forced(ctx, monkeypatch, shape):
    """LORB_SPEC_SPOIL=1 before step 2 flips an entry of the kept pattern on the host: the device's
    check passes and the speculative solve does real work, the host's verification finds a changed
    pattern, builds again and solves again.  Step 2 falls back, step 3 speculates and hits; bit for
    bit the LORB_NO_SPEC=1 chain"""
    seq = sequence(shape, 4)
    W = SHAPES[shape]["n_kf"]
    ref = run(ctx, monkeypatch, seq, 4, spec=False)
    got = run(ctx, monkeypatch, seq, 4, spec=True, spoil_at=(2,))
    fb = check_chain(got, ref, W, forced=(2,))
    assert fb == [0, 0, 1, 1] and got[3]["speculated_builds"] == 3


def test_spec_buffer_growth(ctx, monkeypatch):
    """a map created from a third of the window's points: the plan's grow-only buffers are sized for
    that sparse window (capacity = 1.25 x the first build's need), and the stream's keyframes then add
    points at the full rate, so within a few steps the point groups outgrow the capacity.  The pattern
    stays the same throughout (checked), so the one fallback is the growth test's; bit for bit the
    LORB_NO_SPEC=1 chain"""
    n = 8
    seq = sequence("kf24", n)
    init = seq["init"]
    keep = np.zeros(len(init["point_init"]), bool)
    keep[::3] = True
    newid = np.cumsum(keep) - 1
    om = keep[init["obs_point"]]
    thin = dict(init, point_init=init["point_init"][keep], point_desc=init["point_desc"][keep],
                point_truth=init["point_truth"][keep], obs_point=newid[init["obs_point"][om]].astype(np.int32),
                obs_kf=init["obs_kf"][om], obs_uv=init["obs_uv"][om])
    ref = run(ctx, monkeypatch, seq, n, spec=False, init=thin)
    adj = [adjacency(g, 24) for g in ref]
    assert all(np.array_equal(adj[0], a) for a in adj[1:]), "the thinned window's pattern changes"
    groups0 = (ref[0]["points"] + ref[0]["observations"]) // 250 + 1
    groups1 = (ref[-1]["points"] + ref[-1]["observations"]) // 250 + 1
    assert groups1 > 1.3 * max(groups0, 16), (groups0, groups1)  # the window outgrew its first capacity
    got = run(ctx, monkeypatch, seq, n, spec=True, init=thin)
    for i, (a, b) in enumerate(zip(got, ref)):
        same_bits(a, b, f"step {i}")
        assert a["speculated_builds"] == i
    assert got[-1]["spec_fallbacks"] >= 1, got[-1]["spec_fallbacks"]
    assert got[-1]["spec_fallbacks"] <= 3, got[-1]["spec_fallbacks"]  # growth is by a quarter: a few times at most


def test_spec_overlapped_chain(ctx, monkeypatch):
    """the bench's regime on the 24-keyframe shape: 6 keyframes back to back, overlap on, no sync,
    speculation on, against the serial LORB_NO_SPEC=1 chain: bit for bit, 5 speculated builds, none
    fell back, 5 overlapped steps"""
    n = 6
    seq = sequence("kf24", n)
    ref = run(ctx, monkeypatch, seq, n, spec=False)
    got = run(ctx, monkeypatch, seq, n, spec=True, overlap=True)[0]
    same_bits(got, ref[-1], "overlapped chain")
    assert got["overlapped_steps"] == n - 1 and ref[-1]["overlapped_steps"] == 0
    assert got["speculated_builds"] == n - 1 and got["spec_fallbacks"] == 0
