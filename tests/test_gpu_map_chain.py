"""GPU: the map step's serial chain between one solve and the next: the slide's cull and
scans run behind the append on the map's side stream, under the previous solve (LORB_NO_SIDE_CULL=1
keeps them on the ctx stream).  No arithmetic is touched, so every comparison here is bit for bit:
six keyframes stepped back to back with no host synchronisation in between, then every array of
lorb_map_read, the LM summary and the last solve's trace records.

Two window shapes (synth.mapping_sequence), confirmed through lorb_ba_plan_info:
  24 keyframes + 2 fixed, 40 new points and 400 keypoints per keyframe: 144 camera rows, the two-sided
     Cholesky (kind 2), whose fused iterations fold their tail;
   8 keyframes + 2 fixed, 24 new points and 256 keypoints per keyframe: another Cholesky kind, no fold.
The serial chains (overlap off) and the default overlapped chains are computed once per module."""
import contextlib
import os

import numpy as np
import pytest

from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth
from lorb_slam_amd.runtime import LocalMap, LorbError

pytestmark = pytest.mark.gpu
OPT10 = A.LMOptions.default(max_num_iterations=10, function_tolerance=0.0, gradient_tolerance=0.0,
                            parameter_tolerance=0.0)
N = 6
SHAPES = {24: dict(n_kf=24, n_fixed=2, n_new=40, n_kps=400), 8: dict(n_kf=8, n_fixed=2, n_new=24, n_kps=256)}
SCALARS = ("t0", "points", "observations", "keypoints", "new_points", "new_observations", "matches")
ARRAYS = ("point", "point_desc", "obs_point", "obs_kf", "obs_uv", "obs_frame", "pose", "fixed_pose", "match_train")
SWITCHES = ("LORB_NO_SIDE_CULL", "LORB_NO_FOLD", "LORB_NO_SPEC", "LORB_SPEC_SPOIL")


@contextlib.contextmanager
def env(**kv):
    """the library reads its switches at every step / build / solve: set around the steps"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b, label, map_only=False):
    """every array of lorb_map_read, the counts, the summary and the trace records, bit for bit
    (map_only: without the last call's own keypoint counts and matches, which a refused step sets)"""
    for k in SCALARS[:3] if map_only else SCALARS:
        assert a[k] == b[k], (label, k, a[k], b[k])
    for k in ARRAYS[:-1] if map_only else ARRAYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (label, k)
    assert a["summary"] == b["summary"], (label, a["summary"], b["summary"])
    assert a["trace"] == b["trace"], (label, "trace")


def read(M):
    g = M.read()
    g["trace"] = M.trace()
    return g


def upload(ctx, kfs):
    return [(k["pose"], k["Tcw"], len(k["x"]), ctx.to_device(A.u8(k["desc"])), ctx.to_device(A.f32(k["x"])),
             ctx.to_device(A.f32(k["y"])), ctx.to_device(A.f32(k["depth"]))) for k in kfs]


def free(dev):
    for d in dev:
        for a in d[3:]:
            a.free()


def chain(ctx, init, dev, opt=OPT10, overlap=True, step_env=None, before=None, reads=(), **create):
    """steps dev's keyframes back to back.  step_env: {step: switches} (key None: every step);
    before: {step: f(M)} called before that step; reads: steps after which the map is read with no
    explicit synchronisation first.  Returns (final read, {step: read}, plan info)."""
    assert not any(os.environ.get(k) for k in SWITCHES), "a switch is set outside the test"
    step_env = step_env or {}
    M = LocalMap(ctx, init, **create)
    fp = A.make_frame_params(synth.frame_params())
    mid = {}
    try:
        M.set_overlap(overlap)
        for i, (pose, Tcw, nk, dd, dx, dy, dz) in enumerate(dev):
            if before and i in before:
                before[i](M)
            with env(**dict(step_env.get(None, {}), **step_env.get(i, {}))):
                M.step_dev(fp, pose, Tcw, nk, dd, dx, dy, dz, opt)
            if i + 1 in reads:
                mid[i + 1] = read(M)
        return read(M), mid, M.plan_info()
    finally:
        M.close()


@pytest.fixture(scope="module")
def data(ctx):
    """per shape: the sequence, its keyframes in HBM (complete before any step), the serial chain read
    after steps 3 and 6, and the default overlapped chain"""
    out = {}
    for kf, shape in SHAPES.items():
        seq = synth.mapping_sequence(seed=7, obs_lens=(7, 8), steps=N, **shape)
        dev = upload(ctx, seq["steps"][:N])
        ctx.sync()
        serial, mid, info = chain(ctx, seq["init"], dev, overlap=False, reads=(3,))
        new, _, _ = chain(ctx, seq["init"], dev)
        out[kf] = dict(seq=seq, dev=dev, serial=serial, serial3=mid[3], new=new, info=info)
    yield out
    for d in out.values():
        free(d["dev"])


@pytest.mark.parametrize("kf", [24, 8])
def test_new_path_equals_serial(data, kf):
    """1. overlap on (cull and scans on the side stream) against overlap off"""
    d = data[kf]
    assert d["info"]["cameras"] == kf
    assert (d["info"]["cholesky"] == 2) == (kf == 24), d["info"]  # the two-sided kind and its fold, or not
    assert d["serial"]["overlapped_steps"] == 0
    g = d["new"]
    assert g["overlapped_steps"] == N - 1, g["overlapped_steps"]
    # builds speculated and at least one assumption held: the chain ran the bench's regime
    assert g["speculated_builds"] > g["spec_fallbacks"] >= 0, (g["speculated_builds"], g["spec_fallbacks"])
    same(g, d["serial"], f"{kf} KF overlapped vs serial")


@pytest.mark.parametrize("switch", ["LORB_NO_SIDE_CULL", "LORB_NO_FOLD"])
def test_switch_equals_default(ctx, data, switch):
    """2. each switch restores an old path (the cull and scans on the ctx stream; every iteration's
    tail as a kernel of its own) and changes no bit"""
    d = data[24]
    g, _, _ = chain(ctx, d["seq"]["init"], d["dev"], step_env={None: {switch: 1}})
    assert g["overlapped_steps"] == N - 1
    same(g, d["new"], switch)


def test_speculation_miss_equals_no_speculation(ctx, data):
    """3. LORB_SPEC_SPOIL=1 on step 3: the verification misses, the general build (with its copy) and
    a second solve follow; against LORB_NO_SPEC=1 throughout"""
    d = data[24]
    g, _, _ = chain(ctx, d["seq"]["init"], d["dev"], step_env={3: {"LORB_SPEC_SPOIL": 1}})
    assert g["spec_fallbacks"] >= 1, g["spec_fallbacks"]
    ref, _, _ = chain(ctx, d["seq"]["init"], d["dev"], step_env={None: {"LORB_NO_SPEC": 1}})
    assert ref["speculated_builds"] == 0
    same(g, ref, "spoiled vs no speculation")
    same(g, d["new"], "spoiled vs default")


def test_ceres_defaults_fold_switch(ctx, data):
    """4. Ceres-default options: a solve may end before its budget, in an iteration's head or tail;
    summaries and trace lengths with and without LORB_NO_FOLD=1"""
    d = data[24]
    opt = A.LMOptions.default()
    a, _, _ = chain(ctx, d["seq"]["init"], d["dev"], opt=opt)
    b, _, _ = chain(ctx, d["seq"]["init"], d["dev"], opt=opt, step_env={None: {"LORB_NO_FOLD": 1}})
    assert a["summary"] == b["summary"], (a["summary"], b["summary"])
    assert len(a["trace"]) == len(b["trace"]) > 0
    s, _, _ = chain(ctx, d["seq"]["init"], d["dev"], opt=opt, overlap=False)
    same(a, s, "Ceres defaults, overlapped vs serial")


def _with_keyframe(ctx, d, i, kf):
    dev = list(d["dev"])
    dev[i] = upload(ctx, [kf])[0]
    ctx.sync()
    return dev


def test_empty_keyframe(ctx, data):
    """5. a keyframe with n = 0 keypoints: nothing is appended, the cull still slides the window"""
    d = data[8]
    k = d["seq"]["steps"][2]
    dev = _with_keyframe(ctx, d, 2, dict(k, x=k["x"][:0], y=k["y"][:0], desc=k["desc"][:0], depth=k["depth"][:0]))
    try:
        g, mid, _ = chain(ctx, d["seq"]["init"], dev, reads=(3,))
        s, smid, _ = chain(ctx, d["seq"]["init"], dev, overlap=False, reads=(3,))
        assert mid[3]["keypoints"] == 0 and mid[3]["new_points"] == 0 and mid[3]["new_observations"] == 0
        assert mid[3]["t0"] == 3
        same(mid[3], smid[3], "empty keyframe, step 3")
        same(g, s, "empty keyframe, step 6")
    finally:
        free([dev[2]])


def test_distractor_keyframe(ctx, data):
    """6. a keyframe whose keypoints are all distractors (random descriptors, no stereo depth): no new
    point, so beside the crossCheck's matches only the slide changes the map.  (No match at all
    cannot be had from random descriptors: the reference's filter keeps d <= max(2 minDist, 30),
    and minDist is then large, so the mutual nearest pairs pass.)"""
    d = data[8]
    k = d["seq"]["steps"][2]
    rng = np.random.default_rng(66)
    kf = dict(k, desc=rng.integers(0, 256, k["desc"].shape, dtype=np.uint8), depth=np.full_like(k["depth"], -1.0))
    dev = _with_keyframe(ctx, d, 2, kf)
    try:
        g, mid, _ = chain(ctx, d["seq"]["init"], dev, reads=(3,))
        s, smid, _ = chain(ctx, d["seq"]["init"], dev, overlap=False, reads=(3,))
        assert mid[3]["new_points"] == 0 and mid[3]["new_observations"] == mid[3]["matches"]
        same(mid[3], smid[3], "distractor keyframe, step 3")
        same(g, s, "distractor keyframe, step 6")
    finally:
        free([dev[2]])


@pytest.mark.parametrize("kf", [24, 8])
def test_read_in_the_middle(ctx, data, kf):
    """7. lorb_map_read after 3 overlapped steps with no explicit synchronisation before it, then 3
    more steps: both reads equal the serial chain's at the same points"""
    d = data[kf]
    g, mid, _ = chain(ctx, d["seq"]["init"], d["dev"], reads=(3,))
    same(mid[3], d["serial3"], "read after 3 steps")
    same(g, d["serial"], "read after 6 steps")


def test_overlap_off_and_on_again(ctx, data):
    """8. lorb_map_set_overlap(0) in the middle of a chain, then on again"""
    d = data[24]
    g, _, _ = chain(ctx, d["seq"]["init"], d["dev"],
                    before={2: lambda M: M.set_overlap(False), 4: lambda M: M.set_overlap(True)})
    assert g["overlapped_steps"] == 3, g["overlapped_steps"]  # steps 1, 4, 5
    same(g, d["serial"], "overlap off and on again")


def test_capacity_error_overlapped(ctx, data):
    """9. test_local_mapping_capacity_error at the 8-KF shape with the overlap on: after one good step
    (so that the refused one runs overlapped, through the capacity branch) a keyframe of some 300 new
    points overflows the point capacity: LORB_E_NOMEM, and the map read afterwards equals the map
    before the call; the steps after it equal the serial chain's"""
    d = data[8]
    init = d["seq"]["init"]
    cap = dict(max_points=len(init["point_init"]) + 100, max_keypoints=512)
    k = d["seq"]["steps"][1]
    rng = np.random.default_rng(67)
    # 512 keypoints with random descriptors and a stereo depth: the crossCheck pairs about
    # 512 P / (512 + P) of them with the map's P (about 360) points, the rest (about 300) would be new
    # points against a capacity of 100 more than the initial map's
    big = dict(k, desc=rng.integers(0, 256, (512, 32), dtype=np.uint8), x=np.tile(k["x"], 2), y=np.tile(k["y"], 2),
               depth=np.full(512, 5.0, np.float32))
    bad = upload(ctx, [big])[0]
    ctx.sync()
    fp = A.make_frame_params(synth.frame_params())
    seen = {}

    def refused(M):
        before = read(M)
        with pytest.raises(LorbError, match=r"rc=-3: map capacity exceeded"):  # LORB_E_NOMEM
            M.step_dev(fp, *bad, OPT10)
        after = read(M)
        same(after, before, "after the refused step", map_only=True)
        assert after["new_points"] == 0 and after["new_observations"] == 0
        seen["overlapped"] = after["overlapped_steps"]

    try:
        g, _, _ = chain(ctx, init, d["dev"], before={1: refused}, **cap)
        assert seen["overlapped"] == 1  # the refused step ran its match and append on the side stream
        s, _, _ = chain(ctx, init, d["dev"], overlap=False, before={1: refused}, **cap)
        same(g, s, "chain around a refused step")
    finally:
        free([bad])
