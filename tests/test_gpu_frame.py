"""GPU parity of the stereo Frame constructor as one call (lorb_frame_builder_* / lorb_frame_build(_dev),
lorb_slam_amd.frame.FrameBuilder) against the oracle composition O.orb_extract(left),
O.orb_extract(right), O.compute_stereo_matches on the two O.orb_pyramids -- and against today's
ctx.orb_extract x 2 + ctx.compute_stereo_matches.  Everything is np.array_equal.  Every case first
asserts, from the oracle alone, the property that makes it that case."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import golden_io
import oracle as O
import lorb_slam_amd.window as W
from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth
from lorb_slam_amd.frame import FrameBuilder
from lorb_slam_amd.runtime import LorbError, lib

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "octave", "size", "angle", "response", "desc", "level_off")
LDS_MAX_N = 252  # k_orb_octree's LDS path: node_cap = 4 max(N, 4) + 16 <= 1024

# name -> seed, rows, cols, levels, nfeatures, kind, pixel noise, depth > 0 found when the case was chosen
PAIRS = {
    "752x480": (500, 480, 752, 8, 1000, "scene", 2, 553),
    "320x256": (500, 256, 320, 8, 500, "scene", 2, 254),
    "376x240": (500, 240, 376, 4, 400, "scene", 2, 125),
    "160x120": (500, 120, 160, 3, 200, "scene", 2, 39),
    "1241x376": (508, 376, 1241, 8, 2000, "scene", 2, 1186),
    "noise256": (508, 256, 256, 8, 2000, "noise", 0, 314),
    "noise9000": (508, 480, 752, 8, 9000, "noise", 0, 2104),
    # further pairs of the 320 x 256 geometry (reuse) and the moved frame of the device chain
    "320x256-b": (501, 256, 320, 8, 500, "scene", 2, 0),
    "320x256-noise": (508, 256, 320, 8, 500, "noise", 0, 0),
}


@functools.lru_cache(maxsize=None)
def pattern():
    return golden_io.load(os.path.join(os.path.dirname(__file__), "golden", "orb.npz"))["pattern"]


def geometry(rows, cols, L, nf):
    fp = dict(synth.frame_params(width=cols, height=rows), n_levels=L)
    return fp, synth.scale_factors(n_levels=L), O.orb_features_per_level(nf)[:L]


def compose(left, right, fp, sf, nd):
    """The oracle composition that defines the expected frame."""
    ol, orr = O.orb_extract(left, nd, sf, pattern()), O.orb_extract(right, nd, sf, pattern())
    pl, pr = O.orb_pyramid(left, sf), O.orb_pyramid(right, sf)
    ur, dp, npair = O.compute_stereo_matches(fp, ol, orr, pl, pr)
    return dict(left=ol, right=orr, pyr_l=pl, pyr_r=pr, u_right=ur, depth=dp, npair=npair,
                counts=np.array([len(ol["x"]), len(orr["x"])], np.int32))


@functools.lru_cache(maxsize=None)
def case(name, shift=0, noise_seed=None):
    """Images, parameters and the oracle's frame of one pair; computed once, never modified."""
    seed, rows, cols, L, nf, kind, noise, fig = PAIRS[name]
    left, right = synth.stereo_pair(seed, rows, cols, kind=kind, noise=noise, shift=shift, noise_seed=noise_seed)
    fp, sf, nd = geometry(rows, cols, L, nf)
    return dict(left=left, right=right, fp=fp, sf=sf, nd=nd, o=compose(left, right, fp, sf, nd), fig=fig,
                geom=(rows, cols, L, nf))


@functools.lru_cache(maxsize=None)
def blank_case(rows, cols, L, nf, which):
    """which: 'right', 'left' or 'both' blank (a uniform grey 100); the other side is the 500 scene."""
    left, right = synth.stereo_pair(500, rows, cols)
    blank = np.full((rows, cols), 100, np.uint8)
    left = blank if which in ("left", "both") else left
    right = blank if which in ("right", "both") else right
    fp, sf, nd = geometry(rows, cols, L, nf)
    return dict(left=left, right=right, fp=fp, sf=sf, nd=nd, o=compose(left, right, fp, sf, nd))


def n_ini_of(shape):
    q = np.float32(shape[1] - 32) / np.float32(shape[0] - 32)
    return int(math.floor(float(q) + 0.5))


def guard(name):
    """The property that makes the pair its case, from the oracle alone."""
    c = case(name)
    o = c["o"]
    nl, nr = o["counts"]
    assert nl != nr and nl > 0 and nr > 0
    assert int((o["depth"] > 0).sum()) * 2 >= c["fig"]
    assert ((o["depth"] > 0) == (o["u_right"] >= 0)).all() and (o["depth"][o["depth"] <= 0] == -1).all()
    if name == "1241x376":
        assert [n_ini_of(p.shape) for p in o["pyr_l"]] == [4] * 8
        cells = [O.orb_cells(*p.shape)[0] for p in o["pyr_l"]]
        assert sum(int(((g[:, 2] == 0) | (g[:, 3] == 0)).sum()) for g in cells) >= 1
    elif name == "noise256":
        assert (c["nd"] > LDS_MAX_N).any()
    elif name == "noise9000":
        assert nr > 8192


@pytest.fixture(scope="module")
def builders(ctx):
    """One FrameBuilder per geometry, made on first use and shared by the tests of this module."""
    made = {}

    def get(rows, cols, L, nf):
        key = (rows, cols, L, nf)
        if key not in made:
            fp, _, nd = geometry(rows, cols, L, nf)
            made[key] = FrameBuilder(ctx, fp, rows, cols, nd, pattern())
        return made[key]

    yield get
    for b in made.values():
        b.close()


def assert_frame(g, o, what=""):
    assert np.array_equal(g["counts"], o["counts"]), (what, g["counts"], o["counts"])
    for side in ("left", "right"):
        for k in KEYS:
            assert np.array_equal(g[side][k], o[side][k]), (what, side, k)
    assert np.array_equal(g["u_right"], o["u_right"]), (what, "u_right")
    assert np.array_equal(g["depth"], o["depth"]), (what, "depth")


def sentinel_intact(a, first):
    return bool((np.ascontiguousarray(a[first:]).view(np.uint8) == W.ORB_SENTINEL).all())


def assert_write_bounds(d, o, cap, pb, n_levels):
    """Every device buffer of a device_resident build carries the sentinel past what the call owns."""
    raw = d["raw"]
    for side, n in (("left", int(o["counts"][0])), ("right", int(o["counts"][1]))):
        for k in ("x", "y", "octave", "size", "angle", "response", "desc"):
            assert len(raw[side][k]) == cap + W.ORB_GUARD and sentinel_intact(raw[side][k], n), (side, k)
        assert sentinel_intact(raw[side]["level_off"], n_levels + 1), side
        assert len(raw[side]["pyramid"]) == pb + W.ORB_GUARD and sentinel_intact(raw[side]["pyramid"], pb), side
        levels = o["pyr_l"] if side == "left" else o["pyr_r"]
        assert np.array_equal(raw[side]["pyramid"][:pb], np.concatenate([p.reshape(-1) for p in levels])), side
    nl = int(o["counts"][0])
    assert len(raw["u_right"]) == cap + W.ORB_GUARD and sentinel_intact(raw["u_right"], nl)
    assert len(raw["depth"]) == cap + W.ORB_GUARD and sentinel_intact(raw["depth"], nl)
    assert sentinel_intact(raw["counts"], 2)


@pytest.mark.parametrize("name", ["752x480", "320x256", "376x240", "160x120", "1241x376", "noise256", "noise9000"])
def test_parity_and_write_bounds(ctx, builders, name):
    """build (host arrays) and build(device_resident=True) equal the oracle composition and today's
    ctx.orb_extract x 2 + ctx.compute_stereo_matches on the same context, key by key; the device form
    writes nothing past n_left / n_right entries (they differ), past pyramid_bytes or past counts[2]."""
    guard(name)
    c = case(name)
    o = c["o"]
    b = builders(*c["geom"])
    cap, pb = W.orb_extract_capacity(*c["left"].shape, c["nd"], c["sf"])
    assert (b.capacity, b.pyramid_bytes) == (cap, pb)
    assert_frame(b.build(c["left"], c["right"]), o, "host")
    d = b.build(c["left"], c["right"], device_resident=True)
    assert_frame(d, o, "dev")
    assert_write_bounds(d, o, cap, pb, len(c["sf"]))
    tl = ctx.orb_extract(c["left"], c["nd"], c["sf"], pattern())
    tr = ctx.orb_extract(c["right"], c["nd"], c["sf"], pattern())
    ur, dp = ctx.compute_stereo_matches(c["fp"], tl, tr, o["pyr_l"], o["pyr_r"])
    today = dict(left=tl, right=tr, u_right=ur, depth=dp, counts=np.array([len(tl["x"]), len(tr["x"])], np.int32))
    assert_frame(d, today, "dev vs today's sequence")


@pytest.mark.parametrize("which", ["right", "left", "both"])
def test_empty_sides(ctx, builders, which):
    """A blank right image: n_right == 0 and every depth -1.  A blank left image: n_left == 0 and
    u_right / depth untouched (the sentinel intact from entry 0).  Both blank."""
    geom = (256, 320, 8, 500)
    c = blank_case(*geom, which)
    o = c["o"]
    if which == "right":
        assert o["counts"][0] > 0 and o["counts"][1] == 0 and (o["depth"] == -1).all() and (o["u_right"] == -1).all()
    elif which == "left":
        assert o["counts"][0] == 0 and o["counts"][1] > 0
    else:
        assert (o["counts"] == 0).all()
    b = builders(*geom)
    assert_frame(b.build(c["left"], c["right"]), o, "host")
    d = b.build(c["left"], c["right"], device_resident=True)
    assert_frame(d, o, "dev")
    assert_write_bounds(d, o, b.capacity, b.pyramid_bytes, 8)
    if which != "right":
        assert sentinel_intact(d["raw"]["u_right"], 0) and sentinel_intact(d["raw"]["depth"], 0)


def padded_view(img, pad, fill):
    big = np.full((img.shape[0], img.shape[1] + pad), fill, np.uint8)
    big[:, :img.shape[1]] = img
    v = big[:, :img.shape[1]]
    assert v.strides == (img.shape[1] + pad, 1) and not v.flags["C_CONTIGUOUS"]
    return v


def test_strides(ctx, builders):
    """Both images as views into wider buffers (row stride cols + 13), left and right padded with
    different bytes (255 / 0, then 0 / 255): host and device forms equal the contiguous result."""
    guard("320x256")
    c = case("320x256")
    b = builders(*c["geom"])
    for fl, fr in ((255, 0), (0, 255)):
        vl, vr = padded_view(c["left"], 13, fl), padded_view(c["right"], 13, fr)
        assert_frame(b.build(vl, vr), c["o"], ("host", fl))
        assert_frame(b.build(vl, vr, device_resident=True), c["o"], ("dev", fl))
    # different strides on the two sides
    vl = padded_view(c["left"], 13, 255)
    assert_frame(b.build(vl, c["right"]), c["o"], "host, left padded only")
    assert_frame(b.build(vl, c["right"], device_resident=True), c["o"], "dev, left padded only")


def test_reuse(ctx, builders):
    """One builder through A, B, blank / blank, a noise pair, A: each result equals its oracle and the
    second A the first.  In between, one ctx.orb_extract of another size and one
    ctx.compute_stereo_matches on the same context equal their oracles: the builder's scratch is its
    own.  Then two builders of different geometry alternate on the context."""
    geom = (256, 320, 8, 500)
    b = builders(*geom)
    small = case("160x120")
    seq = [case("320x256"), case("320x256-b"), blank_case(*geom, "both"), case("320x256-noise"), case("320x256")]
    assert not np.array_equal(seq[0]["left"], seq[1]["left"]) and seq[3]["o"]["counts"].min() > 0
    first = None
    for step, c in enumerate(seq):
        for dev in (False, True):
            g = b.build(c["left"], c["right"], device_resident=dev)
            assert_frame(g, c["o"], (step, dev))
        if step == 0:
            first = g
        if step == 1:
            t = ctx.orb_extract(small["left"], small["nd"], small["sf"], pattern())
            for k in KEYS:
                assert np.array_equal(t[k], small["o"]["left"][k]), k
        if step == 2:
            so = small["o"]
            ur, dp = ctx.compute_stereo_matches(small["fp"], so["left"], so["right"], so["pyr_l"], so["pyr_r"])
            assert np.array_equal(ur, so["u_right"]) and np.array_equal(dp, so["depth"])
    assert_frame(g, first, "second A vs first A")
    big = case("752x480")
    b_big, b_small = builders(*big["geom"]), builders(*small["geom"])
    for rnd in range(2):
        assert_frame(b_big.build(big["left"], big["right"], device_resident=True), big["o"], ("big", rnd))
        assert_frame(b_small.build(small["left"], small["right"], device_resident=True), small["o"], ("small", rnd))
        assert_frame(b_small.build(small["left"], small["right"]), small["o"], ("small host", rnd))
        assert_frame(b_big.build(big["left"], big["right"]), big["o"], ("big host", rnd))


def test_device_chain(ctx, builders):
    """Frame A and frame B (every band shifted 2 pixels further, other pixel noise) are built on the
    device; only the two counts records cross to the host.  lorb_unproject_stereo_dev on A's device
    arrays, then lorb_search_by_projection_frame_dev with B's device arrays as the current keypoints
    and A's arrays + the unprojected points + A's descriptors as the last frame: assign and nmatches
    equal O.search_by_projection_frame on the oracle's frames."""
    ca, cb = case("752x480"), case("752x480", 2, 777)
    oa, ob = ca["o"], cb["o"]
    fp, th = ca["fp"], 15.0
    I = np.eye(4, dtype=np.float32)
    has_mp = (oa["depth"] > 0).astype(np.uint8)
    locked = np.zeros(len(has_mp), np.uint8)
    last = dict(Tcw=I, has_mp=has_mp, outlier=None, mp_locked=locked,
                mp_pos=O.unproject_stereo(fp, I, oa["left"]["x"], oa["left"]["y"], oa["depth"]),
                mp_desc=oa["left"]["desc"], octave=oa["left"]["octave"], angle=oa["left"]["angle"])
    cur = dict({k: ob["left"][k] for k in ("x", "y", "octave", "angle", "desc")}, u_right=ob["u_right"])
    want, want_n = O.search_by_projection_frame(fp, I, cur, None, last, th)
    assert want_n > 20 and not np.array_equal(oa["u_right"], ob["u_right"][:len(oa["u_right"])])
    b = builders(*ca["geom"])
    fa = b.build_device(ca["left"], ca["right"])
    fb = b.build_device(cb["left"], cb["right"])
    held = []
    try:
        na, nb = fa.read_counts(), fb.read_counts()
        assert np.array_equal(na, oa["counts"]) and np.array_equal(nb, ob["counts"])
        n_last = int(na[0])
        fps = A.make_frame_params(fp)
        T = A.f32(I).reshape(16)
        pos = ctx.empty((max(n_last, 1), 3), np.float32)
        held.append(pos)
        ctx.check(lib().lorb_unproject_stereo_dev(ctx.handle, C.byref(fps), A.ptr(T, C.c_float), C.c_int32(n_last),
                                                  fa.left["x"].ptr, fa.left["y"].ptr, fa.depth.ptr, pos.ptr),
                  "lorb_unproject_stereo_dev")
        d_has, d_lock = ctx.to_device(has_mp), ctx.to_device(locked)  # the mask is uploaded, no keypoint is
        held += [d_has, d_lock]
        lf = A.LastFrameDev(n_last, A.ptr(T, C.c_float), d_has.ptr, None, d_lock.ptr, pos.ptr, fa.left["desc"].ptr,
                            fa.left["octave"].ptr, fa.left["angle"].ptr)
        k = fb.keypoints(int(nb[0]))
        asg, nm = ctx.empty(max(k.n, 1), np.int32), ctx.empty(1, np.int32)
        held += [asg, nm]
        ctx.check(lib().lorb_search_by_projection_frame_dev(ctx.handle, C.byref(fps), A.ptr(T, C.c_float), C.byref(k),
                                                            None, C.byref(lf), C.c_float(th), asg.ptr, nm.ptr),
                  "lorb_search_by_projection_frame_dev")
        assert int(nm.numpy()[0]) == want_n
        assert np.array_equal(asg.numpy()[:k.n], want)
    finally:
        fa.free()
        fb.free()
        for a in held:
            a.free()


def test_errors(ctx, builders):
    """create rejects the geometries lorb_orb_extract rejects and a null pattern; build rejects a step
    below cols.  After each rejection the context and an existing builder still give correct results."""
    small = case("160x120")
    b = builders(*small["geom"])

    def still_fine():
        t = ctx.orb_extract(small["left"], small["nd"], small["sf"], pattern())
        for k in KEYS:
            assert np.array_equal(t[k], small["o"]["left"][k]), k
        assert_frame(b.build(small["left"], small["right"], device_resident=True), small["o"], "after an error")

    def rejects_create(rows, cols, L, nf, pat="default"):
        fp, _, nd = geometry(rows, cols, L, nf)
        with pytest.raises(LorbError):
            FrameBuilder(ctx, fp, rows, cols, nd, pattern() if pat == "default" else pat)
        still_fine()

    assert 5 in [n_ini_of(p.shape) for p in O.orb_pyramid(np.zeros((230, 824), np.uint8), synth.scale_factors())]
    rejects_create(230, 824, 8, 600)          # 5 initial quadtree nodes on one level
    assert n_ini_of((300, 120)) == 0
    rejects_create(300, 120, 1, 100)          # 0 initial nodes
    assert int(np.float32(61 - 32) / np.float32(30)) == 0
    rejects_create(61, 62, 1, 50)             # no 30-pixel cell row
    rejects_create(120, 160, 3, 200, pat=None)  # null pattern
    rejects_create(4097, 160, 1, 100)         # more rows than the stereo row table holds
    for dev in (False, True):
        with pytest.raises(LorbError):
            b.build(small["left"], small["right"], device_resident=dev, step=small["left"].shape[1] - 1)
        still_fine()
