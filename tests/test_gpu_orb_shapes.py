"""GPU parity of the ORB extractor and the stereo matcher away from the one 752 x 480 geometry of
tests/test_gpu_window.py: 1, 3 and 4 initial quadtree nodes (and pyramids whose levels disagree),
skipped cells, sparse / empty levels, N = 0 and 1, padded rows, the device-resident entry points,
scratch reuse across image sizes, and more right keypoints than the stereo band cache holds.
Everything is np.array_equal against the oracle (tests/test_oracle_window.py pins the oracle to
pyref at these geometries).  Every case first asserts, from the oracle or the geometry alone, the
property that makes it that case."""
import functools
import math
import os

import numpy as np
import pytest

import golden_io
import oracle as O
import lorb_slam_amd.window as W
from lorb_slam_amd import synth
from lorb_slam_amd.frame import FrameBuilder
from lorb_slam_amd.runtime import LorbError

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "octave", "size", "angle", "response", "desc", "level_off")
DETECT_KEYS = ("x", "y", "octave", "size", "response", "level_off")
LDS_MAX_N = 252  # k_orb_octree's LDS path: node_cap = 4 max(N, 4) + 16 <= 1024

# row of the issue's table -> rows, cols, levels, nfeatures, image kind
CASES = {
    1: (480, 640, 8, 1000, "scene"),
    2: (256, 256, 8, 2000, "noise"),
    3: (256, 256, 8, 8, "scene"),
    4: (300, 813, 8, 600, "scene"),
    5: (232, 813, 3, 600, "scene"),
    6: (255, 550, 8, 500, "scene"),
    7: (300, 240, 6, 300, "scene"),
    8: (376, 1241, 8, 2000, "scene"),
    9: (256, 300, 8, 500, "sparse"),
    10: (256, 256, 8, 500, "blank"),
    11: (62, 62, 1, 50, "noise"),
}
SEEDS = {3: 204}  # 203 leaves a level of row 3 with 3 keypoints; its guard wants the reference's 4 per level


@functools.lru_cache(maxsize=None)
def pattern():
    return golden_io.load(os.path.join(os.path.dirname(__file__), "golden", "orb.npz"))["pattern"]


def make_image(kind, rows, cols, seed):
    if kind == "scene":
        return synth.orb_scene(seed, rows, cols, n_shapes=max(20, rows * cols // 3000))
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)
    img = np.full((rows, cols), 100, np.uint8)
    if kind == "sparse":
        img[60:90, 200:240] = 230  # a 30 x 40 bright rectangle
        img[190:192, 40:43] = 10   # a 2 x 3 dark dot
    return img


def n_ini_of(shape):
    """nIni of DistributeOctTree (src/ORBextractor.cpp:559): std::round of a float quotient."""
    q = np.float32(shape[1] - 32) / np.float32(shape[0] - 32)
    return int(math.floor(float(q) + 0.5))


def skipped_cells(shape):
    c, _, _ = O.orb_cells(*shape)
    return int(((c[:, 2] == 0) | (c[:, 3] == 0)).sum())


@functools.lru_cache(maxsize=None)
def case(row):
    """Image, parameters and the oracle's results of one table row; computed once, never modified."""
    rows, cols, L, nf, kind = CASES[row]
    img = make_image(kind, rows, cols, SEEDS.get(row, 200 + row))
    sf = synth.scale_factors(n_levels=L)
    nd = O.orb_features_per_level(nf)[:L]
    pyr = O.orb_pyramid(img, sf)
    o = O.orb_extract(img, nd, sf, pattern())
    return dict(img=img, sf=sf, nd=nd, pyr=pyr, o=o, counts=np.diff(o["level_off"]),
                n_ini=[n_ini_of(p.shape) for p in pyr], skipped=sum(skipped_cells(p.shape) for p in pyr))


def guard(row):
    """The property that makes the row that case, from the oracle / geometry alone."""
    c = case(row)
    ni, nd, cnt = c["n_ini"], c["nd"], c["counts"]
    if row == 1:
        assert ni == [1] * 8 and (nd <= LDS_MAX_N).all()
    elif row == 2:
        assert ni == [1] * 8 and (nd[:3] > LDS_MAX_N).all() and (cnt[-2:] < nd[-2:]).all() and (cnt[-2:] > 0).all()
    elif row == 3:
        assert nd.tolist() == [2, 1, 1, 1, 1, 1, 1, 0] and cnt.tolist() == [4] * 8
    elif row == 4:
        assert ni == [3] * 6 + [4] * 2 and c["skipped"] >= 1
    elif row == 5:
        assert ni == [4] * 3 and c["skipped"] >= 1 and len(c["pyr"]) == 3
    elif row == 6:
        assert ni == [2] * 4 + [3] * 4
    elif row == 7:
        assert ni == [1] * 6 and c["img"].shape[0] > c["img"].shape[1]
    elif row == 8:
        assert ni == [4] * 8 and c["skipped"] >= 1 and (nd > LDS_MAX_N).any()
    elif row == 9:
        assert (cnt == 0).any() and (cnt == 1).any() and (cnt < nd).all() and cnt.sum() > 2
    elif row == 10:
        assert len(c["o"]["x"]) == 0 and (c["o"]["level_off"] == 0).all()
    elif row == 11:
        cells, nc, nr = O.orb_cells(62, 62)
        assert (nc, nr) == (1, 1) and tuple(cells[0][2:]) == (30, 30) and len(c["o"]["x"]) > 0


def assert_same(g, o, keys=KEYS, what=""):
    for k in keys:
        assert np.array_equal(g[k], o[k]), (what, k)


def extract(ctx, row, img=None, **kw):
    c = case(row)
    return ctx.orb_extract(c["img"] if img is None else img, c["nd"], c["sf"], pattern(), **kw)


@pytest.mark.parametrize("row", sorted(CASES))
def test_extract_shapes(ctx, row):
    """lorb_orb_extract vs the oracle at every geometry of the table; for rows 1, 4 and 8 also the
    stages (pyramid, FAST cells with their cell tables, detection) against their oracles."""
    guard(row)
    c = case(row)
    assert_same(extract(ctx, row), c["o"], what=row)
    if row in (1, 4, 8):
        for a, b in zip(ctx.orb_pyramid(c["img"], c["sf"]), c["pyr"]):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert_same(ctx.orb_fast_cells(c["pyr"]), O.orb_fast_cells(c["pyr"]),
                    ("cell_base", "cell_off", "x", "y", "response"), row)
        assert_same(ctx.orb_detect(c["pyr"], c["nd"], c["sf"]), O.orb_detect(c["pyr"], c["nd"], c["sf"]),
                    DETECT_KEYS, row)


def sentinel_intact(a, first):
    return bool((np.ascontiguousarray(a[first:]).view(np.uint8) == W.ORB_SENTINEL).all())


@pytest.mark.parametrize("row", [1, 2, 4, 9, 10])
def test_extract_dev(ctx, row):
    """lorb_orb_extract_dev (device image, pattern, pyramid and outputs; d_n and d_level_off read
    after the stream is synchronised) equals the host form and the oracle bit for bit, writes
    nothing past n keypoints or past the pyramid bytes, and lorb_orb_extract_capacity returns the
    documented bound."""
    guard(row)
    c = case(row)
    cap, pb = W.orb_extract_capacity(*c["img"].shape, c["nd"], c["sf"])
    assert cap == sum(4 * max(int(N), 4) + 16 for N in c["nd"])
    assert pb == sum(p.size for p in c["pyr"])
    h = extract(ctx, row)
    d = extract(ctx, row, device_resident=True)
    assert d["capacity"] == cap and d["pyramid_bytes"] == pb
    assert d["n"] == len(h["x"]) == len(c["o"]["x"])
    assert_same(d, h, what="dev vs host")
    assert_same(d, c["o"], what="dev vs oracle")
    n = d["n"]
    for k in ("x", "y", "octave", "size", "angle", "response", "desc"):
        assert len(d["raw"][k]) == cap + W.ORB_GUARD and sentinel_intact(d["raw"][k], n), k
    assert sentinel_intact(d["raw"]["level_off"], len(c["sf"]) + 1) and sentinel_intact(d["raw"]["n"], 1)
    assert len(d["raw_pyramid"]) == pb + W.ORB_GUARD and sentinel_intact(d["raw_pyramid"], pb)
    assert np.array_equal(d["raw_pyramid"][:pb], np.concatenate([p.reshape(-1) for p in c["pyr"]]))


def check_extract_dev(ctx, row, what):
    c = case(row)
    d = extract(ctx, row, device_resident=True)
    assert d["n"] == len(c["o"]["x"]), what
    assert_same(d, c["o"], what=what)
    for k in ("x", "y", "octave", "size", "angle", "response", "desc"):
        assert sentinel_intact(d["raw"][k], d["n"]), (what, k)
    assert sentinel_intact(d["raw"]["level_off"], len(c["sf"]) + 1) and sentinel_intact(d["raw"]["n"], 1), what
    assert sentinel_intact(d["raw_pyramid"], d["pyramid_bytes"]), what


@pytest.mark.parametrize("row", [11, 9])
def test_extract_dev_around_frame_build(ctx, row):
    """A one-image call launches the stereo pair's kernels with the image grid dimension at extent 1
    and the second image's arguments zeroed.  lorb_orb_extract_dev twice on one context, with a
    FrameBuilder build of another geometry (120 x 160, 3 levels, both images) in between: both calls
    equal the oracle with every sentinel intact, and so does the pair."""
    guard(row)
    assert case(row)["img"].shape != (120, 160)
    check_extract_dev(ctx, row, "before the pair")
    left, right = synth.stereo_pair(500, 120, 160)
    sf, nd = synth.scale_factors(n_levels=3), O.orb_features_per_level(200)[:3]
    fb = FrameBuilder(ctx, dict(synth.frame_params(width=160, height=120), n_levels=3), 120, 160, nd, pattern())
    try:
        f = fb.build(left, right, device_resident=True)
    finally:
        fb.close()
    for side, img in (("left", left), ("right", right)):
        o = O.orb_extract(img, nd, sf, pattern())
        assert len(o["x"]) > 0
        assert_same(f[side], o, what=side)
    check_extract_dev(ctx, row, "after the pair")


@pytest.mark.parametrize("shape", [(333, 517), (300, 813)])
def test_extract_dev_pyramid(ctx, shape):
    """lorb_orb_pyramid_dev vs the oracle (the wrapper raises if a byte past the pyramid changed)."""
    img = make_image("scene", *shape, seed=300)
    o = O.orb_pyramid(img, synth.scale_factors())
    g = ctx.orb_pyramid(img, synth.scale_factors(), device_resident=True)
    assert len(g) == len(o) == 8
    for a, b in zip(g, o):
        assert a.shape == b.shape and np.array_equal(a, b)


def padded_view(img, pad, fill):
    big = np.full((img.shape[0], img.shape[1] + pad), fill, np.uint8)
    big[:, :img.shape[1]] = img
    v = big[:, :img.shape[1]]
    assert v.strides == (img.shape[1] + pad, 1) and not v.flags["C_CONTIGUOUS"]
    return v


@pytest.mark.parametrize("row", [1, 4])
def test_strides_image(ctx, row):
    """The image as a view into a wider buffer (row stride cols + 13, pad bytes 255, then 0): the
    host and device extractors and both pyramid entry points equal the contiguous result."""
    c = case(row)
    h = extract(ctx, row)
    assert_same(h, c["o"], what="contiguous")
    for fill in (255, 0):
        v = padded_view(c["img"], 13, fill)
        assert_same(extract(ctx, row, img=v), h, what=("host", fill))
        assert_same(extract(ctx, row, img=v, device_resident=True), h, what=("dev", fill))
        for dev in (False, True):
            for a, b in zip(ctx.orb_pyramid(v, c["sf"], device_resident=dev), c["pyr"]):
                assert a.shape == b.shape and np.array_equal(a, b), (fill, dev)


@functools.lru_cache(maxsize=None)
def describe_problem():
    pr = synth.orb_problem(seed=35, n_kps=1500, width=640, height=360)
    nd = O.orb_features_per_level(800)
    return dict(pr=pr, nd=nd, desc=O.orb_describe(pr["pyr"], pr["x"], pr["y"], pr["level"], pr["pattern"]),
                cells=O.orb_fast_cells(pr["pyr"]), det=O.orb_detect(pr["pyr"], nd, synth.scale_factors()))


def test_strides_pyramid(ctx):
    """A pyramid with padded rows (step = cols + 13, pad and inter-level gap 255, then 0) through
    orb_describe (host and device-resident), orb_fast_cells and orb_detect: equal to the unpadded
    result and to the oracle."""
    p = describe_problem()
    pr, sf = p["pr"], synth.scale_factors()
    args = (pr["pyr"], pr["x"], pr["y"], pr["level"], pr["pattern"])
    assert len(pr["pyr"]) == 8 and pr["pyr"][0].shape == (360, 640)
    for dev in (False, True):
        plain = ctx.orb_describe(*args, device_resident=dev)
        assert np.array_equal(plain[0], p["desc"][0]) and np.array_equal(plain[1], p["desc"][1])
        for fill in (255, 0):
            ang, desc = ctx.orb_describe(*args, device_resident=dev, row_pad=13, fill=fill)
            assert np.array_equal(ang, p["desc"][0]), (dev, fill)
            assert np.array_equal(desc, p["desc"][1]), (dev, fill)
    cell_keys = ("cell_base", "cell_off", "x", "y", "response")
    assert_same(ctx.orb_fast_cells(pr["pyr"]), p["cells"], cell_keys)
    assert_same(ctx.orb_detect(pr["pyr"], p["nd"], sf), p["det"], DETECT_KEYS)
    for fill in (255, 0):
        assert_same(ctx.orb_fast_cells(pr["pyr"], row_pad=13, fill=fill), p["cells"], cell_keys, fill)
        assert_same(ctx.orb_detect(pr["pyr"], p["nd"], sf, row_pad=13, fill=fill), p["det"], DETECT_KEYS, fill)


@functools.lru_cache(maxsize=None)
def stereo_case(which):
    """One of the two stereo problems with more right keypoints than k_st_rows keeps bands for, the
    oracle's result, and the best right index of every accepted left keypoint (frame.cpp:176-211)."""
    if which == "640x360":
        pr = synth.stereo_problem(seed=26, n_left=300, n_distract=8000, width=640, height=360)
    else:
        pr = synth.stereo_problem(seed=26, n_left=400, n_distract=8100)
    ur, dp, npair = O.compute_stereo_matches(pr["fp"], pr["left"], pr["right"], pr["pyr_l"], pr["pyr_r"])
    L, R, fp = pr["left"], pr["right"], pr["fp"]
    sf = np.asarray(fp["scale_factors"], np.float32)
    n_rows = pr["pyr_l"][0].shape[0]
    r = np.float32(2.0) * sf[R["octave"]]
    lo = np.maximum(np.floor(R["y"] - r).astype(np.int64), 0)
    hi = np.minimum(np.ceil(R["y"] + r).astype(np.int64), n_rows - 1)
    max_d = np.float32(fp["bf"]) / np.float32(fp["b"])
    bits = np.unpackbits(R["desc"], axis=1)
    best = []
    for i in np.flatnonzero(ur >= 0):
        v, u, lv = int(L["y"][i]), L["x"][i], int(L["octave"][i])
        m = (lo <= v) & (v <= hi) & (np.abs(R["octave"] - lv) <= 1) & (R["x"] >= np.float32(u - max_d)) & (R["x"] <= u)
        idx = np.flatnonzero(m)
        dist = (bits[idx] != np.unpackbits(L["desc"][i])).sum(axis=1)
        best.append(int(idx[np.argmin(dist)]))  # first minimum = the reference's strict <
    return dict(pr=pr, ur=ur, dp=dp, npair=npair, best=np.array(best))


def stereo_guard(s):
    assert len(s["pr"]["right"]["x"]) > 8192 and s["npair"] > 100
    # the recompute branch of k_st_rows decides accepted matches only if such right keypoints win
    assert (s["best"] >= 8192).any()


@pytest.mark.parametrize("row_pad", [0, 13])
@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("which", ["640x360", "752x480"])
def test_stereo_many_right_keys(ctx, which, dev, row_pad):
    """ComputeStereoMatches with more than 8192 right keypoints (bands past the LDS cache are
    recomputed), at 360 rows as well as 480, with padded pyramid rows, host and device-resident."""
    s = stereo_case(which)
    stereo_guard(s)
    pr = s["pr"]
    if which == "640x360":
        assert pr["pyr_l"][0].shape == (360, 640)
    ur, dp = ctx.compute_stereo_matches(pr["fp"], pr["left"], pr["right"], pr["pyr_l"], pr["pyr_r"],
                                        device_resident=dev, row_pad=row_pad)
    assert np.array_equal(ur, s["ur"]) and np.array_equal(dp, s["dp"])
    if row_pad:
        ur, dp = ctx.compute_stereo_matches(pr["fp"], pr["left"], pr["right"], pr["pyr_l"], pr["pyr_r"],
                                            device_resident=dev, row_pad=row_pad, fill=0)
        assert np.array_equal(ur, s["ur"]) and np.array_equal(dp, s["dp"])


def test_scratch_reuse(ctx):
    """One context, image sizes in an order that grows and shrinks every ORB scratch slot: blank,
    the largest, sparse, the smallest, the largest again, blank again -- with one stereo call (it
    shares the slots) in between.  Every result equals the oracle, so stale contents of a larger
    earlier call change nothing."""
    s = stereo_case("640x360")
    seen = {}
    for step, row in enumerate((10, 8, 9, 11, 8, 10)):
        guard(row)
        g = extract(ctx, row)
        assert_same(g, case(row)["o"], what=(step, row))
        if row in seen:
            assert_same(g, seen[row], what=("repeat", row))
        seen[row] = g
        if step == 2:
            pr = s["pr"]
            ur, dp = ctx.compute_stereo_matches(pr["fp"], pr["left"], pr["right"], pr["pyr_l"], pr["pyr_r"])
            assert np.array_equal(ur, s["ur"]) and np.array_equal(dp, s["dp"])


def test_shape_errors(ctx):
    """Geometries and capacities the device does not support are LorbErrors, never wrong keypoints,
    and the context stays usable: a valid call after each one is still correct."""
    pat = pattern()

    def still_fine():
        assert_same(extract(ctx, 11), case(11)["o"], what="after an error")

    def rejects(img, L, nf, **kw):
        with pytest.raises(LorbError):
            ctx.orb_extract(img, O.orb_features_per_level(nf)[:L], synth.scale_factors(n_levels=L), pat, **kw)
        still_fine()

    guard(11)
    wide = make_image("scene", 230, 824, 401)
    assert 5 in [n_ini_of(p.shape) for p in O.orb_pyramid(wide, synth.scale_factors())]
    rejects(wide, 8, 600)                                  # 5 initial nodes on one level
    rejects(wide, 8, 600, device_resident=True)
    assert n_ini_of((300, 120)) == 0
    rejects(make_image("scene", 300, 120, 402), 1, 100)    # 0 initial nodes
    assert int(np.float32(61 - 32) / np.float32(30)) == 0
    rejects(make_image("noise", 61, 62, 403), 1, 50)       # no 30-pixel cell row
    c = case(1)
    rejects(c["img"], 8, 1000, step=c["img"].shape[1] - 1)  # step < cols
    rejects(c["img"], 8, 1000, step=c["img"].shape[1] - 1, device_resident=True)
    with pytest.raises(LorbError):
        ctx.orb_pyramid(c["img"], c["sf"], step=c["img"].shape[1] - 1)
    with pytest.raises(LorbError):
        ctx.orb_pyramid(c["img"], c["sf"], step=c["img"].shape[1] - 1, device_resident=True)
    cap, pb = W.orb_extract_capacity(*c["img"].shape, c["nd"], c["sf"])
    rejects(c["img"], 8, 1000, device_resident=True, max_keypoints=cap - 1)
    rejects(c["img"], 8, 1000, device_resident=True, pyramid_bytes=pb - 1)
    d = extract(ctx, 1, device_resident=True, max_keypoints=cap, pyramid_bytes=pb)  # exactly the bound is enough
    assert_same(d, c["o"], what="at the bound")
