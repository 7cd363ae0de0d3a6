"""GPU parity on the hand-built windowed-matcher cases (tests/window_cases.py): assignments and counts
bit-exact against the oracle, through the host-array calls, the device-pointer a4 and (path shapes)
the fused local-map chain.  test_oracle_window_cases.py pins the oracle on the same cases."""
import functools

import numpy as np
import pytest

import oracle as O
import lorb_slam_amd.window  # noqa: F401  (binds Context methods)
import window_cases as W

pytestmark = pytest.mark.gpu

ALL = sorted(W.SEMANTIC) + sorted(W.PATH)
A4 = [n for n in sorted(W.SEMANTIC) if W.get(n)["kind"] == "a4"] + [n for n in sorted(W.PATH) if n.startswith("a4_")]


@functools.lru_cache(maxsize=None)
def reference(name):
    case = W.get(name)
    fn = O.search_by_projection_frame if case["kind"] == "a4" else O.search_by_projection_local
    a, n = fn(*case["args"])
    a.setflags(write=False)
    return a, n


def check(name, got):
    a, n = reference(name)
    assert got[1] == n
    assert np.array_equal(got[0], a), np.nonzero(got[0] != a)[0][:10]
    exp = W.get(name)["expect"]
    if exp is not None:
        assert got[1] == exp[1] and np.array_equal(got[0], exp[0])


def run_host(ctx, name):
    case = W.get(name)
    fn = ctx.search_by_projection_frame if case["kind"] == "a4" else ctx.search_by_projection_local
    return fn(*case["args"])


@pytest.mark.parametrize("name", ALL)
def test_host_call(ctx, name):
    check(name, run_host(ctx, name))


@pytest.mark.parametrize("name", A4)
def test_frame_dev(ctx, name):
    """lorb_search_by_projection_frame_dev on the a4 cases (a case without a slot array runs on the
    call's own all-EMPTY buffer)"""
    check(name, ctx.search_by_projection_frame_dev(*W.get(name)["args"]))


@pytest.mark.parametrize("name", sorted(W.PATH_SHAPES))
def test_track_local_map_shapes(ctx, name):
    """The fused frustum + candidate kernel (k_cand_local_fr) at every path shape."""
    pr = W.path_local_map(name)
    g = ctx.track_local_map(pr["fp"], pr["Tcw"], pr["kps"], pr["slot_state"], pr["pts"], 0.5, 1.0)
    fr, assign, nm = O.track_local_map(pr["fp"], pr["Tcw"], pr["kps"], pr["slot_state"], pr["pts"], 0.5, 1.0)
    assert np.array_equal(g["in_view"], fr["in_view"])
    m = fr["in_view"].astype(bool)
    assert m.sum() > 20
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos", "pred_level"):
        assert np.array_equal(g[k][m], fr[k][m]), k
    assert g["nmatches"] == nm and nm > 5
    assert np.array_equal(g["assign"], assign)


@pytest.mark.parametrize("first,between", [("a4_stage_at", "a5_resolve_mode1"), ("chain_a5_200", "a4_strided_over"),
                                           ("levels_a4_forward", "a4_grid_global"), ("a5_grid_global", "tie_first_wins")])
def test_repeat_around_another_shape(ctx, first, between):
    """The same case before and after a differently shaped one in one context: the scratch slots are
    regrown and reused, the grid and the all-EMPTY slot buffer are rebuilt, and the answer stays."""
    check(first, run_host(ctx, first))
    check(between, run_host(ctx, between))
    check(first, run_host(ctx, first))
    if W.get(first)["kind"] == "a4":
        check(first, ctx.search_by_projection_frame_dev(*W.get(first)["args"]))
        if W.get(between)["kind"] == "a4":
            check(between, ctx.search_by_projection_frame_dev(*W.get(between)["args"]))
        check(first, ctx.search_by_projection_frame_dev(*W.get(first)["args"]))
