"""GPU: the absolute launch counts of the LM solve, for a plan and for a fused plan group.

The launch order is stated once (enqueue_solve in lorb_ba.hip) and issued on a plan or on a group, so
both hold the same kernel nodes.  For an unsharded plan on the two-sided Cholesky with point groups and
block pairs, derived from that sequence:
  no iterations          k_ba_init, k_ba_ls, k_ba_red<0>, k_ba_lm_begin                        4
  the first iteration    k_ba_ls, k_ba_red<0>, k_ba_lm_begin, k_ba_red<1>, Cholesky, k_ba_bs2,
                         k_ba_lm_end                                                           7
  a later (fused) one    k_ba_ls, k_ba_red<2>, Cholesky with head, k_ba_bs2, k_ba_lm_end       5
so 1 + 7 + 5 (n - 1) for n >= 1, and a folding solve drops k_ba_lm_end from every iteration but the
last: n - 1 fewer.  The counts depend neither on the windows of a plan nor on the members of a group.
The windows are test_gpu_lm_fold's, the smallest that reach the two-sided Cholesky."""
import ctypes as C

import pytest

from lorb_slam_amd import _abi as A
from test_gpu_lm_fold import base, identical, solve, three, tol0  # noqa: F401  (base, three: fixtures)

pytestmark = pytest.mark.gpu


# kernel nodes of a solve of max_num_iterations n: {n: (folded, LORB_NO_FOLD=1)}
NODES = {0: (4, 4), 1: (8, 8), 2: (12, 13), 3: (16, 18), 10: (44, 53), 50: (204, 253)}


def expected_nodes(n, fold):
    return NODES[n][0 if fold else 1]


def solve_group(ctx, wins, opt, monkeypatch, fold):
    """a group of one-window plans of `wins`, solved like test_gpu_lm_fold.solve: per member poses,
    points, summary and trace, the Cholesky kind, the kernel launches of the group's graph"""
    from lorb_slam_amd.runtime import BAGroup, BAPlan, lib
    gp = [BAPlan(ctx, [w]) for w in wins]
    G = BAGroup(ctx, gp)
    try:
        with monkeypatch.context() as m:
            if fold:
                m.delenv("LORB_NO_FOLD", raising=False)
            else:
                m.setenv("LORB_NO_FOLD", "1")
            G.solve(opt)
        rd = [p.read() for p in gp]
        v = (C.c_int32 * 4)()
        ctx.check(lib().lorb_ba_group_info(G._p, v, C.c_int32(4)), "lorb_ba_group_info")
        assert v[1] == 1, list(v)  # fused_solves: one set of launches
        kinds = {p.info()["cholesky"] for p in gp}
        assert len(kinds) == 1, kinds
        return ([r[0][0] for r in rd], [r[1][0] for r in rd], [r[2][0] for r in rd], [p.trace(0) for p in gp],
                kinds.pop(), int(v[3]))
    finally:
        G.close()
        for p in gp:
            p.close()


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 10])
def test_plan_and_group_of_one(ctx, base, monkeypatch, n, fold):
    opt = tol0(max_num_iterations=n)
    a = solve(ctx, [base], opt, monkeypatch, fold)
    b = solve_group(ctx, [base], opt, monkeypatch, fold)
    print(f"n={n} fold={fold}: plan nodes {a[5]}, group nodes {b[5]}, expected {expected_nodes(n, fold)}")
    if n > 0:
        assert a[4] == 2 and b[4] == 2, (a[4], b[4])
    assert a[5] == expected_nodes(n, fold), (n, fold, a[5])
    assert b[5] == a[5], (n, fold, a[5], b[5])
    identical(a, b, f"plan vs group, n={n}")


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_three_windows_default_options(ctx, three, monkeypatch, fold):
    """neither the members of a group nor the windows of a plan change the number of launches"""
    opt = A.LMOptions.default()
    assert opt.max_num_iterations == 50
    g = solve_group(ctx, three, opt, monkeypatch, fold)
    p = solve(ctx, three, opt, monkeypatch, fold)
    print(f"fold={fold}: group nodes {g[5]}, plan nodes {p[5]}, expected {expected_nodes(50, fold)}")
    assert g[4] == 2 and p[4] == 2
    assert g[5] == expected_nodes(50, fold) and p[5] == expected_nodes(50, fold), (fold, g[5], p[5])
    identical(p, g, "three windows: plan vs group")
