"""The windows of plan_edge_cases.py have the properties they claim (checked from obs_point and the slot
indices: run lengths, lane and workgroup positions of the named runs, word spans, group and run
counts, sortedness), and the oracle alone is well behaved on each of them under the options the
reference runs: test_gpu_plan_edges.py then compares the device on the same windows.  No GPU."""
import os
import re

import numpy as np
import pytest

import oracle as O
import plan_edge_cases as E

HAND_BUILT = ["run_lengths", "gaps", "gaps_mult64", "gaps_128", "maxk_255", "maxk_254", "maxk_128", "partial_runs", "idle_and_split"]


def _builder_constant(name):
    """a `constexpr int name = a * b;` of lorb_ba_build.hip, read from the source: the cases straddle the
    builder's thresholds as they are written there, and stop passing here when one moves"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lorb_slam_amd", "csrc", "lorb_ba_build.hip")
    with open(src) as f:
        m = re.search(r"constexpr int %s = ([0-9* ]+);" % name, f.read())
    assert m, name
    return int(np.prod([int(x) for x in m.group(1).split("*")]))


K_DB_WORDS = _builder_constant("kDbWords")
K_DB_FUSE_LDS = _builder_constant("kDbFuseLds")


def counts(w):
    return np.bincount(w["obs_point"], minlength=len(w["point_init"]))


@pytest.mark.parametrize("name", list(E.CASES))
def test_window_is_well_formed(name):
    w, _ = E.case(name)
    op, of = w["obs_point"], w["obs_frame"]
    C, F, P = len(w["pose_init"]), len(w["fixed_pose"]), len(w["point_init"])
    assert len(op) == len(of) == len(w["obs_uv"]) <= 4000
    assert np.all(np.diff(op) >= 0) and op.min() >= 0 and op.max() < P  # sorted by point
    assert of.min() >= -F and of.max() < C
    assert np.all(np.isfinite(w["obs_uv"]))
    key = op.astype(np.int64) * (C + F) + (of + F)
    assert len(np.unique(key)) == len(key)  # no frame twice in a point
    n_opt = np.bincount(op[of >= 0], minlength=P)
    n_fix = np.bincount(op[of < 0], minlength=P)
    seen = counts(w) > 0
    if name == "one_camera":
        assert C == 1 and np.all(n_opt[seen] == 1) and np.all(n_fix[seen] == 2)
    else:
        assert np.all(n_opt[seen] >= 2)
    if name in HAND_BUILT and not name.startswith("maxk"):
        assert np.all((n_fix >= 1) | (counts(w) == 2) | ~seen)  # but the two-observation point
    if not name.startswith("gaps"):
        assert seen.all()


def test_run_lengths_placements():
    w, named = E.case("run_lengths")
    assert (len(w["pose_init"]), len(w["fixed_pose"])) == (50, 40)
    s, n, _ = E.run_starts(w["obs_point"])
    for k in (2, 15, 16, 17, 18, 33, 63, 64, 65, 72, 90):
        assert k in n, k
    named_idx = set(named.values())
    rest = [int(n[i]) for i in range(len(n)) if i not in named_idx and n[i] not in E.SHORT1]
    assert min(rest) >= 3 and max(rest) <= 9 and set(rest) == set(range(3, 10))
    at = {k: (int(s[i]), int(n[i])) for k, i in named.items()}
    assert at == {k: (v[1], v[0]) for k, v in E.RUNS1.items()}
    tail = lambda a, m: a + m - (a - a % E.WAVE + E.WAVE)  # slots past the wave of the first slot
    a, m = at["lane0"]       # starts at lane 0; a whole wave and more
    assert a % E.WAVE == 0 and m > E.WAVE
    a, m = at["late"]        # starts in the last lanes, ends in the next wave
    assert a % E.WAVE >= 60 and (a + m - 1) // E.WAVE == a // E.WAVE + 1
    a, m = at["border"]      # crosses a workgroup border and covers a wave it does not start in
    assert a // E.BLOCK + 1 == (a + m - 1) // E.BLOCK
    k = a // E.WAVE + 1
    assert a < k * E.WAVE and (k + 1) * E.WAVE <= a + m
    for name, batches in (("tail64", 8), ("tail8", 1)):  # tails of whole 8-slot batches
        a, m = at[name]
        assert a % E.WAVE > 0 and tail(a, m) == 8 * batches
    a, m = at["wave"]        # one wave exactly
    assert a % E.WAVE == 0 and m == E.WAVE
    a, m = at["to_end"]      # from inside a wave to its end
    assert a % E.WAVE > 0 and tail(a, m) == 0
    # both forms of the 16-observation loops and of the segment sort (<= 16 in registers, insertion above)
    assert {15, 16, 17} <= set(int(x) for x in n)
    assert len(w["obs_point"]) > 7 * E.BLOCK  # several workgroups


@pytest.mark.parametrize("name", ["gaps", "gaps_mult64", "gaps_128"])
def test_gaps_runs_of_unobserved_points(name):
    w, meta = E.case(name)
    op = w["obs_point"]
    P = len(w["point_init"])
    s, n, p = E.run_starts(op)
    if name == "gaps_128":  # past the fused tables
        C = len(w["pose_init"])
        assert C == 128 and 4 * (C * C + C) > K_DB_FUSE_LDS
    else:  # case 1's observations, point for point
        w1, _ = E.case("run_lengths")
        assert np.array_equal(w["obs_frame"], w1["obs_frame"])
        s1, n1, p1 = E.run_starts(w1["obs_point"])
        assert np.array_equal(s, s1) and np.array_equal(n, n1)
    before = np.diff(np.r_[-1, p]) - 1  # unobserved points in front of each observed one
    assert before[0] == 5
    assert sorted(int(x) for x in before[before > 0]) == sorted(meta["gaps"].values())
    assert {5, 64, 300} <= set(meta["gaps"].values()) and len(meta["gaps"]) == 4
    assert P - 1 - p[-1] == 700
    assert (P % 64 == 0) == (name == "gaps_mult64")
    # the 300 sit in front of a run that starts inside a 256-slot block: that block's slots span more
    # than kDbWords point words, so its later points take the global-atomic bit path
    i = int(np.flatnonzero(before == 300)[0])
    a = int(s[i])
    assert a % E.BLOCK > 0
    b0 = a - a % E.BLOCK
    words = (op[min(b0 + E.BLOCK, len(op)) - 1] >> 6) - (op[b0] >> 6) + 1
    assert words > K_DB_WORDS
    assert (op[a] >> 6) - (op[b0] >> 6) >= K_DB_WORDS
    # the 64 skip exactly one point word
    j = int(np.flatnonzero(before == 64)[0])
    assert (p[j] >> 6) == (p[j - 1] >> 6) + 1 and (p[j] & 63) == ((p[j - 1] + 1) & 63)


def groups(w):
    """k_db_gather's point groups: group g = points [start(g), start(g + 1)), start(g) the first point p
    with off[p] + p >= g S; returns the points per group"""
    S, G, _, _ = E.layout(w)
    c = counts(w)
    off = np.r_[0, np.cumsum(c)][:-1]
    wgt = off + np.arange(len(c))
    start = np.searchsorted(wgt, np.arange(G + 1) * S, side="left")
    return np.diff(start), start


@pytest.mark.parametrize("n,S", [(255, 1), (254, 2), (128, 128)])
def test_maxk_group_bound(n, S):
    w, meta = E.case(f"maxk_{n}")
    assert (len(w["pose_init"]), len(w["fixed_pose"])) == (16, 239)
    c = counts(w)
    K, P = len(w["obs_point"]), len(w["point_init"])
    assert c.max() == n and np.sum(c == n) == 1 and P == 62
    s_, G, SF, NSG = E.layout(w)
    assert s_ == S and G == (K + P - 1) // S + 1
    per, start = groups(w)
    assert per.sum() == P and per.max() <= E.K_GB
    obs_per = np.add.reduceat(np.r_[c, 0], np.minimum(start[:-1], P)) * (per > 0)
    assert obs_per.max() <= E.K_GB and obs_per.max() >= n
    if S == 1:  # one point per group, the groups between them empty and inside the sequence
        assert per.max() == 1 and G == K + P and np.sum(per == 0) == K
        live = np.flatnonzero(per)
        assert np.any(per[live[0]:live[-1]] == 0)
        assert G > 512 and SF == 2 and NSG == (G + 1) // 2
    else:
        assert SF == 1 and NSG == G
    # the far point: fixed cameras and the two optimised cameras farthest apart
    s, m, p = E.run_starts(w["obs_point"])
    fr = w["obs_frame"][s[meta["far"]]:s[meta["far"]] + m[meta["far"]]]
    assert sorted(fr[fr >= 0]) == [0, 15] and np.sum(fr < 0) == 20


def test_partial_runs_counts():
    w, meta = E.case("partial_runs")
    assert (len(w["pose_init"]), len(w["fixed_pose"])) == (20, 230)
    c = counts(w)
    K, P = len(w["obs_point"]), len(w["point_init"])
    assert c.max() == 250 and c[meta["big"]] == 250 and K + P >= 3073
    S, G, SF, NSG = E.layout(w)
    assert S == 6 and G == (K + P - 1) // 6 + 1 and G > 512
    assert SF == (G + 479) // 480 == 2 and NSG == (G + 1) // 2
    per, _ = groups(w)
    assert per.sum() == P


@pytest.mark.parametrize("n_kf", [123, 124, 127])
def test_fuse_table_sizes(n_kf):
    """the camera counts against the builder's constants (read from its source) and db_phase1_issue's LDS
    formula, restated here: 8 kDbWords C bytes of bit words, then 4 (C^2 + C) of tables, fused while the
    tables fit kDbFuseLds.  A plan does not report which k_db_sorted instantiation ran, so "last fused /
    first unfused" rests on this reading of the code."""
    w, _ = E.case(f"fuse_{n_kf}")
    C = len(w["pose_init"])
    assert C == n_kf and len(w["fixed_pose"]) == 2 and len(w["point_init"]) == 600
    tables = 4 * (C * C + C)
    lds = 8 * K_DB_WORDS * C + tables
    assert tables <= K_DB_FUSE_LDS < 4 * (128 * 128 + 128)  # fused through 127 cameras, not at 128
    assert (lds <= 64 * 1024) == (n_kf == 123)              # the launch's dynamic LDS passes 64 KB at 124
    assert counts(w).max() <= 6


def test_idle_and_split_graph():
    w, meta = E.case("idle_and_split")
    op, of = w["obs_point"], w["obs_frame"]
    C = len(w["pose_init"])
    assert C == 12 and not np.any(of == meta["idle"])
    adj = np.eye(C, dtype=bool)
    for q in np.unique(op):
        f = of[(op == q) & (of >= 0)]
        adj[np.ix_(f, f)] = True
    reach = np.linalg.matrix_power(adj.astype(np.int64), C) > 0
    comps = {tuple(np.flatnonzero(r)) for r in reach}
    assert comps == {(0, 1, 2, 3, 4), (5,), (6, 7, 8, 9, 10, 11)}
    assert len(E.case("one_camera")[0]["pose_init"]) == 1


@pytest.mark.parametrize("name", list(E.DUPS))
def test_duplicate_positions(name):
    clean, dup = E.dup_case(name)
    a, i, j = E.DUPS[name]
    s, n, _ = E.run_starts(clean["obs_point"])
    assert 72 in n and a in s and n[list(s).index(a)] == 72
    assert np.sum(clean["obs_frame"] != dup["obs_frame"]) == 1
    f = dup["obs_frame"]
    assert f[a + i] == f[a + j] >= 0 and clean["obs_frame"][a + j] < 0
    si, sj = a + i, a + j
    if name == "beyond_16":
        assert min(i, j) >= 16 and si // E.WAVE == sj // E.WAVE
    elif name == "two_waves":
        assert si // E.WAVE != sj // E.WAVE and si // E.BLOCK == sj // E.BLOCK
    else:
        assert si // E.BLOCK != sj // E.BLOCK


def test_limit_windows():
    good, bad = E.device_limit()
    assert len(good["fixed_pose"]) == len(bad["fixed_pose"]) == 206 and len(bad["pose_init"]) == 50
    assert counts(bad).max() == 256 and counts(good).max() == 90
    assert np.array_equal(good["obs_frame"], E.case("run_lengths")[0]["obs_frame"])
    for n in (256, 257):
        w, at = E.host_limit(n)
        assert counts(w).max() == n == counts(w)[at] and len(w["pose_init"]) == 128
    w, at = E.host_span_127()
    s, m, _ = E.run_starts(w["obs_point"])
    assert sorted(w["obs_frame"][s[at]:s[at] + m[at]]) == [-1, 0, 127]


def well_behaved(w):
    """Ceres-default options: the oracle stops on the function tolerance within 10 iterations, with at
    least 2 accepted steps and no invalid step"""
    _, _, so, ot = O.ba_local_traced(w)
    assert so["termination"] == "FUNCTION_TOLERANCE" and so["iterations"] <= 10, so
    assert so["successful_steps"] >= 2, so
    assert all(t["outcome"] != "invalid" for t in ot), ot


@pytest.mark.parametrize("name", list(E.CASES))
def test_oracle_is_well_behaved(name):
    well_behaved(E.case(name)[0])


@pytest.mark.parametrize("name", ["dup_beyond_16", "dup_two_waves", "dup_two_blocks", "host_256", "host_span_127",
                                  "device_limit_good"])
def test_oracle_is_well_behaved_on_the_limit_windows(name):
    if name.startswith("dup_"):
        w = E.dup_case(name[4:])[0]
    else:
        w = {"host_256": lambda: E.host_limit(256)[0], "host_span_127": lambda: E.host_span_127()[0],
             "device_limit_good": lambda: E.device_limit()[0]}[name]()
    well_behaved(w)
