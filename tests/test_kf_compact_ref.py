"""CPU: the restatement of lorb_kf_store_compact_dev (tests/kf_compact_ref.py) against hand-written stores of a dozen
points -- each of the four keep-conditions alone keeping a point, a culled point going, the first and the last point,
all points gone, none gone, the status-1 paths -- and its two forms (the store dict, the device's arrays over their
whole capacity) against each other."""
import numpy as np
import pytest

import kf_compact_ref as M
import kf_store_cases as KC
import kf_store_ref as R

SENT = 0xAB


def hand():
    """Three keyframes, twelve points:
         p0   bad, unobserved, held by nobody           -> goes (the first point)
         p1   alive, seen by kf0                        -> 0
         p2   bad, still observed by kf0 (its slot there is empty: the observation ALONE keeps it)   -> 1
         p3   bad, unobserved, in kf1's row (the slot ALONE keeps it)                                -> 2
         p4   bad, unobserved, in the table (the table ALONE keeps it)                               -> 3
         p5   not bad, unobserved, held by nobody (not being bad ALONE keeps it)                     -> 4
         p6   culled: bad, unobserved, named only by a table entry PAST the count                    -> goes
         p7   alive, seen by kf0 and kf1                -> 5
         p8   culled                                    -> goes
         p9   alive, seen by kf1                        -> 6
         p10  alive, seen by kf2                        -> 7
         p11  culled                                    -> goes (the last point)
       The table holds p4, p7 twice, a -1, an index outside the store, and p6 past its count."""
    obs = [[], [0], [0], [], [], [], [], [0, 1], [], [1], [2], []]
    obs_slot = [[], [0], [1], [], [], [], [], [2, 0], [], [1], [0], []]
    rows = [[1, -1, 7], [7, 9, 3], [10]]
    bad = [1, 0, 1, 1, 1, 0, 1, 0, 1, 0, 0, 1]
    s = KC.make_store(obs, [0, 0, 0], rows, [[], [], []], [{}, {}, {}], is_bad=bad, seed=90)
    life = dict(visible=np.arange(1, 13, dtype=np.int32), found=np.arange(21, 33, dtype=np.int32),
                first_fid=np.arange(41, 53, dtype=np.int32), recent=np.array([0, 1] * 6, np.uint8), kf_fid=np.array([3, 5, 8], np.int32),
                frame_word=9)
    table = dict(gid=np.array([4, 7, -1, 99, 7, 6], np.int32), n_max=6, count=5)
    return s, obs_slot, life, [table]


MAP = [-1, 0, 1, 2, 3, 4, -1, 5, -1, 6, 7, -1]
KEPT = [1, 2, 3, 4, 5, 7, 9, 10]


def test_hand_store():
    s, slot, life, tables = hand()
    r = M.compact_store(s, slot, life, tables)
    assert list(r["map"]) == MAP and r["dropped"] == [0, 6, 8, 11]
    assert r["rec"] == dict(status=0, n_points_before=12, n_dropped=4, n_points=8, n_bad_kept=3, n_kf_slots_mapped=6, n_gids_mapped=3)
    t = r["store"]
    assert t["n_points"] == 8 and t["kf_slots"] == [[0, -1, 5], [5, 6, 2], [7]]
    assert t["obs"] == [[0], [0], [], [], [], [0, 1], [1], [2]] and r["obs_slot"] == [[0], [1], [], [], [], [2, 0], [1], [0]]
    for k in R.COLS:
        assert np.array_equal(t[k], s[k][KEPT]), k
    for k in M.LIFE_ROWS:
        assert np.array_equal(r["life"][k], life[k][KEPT]), k
    assert np.array_equal(r["life"]["kf_fid"], life["kf_fid"]) and r["life"]["frame_word"] == 9
    assert list(r["tables"][0]["gid"]) == [3, 5, -1, 99, 5, 6]   # p7 twice; -1, 99 and the entry past the count stay
    for k in ("kf_bad", "cov", "conn"):
        assert np.array_equal(t[k], s[k]) if k == "kf_bad" else t[k] == s[k]
    # the invariant for the new indices
    for p, (o, sl) in enumerate(zip(t["obs"], r["obs_slot"])):
        for f, j in zip(o, sl):
            assert t["kf_slots"][f][j] in (p, -1)
    # the inputs are not touched
    s2, slot2, life2, tables2 = hand()
    assert s["kf_slots"] == s2["kf_slots"] and np.array_equal(tables[0]["gid"], tables2[0]["gid"]) and s["n_points"] == 12


@pytest.mark.parametrize("which, point", [("observation", 2), ("slot", 3), ("table", 4), ("not_bad", 5)])
def test_each_condition_alone_keeps_a_point(which, point):
    """Take the one hold away and the point goes; with it, it stays."""
    s, slot, life, tables = hand()
    assert M.compact_store(s, slot, life, tables)["map"][point] >= 0
    if which == "observation":
        s["obs"][2], slot[2] = [], []
    elif which == "slot":
        s["kf_slots"][1][2] = -1
    elif which == "table":
        tables[0]["count"] = 0
    else:
        s["is_bad"][5] = 1
    r = M.compact_store(s, slot, life, tables)
    assert r["map"][point] == -1 and r["rec"]["n_dropped"] == 5
    assert r["rec"]["n_bad_kept"] == (3 if which == "not_bad" else 2)


def test_a_table_entry_past_the_count_holds_nothing():
    s, slot, life, tables = hand()
    tables[0]["count"] = 6                                  # now p6 is named by an examined entry
    r = M.compact_store(s, slot, life, tables)
    assert r["map"][6] == 5 and r["rec"]["n_dropped"] == 3 and r["rec"]["n_bad_kept"] == 4
    assert list(r["tables"][0]["gid"]) == [3, 6, -1, 99, 6, 5]


def test_all_points_gone():
    s, slot, life, tables = hand()
    s["is_bad"][:] = 1
    s["obs"], slot = [[] for _ in range(12)], [[] for _ in range(12)]
    s["kf_slots"] = [[-1, -1, -1], [-1, -1, -1], [-1]]
    r = M.compact_store(s, slot, life, [])
    assert r["rec"] == dict(status=0, n_points_before=12, n_dropped=12, n_points=0, n_bad_kept=0, n_kf_slots_mapped=0, n_gids_mapped=0)
    assert list(r["map"]) == [-1] * 12 and r["store"]["n_points"] == 0 and r["store"]["obs"] == []
    assert all(len(r["store"][k]) == 0 for k in R.COLS) and all(len(r["life"][k]) == 0 for k in M.LIFE_ROWS)


def test_none_gone_changes_nothing():
    s, slot, life, tables = hand()
    for p in (0, 6, 8, 11):
        s["is_bad"][p] = 0
    r = M.compact_store(s, slot, life, tables)
    assert r["rec"] == dict(status=0, n_points_before=12, n_dropped=0, n_points=12, n_bad_kept=3, n_kf_slots_mapped=0, n_gids_mapped=0)
    assert list(r["map"]) == list(range(12)) and r["store"]["kf_slots"] == s["kf_slots"]
    assert np.array_equal(r["tables"][0]["gid"], tables[0]["gid"])
    for k in R.COLS:
        assert np.array_equal(r["store"][k], s[k]), k


@pytest.mark.parametrize("fail", ["src_status", "count_negative", "count_above"])
def test_status_1(fail):
    s, slot, life, tables = hand()
    src = 0
    if fail == "src_status":
        src = 3
    else:
        tables[0]["count"] = -1 if fail == "count_negative" else 7
    r = M.compact_store(s, slot, life, tables, src_status=src)
    assert r["rec"] == dict(status=1) and r["map"] is None and r["store"]["n_points"] == 12
    assert r["store"]["kf_slots"] == s["kf_slots"] and np.array_equal(r["tables"][0]["gid"], tables[0]["gid"])


def to_arrays(s, slot, life, slack=3, extra=0):
    """The store as the device keeps it: every array `slack` rows larger than its count, SENT bytes behind the counts
    (is_bad holds 1 there); `extra` more rows in the per-point arrays."""
    P, cn = s["n_points"], R.counts(s)

    def pad(a, n, fill=SENT):
        a = np.asarray(a)
        out = np.empty((n,) + a.shape[1:], a.dtype)
        out.view(np.uint8)[...] = fill
        out[:len(a)] = a
        return out

    a = {k: pad(s[k], P + slack + extra, 1 if k == "is_bad" else SENT) for k in R.COLS}
    off = np.cumsum([0] + [len(o) for o in s["obs"]]).astype(np.int32)
    a["obs_off"] = pad(off, P + slack + extra + 1)
    a["obs_kf"] = pad(np.asarray([f for o in s["obs"] for f in o], np.int32), cn["n_obs"] + slack)
    a["obs_slot"] = pad(np.asarray([j for o in slot for j in o], np.int32), cn["n_obs"] + slack)
    a["kf_slot_point"] = pad(np.asarray([g for r in s["kf_slots"] for g in r], np.int32), cn["n_kf_slots"] + slack)
    for k in M.LIFE_ROWS:
        a["life_" + k] = pad(life[k], P + slack + extra)
    return a, dict(n_points=P, n_obs=cn["n_obs"], n_kf_slots=cn["n_kf_slots"])


@pytest.mark.parametrize("case", ["hand", "all_gone", "none_gone", "refused"])
def test_the_two_forms_agree(case):
    s, slot, life, tables = hand()
    src = 0
    if case == "all_gone":
        s["is_bad"][:] = 1
        s["obs"], slot = [[] for _ in range(12)], [[] for _ in range(12)]
        s["kf_slots"], tables = [[-1, -1, -1], [-1, -1, -1], [-1]], []
    elif case == "none_gone":
        s["is_bad"][:] = 0
    elif case == "refused":
        src = 1
    a, cn = to_arrays(s, slot, life)
    d_map = np.full(15, -9, np.int32)
    r = M.compact_store(s, slot, life, tables, src_status=src)
    q = M.compact_arrays(a, cn, tables, src_status=src, d_map=d_map)
    assert q["rec"] == r["rec"]
    if case == "refused":
        assert all(np.array_equal(q["arrays"][k], a[k]) for k in a) and (q["d_map"] == -9).all()
        return
    assert list(q["d_map"][:12]) == list(r["map"]) and (q["d_map"][12:] == -9).all()
    want, _ = to_arrays(r["store"], r["obs_slot"], r["life"], extra=r["rec"]["n_dropped"])
    n, P = r["rec"]["n_points"], 12
    for k in a:
        got, w = q["arrays"][k], want[k]
        if k in ("obs_kf", "obs_slot", "kf_slot_point"):
            assert np.array_equal(got, w), k                          # the lists do not move; the slots are mapped
            continue
        rows = n + 1 if k == "obs_off" else n
        old = P + 1 if k == "obs_off" else P
        assert np.array_equal(got[:rows], w[:rows]), k
        assert np.array_equal(got[old:], a[k][old:]), k               # nothing at or past the old count is written
        if r["rec"]["n_dropped"]:                                     # a fresh store's state in between
            assert (got[rows:old] == (1 if k == "is_bad" else 0)).all(), k
        else:
            assert np.array_equal(got, a[k]), k
    for t, u in zip(q["tables"], r["tables"]):
        assert np.array_equal(t["gid"], u["gid"])
