"""CPU: the restatement of lorb_kf_store_retire_dev (tests/kf_retire_ref.py) against answers worked out by hand from
Frame::SetBadFlag (src/frame.cpp:684-714), Frame::EraseConnection (:791-798, :754-774) and MapPoint::EraseObservation
(src/map_point.cpp:141-153, :184-199) on hand-written stores, and the order independence the header claims: the same
keyframes in another order of the list leave the same store."""
import itertools

import numpy as np

import kf_ba_ref as B
import kf_retire_cases as RC
import kf_retire_ref as T
import kf_store_ref as R


def run(c, **kw):
    a = dict(lst=c["list"], protect=c["protect"])
    a.update(kw)
    return T.retire(c["store"], c["obs_slot"], c["life"], **a)


def same_out(a, b):
    """Two results leave the same store bytes and the same record."""
    sa, sb = a["store"], b["store"]
    for k in R.COLS + ("kf_bad",):
        assert np.array_equal(sa[k], sb[k]), k
    for k in ("obs", "kf_slots", "cov", "conn"):
        assert sa[k] == sb[k], k
    assert a["obs_slot"] == b["obs_slot"] and a["rec"] == b["rec"] and sorted(a["dead"]) == sorted(b["dead"])


def rec_of(out, **want):
    for k, v in want.items():
        assert out["rec"][k] == v, (k, out["rec"][k], v)


def test_a_point_at_4_3_2_observations_losing_one():
    """p0 {0,1,2,3} -> {1,2,3} stays, its first observer is now 1; p1 {0,1,2} -> 2 left: dies, its slots in kf1 and
    kf2 become -1; p2 {0,1} -> 1 left: dies; p3 {1,2,3} does not observe kf0: untouched."""
    c = RC.build(4, [[0, 1, 2, 3], [0, 1, 2], [0, 1], [1, 2, 3]], lst=[0])
    assert c["store"]["kf_slots"] == [[0, 1, 2], [0, 1, 2, 3], [0, 1, 3], [0, 3]]
    out = run(c)
    s = out["store"]
    assert s["obs"] == [[1, 2, 3], [], [], [1, 2, 3]] and out["obs_slot"] == [[0, 0, 0], [], [], [3, 2, 1]]
    assert list(s["is_bad"]) == [0, 1, 1, 0] and list(s["kf_bad"]) == [1, 0, 0, 0]
    assert s["kf_slots"] == [[-1, -1, -1], [0, -1, -1, 3], [0, -1, 3], [0, 3]]
    assert s["obs"][0][0] == 1                                        # mpRefKF = mObservations.begin()->first
    rec_of(out, status=0, n_retired=1, n_obs_erased=1, n_points_bad=2, n_obs_removed=1 + 3 + 2, n_slots_erased=3, n_obs_bad_slot=0,
           n_obs=6, n_conn_erased=0, n_rows_reordered=0)
    for k in ("pos", "normal", "max_dist", "min_dist", "desc", "locked"):   # the rows of the dead points stay
        assert np.array_equal(s[k], c["store"][k]), k
    B.check_invariant(s, dict(c["geom"], obs_slot=out["obs_slot"]))


def test_a_point_losing_two_in_one_call_in_both_orders():
    """p0 {0,1,2,3,4} loses 0 and 1: 3 left, stays.  p1 {0,1,2,3} loses both: 2 left, dies -- in the order [0, 1] at
    the second erasure, in the order [1, 0] likewise; p2 {0,1,2}: dies at the FIRST erasure with the other retired
    keyframe still in its list.  The store and the record are the same."""
    c = RC.build(5, [[0, 1, 2, 3, 4], [0, 1, 2, 3], [0, 1, 2]], lst=[0, 1])
    a, b = run(c), run(c, lst=[1, 0])
    same_out(a, b)
    assert a["store"]["obs"] == [[2, 3, 4], [], []] and list(a["store"]["is_bad"]) == [0, 1, 1]
    assert a["store"]["kf_slots"] == [[-1, -1, -1], [-1, -1, -1], [0, -1, -1], [0, -1], [0]]
    # slots of keyframes outside V: p1 in kf2 and kf3, p2 in kf2
    rec_of(a, n_retired=2, n_obs_erased=2, n_points_bad=2, n_obs_removed=2 + 4 + 3, n_slots_erased=3, n_obs=3)


def test_a_point_held_in_two_slots_of_the_retired_keyframe():
    """kf0's row holds p0 in slots 0 and 2; the observation names the lowest.  One entry leaves, once."""
    c = RC.build(4, [[0, 1, 2, 3], [0, 1, 2, 3]], rows=[[0, 1, 0], [0, 1], [0, 1], [0, 1]], lst=[0])
    assert c["obs_slot"][0] == [0, 0, 0, 0]
    out = run(c)
    assert out["store"]["obs"] == [[1, 2, 3], [1, 2, 3]] and out["store"]["kf_slots"][0] == [-1, -1, -1]
    rec_of(out, n_obs_erased=2, n_obs_removed=2, n_points_bad=0)


def test_a_bad_point_that_still_carries_observations():
    """Bad or not, the lists are maintained: p0 (bad) {0,1,2,3} -> {1,2,3}; p1 (bad) {0,1,2} runs the cascade again."""
    c = RC.build(4, [[0, 1, 2, 3], [0, 1, 2]], is_bad=[1, 1], lst=[0])
    out = run(c)
    assert out["store"]["obs"] == [[1, 2, 3], []] and list(out["store"]["is_bad"]) == [1, 1]
    assert out["store"]["kf_slots"] == [[-1, -1], [0, -1], [0, -1], [0]]
    rec_of(out, n_points_bad=1, n_obs_erased=1, n_obs_removed=4, n_slots_erased=2)


def test_connections_follow_the_retired_keyframes_map():
    """kf0's map names 1; kf1 names 0 back and loses it.  kf2 names 0 while kf0 does not name 2: the entry stays
    (the reference iterates f's map).  kf1's ordered list held the pair 0 only; rebuilt from ALL of its map it now
    lists 3 (weight 1) and 4 (weight 2), entries below 3 included."""
    conn = [{1: 4}, {0: 4, 3: 1, 4: 2}, {0: 5}, {}, {}]
    c = RC.build(5, [[0, 1, 2, 3]], conn=conn, lst=[0])
    assert c["store"]["cov"] == [[1], [0], [0], [], []]
    out = run(c)
    s = out["store"]
    assert s["conn"] == [{}, {3: 1, 4: 2}, {0: 5}, {}, {}] and s["cov"] == [[], [3, 4], [0], [], []]
    rec_of(out, n_conn_erased=1, n_rows_reordered=1, n_cov=3, n_conn=3)


def test_two_retired_keyframes_connected_to_each_other():
    """0 and 1 name each other and both name 2, which names them back and one more: kf2 loses two keys and is counted
    as one re-sorted row; what 0 and 1 erase from each other is counted nowhere."""
    conn = [{1: 3, 2: 3}, {0: 3, 2: 4}, {0: 3, 1: 4, 3: 1}, {}]
    c = RC.build(4, [[0, 1, 2, 3]], conn=conn, lst=[0, 1])
    a, b = run(c), run(c, lst=[1, 0])
    same_out(a, b)
    assert a["store"]["conn"] == [{}, {}, {3: 1}, {}] and a["store"]["cov"] == [[], [], [3], []]
    rec_of(a, n_retired=2, n_conn_erased=2, n_rows_reordered=1, n_cov=1, n_conn=1)


def test_every_skip_class_and_their_precedence():
    """Six keyframes: kf1 is bad, kf0 and kf5 have kf_fid 0, the protected words name 3, 1 (bad as well: bad wins) and
    5 (kf_fid 0 as well: that wins).  The list: 9 and -1 are outside; the second 2 is a duplicate; the second 1 is bad
    AND a duplicate (duplicate wins); the second 0 likewise; 4 and 2 are retired."""
    c = RC.build(6, [[0, 1, 2, 3, 4, 5]], kf_bad=[0, 1, 0, 0, 0, 0], kf_fid=[0, 7, 8, 9, 10, 0],
                 lst=[9, 2, 2, 1, 1, 0, 3, 0, -1, 4, 5], protect=[3, 1, 5])
    out = run(c)
    assert out["V"] == [2, 4]
    rec_of(out, status=0, n_skip_range=2, n_skip_dup=3, n_skip_bad=1, n_skip_first=2, n_skip_protected=1, n_retired=2)
    assert list(out["store"]["kf_bad"]) == [0, 1, 1, 0, 1, 0] and out["store"]["obs"] == [[0, 1, 3, 5]]
    # only the entries in use are read
    rec_of(run(c, n_list=2, n_max_list=11), n_skip_range=1, n_retired=1, n_skip_dup=0)


def test_a_fresh_store_retires_nothing():
    """kf_fid = 0 everywhere, as create leaves it: the reference's if(mnId == 0) return; keeps every keyframe."""
    c = RC.build(3, [[0, 1, 2]], kf_fid=[0, 0, 0], lst=[0, 1, 2])
    out = run(c)
    rec_of(out, status=0, n_skip_first=3, n_retired=0, n_obs=3)
    same_out(dict(out, rec=None), dict(run(dict(c, list=[])), rec=None))


def test_a_damaged_obs_slot():
    """p0 {0,1,2} dies; its observation in kf1 names slot 5 (outside the row), the one in kf2 a slot that holds p1:
    both are counted and skipped, the rows keep p0.  The verdict came from the lists alone."""
    c = RC.build(3, [[0, 1, 2], [1, 2]], lst=[0])
    assert c["store"]["kf_slots"] == [[0], [0, 1], [0, 1]]
    c["obs_slot"][0] = [0, 5, 1]
    out = run(c)
    assert out["store"]["obs"] == [[], [1, 2]] and out["store"]["kf_slots"] == [[-1], [0, 1], [0, 1]]
    rec_of(out, n_points_bad=1, n_slots_erased=0, n_obs_bad_slot=2, n_obs_removed=3)
    # a list that names kf0 while kf0's row does not hold the point: the lists decide
    c = RC.build(3, [[0, 1, 2], [1, 2]], lst=[0])
    c["store"]["kf_slots"][0] = [-1]
    c["obs_slot"][0] = [0, 0, 0]
    out = run(c)
    assert out["store"]["obs"][0] == [] and out["store"]["is_bad"][0] == 1


def test_an_empty_set_changes_nothing():
    c = RC.build(3, [[0, 1, 2]], conn=[{1: 3}, {0: 3}, {}], kf_bad=[1, 0, 0], lst=[0, 7], protect=[1])
    out = run(dict(c, list=[0, 7, 1]))
    rec_of(out, status=0, n_skip_range=1, n_skip_bad=1, n_skip_protected=1, n_retired=0, n_obs=3, n_cov=2, n_conn=2)
    same_out(dict(out, rec=None, dead=[]), dict(store=c["store"], obs_slot=c["obs_slot"], rec=None, dead=[]))


def test_status_1():
    c = RC.build(3, [[0, 1, 2]], lst=[1])
    for kw in (dict(src_status=2), dict(n_list=-1), dict(n_list=2, n_max_list=1),
               dict(caps=dict(max_kf=2, max_points=9, max_obs=9, max_kf_slots=9))):
        out = run(c, **kw)
        assert out["rec"] == dict(status=1) and out["store"]["obs"] == c["store"]["obs"]


def test_order_independence_on_generated_stores():
    """Every order of three retired keyframes, and the generated cases with their lists reversed."""
    c = RC.generated(300, 7, seed=5, lst=[1, 3, 6], affected=range(0, 300, 7))
    first = run(c)
    assert first["rec"]["n_points_bad"] > 0 and first["rec"]["n_obs_erased"] > 0 and first["rec"]["n_conn_erased"] > 0
    for order in itertools.permutations([1, 3, 6]):
        same_out(first, run(c, lst=list(order)))
    for name in ("points_1023", "every_point_dies", "weight_row_1025"):
        c = RC.cases()[name]
        same_out(run(c), run(c, lst=c["list"][::-1]))


def test_the_cases_are_what_their_names_say():
    cs = RC.cases()
    r = {k: run(c) for k, c in cs.items()}
    for n in (1023, 1024, 1025):
        dead, rec = set(r[f"points_{n}"]["dead"]), r[f"points_{n}"]["rec"]
        assert cs[f"points_{n}"]["store"]["n_points"] == n and rec["n_obs_erased"] > 0 and rec["n_points_bad"] > 0
        assert all(2 in cs[f"points_{n}"]["store"]["obs"][p] for p in (0, n - 1))
    c = cs["points_2049_tile_edges"]
    assert all(1 in c["store"]["obs"][p] for p in (0, 1023, 1024, 2047, 2048))
    assert r["every_point_dies"]["rec"]["n_obs"] == 0 and r["every_point_dies"]["rec"]["n_points_bad"] == 1030
    rec = r["nobody_affected"]["rec"]
    assert rec["n_retired"] == 1 and rec["n_obs_removed"] == rec["n_conn_erased"] == 0
    assert r["nobody_affected"]["store"]["obs"] == cs["nobody_affected"]["store"]["obs"]
    for k in (1, 150, 298):
        out = r[f"point_of_300_loses_{k}"]
        assert len(out["store"]["obs"][1027]) == (300 - k if 300 - k > 2 else 0) and out["rec"]["n_retired"] == k
    assert (1027 in r["point_of_300_loses_298"]["dead"]) and 1027 not in r["point_of_300_loses_150"]["dead"]
    assert len(cs["slot_row_1025"]["store"]["kf_slots"][1]) == 1025
    out = r["weight_row_1025"]
    assert len(cs["weight_row_1025"]["store"]["conn"][1029]) == 1025 and sorted(out["store"]["conn"][1029]) == \
        [f for f in range(1025) if f not in (0, 512, 1024)]
    rec_of(out, n_conn_erased=3, n_rows_reordered=1)
    assert len(out["store"]["cov"][1029]) == 1022 and out["store"]["conn"][3] == {1029: 2}
    rec = r["list_of_1024"]["rec"]
    assert all(rec[k] > 0 for k in ("n_skip_range", "n_skip_dup", "n_skip_bad", "n_skip_first", "n_skip_protected", "n_retired"))
    assert sum(rec[k] for k in T.FIELDS[1:7]) == 1024 and r["list_of_1"]["rec"]["n_retired"] == 1
