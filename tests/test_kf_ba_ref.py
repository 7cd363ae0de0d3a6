"""CPU: the restatement of the store's geometry and of the local-BA gather (tests/kf_ba_ref.py) against answers
written out by hand -- the six-keyframe case of tests/kf_ba_cases.py, the statuses, and the geometry the hand-built
insertions of tests/kf_store_cases.py leave."""
import numpy as np

import kf_ba_cases as BC
import kf_ba_ref as B
import kf_store_cases as KC
import kf_store_ref as R


def test_hand_case():
    c = BC.hand_case()
    B.check_invariant(c["store"], c["geom"])
    g = B.gather(c["store"], c["geom"], c["kf"])
    w = c["want"]
    assert g["rec"] == w["rec"]
    for k in ("local_kf", "l2g", "fixed_kf", "obs_point", "obs_frame"):
        assert g[k].tolist() == w[k], k
    assert g["obs_uv"].tolist() == w["obs_uv"]
    # point 7's observation in K is slot 0 of row5 = [7, -1, 4, 7, 9], not slot 3
    assert g["obs_uv"][2].tolist() == [500.0, 500.5]
    pose = np.asarray(c["geom"]["kf_pose"], np.float32)
    assert np.array_equal(g["pose_init"], pose[[5, 3, 1]]) and np.array_equal(g["fixed_pose"], pose[[0, 4]])
    assert np.array_equal(g["point_init"], c["store"]["pos"][[7, 4, 2, 0]])


def test_statuses():
    c = BC.hand_case()
    s, g = c["store"], c["geom"]
    assert B.gather(s, g, -1)["rec"] == dict(status=1)
    assert B.gather(s, g, 6)["rec"] == dict(status=1)
    assert B.gather(s, g, 5, src_status=2)["rec"] == dict(status=1)
    # kf 4 holds p4 alone and has no covisible frame: one pose, one point, kf3 and kf5 fixed, kf2 bad
    r = B.gather(s, g, 4)
    assert r["rec"] == dict(status=0, kf=4, n_poses=1, n_fixed=2, n_points=1, n_obs=3, n_cov_bad=0, n_obs_bad_kf=1,
                            n_obs_bad_slot=0, written=0)
    assert r["fixed_kf"].tolist() == [3, 5] and r["obs_frame"].tolist() == [-1, 0, -2]
    # a keyframe whose only point is bad: no points -> status 3
    s2 = KC.make_store([[0]], [0], [[0]], [[]], [{}], is_bad=[1])
    g2 = dict(kf_pose=[np.zeros(6, np.float32)], kf_slot_uv=[np.zeros((1, 2), np.float32)], obs_slot=[[0]])
    assert B.gather(s2, g2, 0)["rec"]["status"] == 3
    # more than 128 local frames, and a point with 256 usable observations
    st = BC.status_cases()
    assert B.gather(st["local_129"]["store"], st["local_129"]["geom"], st["local_129"]["kf"])["rec"] == dict(status=2)
    assert B.gather(st["obs_256"]["store"], st["obs_256"]["geom"], st["obs_256"]["kf"])["rec"]["status"] == 4
    sz = BC.size_cases()
    r = B.gather(sz["obs_255"]["store"], sz["obs_255"]["geom"], sz["obs_255"]["kf"])["rec"]
    assert r["status"] == 0 and r["n_fixed"] == 251
    r = B.gather(sz["local_128"]["store"], sz["local_128"]["geom"], sz["local_128"]["kf"])["rec"]
    assert r["status"] == 0 and r["n_poses"] == 128
    for n in (1023, 1024, 1025):
        c = sz[f"points_{n}"]
        assert B.gather(c["store"], c["geom"], c["kf"])["rec"]["n_points"] == n
    r = B.gather(sz["fixed_1025"]["store"], sz["fixed_1025"]["geom"], sz["fixed_1025"]["kf"])["rec"]
    assert r["status"] == 0 and r["n_fixed"] == 1025


def test_a_damaged_slot_is_skipped_and_counted():
    c = BC.hand_case()
    c["geom"]["obs_slot"][7][1] = 3           # p7 in kf3: row3 has three slots
    r = B.gather(c["store"], c["geom"], 5)
    assert r["rec"]["n_obs"] == 8 and r["rec"]["n_obs_bad_slot"] == 1 and r["obs_frame"].tolist() == [-1, 0, 1, -2, 0, 2, 1, 2]


def test_insertion_geometry_by_hand():
    """two_slots: p0 sits in slots 0 and 1 of K = 2 and p2 in slot 2 -> K joins p0 with slot 0 and p2 with slot 2.
    gid_outside: slots 0 and 1 are adopted as points 2 and 3, slot 2 creates point 4, slot 4 observes p1."""
    pose6 = np.arange(6, dtype=np.float32) * 0.25
    c = KC.two_slots_case()
    g0 = BC.geometry_for(c["store"], seed=1)
    B.check_invariant(c["store"], g0)
    r = R.insert_keyframe(c["store"], c["caps"], c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], c["n_max_cur"], c["gate"])
    g = B.insert_geometry(g0, r, c["frame"], pose6, c["n_cur"])
    B.check_invariant(r["store"], g)
    assert g["obs_slot"][0][-1] == 0 and g["obs_slot"][2][-1] == 2 and len(g["obs_slot"][1]) == 1
    assert np.array_equal(g["kf_pose"][2], pose6) and g["kf_slot_uv"][2].shape == (9, 2)
    assert g["kf_slot_uv"][2][4].tolist() == [c["frame"]["x"][4], c["frame"]["y"][4]]
    c = KC.gid_outside_case()
    g0 = BC.geometry_for(c["store"], seed=2)
    r = R.insert_keyframe(c["store"], c["caps"], c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], c["n_max_cur"], c["gate"])
    g = B.insert_geometry(g0, r, c["frame"], pose6, c["n_cur"])
    B.check_invariant(r["store"], g)
    assert [g["obs_slot"][p] for p in (2, 3, 4)] == [[0], [1], [2]] and g["obs_slot"][1][-1] == 4
    # a refused insertion leaves the geometry alone
    c = KC.gate_cases()["gate_8_of_20"]
    g0 = BC.geometry_for(c["store"], seed=3)
    r = R.insert_keyframe(c["store"], c["caps"], c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], c["n_max_cur"], c["gate"])
    assert B.insert_geometry(g0, r, c["frame"], pose6, c["n_cur"]) is g0


def test_generated_cases_keep_the_invariant():
    for c in list(BC.size_cases().values()) + [BC.random_case(9, 200, seed=1), BC.solve_scene()]:
        B.check_invariant(c["store"], c["geom"])
    s = BC.solve_scene()
    r = B.gather(s["store"], s["geom"], s["kf"])["rec"]
    assert r["status"] == 0 and r["n_fixed"] >= 2 and r["n_points"] >= 140
    flat = B.flat_geometry(s["geom"])
    c = R.counts(s["store"])
    assert flat["kf_pose"].shape == (c["n_kf"], 6) and flat["kf_slot_uv"].shape == (c["n_kf_slots"], 2)
    assert flat["obs_slot"].shape == (c["n_obs"],)
