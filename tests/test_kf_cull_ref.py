"""CPU: the restatement tests/kf_cull_ref.py (the points' life through an insertion, observe, cull) against stores
built by hand with the answers written out."""
import numpy as np

import kf_cull_cases as CC
import kf_cull_ref as L
import kf_store_cases as KC
import kf_store_ref as R

LOCKED, FREE, EMPTY = R.LOCKED, R.FREE, R.EMPTY


def test_verdict_branches_and_their_precedence():
    assert L.verdict(1, 5, 9, 0, 1) == "bad_before"           # bad comes first, whatever else holds
    assert L.verdict(1, 5, 9, 0, 0) == "ratio"                # fails the ratio AND the observation rule: ratio
    assert L.verdict(1, 1, 9, 0, 0) == "obs"
    assert L.verdict(1, 1, 9, 3, 0) == "aged_out"
    assert L.verdict(1, 1, 0, 0, 0) == "stays"


def test_age_exactly_at_the_thresholds():
    ratio, age_obs, min_obs, age_out = L.REFERENCE
    assert L.verdict(1, 1, age_obs - 1, min_obs - 1, 0) == "stays"
    assert L.verdict(1, 1, age_obs, min_obs - 1, 0) == "obs"
    assert L.verdict(1, 1, age_obs, min_obs, 0) == "stays"
    assert L.verdict(1, 1, age_out - 1, min_obs, 0) == "stays"
    assert L.verdict(1, 1, age_out, min_obs, 0) == "aged_out"
    # the parameters are the host's: other thresholds move the edges with them
    assert L.verdict(1, 1, 4, 0, 0, (0.25, 5, 3, 9)) == "stays" and L.verdict(1, 1, 5, 0, 0, (0.25, 5, 3, 9)) == "obs"


def test_ratio_exactly_a_quarter_is_kept():
    assert L.verdict(1, 4, 0, 5, 0) == "stays"     # (float)1 / (float)4 is 0.25f itself: not below
    assert L.verdict(1, 5, 0, 5, 0) == "ratio"
    assert L.verdict(2, 8, 0, 5, 0) == "stays" and L.verdict(2, 9, 0, 5, 0) == "ratio"


def test_the_hand_store():
    c = CC.hand_case()
    r = L.cull(c["store"], c["obs_slot"], c["life"], c["kf"], frame=c["frame"])
    assert r["verdicts"] == {0: "bad_before", 1: "ratio", 2: "obs", 3: "stays", 4: "aged_out", 5: "stays"}
    assert r["culled"] == [1, 2]
    assert r["rec"] == dict(status=0, kf=3, n_examined=6, n_bad_before=1, n_culled_ratio=1, n_culled_obs=1, n_aged_out=1,
                            n_recent=2, n_obs_removed=3, n_slots_erased=3, n_frame_slots_emptied=2, n_obs_bad_slot=0, n_obs=10)
    s = r["store"]
    assert list(s["is_bad"]) == [1, 1, 1, 0, 0, 0, 0]
    assert s["obs"] == [[0], [], [], [3], [0, 1, 2], [0, 1, 2], [0, 3]]
    assert r["obs_slot"] == [[0], [], [], [0], [3, 1, 0], [4, 2, 1], [5, 1]]
    assert s["kf_slots"] == [[0, -1, -1, 4, 5, 6], [-1, 4, 5], [4, 5], [3, 6]]
    assert list(r["life"]["recent"]) == [0, 0, 0, 1, 0, 1, 0]
    # the frame: the slots of p1 and p2 are emptied; p0 (bad before the call) and the others stay
    assert list(r["state"]) == [EMPTY, LOCKED, EMPTY, LOCKED, FREE, LOCKED] and list(r["gid"]) == [-1, 0, -1, 5, -1, 9]
    # untouched, as in the reference
    for k in ("visible", "found", "first_fid", "kf_fid"):
        assert np.array_equal(r["life"][k], c["life"][k]), k
    for k in ("pos", "normal", "max_dist", "min_dist", "desc", "locked"):
        assert np.array_equal(s[k], c["store"][k]), k
    assert s["cov"] == c["store"]["cov"] and s["conn"] == c["store"]["conn"]
    # the invariant
    for p, (o, sl) in enumerate(zip(s["obs"], r["obs_slot"])):
        assert all(s["kf_slots"][f][j] == p for f, j in zip(o, sl))
    # the inputs were not changed
    assert c["store"]["obs"][1] == [0] and c["store"]["kf_slots"][0][1] == 1 and c["life"]["recent"][1] == 1


def test_status_1_changes_nothing():
    c = CC.hand_case()
    for kw in (dict(kf=-1), dict(kf=4), dict(kf=3, src_status=1)):
        r = L.cull(c["store"], c["obs_slot"], c["life"], kw["kf"], src_status=kw.get("src_status", 0), frame=c["frame"])
        assert r["rec"] == dict(status=1)
        assert r["store"]["obs"] == c["store"]["obs"] and np.array_equal(r["life"]["recent"], c["life"]["recent"])
        assert np.array_equal(r["gid"], c["frame"]["gid"])


def test_a_damaged_obs_slot_is_counted_and_skipped():
    c = CC.hand_case()
    slot = [list(x) for x in c["obs_slot"]]
    slot[1] = [0]        # p1's observation names slot 0 of kf0, which holds p0
    slot[2] = [2, 99]    # p2's second observation names a slot outside kf1's row
    r = L.cull(c["store"], slot, c["life"], c["kf"])
    assert r["rec"]["n_slots_erased"] == 1 and r["rec"]["n_obs_bad_slot"] == 2 and r["rec"]["n_obs_removed"] == 3
    assert r["store"]["kf_slots"][0] == [0, 1, -1, 4, 5, 6] and r["store"]["kf_slots"][1] == [2, 4, 5]
    assert r["store"]["obs"][1] == [] and r["store"]["obs"][2] == [] and r["rec"]["n_obs"] == 10


def test_found_slots_keeps_a_point_the_reference_rule_culls():
    """A point created at frame 10 and held in one slot of frames 11-14: the reference never calls IncreaseFound, so
    found / visible = 1 / 5 and the next keyframe culls it; counted per held slot it is 5 / 5."""
    for rule, want in ((L.FOUND_NEVER, "ratio"), (L.FOUND_SLOTS, "stays")):
        life = L.new_life(1, 2)
        life["first_fid"][:] = 10
        for fid in (11, 12, 13, 14):
            life, rec = L.observe(life, 2, fid, 3, 4, state=[LOCKED, EMPTY, FREE], gid=[1, 0, -1], lid=[0, -1, -1], l2g=[1, 0],
                                  n_local=2, max_local=8, in_view=[0, 0], found_rule=rule)
            assert rec == dict(status=0, n_held=2, n_in_view=0, n_found=1 if rule else 0)
        assert life["frame_word"] == 14 and list(life["visible"]) == [5, 5]
        assert list(life["found"]) == ([1, 5] if rule else [1, 1])
        assert L.verdict(int(life["found"][1]), int(life["visible"][1]), 1, 1, 0) == want
        assert L.verdict(int(life["found"][0]), int(life["visible"][0]), 1, 1, 0) == "ratio"   # slot 1 is EMPTY: not found


def test_observe_by_hand():
    life = L.new_life(1, 4)
    a = dict(n_points=4, frame_id=7, n_cur=5, n_max_cur=6, state=[LOCKED, LOCKED, EMPTY, FREE, LOCKED], gid=[2, 2, 1, 9, -1],
             lid=[1, -1, -1, 5, 0], l2g=[3, 2, 7], n_local=3, max_local=4, in_view=[1, 0, 1])
    out, rec = L.observe(life, found_rule=L.FOUND_SLOTS, **a)
    # c: p2 twice (two slots), p1 once (no state test), gid 9 and -1 outside; d: row 0 -> p3, row 2 -> 7 outside
    assert list(out["visible"]) == [1, 2, 3, 2] and out["frame_word"] == 7
    # e: slot 0 lid 1 -> p2; slot 1 gid 2 -> p2; slot 2 EMPTY; slot 3 lid 5 outside the local rows; slot 4 lid 0 -> p3
    assert list(out["found"]) == [1, 1, 3, 2]
    assert rec == dict(status=0, n_held=3, n_in_view=1, n_found=3)
    for kw in (dict(n_cur=7), dict(n_cur=-1), dict(n_local=5), dict(update_status=2), dict(local_status=1)):
        out, rec = L.observe(life, **dict(a, **kw))
        assert rec == dict(status=1) and out["frame_word"] == 0 and list(out["visible"]) == [1, 1, 1, 1]


def _inserted(c, frame_word):
    s = c["store"]
    life = L.new_life(len(s["kf_bad"]), s["n_points"])
    life["frame_word"] = frame_word
    res = R.insert_keyframe(s, c["caps"], c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"], c["n_max_cur"], c["gate"])
    return L.insert_life(life, s, c["frame"], c["slots"], c["gid"], res), res


def test_a_duplicate_held_old_point_enters_the_list():
    life, res = _inserted(KC.two_slots_case(), 12)   # p0 in slots 0 and 1, p2 in slot 2
    assert res["inserted"] and list(life["recent"]) == [1, 0, 0] and list(life["kf_fid"]) == [0, 0, 12]
    assert list(life["visible"]) == [1, 1, 1] and list(life["first_fid"]) == [0, 0, 0]


def test_an_adopted_point_does_not_enter_the_list_a_created_one_does():
    life, res = _inserted(KC.gid_outside_case(), 31)   # points 2, 3 adopted, 4 created
    assert list(life["recent"]) == [0, 0, 0, 0, 1] and list(life["first_fid"]) == [0, 0, 31, 31, 31]
    assert list(life["visible"]) == [1] * 5 and list(life["found"]) == [1] * 5 and list(life["kf_fid"]) == [0, 31]


def test_a_held_bad_point_and_a_refused_insertion_change_nothing():
    life, res = _inserted(KC.held_bad_case(), 5)
    assert list(life["recent"]) == [0, 0]
    life, res = _inserted(KC.gate_cases()["gate_8_of_20"], 5)
    assert not res["inserted"] and len(life["kf_fid"]) == 1 and list(life["recent"]) == [0] * 8


def test_the_reference_defaults_cull_almost_every_created_point():
    """The worked consequence: a point created at keyframe frame f and seen in the next four frames has
    found / visible = 1 / 5 at the next keyframe; one that is not seen at all is two frames old with one observation."""
    assert L.verdict(1, 1 + 4, 4, 2, 0) == "ratio"
    assert L.verdict(1, 1, 2, 1, 0) == "obs"
    assert L.verdict(1, 1 + 3, 3, 3, 0) == "aged_out"   # survives only with three observations inside three frames


def test_the_generated_cases_take_every_branch():
    seen = set()
    for name, c in CC.cull_cases().items():
        r = L.cull(c["store"], c["obs_slot"], c["life"], c["kf"], c["params"], frame=c["frame"])
        seen |= set(r["verdicts"].values())
        for p, (o, sl) in enumerate(zip(r["store"]["obs"], r["obs_slot"])):   # the invariant holds afterwards
            assert all(r["store"]["kf_slots"][f][j] == p for f, j in zip(o, sl)), name
    assert seen == set(L.VERDICTS)
