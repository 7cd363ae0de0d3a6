"""CPU: the restatement of VisualOdometry::UpdateLocalMap (tests/local_map_ref.py) against answers
written out by hand for each numbered case of tests/test_gpu_local_map.py (tests/local_map_cases.py), so
that the model the device is compared with is not only checked against itself."""
import numpy as np
import pytest

import local_map_cases as LC
import local_map_ref as R

CASES = LC.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_hand_answer(name):
    c = CASES[name]
    r = R.update_local_map(c["store"], c["state"], c["gid"], c["n_cur"], c["max_local"], c["ids"])
    for k, want in c["want"].items():
        got = r[k]
        assert np.array_equal(np.asarray(got), np.asarray(want)), (name, k, got, want)
    # what holds for every case
    assert r["n_local"] == len(set(p for kf in r["local_kf"] for p in c["store"]["kf_slots"][kf]
                                   if p >= 0 and not (c["store"]["is_bad"] is not None and c["store"]["is_bad"][p])))
    if r["status"] == 0:
        assert r["l2g"] == sorted(r["l2g"]) and (r["g2l"][r["l2g"]] == np.arange(r["n_local"])).all()
        assert (np.delete(r["g2l"], r["l2g"]) == -1).all()
        for k in R.COLS:
            assert r["n_local"] == 0 or np.array_equal(r["rows"][k], c["store"][k][r["l2g"]])
    else:
        assert r["n_local"] > c["max_local"] and r["slot_id"] is None and (r["g2l"] == -1).all()


def test_overflow_keeps_steps_c_and_d():
    """Status 2 changes nothing about the slots, the votes, the list and pFMax."""
    a, b = CASES["exact_fit"], CASES["overflow"]
    ra = R.update_local_map(a["store"], a["state"], a["gid"], a["n_cur"], a["max_local"])
    rb = R.update_local_map(b["store"], b["state"], b["gid"], b["n_cur"], b["max_local"])
    assert (ra["status"], rb["status"], rb["n_local"]) == (0, 2, 3)
    for k in ("state", "gid", "votes", "local_kf", "refer_kf", "n_held", "n_nulled", "n_voted", "n_local"):
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k


def test_id_source_equals_direct_gids():
    a, b = CASES["ids_given"], CASES["ids_direct"]
    ra = R.update_local_map(a["store"], a["state"], a["gid"], a["n_cur"], a["max_local"], a["ids"])
    rb = R.update_local_map(b["store"], b["state"], b["gid"], b["n_cur"], b["max_local"])
    for k in ("state", "gid", "votes", "local_kf", "l2g", "slot_id"):
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k


def test_unchanged_code_without_given_slots_drops_the_gid():
    c = CASES["ids_given"]
    for pass_, given in ((0, 1), (1, 0)):
        g = R.entry_gids(c["gid"], c["n_cur"], 4, dict(c["ids"], pass_=pass_, given=given))
        assert list(g) == [1, -1, -1, -1, 0]


def test_ids_back_by_hand():
    """10: slot 0 was matched in the local stage (local row 2 -> global 7); slot 1 was emptied by step c;
    slot 2 holds a point outside the local map and keeps its gid; slot 3 a created point (-1 stays)."""
    g = R.ids_back(state=[LC.LOCKED, LC.EMPTY, LC.FREE, LC.FREE], slot_id=[2, -1, -1, -1], gid=[-1, -1, 11, -1], l2g=[4, 5, 7])
    assert list(g) == [7, -1, 11, -1]
