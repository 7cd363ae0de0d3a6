"""CPU: the restatement of the keyframe insertion (tests/kf_store_ref.py) against the answers written out by hand
in tests/kf_store_cases.py, so that the model the GPU tests compare with is not its own judge; its unprojection
against the oracle's; its step-d arithmetic against a value worked out in exact fractions."""
import os
import sys

import numpy as np
import pytest

import kf_store_cases as KC
import kf_store_ref as R

CASES = KC.all_cases()


def run(c):
    return R.insert_keyframe(c["store"], c["caps"], c["fp"], c["frame"], c["pose"], c["slots"], c["gid"], c["n_cur"],
                             c["n_max_cur"], c["gate"])


def test_the_issue_s_cases_are_all_here():
    for name in ("gate_7_of_20", "gate_8_of_20", "empty_frame", "two_slots", "held_bad", "gid_outside", "weights_2_3_3",
                 "fallback_largest", "below3_enters", "empty_store_none", "cap_max_kf", "cap_max_points", "cap_max_obs",
                 "cap_max_kf_slots", "cap_exact"):
        assert name in CASES, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_hand_answer(name):
    c = CASES[name]
    before = R.counts(c["store"])
    r = run(c)
    s, n = r["store"], c["n_cur"]
    for k, want in c["want"].items():
        if k in R.FIELDS:
            got = r["rec"].get(k)
        else:
            got = dict(gid=list(r["gid"][:n]), state=list(r["state"][:n]), row=s["kf_slots"][-1] if r["inserted"] else None,
                       obs=s["obs"], cov=s["cov"], conn=s["conn"], locked=list(s["locked"][before["n_points"]:]))[k]
        assert got == want, (name, k, got, want)
    if not r["inserted"]:  # nothing but the record
        assert r["store"] is c["store"] and R.counts(r["store"]) == before
        assert np.array_equal(r["gid"], c["gid"]) and all(np.array_equal(r[k], c["slots"][k]) for k in ("state", "pos", "desc"))
        assert set(r["rec"]) == ({"status", "inserted", "n_map"} if r["rec"]["status"] == 0 else set(R.FIELDS))
    else:
        assert set(r["rec"]) == set(R.FIELDS)
        c1 = R.counts(s)
        assert (r["rec"]["n_points"], r["rec"]["n_kf"], r["rec"]["n_obs"]) == (c1["n_points"], c1["n_kf"], c1["n_obs"])
        assert all(o == sorted(set(o)) for o in s["obs"])          # ascending, K once
        assert all(list(c) == sorted(c) for c in s["conn"])
        assert s["kf_bad"][-1] == 0 and len(s["kf_slots"][-1]) == n


def test_status_1():
    c = CASES["two_slots"]
    a = (c["store"], c["caps"], c["fp"], c["frame"])
    for kw in (dict(n_cur=-1), dict(n_cur=c["n_max_cur"] + 1), dict(src_status=3), dict(pose=dict(c["pose"], status=1))):
        k = dict(pose=c["pose"], n_cur=c["n_cur"], src_status=0)
        k.update(kw)
        r = R.insert_keyframe(*a, k["pose"], c["slots"], c["gid"], k["n_cur"], c["n_max_cur"], c["gate"], src_status=k["src_status"])
        assert r["rec"] == dict(status=1) and r["store"] is c["store"] and not r["inserted"], kw


def test_gate_none_ignores_the_ratio():
    c = dict(CASES["gate_8_of_20"], gate=R.GATE_NONE)
    r = run(c)
    assert r["inserted"] and r["rec"]["n_map"] == 8 and r["rec"]["n_observed"] == 8 and r["store"]["cov"] == [[1], [0]]


def test_new_point_columns_by_hand():
    """One created point worked out with exact fractions: Twc = [I | (1, 2, 3)], a keypoint at the principal point
    with depth 4 lands on (1, 2, 7); d = (0, 0, 4): the normal is (0, 0, 1), dist = 4, octave 2 of scale 1.2 gives
    max_dist = 4 * 1.44f and min_dist = that over scale_factors[7]."""
    fp = KC.synth.frame_params()
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 3] = [1, 2, 3]
    pos = R.unproject(fp, Twc.reshape(16), fp["cx"], fp["cy"], 4.0)
    assert pos.dtype == np.float32 and list(pos) == [1.0, 2.0, 7.0]
    assert list(R.unproject(fp, Twc.reshape(16), 10.0, 20.0, 0.0)) == [0.0, 0.0, 0.0]   # no depth: the origin
    nrm, mx, mn = R.normal_and_depth(pos, (1, 2, 3), 2, fp)
    sf = fp["scale_factors"]
    assert list(nrm) == [0.0, 0.0, 1.0] and mx == np.float32(4.0) * sf[2] and mn == mx / sf[7]
    assert all(isinstance(v, np.float32) for v in (mx, mn)) and nrm.dtype == np.float32
    # a direction that needs the double accumulation: the norm of (3, 4, 12) is 13 exactly
    nrm, mx, _ = R.normal_and_depth((4, 6, 15), (1, 2, 3), 0, fp)
    inv = np.float32(1.0 / 13.0)
    assert list(nrm) == [np.float32(3) * inv, np.float32(4) * inv, np.float32(12) * inv] and mx == np.float32(13.0)


def test_unprojection_has_the_oracle_s_bits():
    """R.unproject under Twc = inv(Tcw) against the oracle's UnprojectStereo (the bits of lorb_unproject_stereo_dev)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle as O
    rng = np.random.default_rng(5)
    fp = KC.synth.frame_params()
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3] = O.pose_to_Tcw([0.1, -0.2, 0.05], [0, 0, 0])[:3, :3]
    Tcw[:3, 3] = [0.4, -0.1, 2.0]
    Twc = O.inv4_f32(Tcw)[0].reshape(16)
    x, y = rng.uniform(0, 700, 200).astype(np.float32), rng.uniform(0, 400, 200).astype(np.float32)
    d = np.where(rng.uniform(size=200) < 0.8, rng.uniform(0.5, 40, 200), -1).astype(np.float32)
    want = O.unproject_stereo(fp, Tcw, x, y, d)
    got = np.stack([R.unproject(fp, Twc, x[i], y[i], d[i]) for i in range(200)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_chain_s_frames_by_hand():
    """The four frames of tests/test_gpu_kf_store_chain.py: the restatement applied in turn gives what
    kf_store_cases.chain_frames says -- insert, insert, refuse, insert -- with the lists worked out by hand."""
    refs = KC.chain_restate(KC.chain_frames())
    assert [r["inserted"] for r in refs] == [True, True, False, True] and [r["kf"] for r in refs] == [0, 1, -1, 2]
    assert [R.counts(r["store"])["n_points"] for r in refs] == [10, 15, 15, 22]
    s = refs[3]["store"]
    assert s["conn"] == [{1: 5, 2: 4}, {0: 5, 2: 8}, {0: 4, 1: 8}] and s["cov"] == [[2, 1], [0, 2], [0, 1]]
    assert s["obs"][2] == [0, 1, 2] and s["obs"][10] == [1, 2] and s["obs"][5] == [0] and s["obs"][21] == [2]
    assert refs[2]["rec"] == dict(status=0, inserted=0, n_map=5)
    assert refs[3]["rec"]["n_observed"] == 7 and refs[3]["rec"]["n_adopted"] == 2 and refs[3]["rec"]["n_created"] == 5


def test_size_cases_insert():
    """The generated stores of the GPU test: every one is an insertion, and the window case really sorts rows
    longer than a wavefront and longer than the sort's thread count."""
    cs = KC.size_cases(1024, 1024, 1024)
    for name, c in cs.items():
        r = run(c)
        assert r["inserted"], name
    r = run(cs["window_plus"])
    assert len(r["store"]["cov"][3]) == 64 + 6 + 1 and len(r["store"]["cov"][1024]) == 1025
    assert r["rec"]["n_connected"] >= 3 and r["rec"]["kf"] == 1025
    r = run(cs["walk_plus"])
    assert r["rec"]["n_cur"] == 1030 and min(r["rec"]["n_observed"], r["rec"]["n_adopted"], r["rec"]["n_created"]) > 10
    r = run(cs["two_tiles"])
    assert r["rec"]["n_observed"] == 8 and r["rec"]["n_created"] == 4 and r["rec"]["n_points"] == 2 * 1024 + 3 + 4
