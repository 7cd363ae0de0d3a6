"""CPU: the restatement of lorb_kf_store_refresh_dev (tests/kf_refresh_ref.py) against the hand case's written-out
answer, its descriptor half against oracle.compute_descriptor on the gathered lists of every case, and the normal of
a one-observation point against the insertion's one-observation form (tests/kf_store_ref.py) bit for bit."""
import numpy as np
import pytest

import kf_ba_ref as B
import kf_refresh_cases as RC
import kf_refresh_ref as RR
import kf_store_ref as R
import oracle as O
from lorb_slam_amd import synth

F = np.float32
CASES = RC.all_cases()
FP = synth.frame_params()


def window_of(c):
    w = B.gather(c["store"], c["geom"], c["kf"])
    assert w["rec"]["status"] == 0
    return dict(kf=c["kf"], local_kf=w["local_kf"], l2g=w["l2g"])


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_hand_case():
    c = RC.hand_case()
    want, s, app = c["want"], c["store"], c["app"]
    win = window_of(c)
    assert win["l2g"].tolist() == want["l2g"]
    r = RR.refresh(s, c["geom"], app, win, app["kf_center"], FP)
    assert r["rec"] == want["rec"]
    assert r["chosen"] == want["chosen"]
    sf = np.asarray(FP["scale_factors"], F)
    for i, g in enumerate(want["l2g"]):
        assert np.array_equal(raw(r["normal"][g]), raw(np.array(want["normal"][i], F))), g
        mx = F(F(want["dist"][i]) * sf[want["octave"][i]])
        assert raw(r["max_dist"][g]).tobytes() == raw(mx).tobytes() and raw(r["min_dist"][g]).tobytes() == raw(F(mx / sf[7])).tobytes(), g
        assert np.array_equal(r["desc"][g], RC.low_bits(want["took"][i])), g
    others = [p for p in range(s["n_points"]) if p not in want["l2g"]]
    for k in ("normal", "max_dist", "min_dist", "desc"):           # rows outside the window stay
        assert np.array_equal(raw(r[k][others]), raw(np.asarray(s[k])[others])), k


def test_hand_case_flags_and_status():
    c = RC.hand_case()
    s, app, win = c["store"], c["app"], window_of(c)
    both = RR.refresh(s, c["geom"], app, win, app["kf_center"], FP)
    n = RR.refresh(s, c["geom"], app, win, app["kf_center"], FP, what=RR.NORMAL_DEPTH)
    d = RR.refresh(s, c["geom"], app, win, app["kf_center"], FP, what=RR.DESCRIPTOR)
    assert np.array_equal(n["desc"], s["desc"]) and n["rec"]["n_desc_changed"] == 0
    assert all(np.array_equal(raw(n[k]), raw(both[k])) for k in ("normal", "max_dist", "min_dist"))
    assert all(np.array_equal(raw(d[k]), raw(s[k])) for k in ("normal", "max_dist", "min_dist"))
    assert np.array_equal(d["desc"], both["desc"]) and d["rec"] == both["rec"]
    for status in (1, 3):
        r = RR.refresh(s, c["geom"], app, win, app["kf_center"], FP, ba_status=status)
        assert r["rec"] == dict(status=1) and all(np.array_equal(raw(r[k]), raw(s[k])) for k in ("normal", "max_dist", "min_dist", "desc"))
    assert RR.refresh(s, c["geom"], app, win, app["kf_center"], FP, written=1)["rec"]["n_centers"] == 3
    assert RR.refresh(s, c["geom"], app, win, app["kf_center"], FP, what=RR.NORMAL_DEPTH, written=1)["rec"]["n_centers"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_descriptor_half_against_the_oracle(name):
    """The usable descriptors of every window point, gathered into one CSR, through oracle.compute_descriptor."""
    c = CASES[name]
    s, g, app, win = c["store"], c["geom"], c["app"], window_of(c)
    r = RR.refresh(s, g, app, win, app["kf_center"], FP, what=RR.DESCRIPTOR)
    off, rows = [0], []
    for p in win["l2g"]:
        use = [] if s["is_bad"][p] else [(f, j) for f, j in RR.split(s, g, int(p))[0] if not s["kf_bad"][f]]
        rows += [app["kf_slot_desc"][f][j] for f, j in use]
        off.append(len(rows))
    best = O.compute_descriptor(np.asarray(off, np.int32), np.asarray(rows, np.uint8).reshape(-1, 32))
    assert best.tolist() == r["chosen"]                            # -1: no candidate
    for i, p in enumerate(win["l2g"]):
        want = rows[off[i] + best[i]] if best[i] >= 0 else s["desc"][p]
        assert np.array_equal(r["desc"][p], want), p
    assert any(b >= 0 for b in best)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_observation_is_the_insertion_form(name):
    """A point with one observation inside the store: normal, max_dist and min_dist have the bits of
    kf_store_ref.normal_and_depth, the form k_kf_head's new_point restates."""
    c = CASES[name]
    s, g, app, win = c["store"], c["geom"], c["app"], window_of(c)
    r = RR.refresh(s, g, app, win, app["kf_center"], FP, what=RR.NORMAL_DEPTH)
    seen = 0
    for p in (int(v) for v in win["l2g"]):
        obs = RR.split(s, g, p)[0]
        if len(obs) != 1 or s["is_bad"][p]:
            continue
        f, j = obs[0]
        nrm, mx, mn = R.normal_and_depth(s["pos"][p], app["kf_center"][f], app["kf_slot_octave"][f][j], FP)
        assert raw(r["normal"][p]).tobytes() == raw(nrm).tobytes() and F(r["max_dist"][p]).tobytes() == F(mx).tobytes()
        assert F(r["min_dist"][p]).tobytes() == F(mn).tobytes(), p
        seen += 1
    assert seen > 0 or name in ("identical",)


def test_centers_restate_the_pose_block():
    """Step b on the host: the translation column of inv(pose_to_Tcw) -- what lorb_frame_pose_from_Tcw gives -- and
    the identity branch for a zero rotation vector: the centre is -t exactly."""
    c = RC.hand_case()
    pose = np.asarray(c["geom"]["kf_pose"], F).reshape(-1, 6).copy()
    pose[3, :3] = 0
    out = RR.centers(pose, [5, 3], np.zeros((6, 3), F), O.pose_to_Tcw, O.inv4_f32)
    assert np.array_equal(out[3], -pose[3, 3:]) and not out[[0, 1, 2, 4]].any()
    Twc = O.inv4_f32(O.pose_to_Tcw(pose[5, :3], pose[5, 3:]))[0]
    assert np.array_equal(out[5], Twc[:3, 3])
