"""CPU: the numpy restatement of the pose hand-over (tests/motion_model_ref.py) against answers worked out
by hand -- one per branch of cv::Rodrigues matrix -> vector -- and against the round trip through
O.pose_to_Tcw, plus the gemm convention and Frame::SetPose.

Tolerance of the hand answers: the nine entries of a float rotation carry up to 2^-24 each, so r =
(R21 - R12, ...) is off by up to 2^-23 per component and c by 1.5 * 2^-24; the vector r * theta / (2 s)
then moves by about (2^-23 / (2 s)) * theta + (1.5 * 2^-24 / s), under 4e-7 * max(1, theta / s)."""
import numpy as np
import pytest

import motion_model_ref as M
import oracle as O

POSES = dict(M.hand_poses())
PI32 = np.float32(np.pi)


def vec(name):
    return M.rodrigues_vec(POSES[name][:3, :3], with_s=True)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_identity_is_zero():
    r, s = vec("identity")
    assert same(r, np.zeros(3, np.float32)) and s == 0.0


@pytest.mark.parametrize("name,k", [("pi_x", 0), ("pi_y", 1), ("pi_z", 2)])
def test_half_turns(name, k):
    """diag(1, -1, -1) and its two siblings: s = 0, c = -1, the square-root branch; pi on one axis."""
    r, s = vec(name)
    want = np.zeros(3, np.float32)
    want[k] = PI32
    assert s == 0.0 and same(r, want)


def test_quarter_turn_about_z():
    r, s = vec("quarter_z")
    assert s == 1.0 and same(r, np.array([0, 0, np.pi / 2], np.float32))


def test_tiny_rotation_is_zero():
    """5e-6 rad: s < 1e-5 with c > 0."""
    r, s = vec("tiny")
    assert 4e-6 < s < 6e-6 and same(r, np.zeros(3, np.float32))
    assert np.abs(POSES["tiny"][:3, :3] - np.eye(3)).max() > 1e-6  # the matrix is not the identity


def test_near_pi_takes_the_sign_branch():
    """pi - 1e-7 about (1, 2, 3) / sqrt(14): s < 1e-5 with c <= 0; both signs come from R01 and R02."""
    r, s = vec("near_pi")
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    assert s < 1e-5 and abs(s - 1e-5) > 1e-9
    assert np.abs(r.astype(np.float64) - (np.pi - 1e-7) * axis).max() < 2e-6 and (r > 0).all()
    # the mirrored axis (1, -2, 3): R01 < 0 flips y; R12 < 0 against ry * rz < 0 leaves z alone
    ax2 = axis * [1, -1, 1]
    R2 = O.pose_to_Tcw(((np.pi - 1e-7) * ax2).astype(np.float32), np.zeros(3, np.float32))[:3, :3]
    r2, s2 = M.rodrigues_vec(R2, with_s=True)
    assert s2 < 1e-5 and np.abs(r2.astype(np.float64) - (np.pi - 1e-7) * ax2).max() < 2e-6


def test_rz_is_negated_when_rx_is_smallest():
    """The half turn about (0.1, 0.7, -0.7) / |.|: R01 > 0 and R02 < 0 give (+, +, -) at once; about
    (0.1, -0.7, -0.7) / |.| both R01 and R02 are negative, (+, -, -), a vector equivalent at theta = pi.
    The |rx| smallest rule is needed when R01 and R02 vanish: the axis (0, 1, -1) / sqrt(2)."""
    a = np.array([0.0, 1.0, -1.0]) / np.sqrt(2.0)
    R = (2.0 * np.outer(a, a) - np.eye(3)).astype(np.float32)
    r, s = M.rodrigues_vec(R, with_s=True)
    assert s == 0.0 and r[0] == 0 and r[1] > 0 and r[2] < 0  # R12 < 0 while ry * rz would be > 0
    assert np.abs(np.abs(r[1:].astype(np.float64)) - np.pi / np.sqrt(2.0)).max() < 1e-6


def test_entry_of_100_is_zero():
    r, s = vec("entry_100")
    assert s is None and same(r, np.zeros(3, np.float32))
    for bad in (np.nan, np.inf, -100.5):
        R = np.eye(3, dtype=np.float32)
        R[1, 2] = bad
        assert same(M.rodrigues_vec(R), np.zeros(3, np.float32))
    R = np.eye(3, dtype=np.float32)
    R[1, 2] = -100.0  # the lower bound is inside the range
    assert M.rodrigues_vec(R, with_s=True)[1] is not None


@pytest.mark.parametrize("theta", [1e-3, 0.1, 1.0, 3.0])
def test_round_trip(theta):
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    r, s = vec(f"theta_{theta}")
    assert abs(s - np.sin(theta)) < 1e-6 and abs(s - 1e-5) > 1e-9
    assert np.abs(r.astype(np.float64) - theta * axis).max() <= 4e-7 * max(1.0, theta / s)


def test_gemm_convention():
    """Double accumulation in k order, one rounding: a row whose float sum differs from it."""
    A = np.eye(4, dtype=np.float32)
    B = np.eye(4, dtype=np.float32)
    A[0] = [1.0, 2.0 ** -24, 2.0 ** -24, 0.0]
    B[:, 0] = [1.0, 1.0, 1.0, 0.0]
    C = M.gemm4(A, B)
    assert C[0, 0] == np.float32(1.0 + 2.0 ** -23)  # float accumulation would stay at 1
    assert C.dtype == np.float32 and same(M.gemm4(np.eye(4), B), B)


def test_set_pose_predict_finish():
    T = POSES["theta_1.0"]
    blk = M.set_pose(T)
    assert same(blk["Tcw"], T) and same(blk["Twc"], O.inv4_f32(T)[0]) and same(blk["pose"][3:], T[:3, 3]) and blk["status"] == 0
    Tcc = np.eye(4, dtype=np.float32)
    Tcc[0, 3] = 0.1
    p = M.predict(blk, Tcc)
    assert same(p["Tcw"], M.gemm4(T, Tcc)) and same(p["Tcw"][:3, :3], T[:3, :3])
    assert same(p["pose"][3:], p["Tcw"][:3, 3]) and M.vec_close(p["pose"][:3], blk["pose"][:3], blk["s"])
    pose64 = np.array([0.01, 0.02, 0.03, 0.1, 0.2, 0.3]) + 1e-9
    pin = np.arange(6, dtype=np.float32)
    cur, mTcc = M.finish(p["Tcw"], 1, pose64, pin, blk)
    assert same(cur["pose"], pose64.astype(np.float32)) and same(mTcc, M.gemm4(blk["Twc"], p["Tcw"]))
    assert same(cur["Twc"], O.inv4_f32(p["Tcw"])[0])
    assert same(M.finish(p["Tcw"], 0, pose64, pin, blk)[0]["pose"], pin)
    assert np.abs(mTcc - Tcc).max() < 1e-6  # last^-1 * (last * Tcc) is Tcc up to rounding
