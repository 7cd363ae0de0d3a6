"""The pose hand-over between frames restated in numpy: what lorb_Tcw_to_pose, lorb_frame_pose_from_Tcw,
the prediction of lorb_track_motion_frames_pose_dev and lorb_frame_pose_finish_dev must compute.

  rodrigues_vec     cv::Rodrigues, matrix -> vector: OpenCV 3.x cvRodrigues2's 3 x 3 branch, all in double,
                    R <- U V^T through np.linalg.svd (the library uses an iteration of its own: the two
                    agree within vec_tol, below)
  gemm4             a 4 x 4 CV_32F product through cv::gemm: float operands, double accumulation in k
                    order, one rounding to float (the convention of oracle/match.c's gemv3_row)
  set_pose          Frame::SetPose(Tcw) -> UpdatePoseVector        src/frame.cpp:570-575, 596-605
  predict           mCurrFrame->SetPose(pF->GetPose() * mTcc)      src/visual_odometry.cpp:119
  finish            mTcc = mPrevFrame->GetInvPose() * mCurrFrame->GetPose() after the local stage
                                                                    src/visual_odometry.cpp:65
The inverse is oracle.inv4_f32 (cv::Mat::inv() of a 4 x 4 CV_32F).  A block is a dict(Tcw (4, 4) float32,
Twc (4, 4) float32, pose (6,) float32, status)."""
import numpy as np

import oracle as O


def rodrigues_vec(R, with_s=False):
    """R: 3 x 3 (float32 values).  Returns the float32 vector, and with_s also s = |r| / 2 before the
    scaling (what the tolerance is stated in) or None where the matrix is out of range."""
    R = np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)
    if not (np.isfinite(R).all() and (R >= -100.0).all() and (R < 100.0).all()):  # cv::checkRange(-100, 100)
        z = np.zeros(3, np.float32)
        return (z, None) if with_s else z
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25)
    c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5, -1.0), 1.0)
    theta = np.arccos(c)
    if s < 1e-5:
        if c > 0:
            r = np.zeros(3)
        else:
            sgn = lambda x: -1.0 if x < 0 else 1.0  # noqa: E731
            r = np.array([np.sqrt(max((R[0, 0] + 1) * 0.5, 0.0)),
                          np.sqrt(max((R[1, 1] + 1) * 0.5, 0.0)) * sgn(R[0, 1]),
                          np.sqrt(max((R[2, 2] + 1) * 0.5, 0.0)) * sgn(R[0, 2])])
            if abs(r[0]) < abs(r[1]) and abs(r[0]) < abs(r[2]) and (R[1, 2] > 0) != (r[1] * r[2] > 0):
                r[2] = -r[2]
            theta /= np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            r = r * theta
    else:
        vth = 1 / (2 * s)
        vth *= theta
        r = r * vth
    out = r.astype(np.float32)
    return (out, float(s)) if with_s else out


def hand_poses():
    """[(name, Tcw 4 x 4 float32)]: the poses every test of the vector runs -- one per branch of
    rodrigues_vec, with a translation that has no exact inverse in float."""
    t = np.array([0.3, -0.1, 0.2], np.float32)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)

    def T(R):
        out = np.eye(4, dtype=np.float32)
        out[:3, :3] = np.asarray(R, np.float32)
        out[:3, 3] = t
        return out

    def rot(theta, ax=axis):
        return O.pose_to_Tcw((theta * np.asarray(ax)).astype(np.float32), np.zeros(3, np.float32))[:3, :3]

    big = np.eye(3, dtype=np.float32)
    big[0, 1] = 100.0
    out = [("identity", T(np.eye(3))), ("pi_x", T(np.diag([1, -1, -1]))), ("pi_y", T(np.diag([-1, 1, -1]))),
           ("pi_z", T(np.diag([-1, -1, 1]))), ("quarter_z", T([[0, -1, 0], [1, 0, 0], [0, 0, 1]])),
           ("tiny", T(rot(5e-6))), ("near_pi", T(rot(np.pi - 1e-7))), ("entry_100", T(big))]
    out += [(f"theta_{th}", T(rot(th))) for th in (1e-3, 0.1, 1.0, 3.0)]
    return out


def seeded_poses(n, seed):
    """n products of two rotations (through gemm4, as the motion model forms them) with translations."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        Ts = []
        for _ in range(2):
            ax = rng.normal(size=3)
            th = rng.uniform(1e-3, 3.1)
            Ts.append(O.pose_to_Tcw((th * ax / np.linalg.norm(ax)).astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32)))
        out.append(gemm4(Ts[0], Ts[1]))
    return out


def vec_tol(ref, s):
    """Per component: 2^-22 |ref| + 1e-13 / s_ref.  Two correct double evaluations differ in the last
    bits of U V^T and of acos: an error d of a few double ulps in c moves theta by d / sin(theta) = d / s,
    and the final rounding to float can then fall on either side of a boundary (two float ulps)."""
    ref = np.asarray(ref, np.float64)
    return 2.0 ** -22 * np.abs(ref) + (1e-13 / s if s else 0.0)


def vec_close(got, ref, s):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.abs(got - ref) <= vec_tol(ref, s)).all())


def gemm4(A, B):
    A, B = np.asarray(A, np.float32).reshape(4, 4), np.asarray(B, np.float32).reshape(4, 4)
    out = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float64(A[i, 0]) * np.float64(B[0, j])
            for k in range(1, 4):
                s = s + np.float64(A[i, k]) * np.float64(B[k, j])
            out[i, j] = np.float32(s)
    return out


def set_pose(Tcw):
    """Frame::SetPose(Tcw): the matrix as given, its vector | column 3, Twc = Tcw.inv()."""
    T = np.array(Tcw, np.float32).reshape(4, 4)
    rvec, s = rodrigues_vec(T[:3, :3], with_s=True)
    return dict(Tcw=T, Twc=O.inv4_f32(T)[0], pose=np.concatenate([rvec, T[:3, 3]]).astype(np.float32), status=0, s=s)


def predict(last, Tcc):
    return set_pose(gemm4(last["Tcw"], Tcc))


def finish(Tcw, local_ok, local_pose, pose_in, last):
    """(the frame's block, mTcc) from the local stage's record: Tcw, local.ok, local.pose, pose_in."""
    T = np.array(Tcw, np.float32).reshape(4, 4)
    pose = np.asarray(local_pose, np.float64).astype(np.float32) if local_ok else np.asarray(pose_in, np.float32)
    return dict(Tcw=T, Twc=O.inv4_f32(T)[0], pose=pose, status=0), gemm4(last["Twc"], T)
