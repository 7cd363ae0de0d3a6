"""ctypes bindings of the windowed matchers and frame callees (a4, a5, a8, a20) of liblorb.so."""
import ctypes as C

import numpy as np

from . import _abi as A
from .runtime import Context, LorbError, lib


def _search_by_projection_frame(self, fp, cur_Tcw, cur_kps, cur_slot_state, last, th):
    keep = A.KeepAlive()
    fps = A.make_frame_params(fp)
    k = A.make_keypoints(cur_kps, keep)
    lf = A.make_last_frame(last, keep)
    T = keep.keep(A.f32(cur_Tcw).reshape(16))
    ss = keep.keep(A.u8(cur_slot_state)) if cur_slot_state is not None else None
    assign = np.empty(max(1, k.n), np.int32)
    nm = C.c_int32(0)
    self.check(lib().lorb_search_by_projection_frame(
        self.handle, C.byref(fps), A.ptr(T, C.c_float), C.byref(k), A.ptr(ss, C.c_uint8), C.byref(lf),
        C.c_float(th), A.ptr(assign, C.c_int32), C.byref(nm)), "lorb_search_by_projection_frame")
    return assign[: k.n].copy(), nm.value


def _search_by_projection_local(self, fp, kps, slot_state, pts, th):
    keep = A.KeepAlive()
    fps = A.make_frame_params(fp)
    k = A.make_keypoints(kps, keep)
    lp = A.make_local_points(pts, keep)
    ss = keep.keep(A.u8(slot_state)) if slot_state is not None else None
    assign = np.empty(max(1, k.n), np.int32)
    nm = C.c_int32(0)
    self.check(lib().lorb_search_by_projection_local(
        self.handle, C.byref(fps), C.byref(k), A.ptr(ss, C.c_uint8), C.byref(lp), C.c_float(th),
        A.ptr(assign, C.c_int32), C.byref(nm)), "lorb_search_by_projection_local")
    return assign[: k.n].copy(), nm.value


def _is_in_frustum(self, fp, Tcw, fpts, cos_limit=0.5):
    keep = A.KeepAlive()
    fps = A.make_frame_params(fp)
    p = A.make_frustum_points(fpts, keep)
    T = keep.keep(A.f32(Tcw).reshape(16))
    n = p.n
    out = dict(in_view=np.zeros(max(n, 1), np.uint8), proj_x=np.zeros(max(n, 1), np.float32),
               proj_y=np.zeros(max(n, 1), np.float32), proj_xr=np.zeros(max(n, 1), np.float32),
               pred_level=np.zeros(max(n, 1), np.int32), view_cos=np.zeros(max(n, 1), np.float32))
    self.check(lib().lorb_is_in_frustum(
        self.handle, C.byref(fps), A.ptr(T, C.c_float), C.byref(p), C.c_float(cos_limit),
        A.ptr(out["in_view"], C.c_uint8), A.ptr(out["proj_x"], C.c_float), A.ptr(out["proj_y"], C.c_float),
        A.ptr(out["proj_xr"], C.c_float), A.ptr(out["pred_level"], C.c_int32),
        A.ptr(out["view_cos"], C.c_float)), "lorb_is_in_frustum")
    return {k_: v[:n] for k_, v in out.items()}


def _unproject_stereo(self, fp, Tcw, x, y, depth):
    fps = A.make_frame_params(fp)
    T = A.f32(Tcw).reshape(16)
    x = A.f32(x); y = A.f32(y); d = A.f32(depth)
    out = np.zeros((max(len(x), 1), 3), np.float32)
    self.check(lib().lorb_unproject_stereo(self.handle, C.byref(fps), A.ptr(T, C.c_float), C.c_int32(len(x)),
                                           A.ptr(x, C.c_float), A.ptr(y, C.c_float), A.ptr(d, C.c_float),
                                           A.ptr(out, C.c_float)), "lorb_unproject_stereo")
    return out[: len(x)]


def _track_local_map(self, fp, Tcw, kps, slot_state, pts, cos_limit=0.5, th=1.0):
    """lorb_track_local_map_dev on device copies of the inputs (they stay resident for the call)."""
    keep = []

    def dev(a, dtype):
        d = self.to_device(np.ascontiguousarray(a, dtype))
        keep.append(d)
        return d.ptr

    nk, npt = len(kps["x"]), len(pts["max_dist"])
    k = A.KeypointsDev(nk, dev(kps["x"], np.float32), dev(kps["y"], np.float32), dev(kps["octave"], np.int32),
                       dev(kps["angle"], np.float32),
                       dev(kps["u_right"], np.float32) if kps.get("u_right") is not None else None,
                       dev(kps["desc"], np.uint8))
    m = A.MapPointsDev(npt, dev(pts["pos"], np.float32), dev(pts["normal"], np.float32), dev(pts["max_dist"], np.float32),
                       dev(pts["min_dist"], np.float32), dev(pts["desc"], np.uint8), dev(pts["locked"], np.uint8),
                       dev(pts["is_bad"], np.uint8) if pts.get("is_bad") is not None else None,
                       dev(pts["in_frame"], np.uint8) if pts.get("in_frame") is not None else None)
    ss = dev(slot_state, np.uint8) if slot_state is not None else None
    iv, tr, lv = self.empty(max(npt, 1), np.uint8), self.empty((4, max(npt, 1)), np.float32), self.empty(max(npt, 1), np.int32)
    asg, nm = self.empty(max(nk, 1), np.int32), self.empty(1, np.int32)
    fps = A.make_frame_params(fp)
    T = A.f32(Tcw).reshape(16)
    self.check(lib().lorb_track_local_map_dev(self._p, C.byref(fps), A.ptr(T, C.c_float), C.byref(k), ss, C.byref(m),
                                              C.c_float(cos_limit), C.c_float(th), iv.ptr, tr.ptr, lv.ptr, asg.ptr, nm.ptr),
               "lorb_track_local_map_dev")
    trk = tr.numpy().reshape(4, -1)[:, :npt] if npt else np.zeros((4, 0), np.float32)
    out = dict(in_view=iv.numpy()[:npt], proj_x=trk[0], proj_y=trk[1], proj_xr=trk[2], view_cos=trk[3],
               pred_level=lv.numpy()[:npt], assign=asg.numpy()[:nk], nmatches=int(nm.numpy()[0]))
    for a in keep + [iv, tr, lv, asg, nm]:
        a.free()
    return out


class _Staged:
    """Device copies of host arrays for one call (freed by close())."""

    def __init__(self, ctx):
        self.ctx, self.arrs = ctx, []

    def dev(self, a, dtype):
        if a is None:
            return None
        d = self.ctx.to_device(np.ascontiguousarray(a, dtype))
        self.arrs.append(d)
        return d.ptr

    def empty(self, shape, dtype):
        d = self.ctx.empty(shape, dtype)
        self.arrs.append(d)
        return d

    def keypoints(self, kps):
        return A.KeypointsDev(len(kps["x"]), self.dev(kps["x"], np.float32), self.dev(kps["y"], np.float32),
                              self.dev(kps["octave"], np.int32), self.dev(kps["angle"], np.float32),
                              self.dev(kps.get("u_right"), np.float32), self.dev(kps["desc"], np.uint8))

    def last_frame(self, last, keep):
        T = keep.keep(A.f32(last["Tcw"]).reshape(16))
        return A.LastFrameDev(len(last["has_mp"]), A.ptr(T, C.c_float), self.dev(last["has_mp"], np.uint8),
                              self.dev(last.get("outlier"), np.uint8), self.dev(last["mp_locked"], np.uint8),
                              self.dev(last["mp_pos"], np.float32), self.dev(last["mp_desc"], np.uint8),
                              self.dev(last["octave"], np.int32), self.dev(last["angle"], np.float32))

    def close(self):
        for a in self.arrs:
            a.free()


def _search_by_projection_frame_dev(self, fp, cur_Tcw, cur_kps, cur_slot_state, last, th):
    """lorb_search_by_projection_frame_dev on device copies of the inputs -> (assign, nmatches)."""
    keep, st = A.KeepAlive(), _Staged(self)
    try:
        k, lf = st.keypoints(cur_kps), st.last_frame(last, keep)
        ss = st.dev(cur_slot_state, np.uint8)
        asg, nm = st.empty(max(k.n, 1), np.int32), st.empty(1, np.int32)
        fps = A.make_frame_params(fp)
        T = A.f32(cur_Tcw).reshape(16)
        self.check(lib().lorb_search_by_projection_frame_dev(self._p, C.byref(fps), A.ptr(T, C.c_float), C.byref(k), ss,
                                                             C.byref(lf), C.c_float(th), asg.ptr, nm.ptr),
                   "lorb_search_by_projection_frame_dev")
        return asg.numpy()[: k.n], int(nm.numpy()[0])
    finally:
        st.close()


def _ba_pose_only_dev(self, pb, opt=None):
    """lorb_ba_pose_only_dev on device copies of the batch -> (pose, summaries)."""
    st = _Staged(self)
    try:
        nf = len(pb["res_off"]) - 1
        d = A.PoseProblemBatchDev(nf, st.dev(pb["res_off"], np.int32), st.dev(pb["intr"], np.float32),
                                  st.dev(pb["pose_init"], np.float32), st.dev(pb["pts3d"], np.float32),
                                  st.dev(pb["obs2d"], np.float32))
        opt = opt or A.LMOptions.default()
        pose, summ = st.empty((max(nf, 1), 6), np.float64), st.empty(max(nf, 1) * C.sizeof(A.BASummary), np.uint8)
        self.check(lib().lorb_ba_pose_only_dev(self._p, C.byref(d), C.byref(opt), pose.ptr, summ.ptr),
                   "lorb_ba_pose_only_dev")
        sums = (A.BASummary * max(nf, 1)).from_buffer_copy(summ.numpy().tobytes())
        return pose.numpy()[:nf], [sums[i].as_dict() for i in range(nf)]
    finally:
        st.close()


def _track_motion(self, fp, cur_Tcw, pose_init, cur_kps, slot_state, slot_pos, last, th_first=15.0, th_retry=30.0,
                  min_matches=20, fy_eff=None, opt=None, device_resident=True):
    """VisualOdometry::EstimatePoseMotion as one call (lorb_track_motion / lorb_track_motion_dev).
    device_resident=True stages the inputs in device memory first and calls the _dev form.  Returns
    assign, pass_, nmatches_first, nmatches_retry, n_residuals, pose, summary and Tcw."""
    fps = A.make_frame_params(fp)
    par = A.TrackMotionParams(th_first, th_retry, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    T = A.f32(cur_Tcw).reshape(16)
    pi = A.f32(pose_init).reshape(6)
    nk = len(cur_kps["x"])
    rec = A.TrackMotionResult()
    Tout = np.zeros((4, 4), np.float32)
    if device_resident:
        keep, st = A.KeepAlive(), _Staged(self)
        try:
            k, lf = st.keypoints(cur_kps), st.last_frame(last, keep)
            ss = st.dev(slot_state, np.uint8)
            sp = st.dev(slot_pos, np.float32) if slot_state is not None else None
            asg, drec = st.empty(max(nk, 1), np.int32), st.empty(C.sizeof(rec), np.uint8)
            self.check(lib().lorb_track_motion_dev(self._p, C.byref(fps), A.ptr(T, C.c_float), A.ptr(pi, C.c_float),
                                                   C.byref(k), ss, sp, C.byref(lf), C.byref(par), C.byref(opt), asg.ptr,
                                                   drec.ptr), "lorb_track_motion_dev")
            assign = asg.numpy()[:nk]
            rec = A.TrackMotionResult.from_buffer_copy(drec.numpy().tobytes())
        finally:
            st.close()
        rv, tv = A.f32(rec.pose[:3]), A.f32(rec.pose[3:])  # Frame::SetPose from the rounded pose
        lib().lorb_pose_to_Tcw(A.ptr(rv, C.c_float), A.ptr(tv, C.c_float), A.ptr(Tout, C.c_float))
    else:
        keep = A.KeepAlive()
        k, lf = A.make_keypoints(cur_kps, keep), A.make_last_frame(last, keep)
        ss = keep.keep(A.u8(slot_state)) if slot_state is not None else None
        sp = keep.keep(A.f32(slot_pos)) if slot_state is not None else None
        assign = np.empty(max(nk, 1), np.int32)
        self.check(lib().lorb_track_motion(self._p, C.byref(fps), A.ptr(T, C.c_float), A.ptr(pi, C.c_float), C.byref(k),
                                           A.ptr(ss, C.c_uint8), A.ptr(sp, C.c_float), C.byref(lf), C.byref(par),
                                           C.byref(opt), A.ptr(assign, C.c_int32), C.byref(rec),
                                           A.ptr(Tout, C.c_float)), "lorb_track_motion")
        assign = assign[:nk].copy()
    return dict(assign=assign, pass_=rec.pass_, nmatches_first=rec.nmatches_first, nmatches_retry=rec.nmatches_retry,
                n_residuals=rec.n_residuals, pose=np.array(rec.pose[:], np.float64), summary=rec.summary.as_dict(),
                Tcw=Tout)


def _track_local(self, fp, Tcw, pose_init, kps, slot_state, slot_pos, pts, cos_limit=0.5, th=1.0, min_matches=20,
                 fy_eff=None, device_resident=True, opt=None):
    """VisualOdometry::EstimatePoseLocal after UpdateLocalMap as one call (lorb_track_local /
    lorb_track_local_dev).  device_resident=True stages the inputs in device memory first and calls
    the _dev form.  Returns assign, in_view, proj_x, proj_y, proj_xr, view_cos, pred_level, ok,
    nmatches, n_in_view, n_residuals, pose, summary and Tcw."""
    fps = A.make_frame_params(fp)
    par = A.TrackLocalParams(cos_limit, th, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    T = A.f32(Tcw).reshape(16)
    pi = A.f32(pose_init).reshape(6)
    nk, npt = len(kps["x"]), len(pts["max_dist"])
    rec = A.TrackLocalResult()
    Tout = np.zeros((4, 4), np.float32)
    if slot_state is None:
        slot_pos = None
    if device_resident:
        st = _Staged(self)
        try:
            k = st.keypoints(kps)
            m = A.MapPointsDev(npt, st.dev(pts["pos"], np.float32), st.dev(pts["normal"], np.float32),
                               st.dev(pts["max_dist"], np.float32), st.dev(pts["min_dist"], np.float32),
                               st.dev(pts["desc"], np.uint8), st.dev(pts["locked"], np.uint8),
                               st.dev(pts.get("is_bad"), np.uint8), st.dev(pts.get("in_frame"), np.uint8))
            ss, sp = st.dev(slot_state, np.uint8), st.dev(slot_pos, np.float32)
            iv, tr, lv = (st.empty(max(npt, 1), np.uint8), st.empty((4, max(npt, 1)), np.float32),
                          st.empty(max(npt, 1), np.int32))
            asg, drec = st.empty(max(nk, 1), np.int32), st.empty(C.sizeof(rec), np.uint8)
            self.check(lib().lorb_track_local_dev(self._p, C.byref(fps), A.ptr(T, C.c_float), A.ptr(pi, C.c_float),
                                                  C.byref(k), ss, sp, C.byref(m), C.byref(par), C.byref(opt), iv.ptr,
                                                  tr.ptr, lv.ptr, asg.ptr, drec.ptr), "lorb_track_local_dev")
            assign = asg.numpy()[:nk]
            rec = A.TrackLocalResult.from_buffer_copy(drec.numpy().tobytes())
            in_view, level = iv.numpy()[:npt], lv.numpy()[:npt]
            trk = tr.numpy().reshape(4, -1)[:, :npt] if npt else np.zeros((4, 0), np.float32)
        finally:
            st.close()
        rv, tv = A.f32(rec.pose[:3]), A.f32(rec.pose[3:])  # Frame::SetPose from the rounded pose
        lib().lorb_pose_to_Tcw(A.ptr(rv, C.c_float), A.ptr(tv, C.c_float), A.ptr(Tout, C.c_float))
    else:
        keep = A.KeepAlive()

        def host(a, dtype):
            return None if a is None else keep.keep(np.ascontiguousarray(a, dtype)).ctypes.data

        k = A.make_keypoints(kps, keep)
        m = A.MapPointsDev(npt, host(pts["pos"], np.float32), host(pts["normal"], np.float32),
                           host(pts["max_dist"], np.float32), host(pts["min_dist"], np.float32),
                           host(pts["desc"], np.uint8), host(pts["locked"], np.uint8),
                           host(pts.get("is_bad"), np.uint8), host(pts.get("in_frame"), np.uint8))
        ss = keep.keep(A.u8(slot_state)) if slot_state is not None else None
        sp = keep.keep(A.f32(slot_pos)) if slot_pos is not None else None
        in_view, trk, level = (np.zeros(max(npt, 1), np.uint8), np.zeros((4, max(npt, 1)), np.float32),
                               np.zeros(max(npt, 1), np.int32))
        assign = np.empty(max(nk, 1), np.int32)
        self.check(lib().lorb_track_local(self._p, C.byref(fps), A.ptr(T, C.c_float), A.ptr(pi, C.c_float), C.byref(k),
                                          A.ptr(ss, C.c_uint8), A.ptr(sp, C.c_float), C.byref(m), C.byref(par),
                                          C.byref(opt), A.ptr(in_view, C.c_uint8), A.ptr(trk, C.c_float),
                                          A.ptr(level, C.c_int32), A.ptr(assign, C.c_int32), C.byref(rec),
                                          A.ptr(Tout, C.c_float)), "lorb_track_local")
        assign, in_view, level = assign[:nk].copy(), in_view[:npt], level[:npt]
        trk = trk[:, :npt] if npt else np.zeros((4, 0), np.float32)
    return dict(assign=assign, in_view=in_view, proj_x=trk[0], proj_y=trk[1], proj_xr=trk[2], view_cos=trk[3],
                pred_level=level, ok=rec.ok, nmatches=rec.nmatches, n_in_view=rec.n_in_view,
                n_residuals=rec.n_residuals, pose=np.array(rec.pose[:], np.float64), summary=rec.summary.as_dict(),
                Tcw=Tout)


def _compute_stereo_matches(self, fp, left, right, pyr_l, pyr_r, device_resident=False, row_pad=0, fill=255):
    """Frame::ComputeStereoMatches -> (u_right, depth).  device_resident=True stages every input in
    device memory first and calls lorb_compute_stereo_matches_dev (the async form).  row_pad > 0
    pads the rows of both pyramids (A.pack_pyramid)."""
    fps = A.make_frame_params(fp)
    n = len(left["x"])
    bl, pl = A.pack_pyramid(pyr_l, row_pad, fill)
    br, pr = A.pack_pyramid(pyr_r, row_pad, fill)
    if not device_resident:
        keep = A.KeepAlive()
        kl, kr = A.make_stereo_keys(left, keep), A.make_stereo_keys(right, keep)
        pl.data, pr.data = bl.ctypes.data, br.ctypes.data
        ur, dp = np.empty(max(n, 1), np.float32), np.empty(max(n, 1), np.float32)
        self.check(lib().lorb_compute_stereo_matches(self._p, C.byref(fps), C.byref(kl), C.byref(kr), C.byref(pl),
                                                     C.byref(pr), A.ptr(ur, C.c_float), A.ptr(dp, C.c_float)),
                   "lorb_compute_stereo_matches")
        return ur[:n].copy(), dp[:n].copy()
    keep = []

    def dev(a, dtype):
        d = self.to_device(np.ascontiguousarray(a, dtype))
        keep.append(d)
        return d.ptr

    def keys(k):
        return A.StereoKeys(len(k["x"]), dev(k["x"], np.float32), dev(k["y"], np.float32), dev(k["octave"], np.int32),
                            dev(k["desc"], np.uint8))

    kl, kr = keys(left), keys(right)
    pl.data, pr.data = dev(bl, np.uint8), dev(br, np.uint8)
    ur, dp = self.empty(max(n, 1), np.float32), self.empty(max(n, 1), np.float32)
    keep += [ur, dp]
    self.check(lib().lorb_compute_stereo_matches_dev(self._p, C.byref(fps), C.byref(kl), C.byref(kr), C.byref(pl),
                                                     C.byref(pr), ur.ptr, dp.ptr), "lorb_compute_stereo_matches_dev")
    out = ur.numpy()[:n], dp.numpy()[:n]
    for a in keep:
        a.free()
    return out


def _orb_describe(self, pyr, x, y, level, pattern, device_resident=False, row_pad=0, fill=255):
    """ORBextractor descriptor stage -> (angle, desc).  device_resident=True stages the inputs in
    device memory first and calls lorb_orb_describe_dev.  row_pad > 0 pads the pyramid's rows."""
    buf, P = A.pack_pyramid(pyr, row_pad, fill)
    x, y, level, pattern = A.f32(x), A.f32(y), A.i32(level), A.i32(pattern).reshape(-1)
    n = len(x)
    if not device_resident:
        P.data = buf.ctypes.data
        ang = np.empty(max(n, 1), np.float32)
        desc = np.empty((max(n, 1), 32), np.uint8)
        self.check(lib().lorb_orb_describe(self._p, C.byref(P), C.c_int32(n), A.ptr(x, C.c_float), A.ptr(y, C.c_float),
                                           A.ptr(level, C.c_int32), A.ptr(pattern, C.c_int32), A.ptr(ang, C.c_float),
                                           A.ptr(desc, C.c_uint8)), "lorb_orb_describe")
        return ang[:n].copy(), desc[:n].copy()
    keep = [self.to_device(a) for a in (buf, x, y, level, pattern)]
    P.data = keep[0].ptr
    ang, desc = self.empty(max(n, 1), np.float32), self.empty((max(n, 1), 32), np.uint8)
    keep += [ang, desc]
    self.check(lib().lorb_orb_describe_dev(self._p, C.byref(P), C.c_int32(n), keep[1].ptr, keep[2].ptr, keep[3].ptr,
                                           keep[4].ptr, ang.ptr, desc.ptr), "lorb_orb_describe_dev")
    out = ang.numpy()[:n], desc.numpy()[:n]
    for a in keep:
        a.free()
    return out


def _orb_fast_cells(self, pyr, ini_th=20, min_th=7, max_kp=200000, max_cells=4096, row_pad=0, fill=255):
    """FAST stage of ORBextractor::ComputeKeyPointsOctTree (src/ORBextractor.cpp:803-872): per-cell
    FAST with the empty-cell fallback.  Returns x, y, response (level coordinates) and the
    cell_base / cell_off tables.  row_pad > 0 pads the pyramid's rows."""
    buf, P = A.pack_pyramid(pyr, row_pad, fill)
    P.data = buf.ctypes.data
    x, y, r = np.zeros(max_kp, np.float32), np.zeros(max_kp, np.float32), np.zeros(max_kp, np.float32)
    base = np.zeros(len(pyr) + 1, np.int32)
    off = np.zeros(max_cells + len(pyr) + 1, np.int32)
    n = C.c_int32(0)
    self.check(lib().lorb_orb_fast_cells(self._p, C.byref(P), C.c_int32(ini_th), C.c_int32(min_th),
                                         C.c_int32(max_kp), A.ptr(x, C.c_float), A.ptr(y, C.c_float),
                                         A.ptr(r, C.c_float), C.c_int32(max_cells), A.ptr(base, C.c_int32),
                                         A.ptr(off, C.c_int32), C.byref(n)), "lorb_orb_fast_cells")
    k = n.value
    return dict(x=x[:k].copy(), y=y[:k].copy(), response=r[:k].copy(), cell_base=base,
                cell_off=off[:base[-1] + len(pyr)].copy())


def _orb_detect(self, pyr, n_desired, scale_factors, ini_th=20, min_th=7, max_kp=100000, row_pad=0, fill=255):
    """ComputeKeyPointsOctTree without orientation (src/ORBextractor.cpp:799-892): FAST cells and
    DistributeOctTree on the device.  row_pad > 0 pads the pyramid's rows."""
    buf, P = A.pack_pyramid(pyr, row_pad, fill)
    P.data = buf.ctypes.data
    nd, sf = A.i32(n_desired), A.f32(scale_factors)
    x, y, sz, r = (np.zeros(max_kp, np.float32) for _ in range(4))
    o = np.zeros(max_kp, np.int32)
    lo = np.zeros(len(pyr) + 1, np.int32)
    n = C.c_int32(0)
    self.check(lib().lorb_orb_detect(self._p, C.byref(P), A.ptr(nd, C.c_int32), A.ptr(sf, C.c_float), C.c_int32(ini_th),
                                     C.c_int32(min_th), C.c_int32(max_kp), A.ptr(x, C.c_float), A.ptr(y, C.c_float),
                                     A.ptr(o, C.c_int32), A.ptr(sz, C.c_float), A.ptr(r, C.c_float),
                                     A.ptr(lo, C.c_int32), C.byref(n)), "lorb_orb_detect")
    k = n.value
    return dict(x=x[:k].copy(), y=y[:k].copy(), octave=o[:k].copy(), size=sz[:k].copy(), response=r[:k].copy(),
                level_off=lo)


ORB_SENTINEL = 0xA5  # byte the device_resident extractor / pyramid pre-fill their device buffers with
ORB_GUARD = 64        # extra keypoint slots / pyramid bytes allocated past what was asked for


def orb_extract_capacity(rows, cols, n_desired, scale_factors):
    """lorb_orb_extract_capacity -> (max_keypoints, pyramid_bytes)."""
    nd, sf = A.i32(n_desired), A.f32(scale_factors)
    cap, pb = C.c_int32(0), C.c_int64(0)
    rc = lib().lorb_orb_extract_capacity(C.c_int32(rows), C.c_int32(cols), C.c_int32(len(sf)), A.ptr(sf, C.c_float),
                                         A.ptr(nd, C.c_int32), C.byref(cap), C.byref(pb))
    if rc != 0:
        raise LorbError(f"lorb_orb_extract_capacity failed rc={rc}")
    return cap.value, pb.value


def _orb_extract_dev(self, img, step, nd, sf, pat, ini_th, min_th, max_keypoints, pyramid_bytes):
    """lorb_orb_extract_dev on device copies of the image and pattern.  Every device output holds
    ORB_GUARD more elements than the call is told about and starts as ORB_SENTINEL bytes; the whole
    buffers come back under "raw" (and the pyramid buffer as "raw_pyramid")."""
    rows, cols = img.shape
    cap, pb = orb_extract_capacity(rows, cols, nd, sf)
    cap = cap if max_keypoints is None else max_keypoints
    pb = pb if pyramid_bytes is None else pyramid_bytes
    st = _Staged(self)
    try:
        dimg, dpat = st.dev(A.image_bytes(img), np.uint8), st.dev(pat, np.int32)
        shapes = dict(x=np.float32, y=np.float32, octave=np.int32, size=np.float32, angle=np.float32,
                      response=np.float32)

        def guarded(n, dtype):
            d = self.to_device(np.full(n * np.dtype(dtype).itemsize, ORB_SENTINEL, np.uint8).view(dtype))
            st.arrs.append(d)
            return d

        out = {k: guarded(max(cap, 0) + ORB_GUARD, dt) for k, dt in shapes.items()}
        out["desc"] = guarded((max(cap, 0) + ORB_GUARD) * 32, np.uint8)
        dpyr = guarded(max(pb, 0) + ORB_GUARD, np.uint8)
        dlo, dn = guarded(len(sf) + 1 + ORB_GUARD, np.int32), guarded(1 + ORB_GUARD, np.int32)
        self.check(lib().lorb_orb_extract_dev(
            self._p, dimg, C.c_int32(rows), C.c_int32(cols), C.c_int32(step), C.c_int32(len(sf)), A.ptr(sf, C.c_float),
            A.ptr(nd, C.c_int32), C.c_int32(ini_th), C.c_int32(min_th), dpat, C.c_int32(cap), dpyr.ptr, C.c_int64(pb),
            out["x"].ptr, out["y"].ptr, out["octave"].ptr, out["size"].ptr, out["angle"].ptr, out["response"].ptr,
            out["desc"].ptr, dlo.ptr, dn.ptr), "lorb_orb_extract_dev")
        self.sync()  # detection and description run asynchronously: d_n / d_level_off are valid only now
        n_all, lo_all = dn.numpy(), dlo.numpy()
        n = int(n_all[0])
        if n < 0:
            raise LorbError("lorb_orb_extract_dev: DistributeOctTree exceeded its node capacity (d_n = -1)")
        raw = {k: v.numpy() for k, v in out.items()}
        raw["desc"] = raw["desc"].reshape(-1, 32)
        raw["level_off"], raw["n"] = lo_all, n_all
        res = {k: raw[k][:n].copy() for k in (*shapes, "desc")}
        res.update(level_off=lo_all[:len(sf) + 1].copy(), n=n, raw=raw, raw_pyramid=dpyr.numpy(), capacity=cap,
                   pyramid_bytes=pb)
        return res
    finally:
        st.close()


def _orb_extract(self, img, n_desired, scale_factors, pattern, ini_th=20, min_th=7, max_kp=100000,
                 device_resident=False, max_keypoints=None, pyramid_bytes=None, step=None):
    """The whole ORBextractor::operator() (src/ORBextractor.cpp:1087-1151) on the device.  img may be a
    view with a row stride above its width (a padded cv::Mat); `step` overrides the stride passed on.
    device_resident=True stages image and pattern in device memory, sizes the outputs with
    lorb_orb_extract_capacity (max_keypoints / pyramid_bytes override what the call is told) and calls
    lorb_orb_extract_dev; see _orb_extract_dev for the extra keys it returns."""
    img, addr, rows, cols, stride = A.strided_image(img)
    step = stride if step is None else step
    nd, sf, pat = A.i32(n_desired), A.f32(scale_factors), A.i32(pattern).reshape(-1)
    if device_resident:
        return _orb_extract_dev(self, img, step, nd, sf, pat, ini_th, min_th, max_keypoints, pyramid_bytes)
    x, y, sz, ang, r = (np.zeros(max_kp, np.float32) for _ in range(5))
    o = np.zeros(max_kp, np.int32)
    desc = np.zeros((max_kp, 32), np.uint8)
    lo = np.zeros(len(sf) + 1, np.int32)
    n = C.c_int32(0)
    self.check(lib().lorb_orb_extract(self._p, C.cast(addr, A.u8p), C.c_int32(rows), C.c_int32(cols),
                                      C.c_int32(step), C.c_int32(len(sf)), A.ptr(sf, C.c_float),
                                      A.ptr(nd, C.c_int32), C.c_int32(ini_th), C.c_int32(min_th), A.ptr(pat, C.c_int32),
                                      C.c_int32(max_kp), A.ptr(x, C.c_float), A.ptr(y, C.c_float), A.ptr(o, C.c_int32),
                                      A.ptr(sz, C.c_float), A.ptr(ang, C.c_float), A.ptr(r, C.c_float),
                                      A.ptr(desc, C.c_uint8), A.ptr(lo, C.c_int32), C.byref(n)), "lorb_orb_extract")
    k = n.value
    return dict(x=x[:k].copy(), y=y[:k].copy(), octave=o[:k].copy(), size=sz[:k].copy(), angle=ang[:k].copy(),
                response=r[:k].copy(), desc=desc[:k].copy(), level_off=lo)


def _orb_pyramid(self, img, scale_factors, device_resident=False, step=None):
    """ORBextractor::ComputePyramid on the device -> list of level images.  img may be a view with a
    row stride above its width; `step` overrides the stride passed on.  device_resident=True stages
    the image in device memory and calls lorb_orb_pyramid_dev on a buffer of exactly the needed bytes
    (as the call is told) followed by ORB_GUARD bytes of ORB_SENTINEL, which must come back intact."""
    img, addr, rows, cols, stride = A.strided_image(img)
    step = stride if step is None else step
    sf = A.f32(scale_factors)
    total = int(sum(int(np.rint(np.float32(rows) * (np.float32(1) / s))) *
                    int(np.rint(np.float32(cols) * (np.float32(1) / s))) for s in sf))
    P = A.ImagePyramid()
    if device_resident:
        st = _Staged(self)
        try:
            dimg = st.dev(A.image_bytes(img), np.uint8)
            dout = self.to_device(np.full(total + ORB_GUARD, ORB_SENTINEL, np.uint8))
            st.arrs.append(dout)
            self.check(lib().lorb_orb_pyramid_dev(self._p, dimg, C.c_int32(rows), C.c_int32(cols), C.c_int32(step),
                                                  C.c_int32(len(sf)), A.ptr(sf, C.c_float), dout.ptr, C.c_int64(total),
                                                  C.byref(P)), "lorb_orb_pyramid_dev")
            self.sync()
            out = dout.numpy()
        finally:
            st.close()
        if not (out[total:] == ORB_SENTINEL).all():
            raise LorbError("lorb_orb_pyramid_dev wrote past the bytes it was given")
    else:
        out = np.zeros(total + 16, np.uint8)
        self.check(lib().lorb_orb_pyramid(self._p, C.cast(addr, A.u8p), C.c_int32(rows), C.c_int32(cols),
                                          C.c_int32(step), C.c_int32(len(sf)), A.ptr(sf, C.c_float),
                                          A.ptr(out, C.c_uint8), C.c_int64(len(out)), C.byref(P)), "lorb_orb_pyramid")
    return [out[P.offset[l]:P.offset[l] + P.rows[l] * P.cols[l]].reshape(P.rows[l], P.cols[l]).copy()
            for l in range(len(sf))]


Context.orb_pyramid = _orb_pyramid
Context.orb_extract = _orb_extract
Context.orb_detect = _orb_detect
Context.orb_fast_cells = _orb_fast_cells
Context.orb_describe = _orb_describe
Context.compute_stereo_matches = _compute_stereo_matches
Context.track_local_map = _track_local_map
Context.search_by_projection_frame_dev = _search_by_projection_frame_dev
Context.ba_pose_only_dev = _ba_pose_only_dev
Context.track_motion = _track_motion
Context.track_local = _track_local
Context.search_by_projection_frame = _search_by_projection_frame
Context.search_by_projection_local = _search_by_projection_local
Context.is_in_frustum = _is_in_frustum
Context.unproject_stereo = _unproject_stereo
