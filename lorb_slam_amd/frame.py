"""FrameBuilder: the stereo Frame constructor (Frame::Frame(imgLeft, imgRight, camera),
src/frame.cpp:17-63) as one call of liblorb.so -- lorb_frame_builder_* / lorb_frame_build(_dev).

A builder is made once per geometry (image size, pyramid levels, features per level, thresholds,
pattern); build() then turns two images into the frame arrays the tracking chain reads."""
import ctypes as C

import numpy as np

from . import _abi as A
from .runtime import DeviceArray, LorbError, lib
from .window import ORB_GUARD, ORB_SENTINEL

SIDE_KEYS = ("x", "y", "octave", "size", "angle", "response", "desc")
_DTYPES = dict(x=np.float32, y=np.float32, octave=np.int32, size=np.float32, angle=np.float32, response=np.float32)


class DeviceFrame:
    """The device buffers of one lorb_frame_build_dev call.  Every buffer is ORB_GUARD elements longer
    than the call is told and starts as ORB_SENTINEL bytes.  left / right: dicts of DeviceArrays (x, y,
    octave, size, angle, response, desc, level_off, pyramid); u_right, depth, counts: DeviceArrays."""

    def __init__(self, ctx, cap, pyr_bytes, n_levels):
        self.ctx, self.capacity, self.pyramid_bytes, self.n_levels = ctx, cap, pyr_bytes, n_levels
        self._all = []
        self.left, self.right = self._side(), self._side()
        self.u_right, self.depth = self._guarded(cap, np.float32), self._guarded(cap, np.float32)
        self.counts = self._guarded(2, np.int32)
        self.out = A.FrameOut()
        for s, d in ((self.out.left, self.left), (self.out.right, self.right)):
            for k in (*SIDE_KEYS, "level_off", "pyramid"):
                setattr(s, k, d[k].ptr.value)
        self.out.u_right, self.out.depth, self.out.counts = self.u_right.ptr.value, self.depth.ptr.value, self.counts.ptr.value

    def _guarded(self, n, dtype, width=1):
        n = (n + ORB_GUARD) * width
        d = self.ctx.to_device(np.full(n * np.dtype(dtype).itemsize, ORB_SENTINEL, np.uint8).view(dtype))
        self._all.append(d)
        return d

    def _side(self):
        s = {k: self._guarded(self.capacity, dt) for k, dt in _DTYPES.items()}
        s["desc"] = self._guarded(self.capacity, np.uint8, 32)
        s["level_off"] = self._guarded(self.n_levels + 1, np.int32)
        s["pyramid"] = self._guarded(self.pyramid_bytes, np.uint8)
        return s

    def read_counts(self):
        """{n_left, n_right}: the only numbers that have to cross to the host (waits for the stream)."""
        self.ctx.sync()
        return self.counts.numpy()[:2].copy()

    def keypoints(self, n=None):
        """A.KeypointsDev view of the left arrays as they stand (mvKeysUn = mvKeys)."""
        n = int(self.read_counts()[0]) if n is None else n
        L = self.left
        return A.KeypointsDev(n, L["x"].ptr, L["y"].ptr, L["octave"].ptr, L["angle"].ptr, self.u_right.ptr, L["desc"].ptr)

    def free(self):
        for a in self._all:
            a.free()
        self._all = []


class DeviceSlots:
    """lorb_frame_slots of n_max entries in device memory (Frame::mvpMapPoints as the matchers see it).
    Each array is ORB_GUARD entries longer than the calls are told and starts as ORB_SENTINEL bytes
    (guard bands; an entry state of ORB_SENTINEL is no slot state, so a caller that wants EMPTY slots
    passes state=0 or an array).  state / pos / desc: host arrays of up to n_max entries to start from."""

    def __init__(self, ctx, n_max, state=None, pos=None, desc=None):
        self.ctx, self.n_max = ctx, int(n_max)
        n = self.n_max + ORB_GUARD
        hs, hp, hd = (np.full(n, ORB_SENTINEL, np.uint8), np.full(n * 12, ORB_SENTINEL, np.uint8).view(np.float32).reshape(n, 3),
                      np.full((n, 32), ORB_SENTINEL, np.uint8))
        if state is not None:
            state = np.full(self.n_max, state, np.uint8) if np.isscalar(state) else np.asarray(state, np.uint8)
            hs[:len(state)] = state
        if pos is not None:
            hp[:len(pos)] = np.asarray(pos, np.float32)
        if desc is not None:
            hd[:len(desc)] = np.asarray(desc, np.uint8)
        self.state, self.pos, self.desc = ctx.to_device(hs), ctx.to_device(hp), ctx.to_device(hd)
        self.c = A.FrameSlots(self.state.ptr.value, self.pos.ptr.value, self.desc.ptr.value)

    def numpy(self):
        """The whole guarded arrays: dict(state (n,), pos (n, 3), desc (n, 32)), n = n_max + ORB_GUARD."""
        return dict(state=self.state.numpy(), pos=self.pos.numpy(), desc=self.desc.numpy())

    def free(self):
        for a in (self.state, self.pos, self.desc):
            a.free()


def fill_slots(ctx, fp, Tcw, frame, slots, mode, n_max=None):
    """lorb_frame_slots_fill_dev on a DeviceFrame and a DeviceSlots -> n_created (waits for the stream).
    mode: A.LORB_SLOTS_UPDATE_FRAME or A.LORB_SLOTS_INITIALIZE; n_max defaults to the slots' size."""
    fps = A.make_frame_params(fp)
    T = A.f32(Tcw).reshape(16)
    made = ctx.to_device(np.full(1 + ORB_GUARD, -7, np.int32))
    try:
        ctx.check(lib().lorb_frame_slots_fill_dev(ctx.handle, C.byref(fps), A.ptr(T, C.c_float), C.byref(frame.out),
                                                  C.c_int32(slots.n_max if n_max is None else n_max), C.c_int32(mode),
                                                  C.byref(slots.c), made.ptr), "lorb_frame_slots_fill_dev")
        m = made.numpy()
        if not (m[1:] == -7).all():
            raise LorbError("lorb_frame_slots_fill_dev wrote past d_n_created")
        return int(m[0])
    finally:
        made.free()


def track_motion_frames(ctx, fp, cur_Tcw, pose_init, cur, cur_slots, last_Tcw, last, last_slots, n_max_cur=None,
                        n_max_last=None, cur_slots_given=False, last_outlier=None, th_first=15.0, th_retry=30.0,
                        min_matches=20, fy_eff=None, opt=None, assign_fill=-77):
    """lorb_track_motion_frames_dev on two DeviceFrames and their DeviceSlots: EstimatePoseMotion(pF)
    after its SetPose with both keypoint counts read on the device.  One fetch after the call brings
    back the record; returns dict(status, n_last, n_cur, n_created, the fields of Context.track_motion's
    result, assign: the whole n_max_cur + ORB_GUARD array (pre-filled with assign_fill), cur_slots and
    last_slots: DeviceSlots.numpy())."""
    fps = A.make_frame_params(fp)
    par = A.TrackMotionParams(th_first, th_retry, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    T, TL = A.f32(cur_Tcw).reshape(16), A.f32(last_Tcw).reshape(16)
    pi = A.f32(pose_init).reshape(6)
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    nl = last_slots.n_max if n_max_last is None else int(n_max_last)
    held = [ctx.to_device(np.full(max(nc, 0) + ORB_GUARD, assign_fill, np.int32)),
            ctx.to_device(np.full(C.sizeof(A.TrackFramesResult), ORB_SENTINEL, np.uint8))]
    asg, drec = held
    ol = None
    if last_outlier is not None:
        ol = ctx.to_device(A.u8(last_outlier))
        held.append(ol)
    try:
        ctx.check(lib().lorb_track_motion_frames_dev(
            ctx.handle, C.byref(fps), A.ptr(T, C.c_float), A.ptr(pi, C.c_float), C.byref(cur.out), C.c_int32(nc),
            C.byref(cur_slots.c), C.c_int32(1 if cur_slots_given else 0), A.ptr(TL, C.c_float), C.byref(last.out),
            C.c_int32(nl), C.byref(last_slots.c), ol.ptr if ol else None, C.byref(par), C.byref(opt), asg.ptr, drec.ptr),
            "lorb_track_motion_frames_dev")
        raw = drec.numpy()  # the one fetch: it waits for the stream
        rec = A.TrackFramesResult.from_buffer_copy(raw.tobytes())
        m = rec.motion
        Tout = np.zeros((4, 4), np.float32)
        if rec.status == 0:
            rv, tv = A.f32(m.pose[:3]), A.f32(m.pose[3:])  # Frame::SetPose from the rounded pose
            lib().lorb_pose_to_Tcw(A.ptr(rv, C.c_float), A.ptr(tv, C.c_float), A.ptr(Tout, C.c_float))
        return dict(status=rec.status, n_last=rec.n_last, n_cur=rec.n_cur, n_created=rec.n_created, pass_=m.pass_,
                    nmatches_first=m.nmatches_first, nmatches_retry=m.nmatches_retry, n_residuals=m.n_residuals,
                    pose=np.array(m.pose[:], np.float64), summary=m.summary.as_dict(), Tcw=Tout, record_bytes=raw,
                    assign=asg.numpy(), cur_slots=cur_slots.numpy(), last_slots=last_slots.numpy())
    finally:
        for a in held:
            a.free()


def enqueue_track_motion_frames(ctx, fp, cur_Tcw, pose_init, cur, cur_slots, last_Tcw, last, last_slots, assign, record,
                                n_max_cur=None, n_max_last=None, cur_slots_given=False, last_outlier=None, th_first=15.0,
                                th_retry=30.0, min_matches=20, fy_eff=None, opt=None):
    """lorb_track_motion_frames_dev enqueued and nothing else: assign (n_max_cur int32) and record
    (sizeof(A.TrackFramesResult) bytes) are the caller's DeviceArrays, last_outlier a DeviceArray or None.
    Nothing is fetched and nothing waits, so lorb_track_local_frames_dev can be enqueued behind it."""
    fps = A.make_frame_params(fp)
    par = A.TrackMotionParams(th_first, th_retry, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    T, TL, pi = A.f32(cur_Tcw).reshape(16), A.f32(last_Tcw).reshape(16), A.f32(pose_init).reshape(6)
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    nl = last_slots.n_max if n_max_last is None else int(n_max_last)
    ctx.check(lib().lorb_track_motion_frames_dev(
        ctx.handle, C.byref(fps), A.ptr(T, C.c_float), A.ptr(pi, C.c_float), C.byref(cur.out), C.c_int32(nc),
        C.byref(cur_slots.c), C.c_int32(1 if cur_slots_given else 0), A.ptr(TL, C.c_float), C.byref(last.out),
        C.c_int32(nl), C.byref(last_slots.c), last_outlier.ptr if last_outlier else None, C.byref(par), C.byref(opt),
        assign.ptr, record.ptr), "lorb_track_motion_frames_dev")


def motion_record_addresses(record):
    """(address of motion.pose, address of status) inside a device A.TrackFramesResult: d_pose and
    d_src_status of lorb_track_local_frames_dev in the frame chain."""
    base = record.ptr.value
    return (base + A.TrackFramesResult.motion.offset + A.TrackMotionResult.pose.offset,
            base + A.TrackFramesResult.status.offset)


class DevicePoints:
    """lorb_map_points_dev in device memory, in_frame NULL (lorb_track_local_frames_dev derives it).
    pts: dict(pos, normal, max_dist, min_dist, desc, locked, is_bad or None)."""

    def __init__(self, ctx, pts):
        self.n = len(pts["pos"])
        conv = dict(pos=A.f32, normal=A.f32, max_dist=A.f32, min_dist=A.f32, desc=A.u8, locked=A.u8, is_bad=A.u8)
        self.arrays = {k: ctx.to_device(f(pts[k])) for k, f in conv.items() if pts.get(k) is not None}
        a = self.arrays
        self.c = A.MapPointsDev(self.n, a["pos"].ptr, a["normal"].ptr, a["max_dist"].ptr, a["min_dist"].ptr, a["desc"].ptr,
                                a["locked"].ptr, a["is_bad"].ptr if "is_bad" in a else None, None)

    def free(self):
        for a in self.arrays.values():
            a.free()
        self.arrays = {}


class LocalFramesOut:
    """The device outputs of lorb_track_local_frames_dev for n_points points and a bound of n_max_cur
    keypoints: in_view, track (4 planes of n_points), level, assign and the record, each ORB_GUARD
    entries longer than the call is told.  in_view / track / level / record start as ORB_SENTINEL bytes,
    assign as assign_fill."""

    def __init__(self, ctx, n_points, n_max_cur, assign_fill=-77):
        def sent(n, dtype):
            return ctx.to_device(np.full(n * np.dtype(dtype).itemsize, ORB_SENTINEL, np.uint8).view(dtype))

        self.n_points, self.n_max_cur = int(n_points), int(n_max_cur)
        self.in_view = sent(self.n_points + ORB_GUARD, np.uint8)
        self.track = sent(4 * self.n_points + ORB_GUARD, np.float32)
        self.level = sent(self.n_points + ORB_GUARD, np.int32)
        self.assign = ctx.to_device(np.full(self.n_max_cur + ORB_GUARD, assign_fill, np.int32))
        self.record = sent(C.sizeof(A.TrackLocalFramesResult) + ORB_GUARD, np.uint8)

    def result(self):
        """The record (waits for the stream): A.TrackLocalFramesResult."""
        return A.TrackLocalFramesResult.from_buffer_copy(self.record.numpy().tobytes()[:C.sizeof(A.TrackLocalFramesResult)])

    def free(self):
        for a in (self.in_view, self.track, self.level, self.assign, self.record):
            a.free()


def track_local_frames(ctx, fp, cur, cur_slots, slot_id, d_pose, pts, out=None, n_max_cur=None, d_src_status=None,
                       id_source=None, viewing_cos_limit=0.5, th=1.0, min_matches=20, fy_eff=None, opt=None, fetch=False):
    """lorb_track_local_frames_dev on a DeviceFrame, its DeviceSlots and their ids: EstimatePoseLocal
    after UpdateLocalMap with the count, the pose and the slots read on the device.  slot_id: DeviceArray
    of n_max_cur int32; d_pose / d_src_status: device addresses (motion_record_addresses() in the frame
    chain; d_src_status may be None); pts: DevicePoints; id_source: A.TrackLocalIdSource or None; out: a
    LocalFramesOut (one is made when None: the caller frees it).  The call is only enqueued; returns
    dict(out=..., in_view, track, level, assign, record: the device buffers) and, only with fetch=True
    (which waits for the stream), result: the A.TrackLocalFramesResult."""
    fps = A.make_frame_params(fp)
    par = A.TrackLocalParams(viewing_cos_limit, th, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    made = out is None
    if made:
        out = LocalFramesOut(ctx, pts.n, max(nc, 0))
    try:
        ctx.check(lib().lorb_track_local_frames_dev(
            ctx.handle, C.byref(fps), C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c), slot_id.ptr,
            C.c_void_p(d_pose), C.c_void_p(d_src_status) if d_src_status else None,
            C.byref(id_source) if id_source is not None else None, C.byref(pts.c), C.byref(par), C.byref(opt),
            out.in_view.ptr, out.track.ptr, out.level.ptr, out.assign.ptr, out.record.ptr), "lorb_track_local_frames_dev")
    except LorbError:
        if made:
            out.free()
        raise
    r = dict(out=out, in_view=out.in_view, track=out.track, level=out.level, assign=out.assign, record=out.record)
    if fetch:
        r["result"] = out.result()
    return r


def _sentinel(ctx, n, dtype):
    return ctx.to_device(np.full(n * np.dtype(dtype).itemsize, ORB_SENTINEL, np.uint8).view(dtype))


def _guarded(ctx, a, dtype, width=1):
    """Host array a in a device buffer ORB_GUARD entries longer, the guard band ORB_SENTINEL bytes."""
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    h = np.full((len(a) + ORB_GUARD * width) * np.dtype(dtype).itemsize, ORB_SENTINEL, np.uint8).view(dtype)
    h[:len(a)] = a
    return ctx.to_device(h)


class DeviceMapStore:
    """lorb_map_store in device memory: the map as lorb_local_map_update_dev reads it.
    pts: dict(pos, normal, max_dist, min_dist, desc, locked, is_bad or None) of n_points rows;
    obs: per point the list of observing keyframe indices (MapPoint::GetObservations);
    kf_bad: Frame::IsBad per keyframe; kf_slots: per keyframe its slots' global point indices, -1 for a
    NULL slot (Frame::GetMapPoints); cov: per keyframe its ordered covisible keyframes
    (mvpOrderedKeyFrames).  Every array is ORB_GUARD entries longer than its count."""

    def __init__(self, ctx, pts, obs, kf_bad, kf_slots, cov):
        self.ctx, self.n_points, self.n_kf = ctx, len(pts["pos"]), len(kf_bad)
        if not (len(obs) == self.n_points and len(kf_slots) == len(cov) == self.n_kf):
            raise LorbError("store lists disagree with the point / keyframe counts")

        def csr(lists):
            off = np.zeros(len(lists) + 1, np.int32)
            off[1:] = np.cumsum([len(x) for x in lists])
            flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in lists]) if len(lists) else np.zeros(0, np.int32)
            return off, flat.astype(np.int32)

        (oo, ok), (so, sp), (co, ck) = csr(obs), csr(kf_slots), csr(cov)
        self.host = dict(obs_off=oo, obs_kf=ok, kf_slot_off=so, kf_slot_point=sp, cov_off=co, cov_kf=ck)
        conv = dict(pos=(np.float32, 3), normal=(np.float32, 3), max_dist=(np.float32, 1), min_dist=(np.float32, 1),
                    desc=(np.uint8, 32), locked=(np.uint8, 1), is_bad=(np.uint8, 1))
        a = self.arrays = {k: _guarded(ctx, pts[k], dt, w) for k, (dt, w) in conv.items() if pts.get(k) is not None}
        for k, v in self.host.items():
            a[k] = _guarded(ctx, v, np.int32)
        a["kf_bad"] = _guarded(ctx, kf_bad, np.uint8)
        self.c = A.MapStore(
            A.MapPointsDev(self.n_points, a["pos"].ptr, a["normal"].ptr, a["max_dist"].ptr, a["min_dist"].ptr, a["desc"].ptr,
                           a["locked"].ptr, a["is_bad"].ptr if "is_bad" in a else None, None),
            a["obs_off"].ptr, a["obs_kf"].ptr, a["kf_bad"].ptr, a["kf_slot_off"].ptr, a["kf_slot_point"].ptr,
            a["cov_off"].ptr, a["cov_kf"].ptr, self.n_kf, len(ok), len(sp), len(ck))

    def free(self):
        for a in self.arrays.values():
            a.free()
        self.arrays = {}


class DeviceArrayView(DeviceArray):
    """A DeviceArray over memory somebody else owns: free() leaves it alone."""

    def __init__(self, ctx, addr, shape, dtype):
        super().__init__(ctx, C.c_void_p(addr), shape, dtype)

    def free(self):
        pass


class LocalMap:
    """lorb_local_map: the device object lorb_local_map_update_dev fills.  points: the A.MapPointsDev
    (n = max_local) that track_local_frames takes as pts (through .c and .n, like DevicePoints); l2g,
    g2l, kf_votes, local_kf and the table columns are DeviceArray views of the object's own memory (not
    to be freed; the object gives them no guard band beyond their capacity)."""
    _COLS = dict(pos=(np.float32, 3), normal=(np.float32, 3), max_dist=(np.float32, 1), min_dist=(np.float32, 1),
                 desc=(np.uint8, 32), locked=(np.uint8, 1), is_bad=(np.uint8, 1))

    def __init__(self, ctx, max_local, max_kf, max_points):
        self.ctx = ctx
        self._p = C.c_void_p()
        ctx.check(lib().lorb_local_map_create(ctx.handle, C.c_int32(max_local), C.c_int32(max_kf), C.c_int32(max_points),
                                              C.byref(self._p)), "lorb_local_map_create")
        v = self.view = A.LocalMapArrays()
        ctx.check(lib().lorb_local_map_view(self._p, C.byref(v)), "lorb_local_map_view")
        self.max_local, self.max_kf, self.max_points = v.max_local, v.max_kf, v.max_points
        self.c, self.n = v.points, v.points.n

        def arr(addr, shape, dt):
            return DeviceArrayView(ctx, addr, shape, dt)

        self.l2g, self.g2l = arr(v.l2g, (self.max_local,), np.int32), arr(v.g2l, (self.max_points,), np.int32)
        self.kf_votes, self.local_kf = arr(v.kf_votes, (self.max_kf,), np.int32), arr(v.local_kf, (self.max_kf,), np.int32)
        self.table = {k: arr(getattr(v.points, k), (self.max_local, w) if w > 1 else (self.max_local,), dt)
                      for k, (dt, w) in self._COLS.items()}

    def fill(self, value=ORB_SENTINEL, table=True):
        """Every index array (and, with table, every table column but is_bad) set to `value` bytes:
        what a test does before a call to see afterwards what the call wrote."""
        arrays = [self.l2g, self.g2l, self.kf_votes, self.local_kf]
        arrays += [a for k, a in self.table.items() if k != "is_bad"] if table else []
        for a in arrays:
            self.ctx.check(lib().lorb_memset_dev(self.ctx.handle, a.ptr, C.c_int(value), C.c_size_t(a.nbytes)), "memset")

    def numpy(self):
        """dict of every array of the object as it stands (waits for the stream)."""
        out = dict(l2g=self.l2g.numpy(), g2l=self.g2l.numpy(), kf_votes=self.kf_votes.numpy(), local_kf=self.local_kf.numpy())
        out.update({k: a.numpy() for k, a in self.table.items()})
        return out

    def free(self):
        if self._p:
            lib().lorb_local_map_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def local_map_buffers(ctx, n_max_cur, gid=None, fill=-77):
    """(slot gids, slot local ids, record) for local_map_update: DeviceArrays of n_max_cur + ORB_GUARD
    int32 each -- gids start as `gid` (then `fill`), local ids as `fill` -- and a record of ORB_SENTINEL
    bytes with ORB_GUARD bytes behind it."""
    g = np.full(n_max_cur + ORB_GUARD, fill, np.int32)
    if gid is not None:
        g[:len(gid)] = np.asarray(gid, np.int32)
    return (ctx.to_device(g), ctx.to_device(np.full(n_max_cur + ORB_GUARD, fill, np.int32)),
            _sentinel(ctx, C.sizeof(A.LocalMapResult) + ORB_GUARD, np.uint8))


def local_map_result(record):
    """The A.LocalMapResult in a device record buffer (waits for the stream)."""
    return A.LocalMapResult.from_buffer_copy(record.numpy().tobytes()[:C.sizeof(A.LocalMapResult)])


def local_map_update(ctx, lmap, store, cur, cur_slots, slot_gid, slot_id, record, n_max_cur=None, d_src_status=None,
                     id_source=None):
    """lorb_local_map_update_dev: UpdateLocalMap on a DeviceFrame's slots, enqueued and nothing else.
    lmap: LocalMap; store: DeviceMapStore; slot_gid / slot_id / record: DeviceArrays (local_map_buffers);
    d_src_status: a device address or None; id_source: A.TrackLocalIdSource over GLOBAL ids or None.
    Returns the device address of the record's status: d_src_status of track_local_frames."""
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    ctx.check(lib().lorb_local_map_update_dev(
        ctx.handle, lmap._p, C.byref(store.c), C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c), slot_gid.ptr,
        slot_id.ptr, C.c_void_p(d_src_status) if d_src_status else None,
        C.byref(id_source) if id_source is not None else None, record.ptr), "lorb_local_map_update_dev")
    return record.ptr.value + A.LocalMapResult.status.offset


def local_map_ids_back(ctx, lmap, cur, cur_slots, slot_id, slot_gid, n_max_cur=None, d_local_status=None):
    """lorb_local_map_ids_back_dev: the slots' local rows back to global ids after the local stage
    (enqueued and nothing else).  d_local_status: a device address or None."""
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    ctx.check(lib().lorb_local_map_ids_back_dev(
        ctx.handle, lmap._p, C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c), slot_id.ptr,
        C.c_void_p(d_local_status) if d_local_status else None, slot_gid.ptr), "lorb_local_map_ids_back_dev")


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return off, np.ascontiguousarray(flat, np.int32)


def _uncsr(off, flat):
    return [[int(v) for v in flat[off[i]:off[i + 1]]] for i in range(len(off) - 1)]


class KeyframeStore:
    """lorb_kf_store: the map store as a device object that lorb_kf_store_insert_dev grows (keyframe_insert).
    init: None (empty) or dict(pos, normal, max_dist, min_dist, desc, locked, is_bad or None: n_points rows;
    obs: per point its observing keyframes; kf_bad; kf_slots: per keyframe its slots' point indices; cov: per
    keyframe its ordered covisible keyframes; conn: per keyframe {keyframe: weight}, mConnectedKeyFrameWeights).
    .c is the A.MapStore view with the host's current BOUNDS as counts -- what local_map_update takes as
    store.c; arrays: DeviceArray views of the store's own memory over its whole capacity (not to be freed).
    geom: None, or dict(kf_pose: n_kf x 6; kf_slot_uv: per keyframe its slots' (x, y); obs_slot: per point the slot
    of each observation) -- lorb_kf_store_create_geom.  geometry: the views of kf_pose, kf_slot_uv and obs_slot,
    kept apart from arrays.  life: the views of visible, found, first_fid, recent, kf_fid and the one-word
    frame_word (read_life / write_life; keyframe_observe and keyframe_cull work on them).  compact() reclaims the
    rows of dead points (lorb_kf_store_compact_dev); the views stay valid, the indices in them change.
    keyframe_retire sets kf_bad of the keyframes it is given and takes them out of every list; nothing is renumbered.
    appearance: the views of kf_slot_desc, kf_slot_octave and kf_center (read_appearance / write_appearance; a store
    made with keyframes needs write_appearance before keyframe_refresh)."""
    COUNTS =("n_kf", "n_points", "n_obs", "n_kf_slots", "n_cov", "n_conn")
    # The four groups of arrays.  host: the ctypes struct of host addresses the read / write entry points take; view:
    # the entry point that fills a struct of device addresses, and that struct; fault: write's message for an array of
    # the wrong length; cols: per column (dtype, width, the count it runs over, rows beyond that count).
    GROUPS = dict(
        main=dict(host=A.KfStoreHost, view=("lorb_kf_store_view", A.MapStore), read="lorb_kf_store_read", cols=dict(
            pos=(np.float32, 3, "n_points", 0), normal=(np.float32, 3, "n_points", 0), max_dist=(np.float32, 1, "n_points", 0),
            min_dist=(np.float32, 1, "n_points", 0), desc=(np.uint8, 32, "n_points", 0), locked=(np.uint8, 1, "n_points", 0),
            is_bad=(np.uint8, 1, "n_points", 0), obs_off=(np.int32, 1, "n_points", 1), obs_kf=(np.int32, 1, "n_obs", 0),
            kf_bad=(np.uint8, 1, "n_kf", 0), kf_slot_off=(np.int32, 1, "n_kf", 1), kf_slot_point=(np.int32, 1, "n_kf_slots", 0),
            cov_off=(np.int32, 1, "n_kf", 1), cov_kf=(np.int32, 1, "n_cov", 0), conn_off=(np.int32, 1, "n_kf", 1),
            conn_kf=(np.int32, 1, "n_conn", 0), conn_w=(np.int32, 1, "n_conn", 0))),
        geometry=dict(host=A.KfStoreGeomHost, view=("lorb_kf_store_geom_view", A.KfStoreGeomHost), read="lorb_kf_store_geom_read",
                      cols=dict(kf_pose=(np.float32, 6, "n_kf", 0), kf_slot_uv=(np.float32, 2, "n_kf_slots", 0),
                                obs_slot=(np.int32, 1, "n_obs", 0))),
        life=dict(host=A.KfStoreLifeHost, view=("lorb_kf_store_life_view", A.KfStoreLifeHost), read="lorb_kf_store_life_read",
                  write="lorb_kf_store_life_write", fault="life: {} has {} entries", cols=dict(
                      visible=(np.int32, 1, "n_points", 0), found=(np.int32, 1, "n_points", 0),
                      first_fid=(np.int32, 1, "n_points", 0), recent=(np.uint8, 1, "n_points", 0), kf_fid=(np.int32, 1, "n_kf", 0))),
        appearance=dict(host=A.KfStoreAppearHost, view=("lorb_kf_store_appear_view", A.KfStoreAppearHost),
                        read="lorb_kf_store_appear_read", write="lorb_kf_store_appear_write", fault="appearance: {} has {} rows",
                        cols=dict(kf_slot_desc=(np.uint8, 32, "n_kf_slots", 0), kf_slot_octave=(np.int32, 1, "n_kf_slots", 0),
                                  kf_center=(np.float32, 3, "n_kf", 0))))
    _COLS = tuple(k for k, (_, _, n, plus) in GROUPS["main"]["cols"].items() if n == "n_points" and not plus)  # a point's row

    def __init__(self, ctx, max_kf, max_points, max_obs, max_kf_slots, init=None, geom=None):
        self.ctx = ctx
        self._last_ba_record, self._last_ba_camera = None, None
        self.caps = A.KfStoreCaps(int(max_kf), int(max_points), int(max_obs), int(max_kf_slots))
        self.max_cov = int(max_kf) * int(max_kf)
        self._p = C.c_void_p()
        h, keep = (None, None) if init is None else self._host(init)
        if geom is None:
            ctx.check(lib().lorb_kf_store_create(ctx.handle, C.byref(self.caps), C.byref(h) if h is not None else None,
                                                 C.byref(self._p)), "lorb_kf_store_create")
        else:
            g, gkeep = self._geom_host(geom)
            ctx.check(lib().lorb_kf_store_create_geom(ctx.handle, C.byref(self.caps), C.byref(h) if h is not None else None,
                                                      C.byref(g), C.byref(self._p)), "lorb_kf_store_create_geom")
        self.arrays, self.geometry = self._views("main"), self._geometry_views()
        self.life, self.appearance = self._life_views(), self._appearance_views()

    def _views(self, group):
        """The group's view entry point (no wait): a DeviceArrayView over the whole capacity of every column the view's
        struct has (lorb_map_store keeps the point columns in .points and has no weight maps)."""
        g = self.GROUPS[group]
        v = g["view"][1]()
        self.ctx.check(getattr(lib(), g["view"][0])(self._p, C.byref(v)), g["view"][0])
        cap = dict(n_kf=self.caps.max_kf, n_points=self.caps.max_points, n_obs=self.caps.max_obs,
                   n_kf_slots=self.caps.max_kf_slots, n_cov=self.max_cov)
        at = {k: getattr(v, k, None) or getattr(getattr(v, "points", None), k, None) for k in g["cols"]}
        return {k: DeviceArrayView(self.ctx, at[k], (cap[n] + plus, w) if w > 1 else (cap[n] + plus,), dt)
                for k, (dt, w, n, plus) in g["cols"].items() if at[k]}

    def _host_struct(self, group, n, arrays):
        """The group's host struct with the counts `n` and the addresses of `arrays`."""
        T = self.GROUPS[group]["host"]
        h = T(**{f: int(n[f]) for f, _ in T._fields_ if f in n})
        for k, v in arrays.items():
            setattr(h, k, v.ctypes.data)
        return h

    def _read(self, group):
        """The group's read entry point (waits): (the six true counts, every column's true rows)."""
        g, n = self.GROUPS[group], self.counts()
        a = {k: np.zeros((n[c] + plus, w) if w > 1 else n[c] + plus, dt) for k, (dt, w, c, plus) in g["cols"].items()}
        self.ctx.check(getattr(lib(), g["read"])(self._p, C.byref(self._host_struct(group, n, a))), g["read"])
        return n, a

    def _write(self, group, src, **counts):
        """The group's write entry point (waits): the true rows replaced by every column `src` gives.  counts: the row
        counts the caller states (None: the true ones); an array must have as many rows."""
        g, n = self.GROUPS[group], self.counts()
        n.update({k: int(v) for k, v in counts.items() if v is not None})
        keep = {k: np.ascontiguousarray(src[k], dt).reshape((-1, w) if w > 1 else -1)
                for k, (dt, w, _, _) in g["cols"].items() if src.get(k) is not None}
        for k, v in keep.items():
            if len(v) != n[g["cols"][k][2]]:
                raise LorbError(g["fault"].format(k, len(v)))
        self.ctx.check(getattr(lib(), g["write"])(self._p, C.byref(self._host_struct(group, n, keep))), g["write"])

    def _fill(self, group, views, counts, value, skip=()):
        """`value` bytes in every view of the group, but those in skip, past the given true counts."""
        for k, arr in views.items():
            if k in skip:
                continue
            _, _, n, plus = self.GROUPS[group]["cols"][k]
            at = (counts[n] + plus) * (arr.nbytes // arr.shape[0])
            if at < arr.nbytes:
                self.ctx.check(lib().lorb_memset_dev(self.ctx.handle, C.c_void_p(arr.ptr.value + at), C.c_int(value),
                                                     C.c_size_t(arr.nbytes - at)), "memset")

    def _appearance_views(self):
        """lorb_kf_store_appear_view: kf_slot_desc, kf_slot_octave and kf_center over their whole capacity (no wait)."""
        return self._views("appearance")

    def _life_views(self):
        """lorb_kf_store_life_view / _frame_word_view: visible, found, first_fid, recent, kf_fid over their whole
        capacity and the one-word frame_word (no wait)."""
        out, w = self._views("life"), C.c_void_p()
        self.ctx.check(lib().lorb_kf_store_frame_word_view(self._p, C.byref(w)), "lorb_kf_store_frame_word_view")
        out["frame_word"] = DeviceArrayView(self.ctx, w.value, (1,), np.int32)
        return out

    def _geometry_views(self):
        """lorb_kf_store_geom_view: kf_pose, kf_slot_uv and obs_slot over their whole capacity (no wait)."""
        return self._views("geometry")

    @staticmethod
    def _geom_host(g):
        keep = dict(kf_pose=np.ascontiguousarray(g["kf_pose"], np.float32).reshape(-1, 6),
                    kf_slot_uv=(np.concatenate([np.asarray(r, np.float32).reshape(-1, 2) for r in g["kf_slot_uv"]])
                                if len(g["kf_slot_uv"]) else np.zeros((0, 2), np.float32)),
                    obs_slot=_csr(g["obs_slot"])[1])
        keep["kf_slot_uv"] = np.ascontiguousarray(keep["kf_slot_uv"], np.float32)
        h = A.KfStoreGeomHost(len(keep["kf_pose"]), len(keep["kf_slot_uv"]), len(keep["obs_slot"]))
        for k, a in keep.items():
            setattr(h, k, a.ctypes.data)
        h._keep = keep
        return h, keep

    @staticmethod
    def _host(s):
        n = len(s["pos"])
        cols = KeyframeStore.GROUPS["main"]["cols"]
        keep = {k: np.ascontiguousarray(s[k], cols[k][0]).reshape(-1) for k in KeyframeStore._COLS if s.get(k) is not None}
        (keep["obs_off"], keep["obs_kf"]), (keep["kf_slot_off"], keep["kf_slot_point"]) = _csr(s["obs"]), _csr(s["kf_slots"])
        keep["cov_off"], keep["cov_kf"] = _csr(s["cov"])
        conn = s.get("conn") or [{} for _ in s["kf_bad"]]
        keep["conn_off"], keep["conn_kf"] = _csr([sorted(c) for c in conn])
        keep["conn_w"] = _csr([[c[k] for k in sorted(c)] for c in conn])[1]
        keep["kf_bad"] = np.ascontiguousarray(s["kf_bad"], np.uint8)
        h = A.KfStoreHost(len(keep["kf_bad"]), n, len(keep["obs_kf"]), len(keep["kf_slot_point"]), len(keep["cov_kf"]),
                          len(keep["conn_kf"]))
        for k, a in keep.items():
            setattr(h, k, a.ctypes.data)
        h._keep = keep
        return h, keep

    def view(self):
        """lorb_kf_store_view: the A.MapStore with the host's bounds as counts (no wait)."""
        v = A.MapStore()
        self.ctx.check(lib().lorb_kf_store_view(self._p, C.byref(v)), "lorb_kf_store_view")
        return v

    @property
    def c(self):
        return self.view()

    def counts(self):
        """lorb_kf_store_counts: dict of the six true counts (waits; tightens the host's bounds)."""
        out = np.zeros(6, np.int32)
        self.ctx.check(lib().lorb_kf_store_counts(self._p, out.ctypes.data_as(C.c_void_p), C.c_int32(6)), "lorb_kf_store_counts")
        return dict(zip(self.COUNTS, (int(v) for v in out)))

    def read(self):
        """lorb_kf_store_read (waits): dict(the six counts; the point columns; obs, kf_slots, cov as lists per row;
        kf_bad; conn: per keyframe {keyframe: weight}; csr: the raw offset / index arrays)."""
        n, a = self._read("main")
        out = dict(n)
        out.update({k: a[k] for k in self._COLS})
        out.update(kf_bad=a["kf_bad"], obs=_uncsr(a["obs_off"], a["obs_kf"]), kf_slots=_uncsr(a["kf_slot_off"], a["kf_slot_point"]),
                   cov=_uncsr(a["cov_off"], a["cov_kf"]),
                   conn=[dict(zip(k, w)) for k, w in zip(_uncsr(a["conn_off"], a["conn_kf"]), _uncsr(a["conn_off"], a["conn_w"]))],
                   csr={k: a[k] for k in a if k.endswith("_off") or k in ("obs_kf", "kf_slot_point", "cov_kf", "conn_kf", "conn_w")})
        return out

    def read_geometry(self):
        """lorb_kf_store_geom_read (waits): dict(kf_pose: n_kf x 6, kf_slot_uv: n_kf_slots x 2, obs_slot: n_obs) -- the
        true rows, flat as the store keeps them."""
        return self._read("geometry")[1]

    def read_life(self):
        """lorb_kf_store_life_read (waits): dict(visible, found, first_fid, recent: n_points; kf_fid: n_kf) -- the true
        rows -- and frame_word, the id of the frame the tracker last observed."""
        a = self._read("life")[1]
        a["frame_word"] = int(self.life["frame_word"].numpy()[0])
        return a

    def write_life(self, life, n_kf=None, n_points=None):
        """lorb_kf_store_life_write (waits): replaces the true rows by every array of `life` that is given (keys of
        read_life but frame_word).  n_kf / n_points default to the true counts; they must equal them."""
        self._write("life", life, n_kf=n_kf, n_points=n_points)

    def fill_life(self, counts, value=ORB_SENTINEL):
        """fill() for the life arrays: `value` bytes past the given true counts (the frame word is left alone)."""
        self._fill("life", self.life, counts, value, skip=("frame_word",))

    def read_appearance(self):
        """lorb_kf_store_appear_read (waits): dict(kf_slot_desc: n_kf_slots x 32, kf_slot_octave: n_kf_slots, kf_center:
        n_kf x 3) -- the true rows, flat as the store keeps them."""
        return self._read("appearance")[1]

    def write_appearance(self, app, n_kf=None, n_kf_slots=None):
        """lorb_kf_store_appear_write (waits): replaces the true rows by every array of `app` that is given (keys of
        read_appearance).  n_kf / n_kf_slots default to the true counts; they must equal them.  A store created with
        keyframes has no appearance until one call has given all three."""
        self._write("appearance", app, n_kf=n_kf, n_kf_slots=n_kf_slots)

    def fill_appearance(self, counts, value=ORB_SENTINEL):
        """fill() for the appearance arrays: `value` bytes past the given true counts."""
        self._fill("appearance", self.appearance, counts, value)

    def fill_geometry(self, counts, value=ORB_SENTINEL):
        """fill() for the geometry arrays: `value` bytes past the given true counts."""
        self._fill("geometry", self.geometry, counts, value)

    def ba_window(self, result=None):
        """lorb_kf_ba_window_read (waits): the last gathered window as a dict -- local_kf, fixed_kf, l2g, pose_init,
        fixed_pose, point_init, obs_point, obs_frame, obs_uv, and intr = (fx, fy, cx, cy) of the call that gathered it:
        the dict Context.ba_local and the oracle take.
        result: that call's A.KfBaResult (default: read from the record the last keyframe_local_ba was given)."""
        r = result if result is not None else keyframe_ba_result(self._last_ba_record)
        a = dict(local_kf=np.zeros(r.n_poses, np.int32), fixed_kf=np.zeros(r.n_fixed, np.int32), l2g=np.zeros(r.n_points, np.int32),
                 pose_init=np.zeros((r.n_poses, 6), np.float32), fixed_pose=np.zeros((r.n_fixed, 6), np.float32),
                 point_init=np.zeros((r.n_points, 3), np.float32), obs_point=np.zeros(r.n_obs, np.int32),
                 obs_frame=np.zeros(r.n_obs, np.int32), obs_uv=np.zeros((r.n_obs, 2), np.float32))
        h = A.KfBaWindowHost(r.n_poses, r.n_fixed, r.n_points, r.n_obs)
        for k, v in a.items():
            setattr(h, k, v.ctypes.data)
        self.ctx.check(lib().lorb_kf_ba_window_read(self._p, C.byref(h)), "lorb_kf_ba_window_read")
        a.update(self._last_ba_camera or {})
        return a

    def fill(self, counts, value=ORB_SENTINEL):
        """Every array of the view but is_bad / kf_bad set to `value` bytes past the given true counts (a dict as
        counts() returns): what a test does before a call to see afterwards what the call wrote."""
        self._fill("main", self.arrays, counts, value, skip=("is_bad", "kf_bad"))

    def compact(self, record, tables=(), d_src_status=None, d_map=None):
        """lorb_kf_store_compact_dev enqueued and nothing else: the store's dead point rows -- bad, unobserved, named
        by no keyframe slot and no table -- are reclaimed and the survivors renumbered in their order, behind
        keyframe_local_ba and in front of the next frame's motion stage (never between a frame's local_map_update
        and its local_map_ids_back / keyframe_observe).  tables: at most A.LORB_KF_COMPACT_MAX_TABLES entries
        (slot_gid, count) or (slot_gid, count, n_max) -- a frame's gid DeviceArray and the device ADDRESS of its
        counts[0] (a DeviceFrame's out.counts) or a DeviceArray holding it; n_max defaults to the gid array's
        length.  d_src_status: a device address or None; d_map: a DeviceArray of max_points int32 or None; record: a
        device buffer for the A.KfCompactResult (keyframe_compact_record)."""
        tabs = (A.KfGidTable * max(len(tables), 1))()
        for i, tb in enumerate(tables):
            gid, count = tb[0], tb[1]
            n_max = int(tb[2]) if len(tb) > 2 else int(gid.shape[0])
            addr = count.ptr.value if hasattr(count, "ptr") else (count.value if hasattr(count, "value") else count)
            tabs[i] = A.KfGidTable(gid.ptr.value, n_max, addr)
        self.ctx.check(lib().lorb_kf_store_compact_dev(
            self.ctx.handle, self._p, C.c_void_p(d_src_status) if d_src_status else None, tabs if len(tables) else None,
            C.c_int32(len(tables)), d_map.ptr if d_map is not None else None, record.ptr), "lorb_kf_store_compact_dev")

    def free(self):
        if self._p:
            lib().lorb_kf_store_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def keyframe_insert(ctx, store, fp, cur, cur_slots, slot_gid, cur_pose, record, n_max_cur=None, d_src_status=None,
                    gate=A.LORB_KF_GATE_RATIO, refer_kf=None, update_record=None):
    """lorb_kf_store_insert_dev enqueued and nothing else: the current frame as a keyframe of a KeyframeStore --
    AddKeyFrame's gate and new points, ProcessNewFrames' observations, UpdateConnections.  cur: a DeviceFrame
    (counts[0], the left x, y, octave, desc and depth are read); cur_pose: a DeviceBlock of A.FramePose; record: a
    device buffer for the A.KfInsertResult; d_src_status: a device address or None; refer_kf: the refer_kf_word
    or None; update_record: this frame's local-map record (DeviceArray) or None."""
    fps = A.make_frame_params(fp)
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    ctx.check(lib().lorb_kf_store_insert_dev(
        ctx.handle, store._p, C.byref(fps), C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c), slot_gid.ptr, cur_pose.ptr,
        C.c_void_p(d_src_status) if d_src_status else None, C.c_int32(gate), refer_kf.ptr if refer_kf is not None else None,
        update_record.ptr if update_record is not None else None, record.ptr), "lorb_kf_store_insert_dev")


def _record(ctx, T):
    """A device buffer for a record of ctypes type T: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _sentinel(ctx, C.sizeof(T) + ORB_GUARD, np.uint8)


def _result(record, T):
    """The T in a device record buffer (waits for the stream)."""
    return T.from_buffer_copy(record.numpy().tobytes()[:C.sizeof(T)])


def keyframe_ba_record(ctx):
    """A device buffer for an A.KfBaResult: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _record(ctx, A.KfBaResult)


def keyframe_local_ba(ctx, store, fp, d_kf, record, d_src_status=None, opt=None, gather_only=False, summary=False):
    """lorb_kf_store_local_ba_dev (gather_only: lorb_kf_store_ba_gather_dev): BA::LocalPoseOptimization of the
    keyframe whose index is the device word at address d_kf, on a KeyframeStore -- the window gathered on the device,
    solved by a resident plan, the solution written back into the store's kf_pose and pos rows.  d_kf /
    d_src_status: device addresses (in the chain the kf and status words of an insertion's record); record: a
    device buffer for the A.KfBaResult (keyframe_ba_record).  summary: wait for the solve and return its summary
    dict (else None: the solve and the write-back stay enqueued)."""
    fps = A.make_frame_params(fp)
    store._last_ba_record = record
    store._last_ba_camera = dict(intr=tuple(np.float32(fp[k]) for k in ("fx", "fy", "cx", "cy")))
    src = C.c_void_p(d_src_status) if d_src_status else None
    if gather_only:
        ctx.check(lib().lorb_kf_store_ba_gather_dev(ctx.handle, store._p, C.byref(fps), C.c_void_p(d_kf), src, record.ptr),
                  "lorb_kf_store_ba_gather_dev")
        return None
    opt = opt or A.LMOptions.default()
    summ = A.BASummary() if summary else None
    ctx.check(lib().lorb_kf_store_local_ba_dev(ctx.handle, store._p, C.byref(fps), C.c_void_p(d_kf), src, C.byref(opt),
                                               record.ptr, C.byref(summ) if summ is not None else None),
              "lorb_kf_store_local_ba_dev")
    return summ.as_dict() if summ is not None else None


def keyframe_ba_result(record):
    """The A.KfBaResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfBaResult)


def keyframe_refresh_record(ctx):
    """A device buffer for an A.KfRefreshResult: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _record(ctx, A.KfRefreshResult)


def keyframe_refresh(ctx, store, fp, ba_record, record, what=A.LORB_KF_REFRESH_ALL):
    """lorb_kf_store_refresh_dev enqueued and nothing else: the camera centres of the window's keyframes, then
    UpdateNormalAndDepth and ComputeDescriptor over the points of the window the store last gathered, behind
    keyframe_local_ba (or a gather alone) and in front of KeyframeStore.compact.  fp supplies n_levels and
    scale_factors; ba_record: the device buffer that call wrote its A.KfBaResult to; what: an OR of
    A.LORB_KF_REFRESH_*; record: a device buffer for the A.KfRefreshResult (keyframe_refresh_record)."""
    fps = A.make_frame_params(fp)
    ctx.check(lib().lorb_kf_store_refresh_dev(ctx.handle, store._p, C.byref(fps), ba_record.ptr, C.c_int32(int(what)), record.ptr),
              "lorb_kf_store_refresh_dev")


def keyframe_refresh_result(record):
    """The A.KfRefreshResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfRefreshResult)


def keyframe_observe_record(ctx):
    """A device buffer for an A.KfObserveResult: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _record(ctx, A.KfObserveResult)


def keyframe_observe(ctx, store, frame_id, cur, cur_slots, slot_gid, slot_id, lmap, update_record, in_view, record,
                     n_max_cur=None, d_local_status=None, found_rule=A.LORB_KF_FOUND_NEVER):
    """lorb_kf_store_observe_dev enqueued and nothing else: the tracker's two IncreaseVisible sites on a
    KeyframeStore, behind track_local_frames and in front of local_map_ids_back.  frame_id: mCurrFrame->mnId;
    slot_gid / slot_id: the frame's gids and local rows (DeviceArrays); lmap: a LocalMap or an A.LocalMapArrays;
    update_record: the frame's local-map record; in_view: the local stage's d_in_view; d_local_status: a device
    address or None; record: a device buffer for the A.KfObserveResult."""
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    view = lmap.view if hasattr(lmap, "view") else lmap
    ctx.check(lib().lorb_kf_store_observe_dev(
        ctx.handle, store._p, C.c_int32(int(frame_id)), C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c), slot_gid.ptr,
        slot_id.ptr, C.byref(view), update_record.ptr, in_view.ptr, C.c_void_p(d_local_status) if d_local_status else None,
        C.c_int32(found_rule), record.ptr), "lorb_kf_store_observe_dev")


def keyframe_observe_result(record):
    """The A.KfObserveResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfObserveResult)


def keyframe_cull_record(ctx):
    """A device buffer for an A.KfCullResult: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _record(ctx, A.KfCullResult)


def keyframe_cull(ctx, store, d_kf, record, d_src_status=None, params=A.LORB_KF_CULL_REFERENCE, cur=None, cur_slots=None,
                  slot_gid=None, n_max_cur=None):
    """lorb_kf_store_cull_dev enqueued and nothing else: MapPointsCulling with SetBadFlag on a KeyframeStore, behind
    keyframe_insert and in front of keyframe_local_ba.  d_kf / d_src_status: device addresses (the kf and status
    words of the insertion's record); params: (min_found_ratio, age_obs, min_obs, age_out) or an A.KfCullParams;
    cur, cur_slots, slot_gid: the tracker's objects of the frame that became K, all three or none; record: a device
    buffer for the A.KfCullResult (keyframe_cull_record)."""
    par = params if isinstance(params, A.KfCullParams) else A.KfCullParams(*params)
    nc = 0 if cur_slots is None else (cur_slots.n_max if n_max_cur is None else int(n_max_cur))
    ctx.check(lib().lorb_kf_store_cull_dev(
        ctx.handle, store._p, C.c_void_p(d_kf), C.c_void_p(d_src_status) if d_src_status else None, C.byref(par),
        C.byref(cur.out) if cur is not None else None, C.c_int32(nc), C.byref(cur_slots.c) if cur_slots is not None else None,
        slot_gid.ptr if slot_gid is not None else None, record.ptr), "lorb_kf_store_cull_dev")


def keyframe_cull_result(record):
    """The A.KfCullResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfCullResult)


def keyframe_compact_record(ctx):
    """A device buffer for an A.KfCompactResult: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _record(ctx, A.KfCompactResult)


def keyframe_compact_result(record):
    """The A.KfCompactResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfCompactResult)


def keyframe_retire_record(ctx):
    """A device buffer for an A.KfRetireResult: ORB_SENTINEL bytes with ORB_GUARD bytes behind it."""
    return _record(ctx, A.KfRetireResult)


def keyframe_retire(ctx, store, d_list, d_n_list, record, n_max_list=None, protect=None, n_protect=None, d_src_status=None):
    """lorb_kf_store_retire_dev enqueued and nothing else: Frame::SetBadFlag of a set of keyframes of a KeyframeStore,
    behind keyframe_refresh and in front of KeyframeStore.compact, or anywhere between two frames.  d_list: a
    DeviceArray of int32 keyframe indices (n_max_list defaults to its length, at most A.LORB_KF_RETIRE_MAX_LIST);
    d_n_list: a DeviceArray holding the number in use, or its device address; protect: None, or a DeviceArray (or
    the device address) of up to A.LORB_KF_RETIRE_MAX_PROTECT words (n_protect defaults to the array's length) -- a listed keyframe equal to one of
    them is skipped; d_src_status: a device address or None; record: a device buffer for the A.KfRetireResult
    (keyframe_retire_record)."""
    nl = int(d_list.shape[0]) if n_max_list is None else int(n_max_list)
    npr = (0 if protect is None else int(protect.shape[0])) if n_protect is None else int(n_protect)
    p_at = None if protect is None else (protect.ptr if hasattr(protect, "ptr") else C.c_void_p(protect))
    n_at = d_n_list.ptr if hasattr(d_n_list, "ptr") else C.c_void_p(d_n_list)
    ctx.check(lib().lorb_kf_store_retire_dev(
        ctx.handle, store._p, d_list.ptr, n_at, C.c_int32(nl), p_at, C.c_int32(npr),
        C.c_void_p(d_src_status) if d_src_status else None, record.ptr), "lorb_kf_store_retire_dev")


def keyframe_retire_result(record):
    """The A.KfRetireResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfRetireResult)


def keyframe_insert_result(record):
    """The A.KfInsertResult in a device record buffer (waits for the stream)."""
    return _result(record, A.KfInsertResult)


def Tcw_to_pose(Tcw):
    """lorb_Tcw_to_pose: (rvec, tvec) float32 of a 4 x 4 pose (cv::Rodrigues matrix -> vector; host)."""
    T, r, t = A.f32(Tcw).reshape(16), np.zeros(3, np.float32), np.zeros(3, np.float32)
    if lib().lorb_Tcw_to_pose(A.ptr(T, C.c_float), A.ptr(r, C.c_float), A.ptr(t, C.c_float)) != 0:
        raise LorbError("lorb_Tcw_to_pose failed")
    return r, t


def frame_pose_from_Tcw(Tcw):
    """lorb_frame_pose_from_Tcw: Frame::SetPose(Tcw) as an A.FramePose (host)."""
    T, out = A.f32(Tcw).reshape(16), A.FramePose()
    if lib().lorb_frame_pose_from_Tcw(A.ptr(T, C.c_float), C.byref(out)) != 0:
        raise LorbError("lorb_frame_pose_from_Tcw failed")
    return out


class DeviceBlock:
    """One ctypes struct in device memory (an A.FramePose or an A.MotionModel of the frame loop) with
    ORB_GUARD bytes behind it.  value: the struct to upload; None leaves the whole buffer ORB_SENTINEL
    bytes."""

    def __init__(self, ctx, ctype, value=None):
        self.ctx, self.ctype, self.size = ctx, ctype, C.sizeof(ctype)
        h = np.full(self.size + ORB_GUARD, ORB_SENTINEL, np.uint8)
        if value is not None:
            h[:self.size] = np.frombuffer(bytes(value), np.uint8)
        self.array = ctx.to_device(h)
        self.ptr = self.array.ptr

    def upload(self, value):
        """lorb_memcpy_h2d of a struct (synchronous)."""
        b = np.frombuffer(bytes(value), np.uint8).copy()
        self.ctx.check(lib().lorb_memcpy_h2d(self.ctx.handle, self.ptr, b.ctypes.data_as(C.c_void_p), C.c_size_t(self.size)),
                       "h2d")

    def numpy(self):
        """The whole guarded buffer as bytes (waits for the stream)."""
        return self.array.numpy()

    def read(self):
        """The struct as it stands (waits for the stream)."""
        return self.ctype.from_buffer_copy(self.numpy().tobytes()[:self.size])

    def free(self):
        self.array.free()


def pose_block(ctx, Tcw=None):
    """A device lorb_frame_pose: Frame::SetPose(Tcw), or sentinel bytes (a block the chain will write)."""
    return DeviceBlock(ctx, A.FramePose, None if Tcw is None else frame_pose_from_Tcw(Tcw))


def model_block(ctx, Tcc=None):
    """A device lorb_motion_model: mTcc = Tcc with status 0, or sentinel bytes."""
    if Tcc is None:
        return DeviceBlock(ctx, A.MotionModel)
    m = A.MotionModel()
    m.Tcc[:] = [float(v) for v in A.f32(Tcc).reshape(16)]
    return DeviceBlock(ctx, A.MotionModel, m)


def enqueue_track_motion_frames_pose(ctx, fp, cur_pose, cur, cur_slots, last_pose, model, last, last_slots, assign, record,
                                     n_max_cur=None, n_max_last=None, cur_slots_given=False, last_outlier=None,
                                     th_first=15.0, th_retry=30.0, min_matches=20, fy_eff=None, opt=None):
    """lorb_track_motion_frames_pose_dev enqueued and nothing else: enqueue_track_motion_frames with the
    three poses in device memory.  cur_pose / last_pose: DeviceBlocks of A.FramePose; model: a DeviceBlock
    of A.MotionModel (the prediction runs on the device and writes cur_pose) or None (cur_pose as given)."""
    fps = A.make_frame_params(fp)
    par = A.TrackMotionParams(th_first, th_retry, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    nl = last_slots.n_max if n_max_last is None else int(n_max_last)
    ctx.check(lib().lorb_track_motion_frames_pose_dev(
        ctx.handle, C.byref(fps), cur_pose.ptr, C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c),
        C.c_int32(1 if cur_slots_given else 0), last_pose.ptr, model.ptr if model is not None else None, C.byref(last.out),
        C.c_int32(nl), C.byref(last_slots.c), last_outlier.ptr if last_outlier else None, C.byref(par), C.byref(opt),
        assign.ptr, record.ptr), "lorb_track_motion_frames_pose_dev")


def refer_kf_word(ctx, refer_kf):
    """The one-word device buffer behind d_refer_kf: a DeviceBlock of one int32 holding the keyframe index
    of mReferFrame, which the caller initialises once and lorb_track_motion_refer_pose_dev keeps current."""
    return DeviceBlock(ctx, C.c_int32, C.c_int32(int(refer_kf)))


def enqueue_track_motion_refer_pose(ctx, fp, cur_pose, cur, cur_slots, refer_pose, model, refer, refer_slots, assign, record,
                                    refer_record, first_slots_given=False, n_max_cur=None, n_max_refer=None,
                                    refer_outlier=None, last_gid=None, n_max_last=None, refer_gid=None, cur_gid=None,
                                    refer_kf=-1, kf_word=None, prev_update=None, th_first=15.0, th_retry=30.0, min_matches=20,
                                    fy_eff=None, opt=None):
    """lorb_track_motion_refer_pose_dev enqueued and nothing else: the second motion attempt on the refer
    frame, decided on the device, directly behind enqueue_track_motion_frames_pose with that call's
    cur_pose, cur_slots, model, assign and record.  refer_record: a DeviceBlock of A.TrackReferResult.
    last_gid / refer_gid / cur_gid: DeviceArrays of int32 (all three or none); kf_word (refer_kf_word) /
    prev_update (the previous frame's local-map record, a DeviceArray): both or none."""
    fps = A.make_frame_params(fp)
    par = A.TrackMotionParams(th_first, th_retry, min_matches, fps.fx if fy_eff is None else fy_eff)
    opt = opt or A.LMOptions.default()
    nc = cur_slots.n_max if n_max_cur is None else int(n_max_cur)
    nr = refer_slots.n_max if n_max_refer is None else int(n_max_refer)
    nl = nr if n_max_last is None else int(n_max_last)
    p = lambda h: h.ptr if h is not None else None  # noqa: E731
    ctx.check(lib().lorb_track_motion_refer_pose_dev(
        ctx.handle, C.byref(fps), cur_pose.ptr, C.byref(cur.out), C.c_int32(nc), C.byref(cur_slots.c),
        C.c_int32(1 if first_slots_given else 0), refer_pose.ptr, p(model), C.byref(refer.out), C.c_int32(nr),
        C.byref(refer_slots.c), p(refer_outlier), p(last_gid), C.c_int32(nl), p(refer_gid), p(cur_gid), C.c_int32(int(refer_kf)),
        p(kf_word), p(prev_update), C.byref(par), C.byref(opt), assign.ptr, record.ptr, refer_record.ptr),
        "lorb_track_motion_refer_pose_dev")


def frame_pose_finish(ctx, local_record, last_pose, cur_pose, model):
    """lorb_frame_pose_finish_dev (enqueued and nothing else): the frame's pose block and mTcc from the
    local stage's record.  local_record: the DeviceArray holding the A.TrackLocalFramesResult."""
    ctx.check(lib().lorb_frame_pose_finish_dev(ctx.handle, local_record.ptr, last_pose.ptr, cur_pose.ptr, model.ptr),
              "lorb_frame_pose_finish_dev")


class FrameBuilder:
    """lorb_frame_builder of one geometry.  fp: frame-params dict (n_levels, scale_factors, bf, b are
    read); n_desired: features per level (n_levels entries); pattern: the 256 test pairs (1024 ints)."""

    def __init__(self, ctx, fp, rows, cols, n_desired, pattern, ini_th=20, min_th=7):
        self.ctx, self.rows, self.cols = ctx, int(rows), int(cols)
        cfg = A.FrameConfig()
        cfg.rows, cfg.cols, cfg.frame = self.rows, self.cols, A.make_frame_params(fp)
        self.n_levels = cfg.frame.n_levels
        nd = A.i32(n_desired)
        if len(nd) != self.n_levels:
            raise LorbError(f"n_desired has {len(nd)} entries for {self.n_levels} levels")
        for l in range(self.n_levels):
            cfg.n_desired[l] = int(nd[l])
        cfg.ini_th, cfg.min_th = int(ini_th), int(min_th)
        pat = None if pattern is None else A.i32(pattern).reshape(-1)
        if pat is not None and pat.size != 1024:
            raise LorbError("pattern must hold 1024 ints")
        cfg.pattern = A.ptr(pat, C.c_int32)
        self._p = C.c_void_p()
        ctx.check(lib().lorb_frame_builder_create(ctx.handle, C.byref(cfg), C.byref(self._p)), "lorb_frame_builder_create")
        cap, pb = C.c_int32(0), C.c_int64(0)
        ctx.check(lib().lorb_frame_builder_capacity(self._p, C.byref(cap), C.byref(pb)), "lorb_frame_builder_capacity")
        self.capacity, self.pyramid_bytes = cap.value, pb.value

    def _images(self, left, right, step):
        out = []
        for img in (left, right):
            img, addr, rows, cols, stride = A.strided_image(img)
            if (rows, cols) != (self.rows, self.cols):
                raise LorbError(f"image is {rows} x {cols}, the builder's geometry {self.rows} x {self.cols}")
            out.append((img, addr, stride if step is None else step))
        return out

    def build_device(self, left, right, step=None):
        """lorb_frame_build_dev on device copies of the two images -> DeviceFrame (asynchronous: the
        caller reads counts, or syncs, before it looks at anything)."""
        (li, _, ls), (ri, _, rs) = self._images(left, right, step)
        dl, dr = self.ctx.to_device(A.image_bytes(li)), self.ctx.to_device(A.image_bytes(ri))
        f = DeviceFrame(self.ctx, self.capacity, self.pyramid_bytes, self.n_levels)
        f._all += [dl, dr]
        try:
            self.ctx.check(lib().lorb_frame_build_dev(self._p, dl.ptr, C.c_int32(ls), dr.ptr, C.c_int32(rs), C.byref(f.out)),
                           "lorb_frame_build_dev")
        except LorbError:
            f.free()
            raise
        return f

    def build(self, left, right, device_resident=False, step=None):
        """Two images -> dict(left, right: the extractor's keys; u_right, depth; counts).  The images may
        be views with a row stride above their width; `step` overrides the stride passed on.
        device_resident=True stages the images in device memory and calls lorb_frame_build_dev; the whole
        guarded buffers then come back under "raw" (left, right with "pyramid", u_right, depth, counts)."""
        nl = self.n_levels
        if device_resident:
            f = self.build_device(left, right, step)
            try:
                n = f.read_counts()
                if (n < 0).any():
                    raise LorbError(f"lorb_frame_build_dev: DistributeOctTree exceeded its node capacity (counts {n})")
                raw = dict(u_right=f.u_right.numpy(), depth=f.depth.numpy(), counts=f.counts.numpy())
                res = dict(counts=n, u_right=raw["u_right"][:n[0]].copy(), depth=raw["depth"][:n[0]].copy(), raw=raw,
                           capacity=self.capacity, pyramid_bytes=self.pyramid_bytes)
                for name, side, k in (("left", f.left, int(n[0])), ("right", f.right, int(n[1]))):
                    r = {key: a.numpy() for key, a in side.items()}
                    r["desc"] = r["desc"].reshape(-1, 32)
                    raw[name] = r
                    res[name] = {key: r[key][:k].copy() for key in SIDE_KEYS}
                    res[name]["level_off"] = r["level_off"][:nl + 1].copy()
                return res
            finally:
                f.free()
        (li, la, ls), (ri, ra, rs) = self._images(left, right, step)
        cap = self.capacity
        host = {}
        out = A.FrameOut()
        for name, s in (("left", out.left), ("right", out.right)):
            h = {k: np.zeros(cap, dt) for k, dt in _DTYPES.items()}
            h["desc"] = np.zeros((cap, 32), np.uint8)
            h["level_off"] = np.zeros(nl + 1, np.int32)
            for k, a in h.items():
                setattr(s, k, a.ctypes.data)
            host[name] = h
        ur, dp, cnt = np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros(2, np.int32)
        out.u_right, out.depth, out.counts = ur.ctypes.data, dp.ctypes.data, cnt.ctypes.data
        self.ctx.check(lib().lorb_frame_build(self._p, C.cast(la, A.u8p), C.c_int32(ls), C.cast(ra, A.u8p), C.c_int32(rs),
                                              C.c_int32(cap), C.byref(out)), "lorb_frame_build")
        res = dict(counts=cnt, u_right=ur[:cnt[0]].copy(), depth=dp[:cnt[0]].copy())
        for name, k in (("left", int(cnt[0])), ("right", int(cnt[1]))):
            res[name] = {key: host[name][key][:k].copy() for key in SIDE_KEYS}
            res[name]["level_off"] = host[name]["level_off"]
        return res

    def close(self):
        if self._p:
            lib().lorb_frame_builder_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
