"""FrameBuilder: the stereo Frame constructor (Frame::Frame(imgLeft, imgRight, camera),
src/frame.cpp:17-63) as one call of liblorb.so -- lorb_frame_builder_* / lorb_frame_build(_dev).

A builder is made once per geometry (image size, pyramid levels, features per level, thresholds,
pattern); build() then turns two images into the frame arrays the tracking chain reads."""
import ctypes as C

import numpy as np

from . import _abi as A
from .runtime import LorbError, lib
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
