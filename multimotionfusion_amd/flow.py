"""Dense optical flow after Farneback on the device: the host-side mirror of the flow stage of the
reference's flow_crf segmentation (Core/Segmentation/Segmentation.cpp:779-804: both frames scaled down by four, then
cv::calcOpticalFlowFarneback(.., 0.2, 1, 20, 2, 5, 15/50.0, 0)), over the C ABI -- no fallback.  The flow_crf mode itself
is not part of this library; parity with OpenCV's implementation is not pinned (the specification is the text of
DESIGN.md 4.8, the oracle tests/flow_oracle.py)."""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import check, mmf_flow_config


class FlowConfig:
    """mmf_flow_config with the reference's settings as defaults; keyword arguments replace single fields"""
    FIELDS = ("div", "levels", "winsize", "iterations", "poly_n", "poly_sigma")

    def __init__(self, **overrides):
        self.c = mmf_flow_config()
        check(_capi.load().mmf_flow_default_config(C.byref(self.c)))
        for k, v in overrides.items():
            if k not in self.FIELDS:
                raise TypeError(f"unknown FlowConfig field {k}")
            setattr(self.c, k, v)

    def __getattr__(self, k):
        if k in FlowConfig.FIELDS:
            return getattr(self.c, k)
        raise AttributeError(k)


def make_tables(poly_n, poly_sigma):
    """the expansion's tables for (poly_n, poly_sigma) as the library computes them (host arithmetic, no device):
    g, xg, xxg float32 [poly_n + 1] and ig float32 [4] = {ig11, ig03, ig33, ig55}"""
    n = int(poly_n)
    g, xg, xxg = (np.zeros(max(n, 0) + 1, np.float32) for _ in range(3))
    ig = np.zeros(4, np.float32)
    check(_capi.load().mmf_flow_make_tables(n, float(poly_sigma), _capi.fptr(g), _capi.fptr(xg), _capi.fptr(xxg), _capi.fptr(ig)))
    return g, xg, xxg, ig


def _result_tensors(ctx, getter, *lead):
    """(flow [h,w,2], magnitude [h,w], motion [h,w]) float32 CUDA tensors -- copies -- or None when there is no flow"""
    from .model import _as_tensor
    ptrs = [C.c_void_p() for _ in range(3)]
    w, h = C.c_int(), C.c_int()
    has = getter(*lead, *[C.byref(p) for p in ptrs], C.byref(w), C.byref(h))
    if not has:
        return None
    ctx.synchronize()  # (the copies below run on torch's stream, which need not be the context's)
    shapes = ((h.value, w.value, 2), (h.value, w.value), (h.value, w.value))
    return tuple(_as_tensor(p.value, 4 * int(np.prod(s)), _torch().float32, s, ctx.device, None).clone() for p, s in zip(ptrs, shapes))


def _torch():
    import torch
    return torch


class FarnebackFlow:
    """One engine for frames of width x height: `compute(prev, next)` for a stateless pair, `next(rgb)` for a sequence
    (the first call after creation / reset / compute returns None).  Frames are uint8 [H,W,3] CUDA tensors; the results
    are float32 CUDA tensors of the flow image's size (width / div x height / div): flow [h,w,2] = (x, y) with
    prev(y, x) ~ next(y + flow.y, x + flow.x), magnitude and motion [h,w]."""

    def __init__(self, ctx, width, height, config=None, **overrides):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.config = config if config is not None else FlowConfig(**overrides)
        h = C.c_void_p()
        check(ctx.lib.mmf_flow_create(ctx.handle, self.width, self.height, C.byref(self.config.c), C.byref(h)))
        self.handle = h
        ctx._children.append(weakref.ref(self))  # (the engine dereferences its context when destroyed)
        self.w, self.h = self.width // self.config.div, self.height // self.config.div

    def _frame(self, rgb):
        torch = _torch()
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and tuple(rgb.shape) == (self.height, self.width, 3)
        return rgb.contiguous()

    def _result(self):
        def getter(*a):
            check(self.ctx.lib.mmf_flow_result(*a))
            return True
        return _result_tensors(self.ctx, getter, self.handle)

    def compute(self, prev_rgb, next_rgb):
        a, b = self._frame(prev_rgb), self._frame(next_rgb)
        check(self.ctx.lib.mmf_flow_compute(self.handle, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())))
        return self._result()

    def next(self, rgb):
        a = self._frame(rgb)
        has = C.c_int()
        check(self.ctx.lib.mmf_flow_next(self.handle, C.c_void_p(a.data_ptr()), C.byref(has)))
        return self._result() if has.value else None

    def reset(self):
        check(self.ctx.lib.mmf_flow_reset(self.handle))

    def download(self, name):
        """a stage image as a numpy array (tests): gray / gray0 uint8 [h,w]; smooth / smooth0 / magnitude / motion float32
        [h,w]; R0 / R1 / M float32 [h,w,5]; flow_<i> float32 [h,w,2]"""
        if name in ("gray", "gray0"):
            out = np.empty((self.h, self.w), np.uint8)
        elif name in ("R0", "R1", "M"):
            out = np.empty((self.h, self.w, 5), np.float32)
        elif name.startswith("flow_"):
            out = np.empty((self.h, self.w, 2), np.float32)
        else:
            out = np.empty((self.h, self.w), np.float32)
        check(self.ctx.lib.mmf_flow_download(self.handle, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def tables(self):
        n = self.config.poly_n
        g, xg, xxg = (np.zeros(n + 1, np.float32) for _ in range(3))
        ig = np.zeros(4, np.float32)
        check(self.ctx.lib.mmf_flow_tables(self.handle, _capi.fptr(g), _capi.fptr(xg), _capi.fptr(xxg), _capi.fptr(ig)))
        return g, xg, xxg, ig

    def last_launches(self):
        return self.ctx.lib.mmf_flow_last_launches(self.handle)

    def close(self):
        if self.handle:
            self.ctx.lib.mmf_flow_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
