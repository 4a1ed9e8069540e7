"""The inference of the flow CRF on the device: the host-side mirror of the stage of the reference's
flow_crf segmentation that turns tracks, flow, depth and the models' predictions into fused label probabilities and the
MAP id image (Core/Segmentation/Segmentation.cpp:819-1263), over the C ABI -- no fallback.  What follows it in the
reference (contours, the largest blob, ModelData, hasNewLabel) is flowseg.FlowSegmentation, the flow_crf mode itself
fusion.MultiMotionFusion.setFlowSegmentation; the specification of this stage is the text of
DESIGN.md 4.9, the oracle tests/flowcrf_oracle.py."""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import check, mmf_flowcrf_config, mmf_flowcrf_input, mmf_flowcrf_tracks

MAX_LABELS = 32


class FlowCrfConfig:
    """mmf_flowcrf_config with the reference's settings as defaults; keyword arguments replace single fields"""
    FIELDS = ("div", "iterations", "weight_smoothness", "weight_appearance", "threshold", "max_err", "min_proj_prob")

    def __init__(self, **overrides):
        self.c = mmf_flowcrf_config()
        check(_capi.load().mmf_flowcrf_default_config(C.byref(self.c)))
        for k, v in overrides.items():
            if k not in self.FIELDS:
                raise TypeError(f"unknown FlowCrfConfig field {k}")
            setattr(self.c, k, v)

    def __getattr__(self, k):
        if k in FlowCrfConfig.FIELDS:
            return getattr(self.c, k)
        raise AttributeError(k)


def pad_labels(n_labels):
    """the label width an inference of n_labels labels runs at: the next power of two"""
    p = 1
    while p < n_labels:
        p *= 2
    return p


def pair_geometry(n_cells, padded_labels):
    """(nsplit, nchunk, per) of the pair pass for an image of n_cells cells at a padded label width (mmf_debug_flowcrf_pair_geometry,
    a host function): nsplit ranges of `per` chunks of 256 cells j, nchunk chunks in all"""
    nsplit, nchunk, per = C.c_int(), C.c_int(), C.c_int()
    check(_capi.load().mmf_debug_flowcrf_pair_geometry(int(n_cells), int(padded_labels), C.byref(nsplit), C.byref(nchunk), C.byref(per)))
    return nsplit.value, nchunk.value, per.value


def _torch():
    import torch
    return torch


class FlowCrf:
    """One engine for frames of width x height and the camera (fx, fy, cx, cy): `infer(...)` runs one inference and
    returns (ids [h,w], ids_full [H,W]) uint8 CUDA tensors (copies).  Every image input is a CUDA tensor: depth float32
    [H,W], vertex a list of float32 [H,W,4] (one per model), flow float32 [h,w,2], motion float32 [h,w] (the flow engine's
    results).  `tracks` is a dict of CUDA tensors xy_cur / xy_prev int32 [n,2], co_cur / co_prev float32 [n,3], ts_cur /
    ts_prev int64 [n], ok_cur / ok_prev int32 [n] -- or a Tracker, whose table is read in place -- or None."""

    def __init__(self, ctx, width, height, camera, max_labels=MAX_LABELS, max_tracks=4096, config=None, **overrides):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.config = config if config is not None else FlowCrfConfig(**overrides)
        self.max_labels, self.max_tracks = int(max_labels), int(max_tracks)
        fx, fy, cx, cy = (float(v) for v in camera)
        h = C.c_void_p()
        check(ctx.lib.mmf_flowcrf_create(ctx.handle, self.width, self.height, self.max_labels, self.max_tracks, fx, fy, cx, cy,
                                         C.byref(self.config.c), C.byref(h)))
        self.handle = h
        ctx._children.append(weakref.ref(self))  # (the engine dereferences its context when destroyed)
        self.w, self.h = self.width // 4, self.height // 4
        self.n_labels = self.n_models = 0
        self._keep = None

    def infer(self, ids, T_start, T_end, vertex, depth, flow, motion, tracks=None, allow_new=False, new_id=0):
        self.infer_async(ids, T_start, T_end, vertex, depth, flow, motion, tracks, allow_new, new_id)
        return self.result()

    def infer_async(self, ids, T_start, T_end, vertex, depth, flow, motion, tracks=None, allow_new=False, new_id=0):
        """enqueue one inference on the context's stream and return; `result()` / `download()` read it"""
        torch = _torch()
        M = len(ids)
        H, W, h, w = self.height, self.width, self.h, self.w

        def dev(t, dtype, shape):
            assert t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape, (t.dtype, tuple(t.shape), dtype, shape)
            return t.contiguous()

        vertex = [dev(v, torch.float32, (H, W, 4)) for v in vertex]
        assert len(vertex) == M
        depth, flow, motion = dev(depth, torch.float32, (H, W)), dev(flow, torch.float32, (h, w, 2)), dev(motion, torch.float32, (h, w))
        ids_a = np.ascontiguousarray(ids, np.uint8)
        Ts = np.ascontiguousarray(np.asarray(T_start, np.float32).reshape(M, 16))
        Te = np.ascontiguousarray(np.asarray(T_end, np.float32).reshape(M, 16))
        vp = (C.c_void_p * max(M, 1))(*[v.data_ptr() for v in vertex])
        inp = mmf_flowcrf_input(M, int(bool(allow_new)), int(new_id), ids_a.ctypes.data_as(C.POINTER(C.c_ubyte)), _capi.fptr(Ts),
                                _capi.fptr(Te), C.cast(vp, C.POINTER(C.c_void_p)), depth.data_ptr(), flow.data_ptr(), motion.data_ptr())
        keep = [vertex, depth, flow, motion]
        if tracks is None or isinstance(tracks, dict):
            tr = None
            if tracks is not None:
                n = int(tracks["ts_cur"].shape[0])
                t = {}
                for s in ("cur", "prev"):
                    t["xy_" + s] = dev(tracks["xy_" + s], torch.int32, (n, 2))
                    t["co_" + s] = dev(tracks["co_" + s], torch.float32, (n, 3))
                    t["ts_" + s] = dev(tracks["ts_" + s], torch.int64, (n,))
                    t["ok_" + s] = dev(tracks["ok_" + s], torch.int32, (n,))
                keep.append(t)
                tr = mmf_flowcrf_tracks(*[t[k + s].data_ptr() for s in ("_cur", "_prev") for k in ("xy", "co", "ts", "ok")], n)
            check(self.ctx.lib.mmf_flowcrf_infer(self.handle, C.byref(inp), C.byref(tr) if tr is not None else None))
        else:
            check(self.ctx.lib.mmf_flowcrf_infer_tracker(self.handle, C.byref(inp), tracks.handle))
        self._keep = keep  # (the enqueued work reads them)
        self.n_models, self.n_labels = M, M + int(bool(allow_new))

    def result(self):
        """(ids [h,w], ids_full [H,W]) uint8 CUDA tensors -- copies"""
        from .model import _as_tensor
        torch = _torch()
        p_ids, p_full, p_prob, p_q = (C.c_void_p() for _ in range(4))
        w, h, L = C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_flowcrf_result(self.handle, C.byref(p_ids), C.byref(p_full), C.byref(p_prob), C.byref(p_q), C.byref(w),
                                              C.byref(h), C.byref(L)))
        self.ctx.synchronize()  # (the copies below run on torch's stream, which need not be the context's)
        ids = _as_tensor(p_ids.value, h.value * w.value, torch.uint8, (h.value, w.value), self.ctx.device, None).clone()
        full = _as_tensor(p_full.value, self.width * self.height, torch.uint8, (self.height, self.width), self.ctx.device, None).clone()
        return ids, full

    def download(self, name):
        """a stage image of the last inference as a numpy array (tests): E / U / proj / Q / prob float32 [L,h,w]; label int32
        [h,w]; ids / invalid uint8 [h,w]; ids_full uint8 [H,W]; cell int32 [M,max_tracks]"""
        L = self.n_labels
        if name in ("E", "U", "proj", "Q", "prob"):
            out = np.empty((L, self.h, self.w), np.float32)
        elif name == "label":
            out = np.empty((self.h, self.w), np.int32)
        elif name == "ids_full":
            out = np.empty((self.height, self.width), np.uint8)
        elif name == "cell":
            out = np.empty((self.n_models, max(self.max_tracks, 1)), np.int32)
        else:
            out = np.empty((self.h, self.w), np.uint8)
        check(self.ctx.lib.mmf_flowcrf_download(self.handle, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def last_launches(self):
        return self.ctx.lib.mmf_flowcrf_last_launches(self.handle)

    def close(self):
        if self.handle:
            self.ctx.lib.mmf_flowcrf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
