"""The blob stage of the flow_crf segmentation on the device: the host-side mirror of what the reference
does with the MAP id image of the flow-CRF inference (Core/Segmentation/Segmentation.cpp:1270-1324) -- the largest blob per
model, the filled contours, the resize, ModelData and hasNewLabel -- over the C ABI, no fallback.  The specification is the
text of DESIGN.md 4.10, the oracle tests/flowseg_oracle.py."""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import check, mmf_flowseg_config, mmf_flowseg_summary

MAX_LABELS = 32


class FlowSegConfig:
    """mmf_flowseg_config with the reference's settings as defaults; keyword arguments replace single fields"""
    FIELDS = ("div", "new_model_size", "avg_confidence", "model_spawn_offset", "inhibit_new")

    def __init__(self, **overrides):
        self.c = mmf_flowseg_config()
        check(_capi.load().mmf_flowseg_default_config(C.byref(self.c)))
        for k, v in overrides.items():
            if k not in self.FIELDS:
                raise TypeError(f"unknown FlowSegConfig field {k}")
            setattr(self.c, k, v)

    def __getattr__(self, k):
        if k in FlowSegConfig.FIELDS:
            return getattr(self.c, k)
        raise AttributeError(k)


def summary_dict(s):
    """mmf_flowseg_summary as a dict: model_data (list order, the new label's entry last if it stayed), allow_new,
    has_new_label, new_cells, and area2 / first_cell per table entry"""
    from .segmentation import model_data_dicts
    L = s.n_entries + (1 if s.allow_new and not s.has_new_label and s.n_entries > 0 else 0)
    return dict(model_data=model_data_dicts(s.models, s.n_entries), n_entries=int(s.n_entries), allow_new=bool(s.allow_new),
                has_new_label=bool(s.has_new_label), new_cells=int(s.new_cells), area2=[int(s.area2[i]) for i in range(L)],
                first_cell=[int(s.first_cell[i]) for i in range(L)])


class FlowSegmentation:
    """One engine for frames of width x height: `run(ids, depth, model_ids, ...)` takes the id image uint8 [h,w] (h =
    height / 4, w = width / 4) and the depth float32 [height,width] as CUDA tensors and the models' ids in list order, and
    returns (segm [h,w], full [height,width]) uint8 CUDA tensors (copies) and the summary dict."""

    def __init__(self, ctx, width, height, max_labels=MAX_LABELS, config=None, **overrides):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.config = config if config is not None else FlowSegConfig(**overrides)
        self.max_labels = int(max_labels)
        h = C.c_void_p()
        check(ctx.lib.mmf_flowseg_create(ctx.handle, self.width, self.height, self.max_labels, C.byref(self.config.c), C.byref(h)))
        self.handle = h
        ctx._children.append(weakref.ref(self))  # (the engine dereferences its context when destroyed)
        self.w, self.h = self.width // 4, self.height // 4
        self._keep = None

    def run(self, ids, depth, model_ids, allow_new=False, new_id=0):
        self.run_async(ids, depth, model_ids, allow_new, new_id)
        return self.result()

    def run_async(self, ids, depth, model_ids, allow_new=False, new_id=0):
        """enqueue one run on the context's stream and return; `result()` / `download()` read it"""
        import torch
        assert ids.is_cuda and ids.dtype == torch.uint8 and tuple(ids.shape) == (self.h, self.w), (ids.dtype, tuple(ids.shape))
        assert depth.is_cuda and depth.dtype == torch.float32 and tuple(depth.shape) == (self.height, self.width)
        ids, depth = ids.contiguous(), depth.contiguous()
        table = np.ascontiguousarray(model_ids, np.uint8)
        check(self.ctx.lib.mmf_flowseg_run(self.handle, ids.data_ptr(), depth.data_ptr(), table.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                           len(table), int(bool(allow_new)), int(new_id)))
        self._keep = (ids, depth)  # (the enqueued work reads them)

    def result(self):
        """(segm [h,w], full [H,W]) uint8 CUDA tensors -- copies -- and the summary dict"""
        import torch
        from .model import _as_tensor
        p_segm, p_full, s = C.c_void_p(), C.c_void_p(), mmf_flowseg_summary()
        w, h = C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_flowseg_result(self.handle, C.byref(p_segm), C.byref(p_full), C.byref(s), C.byref(w), C.byref(h)))
        segm = _as_tensor(p_segm.value, self.w * self.h, torch.uint8, (self.h, self.w), self.ctx.device, None).clone()
        full = _as_tensor(p_full.value, self.width * self.height, torch.uint8, (self.height, self.width), self.ctx.device, None).clone()
        return segm, full, summary_dict(s)

    def summary(self):
        s = mmf_flowseg_summary()
        check(self.ctx.lib.mmf_flowseg_result(self.handle, None, None, C.byref(s), None, None))
        return summary_dict(s)

    def download(self, name):
        """a stage image of the last run as a numpy array (tests): component / area2 int32 [h,w]; winner / segm uint8 [h,w];
        full uint8 [H,W]"""
        if name in ("component", "area2"):
            out = np.empty((self.h, self.w), np.int32)
        elif name == "full":
            out = np.empty((self.height, self.width), np.uint8)
        else:
            out = np.empty((self.h, self.w), np.uint8)
        check(self.ctx.lib.mmf_flowseg_download(self.handle, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def last_launches(self):
        return self.ctx.lib.mmf_flowseg_last_launches(self.handle)

    def close(self):
        if self.handle:
            self.ctx.lib.mmf_flowseg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
