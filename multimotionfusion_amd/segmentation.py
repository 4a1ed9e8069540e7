"""The segmentations of Segmentation::performSegmentation on the device, over the C ABI -- no fallback: the dense CRF
(performSegmentationCRF, Core/Segmentation/Segmentation.cpp:159-740; csrc/crf_kernels.hpp) and the branch for a frame that
brings its own label image (:89-147; csrc/mask_kernels.hpp, `mask_segment`).

`segment` is the stand-alone call (per-super-pixel maps in, mask and model data out): what a sharded front end runs in
its segmentation callback on the maps of mmf_shard_gather_maps.  MultiMotionFusion.setCrfSegmentation runs the same
inside processFrame."""
import ctypes as C
from dataclasses import dataclass, fields

import torch

from ._capi import check, mmf_crf_config, mmf_crf_info, mmf_mask_config, mmf_segmentation_model
from .cudafuncs import Context, _p


@dataclass
class CrfConfig:
    """The GUI's settings (GUI/Tools/GUI.h:211-226, pushed by GUI/MainController.cpp:658-670)."""
    sigma_rgb: float = 10.0
    sigma_depth: float = 0.9
    sigma_pos: float = 1.8
    weight_appearance: float = 7.0
    weight_smoothness: float = 2.0
    threshold_new: float = 5.5
    unary_weight_error: float = 75.0
    unary_k_error: float = 0.0375
    iterations: int = 10
    min_rel_size_new: float = 0.005
    max_rel_size_new: float = 0.4
    spixel_size: int = 16
    model_spawn_offset: int = 22
    inhibit_new: int = 0

    def to_c(self):
        c = mmf_crf_config()
        for f in fields(self):
            setattr(c, f.name, getattr(self, f.name))
        return c


def model_data_dicts(arr, n):
    return [dict(id=int(arr[i].id), super_pixel_count=int(arr[i].super_pixel_count), avg_confidence=arr[i].avg_confidence,
                 depth_mean=arr[i].depth_mean, depth_std=arr[i].depth_std) for i in range(n)]


def segment(ctx: Context, rgb, depth, low_maps, ids, next_id, allow_new, cfg: CrfConfig = None, labels=None):
    """rgb [H,W,3] u8, depth [H,W] float32, low_maps [M,2,n] float32 {icp, conf} (CUDA tensors), ids = the M model ids in
    list order.  labels: int32 [H,W] super-pixel label image, or None for the regular grid.
    Returns (mask [H,W] u8 CUDA tensor, model data list of dicts, has_new_label)."""
    cfg = cfg or CrfConfig()
    H, W = depth.shape
    assert rgb.dtype == torch.uint8 and rgb.shape == (H, W, 3) and depth.dtype == torch.float32
    low_maps = low_maps.contiguous()
    assert low_maps.dtype == torch.float32 and low_maps.dim() == 3 and low_maps.shape[0] == len(ids) and low_maps.shape[1] == 2
    if labels is not None:
        assert labels.dtype == torch.int32 and labels.shape == (H, W)
        labels = labels.contiguous()
    rgb, depth = rgb.contiguous(), depth.contiguous()
    mask = torch.empty((H, W), dtype=torch.uint8, device=depth.device)
    M = len(ids)
    c_ids = (C.c_uint * M)(*[int(i) for i in ids])
    out = (mmf_segmentation_model * (M + 1))()
    n_out, has_new = C.c_int(), C.c_int()
    check(ctx.lib.mmf_crf_segment(ctx.handle, C.byref(cfg.to_c()), _p(labels) if labels is not None else None, W, H, _p(rgb),
                                  _p(depth), _p(low_maps), c_ids, M, int(next_id), int(bool(allow_new)), _p(mask), out,
                                  C.byref(n_out), C.byref(has_new)))
    return mask, model_data_dicts(out, n_out.value), bool(has_new.value)


@dataclass
class MaskConfig:
    """The settings the label-image segmentation reads inside processFrame (MultiMotionFusion.setMaskSegmentation)."""
    model_spawn_offset: int = 22
    inhibit_new: int = 0

    def to_c(self):
        c = mmf_mask_config()
        c.model_spawn_offset, c.inhibit_new = int(self.model_spawn_offset), int(self.inhibit_new)
        return c


def mask_segment(ctx: Context, labels, depth, ids, next_id, allow_new, mapping):
    """Segmentation.cpp:89-147 for one frame.  labels [H,W] u8 (arbitrary input labels, 0 = background), depth [H,W] float32
    metres (CUDA tensors); ids = the model ids in list order (ids[0] == 0); mapping = the 256-entry label -> id table as the
    frame finds it (any sequence of 256 values; not modified).
    Returns (mask [H,W] u8 CUDA tensor, model data list of dicts, has_new_label, new_label or -1, the updated table as a
    numpy uint8 array)."""
    import numpy as np
    H, W = depth.shape
    assert labels.dtype == torch.uint8 and labels.shape == (H, W) and depth.dtype == torch.float32
    labels, depth = labels.contiguous(), depth.contiguous()
    table = np.ascontiguousarray(np.asarray(mapping, np.uint8).reshape(256).copy())
    mask = torch.empty((H, W), dtype=torch.uint8, device=depth.device)
    M = len(ids)
    c_ids = (C.c_uint * max(M, 1))(*[int(i) for i in ids])
    out = (mmf_segmentation_model * (M + 1))()
    n_out, has_new, new_label = C.c_int(), C.c_int(), C.c_int()
    check(ctx.lib.mmf_mask_segment(ctx.handle, W, H, _p(labels), _p(depth), c_ids, M, int(next_id), int(bool(allow_new)),
                                   table.ctypes.data_as(C.POINTER(C.c_uint8)), _p(mask), out, C.byref(n_out), C.byref(has_new),
                                   C.byref(new_label)))
    return mask, model_data_dicts(out, n_out.value), bool(has_new.value), new_label.value, table


def _last(fn, handle, device):
    info = mmf_crf_info()
    check(fn(handle, C.byref(info), None, 0, None, None, None, None))
    L, N = info.n_labels, info.n_cells
    U = torch.empty((L, N), dtype=torch.float32, device=device)
    Q = torch.empty((L, N), dtype=torch.float32, device=device)
    raw = torch.empty(N, dtype=torch.uint8, device=device)
    low = torch.empty(N, dtype=torch.uint8, device=device)
    md = (mmf_segmentation_model * max(L, 1))()
    check(fn(handle, C.byref(info), md, L, _p(U), _p(Q), _p(raw), _p(low)))
    return dict(unaries=U, q=Q, raw_map=raw, map=low, model_data=model_data_dicts(md, info.n_models),
                allow_new=bool(info.allow_new), has_new_label=bool(info.has_new_label), range=info.range,
                range_invalid=bool(info.range_invalid), n_components=info.n_components,
                cells=(info.cells_y, info.cells_x))


def last(ctx: Context):
    """What the last segmentation on this context computed: unaries and final Q [L, n], the raw argmax map and the filtered
    map [n] (model ids, 255 = removed), the model data, allow_new, has_new_label, the depth range and the B4 flag."""
    return _last(ctx.lib.mmf_crf_last, ctx.handle, torch.device("cuda", ctx.device))
