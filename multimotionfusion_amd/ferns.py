"""The fern keyframe database on the device: stage one of relocalisation -- ElasticFusion's randomised ferns
(Core/Ferns.{h,cpp}) up to the keyframe findFrame would hand its odometry -- over the C ABI, no fallback.  The specification is
the text of DESIGN.md 4.13, the oracle tests/ferns_oracle.py."""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import check, mmf_ferns_config, mmf_ferns_result_t

FIND, ADD = 1, 2
_ip = C.POINTER(C.c_int)


class FernsConfig:
    """mmf_ferns_config with the reference's settings as defaults; keyword arguments replace single fields"""
    FIELDS = ("num", "max_depth_mm", "capacity", "min_time_gap", "threshold", "min_similarity")

    def __init__(self, **overrides):
        self.c = mmf_ferns_config()
        check(_capi.load().mmf_ferns_default_config(C.byref(self.c)))
        for k, v in overrides.items():
            if k not in self.FIELDS:
                raise TypeError(f"unknown FernsConfig field {k}")
            setattr(self.c, k, v)

    def __getattr__(self, k):
        if k in FernsConfig.FIELDS:
            return getattr(self.c, k)
        raise AttributeError(k)


def make_table(seed, num, w, h, max_depth_mm):
    """a table of `num` ferns {x, y, t_r, t_g, t_b, t_d} (int32 [num, 6]) for w x h small images, deterministically from `seed`
    (host arithmetic, no device)"""
    out = np.zeros((max(int(num), 0), 6), np.int32)
    check(_capi.load().mmf_ferns_make_table(int(seed), int(num), int(w), int(h), int(max_depth_mm), out.ctypes.data_as(_ip)))
    return out


def _table_arg(table, num):
    table = np.ascontiguousarray(np.asarray(table, np.int32).reshape(-1, 6))
    if len(table) != num:
        raise ValueError(f"the table has {len(table)} ferns, the configuration {num}")
    return table


def result_dict(r):
    """mmf_ferns_result_t -> dict (closest_pose a float32 [16] array)"""
    out = {k: getattr(r, k) for k, _ in r._fields_ if k != "closest_pose"}
    for k in ("add_minimum", "closest_dissim", "closest_similarity"):
        out[k] = np.float32(out[k])
    out["closest_pose"] = np.array(r.closest_pose[:], np.float32)
    return out


class _Engine:
    """what FernDatabase and the fusion's hook share: an engine handle that is read from"""
    ARRAYS = {"image": (np.uint8, "px", 4), "vert": (np.float32, "px", 4), "norm": (np.float32, "px", 4), "codes": (np.uint8, "num", 0),
              "co": (np.int32, "cap", 0), "dissim": (np.float32, "cap", 0), "db_codes": (np.uint8, "cap", -1), "db_times": (np.int32, "cap", 0),
              "db_good": (np.int32, "cap", 0)}

    def __init__(self, ctx, handle, width, height, num, capacity):
        self.ctx, self.handle = ctx, handle
        self.width, self.height, self.w, self.h = int(width), int(height), int(width) // 8, int(height) // 8
        self.num, self.capacity = int(num), int(capacity)

    def result(self):
        r = mmf_ferns_result_t()
        check(self.ctx.lib.mmf_ferns_result(self.handle, C.byref(r)))
        return result_dict(r)

    def keyframe(self, index):
        """keyframe `index`: dict(image uint8 [h,w,4], vert / norm float32 [h,w,4] CUDA tensors (views into the database),
        pose float32 [4,4], time, good_codes)"""
        import torch
        from .model import _as_tensor
        p = [C.c_void_p() for _ in range(3)]
        pose = np.zeros(16, np.float32)
        time, good = C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_ferns_keyframe(self.handle, int(index), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), _capi.fptr(pose),
                                              C.byref(time), C.byref(good)))
        px = self.w * self.h
        views = [_as_tensor(q.value, px * b, dt, (self.h, self.w, 4), self.ctx.device, self)
                 for q, b, dt in zip(p, (4, 16, 16), (torch.uint8, torch.float32, torch.float32))]
        return dict(image=views[0], vert=views[1], norm=views[2], pose=pose.reshape(4, 4), time=time.value, good_codes=good.value)

    def download(self, name):
        """an array of the engine as numpy (tests): image / vert / norm [h,w,4], codes [num] (the current frame), co / dissim
        [capacity] (the last search), db_codes [capacity, num], db_times / db_good [capacity]"""
        dt, rows, tail = self.ARRAYS[name]
        n = {"px": self.w * self.h, "num": self.num, "cap": self.capacity}[rows]
        shape = (self.h, self.w, 4) if rows == "px" else ((n, self.num) if tail == -1 else (n,))
        out = np.empty(shape, dt)
        check(self.ctx.lib.mmf_ferns_download(self.handle, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def last_launches(self):
        return self.ctx.lib.mmf_ferns_last_launches(self.handle)


class FernDatabase(_Engine):
    """One database for frames of width x height.  `process(image, vert, norm, pose, time, flags)` takes a model's fill-in
    images -- uint8 [H,W,4] and float32 [H,W,4] CUDA tensors -- and is asynchronous; `result()` waits and returns the record
    as a dict.  table: int32 [num, 6], or None for make_table(seed, ...)."""

    def __init__(self, ctx, width, height, table=None, seed=0, **config):
        cfg = FernsConfig(**config)
        if table is None:
            table = make_table(seed, cfg.num, int(width) // 8, int(height) // 8, cfg.max_depth_mm)
        self.table = _table_arg(table, cfg.num)
        self.config = cfg
        h = C.c_void_p()
        check(ctx.lib.mmf_ferns_create(ctx.handle, int(width), int(height), C.byref(cfg.c), self.table.ctypes.data_as(_ip), C.byref(h)))
        super().__init__(ctx, h, width, height, cfg.num, cfg.capacity)
        ctx._children.append(weakref.ref(self))  # (the engine dereferences its context when destroyed)

    def process(self, image, vert, norm, pose, time, flags=FIND | ADD):
        import torch
        shape = (self.height, self.width, 4)
        assert image.dtype == torch.uint8 and image.is_cuda and tuple(image.shape) == shape
        for t in (vert, norm):
            assert t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == shape
        image, vert, norm = image.contiguous(), vert.contiguous(), norm.contiguous()
        pose = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        check(self.ctx.lib.mmf_ferns_process(self.handle, C.c_void_p(image.data_ptr()), C.c_void_p(vert.data_ptr()), C.c_void_p(norm.data_ptr()),
                                             _capi.fptr(pose), int(time), int(flags)))
        self._keep = (image, vert, norm)  # (until the next call: the launches read them)

    def set_threshold(self, threshold):
        check(self.ctx.lib.mmf_ferns_set_threshold(self.handle, float(threshold)))

    def reset(self):
        check(self.ctx.lib.mmf_ferns_reset(self.handle))

    def close(self):
        if self.handle:
            self.ctx.lib.mmf_ferns_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
