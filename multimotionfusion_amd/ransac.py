"""RigidRANSAC (Core/Utils/RigidRANSAC.h) through the C ABI: keypoint-based pose initialisation, host code; and the same
estimate for batches of independent problems on the device (RansacBatch) -- no fallback."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check


def _pts(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 2 and a.shape[1] == 3
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def fit(p0, p1, mask=None):
    """fit() of RigidRANSAC.cpp:73-120: least-squares T_01 (4x4) with p0 ~ T_01 p1."""
    p0, p1 = _pts(p0), _pts(p1)
    T = np.zeros((4, 4), np.float32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    check(_capi.load().mmf_rigid_fit(_ptr(p0), _ptr(p1), p0.shape[0], None if m is None else _ptr(m), _ptr(T)))
    return T


def apply(T, p0, p1):
    """apply() of RigidRANSAC.cpp:122-126: || p0 - T p1 || per row."""
    p0, p1 = _pts(p0), _pts(p1)
    T = np.ascontiguousarray(T, np.float32)
    d = np.zeros(p0.shape[0], np.float32)
    check(_capi.load().mmf_rigid_apply(_ptr(T), _ptr(p0), _ptr(p1), p0.shape[0], _ptr(d)))
    return d


class RigidRANSAC:
    """RigidRANSAC(iterations, inlier_threshold, inlier_fraction).estimate(p0, p1, mask) -> (T, error, inlier)."""

    def __init__(self, iterations, inlier_threshold, inlier_fraction):
        self.lib = _capi.load()
        h = C.c_void_p()
        check(self.lib.mmf_ransac_create(int(iterations), float(inlier_threshold), float(inlier_fraction), C.byref(h)))
        self.handle = h

    def estimate(self, p0, p1, mask=None):
        p0, p1 = _pts(p0), _pts(p1)
        n = p0.shape[0]
        T = np.zeros((4, 4), np.float32)
        err = C.c_float()
        inl = np.zeros(n, np.uint8)
        has = C.c_int()
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(self.lib.mmf_ransac_estimate(self.handle, _ptr(p0), _ptr(p1), n, None if m is None else _ptr(m), _ptr(T),
                                           C.byref(err), _ptr(inl), C.byref(has)))
        return T, err.value, (inl.astype(bool) if has.value else None)

    def __del__(self):
        try:
            if self.handle:
                self.lib.mmf_ransac_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def hash_float(x):
    """The restated std::hash<float> (csrc/rigid_ransac.hpp: hash_float_bits) beside the C++ library's: two uint64 arrays."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    a, b = np.zeros(x.size, np.uint64), np.zeros(x.size, np.uint64)
    check(_capi.load().mmf_debug_hash_float(_ptr(x), x.size, _ptr(a), _ptr(b)))
    return a, b


def core_host(iterations, inlier_threshold, inlier_fraction, p0, p1):
    """One problem through the device verifier's steps on the host (table, hash, sort, core): what a fresh
    RigidRANSAC(iterations, inlier_threshold, inlier_fraction).estimate(p0, p1) returns."""
    p0, p1 = _pts(p0), _pts(p1)
    n = p0.shape[0]
    cfg = _capi.mmf_ransac_config(int(iterations), float(inlier_threshold), float(inlier_fraction))
    T = np.zeros((4, 4), np.float32)
    err, has = C.c_float(), C.c_int()
    inl = np.zeros(n, np.uint8)
    check(_capi.load().mmf_debug_ransac_core_host(C.byref(cfg), _ptr(p0), _ptr(p1), n, _ptr(T), C.byref(err), _ptr(inl), C.byref(has)))
    return T, err.value, (inl.astype(bool) if has.value else None)


STATUS_OK, STATUS_TOO_FEW, STATUS_TOO_MANY = 0, 1, 2


class RansacBatch:
    """mmf_ransac_batch: RigidRANSAC::estimate for a ragged batch of independent problems on the device, one wave each.
    Per problem, bit for bit, what a fresh RigidRANSAC(iterations, inlier_threshold, inlier_fraction) returns without a mask."""

    def __init__(self, ctx, iterations=10, inlier_threshold=0.03, inlier_fraction=0.8, max_points=1024):
        self.ctx, self.lib = ctx, ctx.lib
        cfg = _capi.mmf_ransac_config(int(iterations), float(inlier_threshold), float(inlier_fraction))
        h = C.c_void_p()
        check(self.lib.mmf_ransac_batch_create(ctx.handle, C.byref(cfg), int(max_points), C.byref(h)))
        self.handle = h
        self.max_points = int(max_points)

    def estimate(self, p0, p1, offsets):
        """p0, p1: float32 CUDA tensors [total, 3]; offsets: n + 1 ascending ints from 0.  Returns a dict of host arrays:
        T [n, 4, 4], error [n], n_inliers [n], has_inlier [n], status [n], inlier [total] (uint8, per problem over its
        hash-sorted rows)."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        n, total = offsets.size - 1, int(offsets[-1])
        assert p0.is_cuda and p1.is_cuda and p0.dtype == p1.dtype and str(p0.dtype) == "torch.float32"
        p0, p1 = p0.contiguous(), p1.contiguous()
        assert p0.numel() == 3 * total and p1.numel() == 3 * total
        res = (_capi.mmf_ransac_result * max(n, 1))()
        inl = np.zeros(max(total, 1), np.uint8)
        check(self.lib.mmf_ransac_batch_estimate(self.handle, C.c_void_p(p0.data_ptr()) if total else None,
                                                 C.c_void_p(p1.data_ptr()) if total else None, _ptr(offsets), n, res, _ptr(inl)))
        r = np.frombuffer(res, dtype=np.dtype([("T", np.float32, (4, 4)), ("error", np.float32), ("n_inliers", np.int32),
                                               ("has_inlier", np.int32), ("status", np.int32)]))[:n]
        return {"T": r["T"].copy(), "error": r["error"].copy(), "n_inliers": r["n_inliers"].copy(),
                "has_inlier": r["has_inlier"].copy(), "status": r["status"].copy(), "inlier": inl[:total]}

    def last_launches(self):
        return self.lib.mmf_ransac_batch_last_launches(self.handle)

    def close(self):
        if self.handle:
            self.lib.mmf_ransac_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
