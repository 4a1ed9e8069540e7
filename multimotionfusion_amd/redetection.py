"""Keypoint redetection of inactive models through the C ABI: the view store (all stored keypoint views of all models in
one device buffer, csrc/redetect_kernels.hpp) and Model::getBestMatch (Core/Model/Model.cpp:781-874) -- no fallback."""
import ctypes as C

import numpy as np
import torch

from ._capi import check, fptr, mmf_debug_redetect_record, mmf_redetection
from .cudafuncs import Context, _p

DIM = 256


class ViewStore:
    """views of a model = list of (descriptor [n,256] float32, coordinate [n,3] float32 in the model's frame), one entry per
    time index of the stored tracks, valid keypoints only (n may be 0)."""

    def __init__(self, ctx: Context, handle=None, owner=None):
        self.ctx, self._owner = ctx, owner  # (a borrowed store lives as long as the fusion that owns it)
        self._own = handle is None
        if handle is None:
            handle = C.c_void_p()
            check(ctx.lib.mmf_viewstore_create(ctx.handle, C.byref(handle)))
        self.handle = handle

    def store(self, model_id, views):
        """Model::store: False when the model has stored views already (nothing changes, Model.cpp:1618-1621)"""
        counts = np.array([len(d) for d, _ in views], np.int32)
        total = int(counts.sum())
        desc = np.zeros((total, DIM), np.float32)
        coord = np.zeros((total, 3), np.float32)
        o = 0
        for d, c in views:
            n = len(d)
            if n:
                desc[o:o + n], coord[o:o + n] = np.asarray(d, np.float32).reshape(n, DIM), np.asarray(c, np.float32).reshape(n, 3)
            o += n
        stored = C.c_int()
        check(self.ctx.lib.mmf_viewstore_store(self.handle, int(model_id), len(views), counts.ctypes.data, desc.ctypes.data,
                                               coord.ctypes.data, C.byref(stored)))
        return bool(stored.value)

    def storeDevice(self, model_id, counts, descriptor: torch.Tensor, coordinate: torch.Tensor):
        """store() with the views' rows on the device (DevicePointTracker.modelViewsDevice): counts [n_views] host,
        descriptor [rows,256] / coordinate [rows,3] float32 CUDA tensors, the views one after the other"""
        counts = np.ascontiguousarray(np.asarray(counts, np.int32).reshape(-1))
        rows = int(counts.sum())
        assert descriptor.is_cuda and coordinate.is_cuda and descriptor.dtype == torch.float32 and coordinate.dtype == torch.float32
        assert descriptor.shape == (rows, DIM) and coordinate.shape == (rows, 3)
        descriptor, coordinate = descriptor.contiguous(), coordinate.contiguous()
        stored = C.c_int()
        check(self.ctx.lib.mmf_viewstore_store_device(self.handle, int(model_id), counts.size, counts.ctypes.data,
                                                      _p(descriptor) if rows else None, _p(coordinate) if rows else None,
                                                      C.byref(stored)))
        return bool(stored.value)

    def forget(self, model_id):
        check(self.ctx.lib.mmf_viewstore_forget(self.handle, int(model_id)))

    def views(self):
        """[(model id, view index inside the model, valid keypoints)] in store order"""
        out = []
        m, i, r = C.c_int(), C.c_int(), C.c_int()
        for v in range(self.ctx.lib.mmf_viewstore_num_views(self.handle)):
            check(self.ctx.lib.mmf_viewstore_view(self.handle, v, C.byref(m), C.byref(i), C.byref(r)))
            out.append((m.value, i.value, r.value))
        return out

    def downloadView(self, view):
        """the rows of the view at store position `view` -> (descriptor [rows,256], coordinate [rows,3]) float32, no padding"""
        rows = C.c_int()
        check(self.ctx.lib.mmf_viewstore_view(self.handle, int(view), None, None, C.byref(rows)))
        desc, coord = np.zeros((rows.value, DIM), np.float32), np.zeros((rows.value, 3), np.float32)
        check(self.ctx.lib.mmf_viewstore_download_view(self.handle, int(view), rows.value, desc.ctypes.data, coord.ctypes.data))
        return desc, coord

    def match(self, query: torch.Tensor):
        """query [nq,256] float32 CUDA tensor against every view -> (trainIdx [views,nq] int32, -1 = unmatched; distance)"""
        assert query.dtype == torch.float32 and query.is_cuda and (query.shape[0] == 0 or query.shape[1] == DIM)
        query = query.contiguous()
        nq, nv = query.shape[0], self.ctx.lib.mmf_viewstore_num_views(self.handle)
        idx, dist = np.full((nv, nq), -1, np.int32), np.zeros((nv, nq), np.float32)
        check(self.ctx.lib.mmf_viewstore_match(self.handle, _p(query) if nq else None, nq, idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def lastLaunches(self):
        return self.ctx.lib.mmf_viewstore_last_launches(self.handle)

    def bestMatch(self, model_id, query: torch.Tensor, coordinate):
        """Model::getBestMatch(keypoints, {10, 0.03, 0.8}) -> dict(found, transformation 4x4, error, inliers, view,
        n_matches, inlier [n_matches] bool over the hash-sorted matches)"""
        assert query.dtype == torch.float32 and query.is_cuda
        query = query.contiguous()
        nq = query.shape[0]
        coord = np.ascontiguousarray(coordinate, np.float32).reshape(nq, 3)
        T = np.zeros((4, 4), np.float32)
        err, inl, view, nm, found = C.c_float(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        mask = np.zeros(max(nq, 1), np.uint8)
        check(self.ctx.lib.mmf_viewstore_best_match(self.handle, int(model_id), _p(query) if nq else None, coord.ctypes.data, nq,
                                                    T.ctypes.data, C.byref(err), C.byref(inl), C.byref(view), C.byref(nm),
                                                    mask.ctypes.data, C.byref(found)))
        return dict(found=bool(found.value), transformation=T, error=err.value, inliers=inl.value, view=view.value,
                    n_matches=nm.value, inlier=mask[:nm.value].astype(bool))

    def setVerifier(self, batch):
        """attaches a ransac.RansacBatch (None detaches it): the store then keeps its coordinates on the device as well and
        bestMatchDevice verifies there.  The batch object must outlive its attachment."""
        self._verifier = batch
        check(self.ctx.lib.mmf_viewstore_set_verifier(self.handle, batch.handle if batch is not None else None))

    def bestMatchDevice(self, model_id, query: torch.Tensor, coordinate: torch.Tensor):
        """bestMatch with the geometric verification on the device, one fresh RigidRANSAC per view: query [nq,256] and
        coordinate [nq,3] float32 CUDA tensors -> the dict of bestMatch"""
        assert query.dtype == torch.float32 and query.is_cuda and coordinate.dtype == torch.float32 and coordinate.is_cuda
        query, coordinate = query.contiguous(), coordinate.contiguous()
        nq = query.shape[0]
        assert coordinate.numel() == 3 * nq
        T = np.zeros((4, 4), np.float32)
        err, inl, view, nm, found = C.c_float(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        mask = np.zeros(max(nq, 1), np.uint8)
        check(self.ctx.lib.mmf_viewstore_best_match_device(self.handle, int(model_id), _p(query) if nq else None,
                                                           _p(coordinate) if nq else None, nq, T.ctypes.data, C.byref(err), C.byref(inl),
                                                           C.byref(view), C.byref(nm), mask.ctypes.data, C.byref(found)))
        return dict(found=bool(found.value), transformation=T, error=err.value, inliers=inl.value, view=view.value,
                    n_matches=nm.value, inlier=mask[:nm.value].astype(bool))

    def bestMatchBatch(self, sets, asked, rule):
        """the batch a frame's redetection runs (mmf_debug_viewstore_best_match_batch): sets = [(descriptor [n,256],
        coordinate [n,3])] host arrays, asked = model ids, rule 0 = host (one engine per pair) / 1 = the attached device
        verifier -> (records[s][a] = the dict of bestMatch with model_id, sets verified by the host core under rule 1)"""
        nq = np.array([len(d) for d, _ in sets], np.int32)
        rows = int(nq.sum())
        desc, coord = np.zeros((rows, DIM), np.float32), np.zeros((rows, 3), np.float32)
        o = 0
        for d, c in sets:
            n = len(d)
            if n:
                desc[o:o + n], coord[o:o + n] = np.asarray(d, np.float32).reshape(n, DIM), np.asarray(c, np.float32).reshape(n, 3)
            o += n
        ids = np.ascontiguousarray(np.asarray(asked, np.int32).reshape(-1))
        stride = max(int(nq.max()) if len(nq) else 0, 1)
        pairs = len(nq) * len(ids)
        rec = (mmf_debug_redetect_record * max(pairs, 1))()
        flags = np.zeros((max(pairs, 1), stride), np.uint8)
        host = C.c_int()
        check(self.ctx.lib.mmf_debug_viewstore_best_match_batch(self.handle, len(nq), nq.ctypes.data, desc.ctypes.data, coord.ctypes.data,
                                                                len(ids), ids.ctypes.data, int(rule), C.addressof(rec),
                                                                flags.ctypes.data, stride, C.byref(host)))
        out = []
        for s in range(len(nq)):
            row = []
            for a in range(len(ids)):
                r = rec[s * len(ids) + a]
                row.append(dict(found=bool(r.found), transformation=np.array(r.T, np.float32).reshape(4, 4), error=r.error,
                                inliers=r.inliers, view=r.view, n_matches=r.n_matches, model_id=r.model_id,
                                inlier=flags[s * len(ids) + a, :r.n_matches].astype(bool)))
            out.append(row)
        return out, host.value

    def close(self):
        if self._own and self.handle and self.ctx.handle:
            self.ctx.lib.mmf_viewstore_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_redetections(ctx, fusion_handle):
    n = C.c_int()
    check(ctx.lib.mmf_fusion_last_redetections(fusion_handle, None, 0, C.byref(n)))
    arr = (mmf_redetection * max(n.value, 1))()
    check(ctx.lib.mmf_fusion_last_redetections(fusion_handle, arr, n.value, C.byref(n)))
    return [dict(label=r.label, model_id=r.model_id, removed_id=r.removed_id, activated=bool(r.activated), error=r.error,
                 inliers=r.inliers, view=r.view, transformation=np.array(r.transformation, np.float32).reshape(4, 4))
            for r in arr[:n.value]]
