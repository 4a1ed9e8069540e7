"""The keypoint track table on the device (mmf_tracker_*, csrc/tracker_kernels.hpp): tracker::PointTracker
(Core/Utils/PointTracker.cpp:27-226), the per-model track sets and Model::getLastTrackTransform (Core/Model/Model.cpp:739-775)
without host bookkeeping, and the `-init kp` front end on top of it -- no fallback.

point_tracker.py keeps the host-side mirror of the same classes (lists like the reference's); the two agree bit for bit
where the table's capacity is not reached."""
import ctypes as C
import weakref

import numpy as np
import torch

from ._capi import check, mmf_backdated_pose, mmf_ransac_config
from .cudafuncs import Context, _p


def backdated_pose_dict(e):
    """one mmf_backdated_pose as a dict of plain values and float32 [4,4] arrays"""
    return dict(stamp=e.stamp, timestamp=e.timestamp, **{"from": e.from_}, both=e.both, nvalid=e.nvalid, status=e.status,
                host_estimated=e.host_estimated, error=np.float32(e.error), n_inliers=e.n_inliers,
                T=np.array(e.T, np.float32).reshape(4, 4), pose=np.array(e.pose, np.float32).reshape(4, 4))


class DevicePointTracker:
    """tracker::PointTracker for pyramid level 0 with the tracks on the device.  Differences from the reference: at most
    `capacity` tracks (appends that do not fit are dropped and counted), NaN coordinates for a keypoint outside the image."""

    def __init__(self, ctx: Context, width, height, intrinsics, capacity=4096, max_keypoints=1024):
        """intrinsics: (fx, fy, cx, cy) of level 0"""
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.capacity, self.max_keypoints = int(capacity), int(max_keypoints)
        fx, fy, cx, cy = (float(v) for v in intrinsics)
        h = C.c_void_p()
        check(ctx.lib.mmf_tracker_create(ctx.handle, self.width, self.height, fx, fy, cx, cy, self.capacity, self.max_keypoints,
                                         C.byref(h)))
        self.handle = h
        self._dev = torch.device("cuda", ctx.device)
        ctx._children.append(weakref.ref(self))

    # ----- PointTracker
    def pixels(self, coordinates):
        """normalised keypoint coordinates [n,2] -> integer pixels, cv::Point(cv::Vec2d): round half to even (:38)"""
        c = np.asarray(coordinates, np.float64).reshape(-1, 2)
        return np.rint(c * np.array([self.width, self.height], np.float64)).astype(np.int32)

    def addKeypoints(self, coordinates, descriptors, timestamp, depth, min_feature_distance=0.7, history=30):
        """coordinates [n,2] normalised to [0,1) (host), descriptors [n,256] (host or CUDA tensor), depth [rows,cols] float32
        CUDA tensor"""
        self.addKeypointsPixels(self.pixels(coordinates), descriptors, timestamp, depth, min_feature_distance, history)

    def addKeypointsPixels(self, xy, descriptors, timestamp, depth, min_feature_distance=0.7, history=30):
        """xy [n,2] integer pixels (host array or int32 CUDA tensor)"""
        if not torch.is_tensor(xy):
            xy = torch.from_numpy(np.ascontiguousarray(xy, np.int32).reshape(-1, 2))
        if not torch.is_tensor(descriptors):
            descriptors = torch.from_numpy(np.ascontiguousarray(descriptors, np.float32))
        xy = xy.to(self._dev, torch.int32).contiguous()
        n = xy.shape[0]
        de = descriptors.to(self._dev, torch.float32).reshape(n, 256).contiguous()
        assert depth.is_cuda and depth.dtype == torch.float32 and depth.shape == (self.height, self.width)
        depth = depth.contiguous()
        check(self.ctx.lib.mmf_tracker_add_keypoints(self.handle, n, _p(xy) if n else None, _p(de) if n else None, _p(depth),
                                                     int(timestamp), float(min_feature_distance), int(history)))

    def addKeypointsDevice(self, n_dev, xy, descriptors, timestamp, depth, min_feature_distance=0.7, history=30):
        """addKeypointsPixels with the number of keypoints on the device and no wait.  n_dev: int32 CUDA tensor (its first
        element) or a device address; xy [max_keypoints,2] int32 / descriptors [max_keypoints,256] float32 CUDA tensors or
        device addresses (superpoint.SuperPoint.deviceFeatures) whose rows from n on may hold anything."""
        assert depth.is_cuda and depth.dtype == torch.float32 and depth.shape == (self.height, self.width) and depth.is_contiguous()
        for a, dt in ((n_dev, torch.int32), (xy, torch.int32), (descriptors, torch.float32)):
            assert not torch.is_tensor(a) or (a.is_cuda and a.dtype == dt and a.is_contiguous())
        ptr = lambda a: _p(a) if torch.is_tensor(a) else a
        check(self.ctx.lib.mmf_tracker_add_keypoints_device(self.handle, ptr(n_dev), ptr(xy), ptr(descriptors), _p(depth),
                                                            int(timestamp), float(min_feature_distance), int(history)))

    def setKeypointStatus(self, status_dev):
        """the DEVICE status word of the keypoint source (int32 CUDA tensor, device address or None): while it is not 0 an
        addKeypointsDevice is a frame without keypoints and counts as failed"""
        self._status = status_dev  # (kept alive)
        check(self.ctx.lib.mmf_tracker_set_keypoint_status(self.handle, _p(status_dev) if torch.is_tensor(status_dev) else status_dev))

    def keypointFailures(self):
        """waits: the addKeypointsDevice calls since creation / reset whose status word was set"""
        n = C.c_int()
        check(self.ctx.lib.mmf_tracker_keypoint_failures(self.handle, C.byref(n)))
        return n.value

    def prune(self, min_kps, min_time):
        check(self.ctx.lib.mmf_tracker_prune(self.handle, int(min_kps), int(min_time)))

    def status(self):
        """(tracks, length, dropped appends); waits for the stream"""
        n, length, dropped = C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_tracker_status(self.handle, C.byref(n), C.byref(length), C.byref(dropped)))
        return n.value, length.value, dropped.value

    def numTracks(self):
        return self.status()[0]

    def lastLaunches(self):
        return self.ctx.lib.mmf_tracker_last_launches(self.handle)

    def reset(self):
        check(self.ctx.lib.mmf_tracker_reset(self.handle))

    # ----- the view log: what Model::store's views are built from
    def setViewLog(self, frames):
        """keep the visible sets of the last `frames` adds on the device (0: off, the default).  The ring is allocated here."""
        check(self.ctx.lib.mmf_tracker_set_view_log(self.handle, int(frames)))

    def frame(self):
        """adds since creation / reset = the stamp of the newest frame"""
        return self.ctx.lib.mmf_tracker_frame(self.handle)

    def modelViewsDevice(self, model_id, frames, poses):
        """-> (counts int32 [n_views] host, descriptor [rows,256] / coordinate [rows,3] CUDA tensors over the tracker's
        buffers, valid until its next call, missing)"""
        from .model import _as_tensor
        fr = np.ascontiguousarray(np.asarray(frames, np.int32).reshape(-1))
        po = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(fr.size, 16))
        cnt, de, co, missing = C.POINTER(C.c_int)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int()
        check(self.ctx.lib.mmf_tracker_model_views(self.handle, int(model_id), fr.size, fr.ctypes.data, po.ctypes.data,
                                                   C.byref(cnt), C.byref(de), C.byref(co), C.byref(missing)))
        counts = np.array([cnt[v] for v in range(fr.size)], np.int32)
        rows = int(counts.sum())
        if rows == 0:
            return counts, torch.zeros((0, 256), dtype=torch.float32, device=self._dev), torch.zeros((0, 3), dtype=torch.float32, device=self._dev), missing.value
        d = _as_tensor(C.cast(de, C.c_void_p).value, rows * 1024, torch.float32, (rows, 256), self.ctx.device, self)
        c = _as_tensor(C.cast(co, C.c_void_p).value, rows * 12, torch.float32, (rows, 3), self.ctx.device, self)
        return counts, d, c, missing.value

    def modelViews(self, model_id, frames, poses):
        """Model::store's views of one model from the log -> ([(descriptor [n,256], coordinate [n,3])] per listed frame, host
        arrays, and the number of frames that are not in the log).  frames: stamps (frame()), poses: [n,4,4] camera -> model"""
        counts, d, c, missing = self.modelViewsDevice(model_id, frames, poses)
        d, c = d.cpu().numpy(), c.cpu().numpy()
        out, o = [], 0
        for n in counts:
            out.append((d[o:o + n].copy(), c[o:o + n].copy()))
            o += int(n)
        return out, missing

    # ----- back-dating: Model::refineTrackSubset (Model.cpp:649-737) from the table and the log
    def reserveBackdate(self, history):
        """the workspace for windows of up to `history` frames (0 frees it); allocated here, never per frame"""
        check(self.ctx.lib.mmf_tracker_reserve_backdate(self.handle, int(history)))

    def backdate(self, label, history, batch):
        """how the tracks labelled `label` (after this frame's associate) moved over the last min(length, history, logged)
        frames -> a list of dicts, oldest first, the last one's pose exactly the identity.  batch: ransac.RansacBatch of the
        same context ({10, 0.03, 0.6} is the reference's).  Waits twice."""
        out = (mmf_backdated_pose * int(history))()
        n = C.c_int()
        check(self.ctx.lib.mmf_tracker_backdate(self.handle, int(label), int(history), batch.handle, out, int(history), C.byref(n)))
        return [backdated_pose_dict(out[j]) for j in range(n.value)]

    def backdateRows(self, entry):
        """test accessor: the (p0 [n,3], p1 [n,3]) rows the last backdate() handed the batch object for entry `entry`"""
        k = min(self.capacity, self.max_keypoints)
        p0, p1, n = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), C.c_int()
        check(self.ctx.lib.mmf_tracker_backdate_rows(self.handle, int(entry), p0.ctypes.data, p1.ctypes.data, k, C.byref(n)))
        return p0[:n.value].copy(), p1[:n.value].copy()

    # ----- the models' track sets
    @staticmethod
    def _ids(model_ids):
        ids = np.ascontiguousarray(np.atleast_1d(np.asarray(model_ids, np.int32)))
        return ids, ids.ctypes.data_as(C.POINTER(C.c_int))

    def associate(self, mask, model_ids):
        """mask: uint8 [rows,cols] CUDA tensor of model ids (textures[MASK]); model_ids: the active models"""
        assert mask.is_cuda and mask.dtype == torch.uint8 and mask.shape == (self.height, self.width)
        ids, p = self._ids(model_ids)
        check(self.ctx.lib.mmf_tracker_associate(self.handle, _p(mask.contiguous()), p, ids.size))

    def associateAll(self, model_ids):
        ids, p = self._ids(model_ids)
        check(self.ctx.lib.mmf_tracker_associate_all(self.handle, p, ids.size))

    def forgetModel(self, model_id):
        check(self.ctx.lib.mmf_tracker_forget_model(self.handle, int(model_id)))

    def lastPairs(self, model_ids):
        """[(p0 [k,3], p1 [k,3])] per listed model: the last two keypoints of its tracks where both exist and are finite"""
        ids, p = self._ids(model_ids)
        p0, p1, cnt, stride = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_int)(), C.c_int()
        check(self.ctx.lib.mmf_tracker_last_pairs(self.handle, p, ids.size, C.byref(p0), C.byref(p1), C.byref(cnt), C.byref(stride)))
        out = []
        for j in range(ids.size):
            k, off = cnt[j], j * stride.value * 3
            a = np.ctypeslib.as_array(p0, (ids.size * stride.value * 3,))[off:off + 3 * k].reshape(k, 3).copy() if k else np.zeros((0, 3), np.float32)
            b = np.ctypeslib.as_array(p1, (ids.size * stride.value * 3,))[off:off + 3 * k].reshape(k, 3).copy() if k else np.zeros((0, 3), np.float32)
            out.append((a, b))
        return out

    def getLastTrackTransform(self, model_id=0, config=(10, 0.03, 0.6)):
        """Model::getLastTrackTransform -> (T 4x4 float32, error, inlier mask or None)"""
        cfg = mmf_ransac_config(int(config[0]), float(config[1]), float(config[2]))
        T = np.zeros((4, 4), np.float32)
        err, has = C.c_float(), C.c_int()
        inl = np.zeros(self.capacity, np.uint8)
        check(self.ctx.lib.mmf_tracker_last_track_transform(self.handle, int(model_id), C.byref(cfg), T.ctypes.data,
                                                            C.byref(err), inl.ctypes.data, C.byref(has)))
        return T, err.value, (inl.astype(bool) if has.value else None)

    def visible(self):
        """the last keypoint of every visible track -> (xy [n,2], coordinate [n,3], descriptor [n,256], uid [n])"""
        n = C.c_int()
        xy = np.zeros((self.capacity, 2), np.int32)
        co = np.zeros((self.capacity, 3), np.float32)
        de = np.zeros((self.capacity, 256), np.float32)
        uid = np.zeros(self.capacity, np.int64)
        check(self.ctx.lib.mmf_tracker_visible(self.handle, self.capacity, C.byref(n), xy.ctypes.data, co.ctypes.data,
                                               de.ctypes.data, uid.ctypes.data))
        k = n.value
        return xy[:k], co[:k], de[:k], uid[:k]

    def download(self):
        """the whole table as a dict of host arrays (tests and tools)"""
        c = self.capacity
        a = dict(desc=np.zeros((c, 256), np.float32), age=np.zeros(c, np.int32), nvalid=np.zeros(c, np.int32),
                 last_stamp=np.zeros(c, np.int64), uid=np.zeros(c, np.int64), xy=np.zeros((2, c, 2), np.int32),
                 coordinate=np.zeros((2, c, 3), np.float32), timestamp=np.zeros((2, c), np.int64),
                 nonnull=np.zeros((2, c), np.int32), member=np.zeros((c, 8), np.uint32), label=np.zeros(c, np.int32))
        n = C.c_int()
        check(self.ctx.lib.mmf_tracker_download(self.handle, c, C.byref(n), *[a[k].ctypes.data for k in (
            "desc", "age", "nvalid", "last_stamp", "uid", "xy", "coordinate", "timestamp", "nonnull", "member", "label")]))
        k = n.value
        out = {key: (v[:, :k].copy() if key in ("xy", "coordinate", "timestamp", "nonnull") else v[:k].copy()) for key, v in a.items()}
        out["n_tracks"], out["length"], out["dropped"] = self.status()
        return out

    def close(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.mmf_tracker_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeKeypointFrontEnd:
    """The keypoint half of processFrame (MultiMotionFusion.cpp:223-248, 312-335) with the tracks on the device: SuperPoint
    features -> DevicePointTracker -> processFrame, which initialises EVERY active model from its own tracks and keeps the
    models' track sets up to date from the frame's segmentation (fusion.setTracker)."""

    def __init__(self, ctx: Context, fusion, kp_predictor, intrinsics, icp_refine=True, capacity=4096, max_keypoints=1024,
                 view_log=0, on_device=False):
        """view_log: frames of the tracker's view log (0: none).  With it and fusion.setEnableRedetection(True) a model that
        leaves the active list stores its keypoint views by itself: redetection needs no history kept by the caller.
        on_device: features, add and prune run inside fusion.processFrame on the frame's device buffers, nothing awaited
        (fusion.setKeypointFrontEnd; kp_predictor must be a superpoint.SuperPoint with max_keypoints <= the tracker's)."""
        self.ctx, self.fusion, self.kp, self.on_device = ctx, fusion, kp_predictor, bool(on_device)
        self.tracker = DevicePointTracker(ctx, fusion.width, fusion.height, intrinsics, capacity, max_keypoints)
        self.tracker.setViewLog(view_log)
        fusion.setTracker(self.tracker, odom_init_kp=True, icp_refine=icp_refine)
        if self.on_device:
            fusion.setKeypointFrontEnd(kp_predictor)

    def processFrame(self, rgb, depth, timestamp, weightMultiplier=1.0, **frame):
        if self.on_device:
            self.fusion.processFrame(rgb, depth, timestamp=timestamp, weightMultiplier=weightMultiplier, **frame)
            return
        coordinates, descriptors = self.kp.getFeatures(rgb)
        self.tracker.addKeypoints(coordinates, descriptors, timestamp, depth, 0.7, 30)
        self.tracker.prune(30, max(int(timestamp) - int(1e9), 0))  # :246
        self.fusion.processFrame(rgb, depth, timestamp=timestamp, weightMultiplier=weightMultiplier, **frame)

    def close(self):
        if self.on_device:
            self.fusion.setKeypointFrontEnd(None)
        self.fusion.setTracker(None)
        self.tracker.close()
