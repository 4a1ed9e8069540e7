"""Plain-Python restatement of the tracker's view log and of the views built from it (mmf_tracker_set_view_log,
mmf_tracker_model_views; csrc/tracker_kernels.hpp), on top of tracker_oracle.OracleTracker, which keeps full histories:

  Model::store / computeTrackProjectionFirstFrame / project_kp   Core/Model/Model.cpp:1617-1644, 508-522, 130-141
  the filter of Model::getBestMatch                              Core/Model/Model.cpp:806-811

The log is a ring of `frames` slots; slot stamp % frames holds the visible set of add number `stamp` (1 = the first add since
creation / reset): uid, camera-frame coordinate and descriptor of THAT frame's keypoint, in table order = uid ascending.
View v of a model = the logged keypoints of frame frames[v], in log order, whose uid is in the table NOW, whose track is in
the model NOW, and whose coordinate in the model's frame is finite.  The transformation is project_kp with every product and
sum rounded on its own (numpy float64 scalars), the result rounded to float32."""
import numpy as np

import tracker_oracle as to


def project(pose, coordinate):
    """float32 pose [4,4] (camera -> model) and coordinate [3] -> float32 [3]: ((r0 x + r1 y) + r2 z) + t in float64"""
    P = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    x, y, z = (np.float64(v) for v in np.asarray(coordinate, np.float32))
    with np.errstate(all="ignore"):
        return np.array([np.float32(((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3]) for r in range(3)], np.float32)


def project_rows(pose, coordinates):
    """project() of every row of coordinates [n,3] at once: the same operations as numpy float64 array ufuncs, each of which
    rounds on its own (tests/test_viewlog_oracle.py checks it against the scalars bit for bit)"""
    P = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    c = np.asarray(coordinates, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        cols = [np.add(np.add(np.add(np.multiply(P[r, 0], c[:, 0]), np.multiply(P[r, 1], c[:, 1])), np.multiply(P[r, 2], c[:, 2])), P[r, 3])
                for r in range(3)]
        return np.stack(cols, 1).astype(np.float32)


class ViewLogOracle:
    def __init__(self, tracker: to.OracleTracker, frames=0):
        self.t = tracker
        self.stamp = 0
        self.set_view_log(frames)

    def set_view_log(self, frames):
        """0: off; any other value: a fresh, empty ring"""
        self.frames = int(frames)
        self.ring = [None] * self.frames
        self.first = self.stamp + 1

    def add(self, *args, **kwargs):
        self.t.add(*args, **kwargs)
        self.stamp += 1
        if self.frames:
            _, co, de, uid = self.t.visible()
            self.ring[self.stamp % self.frames] = dict(stamp=self.stamp, uid=uid.copy(), coordinate=co.copy(), descriptor=de.copy())

    def reset(self):
        t = self.t
        t.tracks, t.models, t.next_uid, t.dropped = [], {}, 0, 0
        self.stamp = 0
        self.set_view_log(self.frames)

    def slot(self, stamp):
        """the logged frame `stamp`, or None when it is not in the ring"""
        if not self.frames or stamp < self.first or stamp > self.stamp or stamp <= self.stamp - self.frames:
            return None
        s = self.ring[stamp % self.frames]
        assert s is not None and s["stamp"] == stamp
        return s

    def model_views(self, model_id, frames, poses):
        """-> ([(descriptor [n,256] float32, coordinate [n,3] float32)] per listed frame, missing)"""
        now = {t.uid for t in self.t.tracks}
        mine = self.t.models.get(int(model_id), set())
        views, missing = [], 0
        for stamp, pose in zip(frames, poses):
            s = self.slot(int(stamp))
            if s is None:
                missing += 1
                views.append((np.zeros((0, 256), np.float32), np.zeros((0, 3), np.float32)))
                continue
            keep = np.array([int(uid) in now and int(uid) in mine for uid in s["uid"]], bool)
            co = project_rows(pose, s["coordinate"])  # (project() of every row)
            keep &= np.all(np.isfinite(co), axis=1)
            views.append((s["descriptor"][keep].reshape(-1, 256).copy(), co[keep].reshape(-1, 3).copy()))
        return views, missing


def same_views(got, want):
    """None when two lists of views are equal bit for bit, else where they differ"""
    if len(got) != len(want):
        return f"{len(got)} views != {len(want)}"
    for v, ((gd, gc), (wd, wc)) in enumerate(zip(got, want)):
        if gd.shape != wd.shape or gc.shape != wc.shape:
            return f"view {v}: shapes {gd.shape} {gc.shape} != {wd.shape} {wc.shape}"
        if not np.array_equal(gd.view(np.uint32), wd.view(np.uint32)):
            return f"view {v}: descriptors differ"
        if not np.array_equal(gc.view(np.uint32), wc.view(np.uint32)):
            return f"view {v}: coordinates differ at {np.argwhere(gc.view(np.uint32) != wc.view(np.uint32))[:4].tolist()}"
    return None


def random_pose(rng, scale=1.0):
    """a rigid float32 pose [4,4]"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.standard_normal(3) * scale
    return T.astype(np.float32)


def unit_rows(rng, n, dim=256):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def make_step(rng, pool, n, width, height, nan_rows=1):
    """keypoints of one frame: n rows of the pool, most of them exact (they continue their tracks), some disturbed past the
    gate (new tracks); pixels anywhere in the image, `nan_rows` of them outside (NaN coordinates); a depth image with holes"""
    pick = rng.choice(pool.shape[0], n, replace=False) if n else np.zeros(0, np.int64)
    desc = pool[pick].copy()
    if n:
        far = rng.random(n) < 0.2
        noisy = desc + 1.5 * unit_rows(rng, n)
        desc[far] = (noisy / np.linalg.norm(noisy, axis=1, keepdims=True)).astype(np.float32)[far]
    xy = np.stack([rng.integers(0, width, n), rng.integers(0, height, n)], 1).astype(np.int32)
    xy[:min(nan_rows, n)] = (width, 3)
    depth = rng.uniform(0.5, 4.0, (height, width)).astype(np.float32)
    depth[rng.random((height, width)) < 0.15] = 0.0
    return xy, desc, depth


def ulp_distance(a, b):
    """per component: how many float32 values lie between a and b (0 = the same bits, or both zero)"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
