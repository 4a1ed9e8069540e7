"""Plain-Python restatement of what the device track table (multimotionfusion_amd/tracker.py) computes, written from the
reference's code with lists like the reference's:

  PointTracker::addKeypoints / prune / getLastActiveKeypoints   Core/Utils/PointTracker.cpp:27-226
  the association of tracks with segments, Model::updateTracks  Core/MultiMotionFusion.cpp:425-436, 584-604, 622-627;
                                                                Core/Model/Model.cpp:630-640
  Model::getLastTrackTransform                                  Core/Model/Model.cpp:739-775

A track is a list of Keypoint-or-None, all tracks of the same length.  The search is oracle.match_descriptors (the CPU
restatement of cv::BFMatcher(NORM_L2, crossCheck) + the distance gate), the fit ransac.RigidRANSAC (host code).
Where the table departs from the reference the oracle follows the table and says so: a capacity (appends that do not fit
are dropped and counted), NaN coordinates for a keypoint outside the image, model sets ordered like `tracks` (the
reference's std::set orders by address), and a pruned track leaves the model sets with the table.
flatten() turns the lists into the arrays DevicePointTracker.download() returns."""
import numpy as np


class Keypoint:
    __slots__ = ("timestamp", "xy", "coordinate", "descriptor")

    def __init__(self, timestamp, xy, coordinate, descriptor):
        self.timestamp, self.xy, self.coordinate, self.descriptor = timestamp, xy, coordinate, descriptor


class Track(list):
    """the reference's Track (a vector of KeypointPtr) plus what the table adds: uid, this frame's label"""

    def __init__(self, kps, uid):
        super().__init__(kps)
        self.uid, self.label = uid, -1


def default_match(query, train, max_distance):
    from oracle import oracle as orc
    return orc.match_descriptors(query, train, max_distance)[0]


class OracleTracker:
    def __init__(self, width, height, intrinsics, capacity=1 << 30, match=default_match):
        self.width, self.height, self.capacity, self.match = width, height, capacity, match
        self.fx, self.fy, self.cx, self.cy = (np.float32(v) for v in intrinsics)
        self.tracks = []
        self.models = {}  # model id -> set of uid: Model::tracks
        self.next_uid, self.dropped = 0, 0

    # ---- PointTracker.cpp:35-56
    def construct(self, xy, descriptor, timestamp, depth):
        x, y = int(xy[0]), int(xy[1])
        v = np.full(3, np.nan, np.float32)
        if 0 <= x < self.width and 0 <= y < self.height:
            z = np.float32(depth[y, x])
            if z > 0:
                v = np.array([np.float32(np.float32(z * np.float32(np.float32(x) - self.cx)) / self.fx),
                              np.float32(np.float32(z * np.float32(np.float32(y) - self.cy)) / self.fy), z], np.float32)
        return Keypoint(int(timestamp), (x, y), v, np.asarray(descriptor, np.float32).copy())

    def _append(self, kps):
        if len(self.tracks) >= self.capacity:
            self.dropped += 1
            return
        self.tracks.append(Track(kps, self.next_uid))
        self.next_uid += 1

    # ---- :205-224
    def last_active(self, history=0):
        active = []
        for track in self.tracks:
            found = None
            for d, kp in enumerate(reversed(track)):
                if history and d >= history:
                    break
                if kp is not None:
                    found = kp
                    break
            active.append(found)
        return active

    # ---- :27-131
    def add(self, xy, descriptors, timestamp, depth, min_feature_distance=0.7, history=30):
        xy = np.asarray(xy, np.int64).reshape(-1, 2)
        descriptors = np.asarray(descriptors, np.float32).reshape(xy.shape[0], 256)
        n = xy.shape[0]
        kp = [self.construct(xy[q], descriptors[q], timestamp, depth) for q in range(n)]
        if not self.tracks:  # :61-66
            for q in range(n):
                self._append([kp[q]])
            return
        active = self.last_active(history)
        for track in self.tracks:  # :71-73
            track.append(None)
        if n == 0:
            return
        valid = [i for i, a in enumerate(active) if a is not None]
        matched = {}
        if valid:
            idx = self.match(descriptors, np.stack([active[i].descriptor for i in valid]), min_feature_distance)
            for q, t in enumerate(idx):
                if t >= 0:
                    matched[q] = valid[int(t)]
        for q, ti in matched.items():  # :107-112
            self.tracks[ti][-1] = kp[q]
        length = len(self.tracks[0])
        for q in range(n):  # :116-121
            if q not in matched:
                self._append([None] * (length - 1) + [kp[q]])

    # ---- :170-203
    def prune(self, min_kps, min_time):
        kept = []
        for track in self.tracks:
            nvalid = sum(k is not None for k in track)
            last_stamp = 0
            for k in track:
                if k is not None:
                    last_stamp = k.timestamp
            if not (nvalid < min_kps and last_stamp < min_time):
                kept.append(track)
        gone = {t.uid for t in self.tracks} - {t.uid for t in kept}
        for s in self.models.values():
            s -= gone
        self.tracks = kept

    # ---- MultiMotionFusion.cpp:425-436, 584-604
    def associate(self, mask, model_ids):
        segm = {}
        for track in self.tracks:
            track.label = -1
            if track[-1] is not None:
                x, y = track[-1].xy
                if 0 <= x < self.width and 0 <= y < self.height:
                    track.label = int(mask[y, x])
                    segm.setdefault(track.label, []).append(track)
        for m in model_ids:
            if m in segm:
                remove = [t for l, ts in segm.items() if l != m for t in ts]
                s = self.models.setdefault(int(m), set())  # Model::updateTracks (Model.cpp:630-640)
                s |= {t.uid for t in segm[m]}
                s -= {t.uid for t in remove}

    # ---- :622-627, Model::initGlobalTracks
    def associate_all(self, model_ids):
        for m in model_ids:
            self.models.setdefault(int(m), set()).update(t.uid for t in self.tracks)

    def forget(self, model_id):
        self.models.pop(int(model_id), None)

    # ---- Model.cpp:747-761
    def last_pairs(self, model_id):
        p0, p1 = [], []
        mine = self.models.get(int(model_id), set())
        for track in self.tracks:
            if track.uid not in mine or len(track) < 2:
                continue
            k0, k1 = track[-2], track[-1]
            if k0 is not None and k1 is not None and np.all(np.isfinite(k0.coordinate)) and np.all(np.isfinite(k1.coordinate)):
                p0.append(k0.coordinate)
                p1.append(k1.coordinate)
        return (np.array(p0, np.float32).reshape(-1, 3), np.array(p1, np.float32).reshape(-1, 3))

    # ---- Model.cpp:763-775
    def last_track_transform(self, model_id, config=(10, 0.03, 0.6)):
        from multimotionfusion_amd.ransac import RigidRANSAC
        p0, p1 = self.last_pairs(model_id)
        if p0.shape[0] < 3:
            return np.eye(4, dtype=np.float32), float("inf"), None
        return RigidRANSAC(*config).estimate(p0, p1)

    def visible(self):
        vis = [t for t in self.tracks if t[-1] is not None]
        return (np.array([t[-1].xy for t in vis], np.int32).reshape(-1, 2),
                np.array([t[-1].coordinate for t in vis], np.float32).reshape(-1, 3),
                np.array([t[-1].descriptor for t in vis], np.float32).reshape(len(vis), 256),
                np.array([t.uid for t in vis], np.int64))

    def flatten(self):
        """the arrays of DevicePointTracker.download(); slot 0 = cur = track[-1], slot 1 = prev = track[-2]; a null slot: zeros"""
        n = len(self.tracks)
        dim = 256
        a = dict(desc=np.zeros((n, dim), np.float32), age=np.zeros(n, np.int32), nvalid=np.zeros(n, np.int32),
                 last_stamp=np.zeros(n, np.int64), uid=np.zeros(n, np.int64), xy=np.zeros((2, n, 2), np.int32),
                 coordinate=np.zeros((2, n, 3), np.float32), timestamp=np.zeros((2, n), np.int64),
                 nonnull=np.zeros((2, n), np.int32), member=np.zeros((n, 8), np.uint32), label=np.zeros(n, np.int32))
        for i, t in enumerate(self.tracks):
            live = [k for k in t if k is not None]
            a["desc"][i] = live[-1].descriptor
            a["age"][i] = next(d for d, k in enumerate(reversed(t)) if k is not None)
            a["nvalid"][i], a["last_stamp"][i], a["uid"][i], a["label"][i] = len(live), live[-1].timestamp, t.uid, t.label
            for s in range(2):
                k = t[-1 - s] if len(t) > s else None
                if k is not None:
                    a["xy"][s, i], a["coordinate"][s, i], a["timestamp"][s, i], a["nonnull"][s, i] = k.xy, k.coordinate, k.timestamp, 1
            for m, s in self.models.items():
                if t.uid in s:
                    a["member"][i, m >> 5] |= np.uint32(1 << (m & 31))
        a["n_tracks"], a["length"], a["dropped"] = n, (len(self.tracks[0]) if n else 0), self.dropped
        return a


def same_table(got, want):
    """None when two flattened tables are equal bit for bit, else the name of the first array that differs"""
    for key, w in want.items():
        g = got[key]
        if isinstance(w, np.ndarray):
            if g.shape != w.shape or g.dtype != w.dtype:
                return f"{key}: shape / dtype {g.shape} {g.dtype} != {w.shape} {w.dtype}"
            gv = g.view(np.uint32) if g.dtype == np.float32 else g
            wv = w.view(np.uint32) if w.dtype == np.float32 else w
            if not np.array_equal(gv, wv):
                return f"{key}: differs at {np.argwhere(gv != wv)[:4].tolist()}"
        elif g != w:
            return f"{key}: {g} != {w}"
    return None
