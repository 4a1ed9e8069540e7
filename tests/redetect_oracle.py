"""Test helper (like crf_oracle.py): numpy restatement of the keypoint redetection of inactive models and the seeded fixture
the CPU and GPU tests share.

Restated: computeTrackProjectionFirstFrame (Core/Model/Model.cpp:508-522), the view construction and the search of
Model::getBestMatch (:781-874) and the decision block of MultiMotionFusion::processFrame (Core/MultiMotionFusion.cpp:425-436,
489-559).  The per-view match is oracle.match_descriptors without a distance gate (cv::BFMatcher(NORM_L2, true)); the rigid
fit is the library's host RigidRANSAC (multimotionfusion_amd.ransac: no device), ONE object per getBestMatch call, views in
ascending index (the reference iterates an unordered_map there)."""
import numpy as np

DIM = 256
RANSAC_CONFIG = (10, 0.03, 0.8)  # MultiMotionFusion.cpp:513


class Kp:
    """tracker::Keypoint as far as redetection reads it"""
    __slots__ = ("timestamp", "xy", "coordinate", "descriptor")

    def __init__(self, timestamp, xy, coordinate, descriptor):
        self.timestamp, self.xy, self.coordinate, self.descriptor = timestamp, xy, np.asarray(coordinate, np.float64), descriptor


def project_first_frame(tracks, poses):
    """computeTrackProjectionFirstFrame: tracks = lists of Kp / None (camera frame), poses = 4x4 float32 per time index
    (camera -> model).  The last len(poses) entries of every non-empty track, in the model's frame (double)."""
    local = []
    for track in tracks:
        if not track:
            continue
        assert len(track) >= len(poses)
        off = len(track) - len(poses)
        row = []
        for ip, P in enumerate(poses):
            kp = track[off + ip]
            if kp is None:
                row.append(None)
                continue
            P = np.asarray(P, np.float32).astype(np.float64)
            row.append(Kp(kp.timestamp, kp.xy, P[:3, :3] @ kp.coordinate + P[:3, 3], kp.descriptor))
        local.append(row)
    return local


def views_of(tracks_local):
    """Model.cpp:798-816: per time index the float32 descriptors / coordinates of the keypoints that exist and are finite"""
    out = []
    if not tracks_local:
        return out
    for i in range(len(tracks_local[0])):
        kps = [t[i] for t in tracks_local if t[i] is not None and np.all(np.isfinite(t[i].coordinate))]
        desc = np.stack([k.descriptor for k in kps]).astype(np.float32) if kps else np.zeros((0, DIM), np.float32)
        coord = np.stack([k.coordinate for k in kps]).astype(np.float32) if kps else np.zeros((0, 3), np.float32)
        out.append((desc, coord))
    return out


def match_views(orc, query_desc, views):
    """per view (train_idx [nq], distance [nq]) of BFMatcher(NORM_L2, crossCheck) -- no gate"""
    q = np.ascontiguousarray(query_desc, np.float32)
    return [orc.match_descriptors(q, np.ascontiguousarray(d, np.float32), 0.0) for d, _ in views]


def get_best_match(orc, query_desc, query_coord, views):
    """Model::getBestMatch -> dict(found, transformation, error, inliers, view, n_matches, inlier) (the keys of
    redetection.ViewStore.bestMatch)"""
    from multimotionfusion_amd.ransac import RigidRANSAC
    best = dict(found=False, transformation=np.eye(4, dtype=np.float32), error=float("inf"), inliers=0, view=-1, n_matches=0,
                inlier=np.zeros(0, bool))
    if not views:
        return best  # "no stored tracks" (:783-786)
    query_coord = np.ascontiguousarray(query_coord, np.float32)
    ransac = RigidRANSAC(*RANSAC_CONFIG)  # one per call (:847)
    for v, ((desc, coord), (idx, _)) in enumerate(zip(views, match_views(orc, query_desc, views))):
        if len(desc) == 0:
            continue  # (:823-830)
        sel = idx >= 0
        if int(sel.sum()) < 3:  # :839
            continue
        T, err, inl = ransac.estimate(query_coord[sel], np.asarray(coord, np.float32)[idx[sel]])
        if inl is None or int(inl.sum()) == 0:  # :859
            continue
        if not best["found"] or np.float32(err) < np.float32(best["error"]):  # first of equals (:870-873)
            best = dict(found=True, transformation=T, error=err, inliers=int(inl.sum()), view=v, n_matches=int(sel.sum()), inlier=inl)
    return best


def inverse_isometry(T):
    """Eigen::Isometry3f::inverse(): [R^T | -(R^T t)] in float32, sums left to right"""
    T = np.asarray(T, np.float32)
    P = np.eye(4, dtype=np.float32)
    P[:3, :3] = T[:3, :3].T
    for r in range(3):
        s = np.float32(T[0, r] * T[0, 3])
        s = np.float32(s + np.float32(T[1, r] * T[1, 3]))
        s = np.float32(s + np.float32(T[2, r] * T[2, 3]))
        P[r, 3] = -s
    return P


def redetect(orc, mask, xy, coordinate, descriptor, active_ids, inactive, has_new_label):
    """MultiMotionFusion.cpp:425-436 + 489-559.  mask [H,W] u8; keypoints xy [n,2] int, coordinate [n,3], descriptor [n,256];
    active_ids = ids of the active list in order; inactive = [(id, views)] in list order.
    -> dict(active_ids, inactive_ids, has_new_label, events=[dict(label, model_id, removed_id, activated, pose, best)])"""
    h, w = mask.shape
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    coordinate = np.asarray(coordinate, np.float32).reshape(-1, 3)
    segm = {}
    for i, (x, y) in enumerate(xy):
        if 0 <= x < w and 0 <= y < h:  # :432
            segm.setdefault(int(mask[y, x]), []).append(i)
    active, inact, events = list(active_ids), list(inactive), []
    for label in sorted(segm):  # (the reference iterates an unordered_map; here labels ascend)
        if label in (0, 255):
            continue
        kp = [i for i in segm[label] if np.all(np.isfinite(coordinate[i]))]
        if len(kp) < 3:  # :507
            continue
        removed = []
        for mid, views in inact:
            best = get_best_match(orc, np.asarray(descriptor, np.float32)[kp], coordinate[kp], views)
            if not (best["found"] and float(np.float32(best["error"])) < 0.01 and best["inliers"] > 5):  # :516
                continue
            has_new_label = False
            ev = dict(label=label, model_id=mid, removed_id=-1, activated=False, pose=None, best=best)
            events.append(ev)
            if label in active:
                if label < mid:  # an older model is not replaced by a newer one (:537-541)
                    continue
                active.remove(label)
                ev["removed_id"] = label
            active.append(mid)
            ev["activated"], ev["pose"] = True, inverse_isometry(best["transformation"])
            removed.append(mid)
        inact = [(m, v) for m, v in inact if m not in removed]
    return dict(active_ids=active, inactive_ids=[m for m, _ in inact], has_new_label=bool(has_new_label), events=events)


# ---- the fixture: a rigid object of K 3-D keypoints with unit descriptors ----------------------------------------------------
def unit_rows(rng, n):
    d = rng.normal(size=(n, DIM)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def rigid(rng, rot=0.4, trans=0.3):
    from multimotionfusion_amd import synth
    return synth.make_pose(rng.normal(size=3) * rot, rng.normal(size=3) * trans).astype(np.float32)


def make_object(seed, k=40, extent=0.15):
    """K points in a box of +-extent metres around (0, 0, 1.5) of the model's frame, one unit descriptor each"""
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-extent, extent, size=(k, 3)) + np.array([0.0, 0.0, 1.5])).astype(np.float32)
    return dict(points=pts, descriptors=unit_rows(rng, k), seed=seed)


def make_tracks(obj, n_views, seed, drop=0.3, desc_noise=0.02, coord_noise=5e-4):
    """V camera-frame observations of the object under known poses: -> (tracks, poses): tracks[j][i] = Kp or None (the
    keypoint j dropped at time i), poses[i] = camera -> model at time i; every observation carries its own slightly noisy
    descriptor (renormalised) and coordinate"""
    rng = np.random.default_rng(seed)
    k = len(obj["points"])
    poses = [rigid(rng) for _ in range(n_views)]
    tracks = [[] for _ in range(k)]
    for i, P in enumerate(poses):
        Pi = np.linalg.inv(P.astype(np.float64))
        for j in range(k):
            if rng.uniform() < drop:
                tracks[j].append(None)
                continue
            d = obj["descriptors"][j] + rng.normal(size=DIM).astype(np.float32) * np.float32(desc_noise / 16.0)
            d = (d / np.linalg.norm(d)).astype(np.float32)
            x = Pi[:3, :3] @ (obj["points"][j].astype(np.float64) + rng.normal(size=3) * coord_noise) + Pi[:3, 3]
            tracks[j].append(Kp(1000 + i, (0, 0), x, d))
    return tracks, poses


def make_query(obj, seed, subset=0.7, distractors=10, desc_noise=0.02, coord_noise=5e-4):
    """the object seen again, moved: -> (descriptor [n,256], coordinate [n,3] camera frame, motion 4x4 with
    X_cam = motion X_model, is_object [n])"""
    rng = np.random.default_rng(seed)
    k = len(obj["points"])
    sel = np.flatnonzero(rng.uniform(size=k) < subset)
    M = rigid(rng).astype(np.float64)
    d = obj["descriptors"][sel] + rng.normal(size=(len(sel), DIM)).astype(np.float32) * np.float32(desc_noise / 16.0)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    x = (obj["points"][sel].astype(np.float64) + rng.normal(size=(len(sel), 3)) * coord_noise) @ M[:3, :3].T + M[:3, 3]
    dd = unit_rows(rng, distractors)
    dx = rng.uniform(-1, 1, size=(distractors, 3)) + np.array([0.0, 0.0, 2.0])
    desc = np.concatenate([d, dd]).astype(np.float32)
    coord = np.concatenate([x, dx]).astype(np.float32)
    order = rng.permutation(len(desc))
    is_obj = np.concatenate([np.ones(len(sel), bool), np.zeros(distractors, bool)])
    return desc[order], coord[order], M.astype(np.float32), is_obj[order]
