"""-m gpu: the device track table inside MultiMotionFusion::processFrame (mmf_fusion_set_tracker; MultiMotionFusion.cpp:223-248,
312-335, 425-436, 584-604, 622-627): 320 x 240, five or six frames.

Single model: tracker.NativeKeypointFrontEnd against the unchanged point_tracker.KeypointFrontEnd, poses bit for bit.
Moving objects: the two-box scene of tests/test_gpu_mask_fusion.py segmented from its label images; every model is
initialised from its own tracks, and the track sets, pairs and transformations are those of tests/tracker_oracle.py run on
the frame's own MASK image."""
import numpy as np
import pytest
import torch

import tracker_oracle as to
from multimotionfusion_amd import synth
from multimotionfusion_amd._capi import MmfError

pytestmark = pytest.mark.gpu
W, H = 320, 240
RAW = np.zeros(256, np.uint8)
RAW[1], RAW[2] = 37, 200


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unit_rows(rng, n, dim=256):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def matmul4(a, b):
    """mmf::host::matmul4 (csrc/pose_algebra.hpp): float, the products summed left to right"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    r = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            acc = np.float32(a[i, 0] * b[0, j])
            for k in range(1, 4):
                acc = np.float32(acc + np.float32(a[i, k] * b[k, j]))
            r[i, j] = acc
    return r


class LandmarkPredictor:
    """SuperPoint::getFeatures with perfect keypoints (as in tests/test_gpu_point_tracker.py): fixed world landmarks taken
    from the first frame's depth, projected into every frame, one constant descriptor each"""

    def __init__(self, frames, poses, K, n=200, seed=0):
        rng = np.random.default_rng(seed)
        d0 = frames[0]["depth"]
        h, w = d0.shape
        ys, xs = np.nonzero(d0 > 0)
        pick = rng.choice(len(ys), n, replace=False)
        z = d0[ys[pick], xs[pick]].astype(np.float64)
        cam = np.stack([z * (xs[pick] - K["cx"]) / K["fx"], z * (ys[pick] - K["cy"]) / K["fy"], z, np.ones(n)], 0)
        self.world = poses[0] @ cam
        self.desc = unit_rows(rng, n)
        self.poses, self.K, self.w, self.h, self.frame = poses, K, w, h, 0

    def getFeatures(self, rgb):
        K = self.K
        cam = np.linalg.inv(self.poses[self.frame]) @ self.world
        self.frame += 1
        x = np.rint(cam[0] / cam[2] * K["fx"] + K["cx"])
        y = np.rint(cam[1] / cam[2] * K["fy"] + K["cy"])
        ok = (cam[2] > 0) & (x >= 0) & (x < self.w) & (y >= 0) & (y < self.h)
        return np.stack([x[ok] / self.w, y[ok] / self.h], 1), self.desc[ok].astype(np.float64)


@pytest.fixture(scope="module")
def landmark_scene():
    n = 5
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(n, seed=5)
    return K, poses, [synth.render(p, W, H, seed=i) for i, p in enumerate(poses)]


@pytest.mark.parametrize("icp_refine", [True, False])
def test_single_model_front_end_reproduces_the_host_front_end(gpu_ctx, landmark_scene, icp_refine):
    """the landmark scene of test_keypoint_front_end_with_good_keypoints: the table's pairs for model 0 are the host mirror's
    (every track joins model 0 at every frame), so the transformation, and with it every pose, is the same bit for bit"""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.point_tracker import KeypointFrontEnd
    from multimotionfusion_amd.tracker import NativeKeypointFrontEnd
    K, poses, frames = landmark_scene
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    runs = []
    for native in (False, True):
        g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"])
        kp = LandmarkPredictor(frames, poses, K)
        fe = (NativeKeypointFrontEnd if native else KeypointFrontEnd)(gpu_ctx, g, kp, intr, icp_refine=icp_refine)
        out = []
        for i, f in enumerate(frames):
            rgb, depth = dev(f["rgb"]), dev(f["depth"])
            fe.processFrame(rgb, depth, timestamp=1000 + 33_000_000 * i)
            out.append(g.getCurrPose().copy())
            if native and i > 0:
                T = g.getLastTrackTransforms()
                assert T.shape == (1, 4, 4) and not np.array_equal(T[0], np.eye(4, dtype=np.float32))
        if native:
            n_tracks, length, dropped = fe.tracker.status()
            assert n_tracks == len(runs[0][1]) and length == len(frames) and dropped == 0
            fe.close()
        else:
            out = (out, fe.tracker.getTracks())
        runs.append(out if not native else (out, None))
        g.close()
    for i, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert np.array_equal(bits(a), bits(b)), (i, a, b)
        gt = np.linalg.inv(poses[0]) @ poses[i]
        assert np.linalg.norm(b[:3, 3] - gt[:3, 3]) < (0.01 if icp_refine else 0.03)


# ---- moving objects ---------------------------------------------------------------------------------------------------
N_FRAMES = 6


@pytest.fixture(scope="module")
def object_scene():
    """the scene of tests/test_gpu_mask_fusion.py; 40 landmarks per box picked on its label in frame 0 and moved by its
    trajectory, 120 on the static scene -> per frame (xy [m,2] pixels, descriptor [m,256], owner [m])"""
    seed = 21
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(N_FRAMES, seed=seed)
    objs = synth.make_objects(2, seed=seed)
    traj = synth.object_trajectories(objs, N_FRAMES, seed=seed)
    frames = [synth.render(p, W, H, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    labels = [RAW[f["ids"].astype(np.uint8)] for f in frames]
    rng = np.random.default_rng(3)
    world, owner = [], []
    for label, count in ((0, 120), (1, 40), (2, 40)):
        ys, xs = np.nonzero((frames[0]["ids"] == label) & (frames[0]["depth"] > 0))
        pick = rng.choice(len(ys), count, replace=False)
        cam = frames[0]["vertex"][ys[pick], xs[pick], :3].astype(np.float64)
        world.append(cam @ poses[0][:3, :3].T + poses[0][:3, 3])
        owner += [label] * count
    world, owner = np.concatenate(world), np.array(owner)
    desc = unit_rows(rng, len(owner))
    kps = []
    for i in range(N_FRAMES):
        w = world.copy()
        for k in (1, 2):
            T = traj[k - 1][i]
            w[owner == k] = world[owner == k] @ T[:3, :3].T + T[:3, 3]
        Pi = np.linalg.inv(poses[i])
        x = w @ Pi[:3, :3].T + Pi[:3, 3]
        u = np.rint(x[:, 0] / x[:, 2] * K["fx"] + K["cx"]).astype(np.int64)
        v = np.rint(x[:, 1] / x[:, 2] * K["fy"] + K["cy"]).astype(np.int64)
        ok = (x[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        kps.append((np.stack([u[ok], v[ok]], 1).astype(np.int32), desc[ok], owner[ok]))
    return K, frames, labels, kps


@pytest.mark.parametrize("icp_refine", [False, True])
def test_every_model_is_initialised_from_its_own_tracks(gpu_ctx, orc, object_scene, icp_refine):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import MaskConfig
    from multimotionfusion_amd.tracker import DevicePointTracker
    K, frames, labels, kps = object_scene
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=2)
    g.setMaskSegmentation(MaskConfig(model_spawn_offset=1))
    trk = DevicePointTracker(gpu_ctx, W, H, intr, capacity=512, max_keypoints=256)
    ora = to.OracleTracker(W, H, intr, capacity=512)
    g.setTracker(trk, odom_init_kp=True, icp_refine=icp_refine)
    keep, checked = [], 0
    for i, f in enumerate(frames):
        ts = 1000 + 33_000_000 * i
        xy, de, _ = kps[i]
        keep.append((dev(f["rgb"]), dev(f["depth"]), dev(labels[i])))
        trk.addKeypointsPixels(xy, de, ts, keep[-1][1], 0.7, 30)
        trk.prune(30, max(ts - int(1e9), 0))
        ora.add(xy, de, ts, f["depth"], 0.7, 30)
        ora.prune(30, max(ts - int(1e9), 0))
        before = {m.id: m.getPose().copy() for m in g.getModels()}
        want = [ora.last_track_transform(m) for m in before]
        for m in before:  # an object model has been associated once: more than 3 finite pairs from the frame after its spawn
            if m != 0:
                assert ora.last_pairs(m)[0].shape[0] > 3, (i, m)
        g.processFrame(*keep[-1][:2], timestamp=ts, mask=keep[-1][2])
        got = g.getLastTrackTransforms()
        if i == 0:
            assert got.shape[0] == 0
        else:
            assert got.shape[0] == len(before)
            for (m, pose), (T, _, _), Tg in zip(before.items(), want, got):
                assert np.array_equal(bits(Tg), bits(T)), (i, m, Tg, T)
                checked += m != 0
        after = {m.id: m.getPose().copy() for m in g.getModels()}
        if i > 0 and not icp_refine:
            for (m, pose), (T, _, _) in zip(before.items(), want):
                if m in after:
                    expect = matmul4(pose, T) if m == 0 else matmul4(T, pose)  # :331 / :334
                    assert np.array_equal(bits(after[m]), bits(expect)), (i, m)
        mask = g.getTexture("MASK").cpu().numpy()
        for m in before:
            if m not in after:
                ora.forget(m)
        if i == 0:
            ora.associate_all([0])
        else:
            ora.associate(mask, list(after))
        diff = to.same_table(trk.download(), ora.flatten())
        assert diff is None, (i, diff)
        for m, (p0, p1) in zip(after, trk.lastPairs(list(after))):
            w0, w1 = ora.last_pairs(m)
            assert np.array_equal(bits(p0), bits(w0)) and np.array_equal(bits(p1), bits(w1)), (i, m)
    assert list(after) == [0, 1, 2] and checked >= 2 * (N_FRAMES - 3)
    f = ora.flatten()
    for m in (1, 2):  # both boxes carry tracks of their own, and none of them is the other's
        mine = (f["member"][:, 0] >> np.uint32(m)) & 1
        assert mine.sum() > 10 and not (mine & (f["member"][:, 0] >> np.uint32(3 - m)) & 1).any()
    g.setTracker(None)
    trk.close()
    g.close()


def test_refusals(gpu_ctx, landmark_scene):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.tracker import DevicePointTracker
    K, poses, frames = landmark_scene
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    trk = DevicePointTracker(gpu_ctx, W, H, intr, capacity=64, max_keypoints=16)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setShard(0, 2)
    with pytest.raises(MmfError) as e:  # like redetection: not on a shard
        g.setTracker(trk)
    assert e.value.status == -4
    g.setTracker(None)
    g.close()
    small = DevicePointTracker(gpu_ctx, W // 2, H // 2, intr, capacity=64, max_keypoints=16)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"])
    with pytest.raises(MmfError) as e:  # another image size
        g.setTracker(small)
    assert e.value.status == -1
    g.setTracker(trk)
    rgb, depth = dev(frames[0]["rgb"]), dev(frames[0]["depth"])
    g.processFrame(rgb, depth, timestamp=1000)
    with pytest.raises(MmfError) as e:  # the caller's init_transforms beside the tracker's
        g.processFrame(rgb, depth, timestamp=2000, initTransform=np.eye(4, dtype=np.float32))
    assert e.value.status == -1 and "init_transforms" in str(e.value)
    assert g.getTick() == 2
    g.setTracker(None)
    g.processFrame(rgb, depth, timestamp=2000, initTransform=np.eye(4, dtype=np.float32))
    assert g.getTick() == 3
    g.close()
    small.close()
    trk.close()


def test_redetection_takes_the_trackers_visible_keypoints(gpu_ctx, orc):
    """The sequence of test_older_newer_rule_and_small_segments up to its last frame: model 2 is inactive with stored views,
    model 3 carries its object.  The keypoints of that frame once through mmf_fusion_set_keypoints, once left to the attached
    tracker (its visible set): the same redetection, the same models, the same pose."""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.tracker import DevicePointTracker
    K = synth.intrinsics(W, H)
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    n = 7
    poses = synth.trajectory(n, seed=21)
    objs = synth.make_objects(2, seed=21)
    traj = synth.object_trajectories(objs, n, seed=21)
    frames = [synth.render(p, W, H, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]

    def model_data(mask, depth, ids):
        out = []
        for i in ids:
            sel = mask == i
            cnt = int(sel.sum())
            mean = float(depth[sel].mean()) if cnt else 0.0
            std = float(np.abs(depth[sel] - mean).mean()) if cnt else 0.0
            out.append(dict(id=i, super_pixel_count=cnt // 256, avg_confidence=0.4, depth_mean=mean, depth_std=std))
        return out

    masks = [np.zeros((H, W), np.uint8), np.where(frames[1]["ids"] == 1, 1, 0),
             np.where(np.isin(frames[2]["ids"], [1, 2]), frames[2]["ids"], 0), np.where(frames[3]["ids"] == 1, 1, 0),
             np.where(frames[4]["ids"] == 1, 1, 0), np.where(frames[5]["ids"] == 1, 1, np.where(frames[5]["ids"] == 2, 3, 0)),
             np.where(frames[6]["ids"] == 1, 1, np.where(frames[6]["ids"] == 2, 3, 0))]
    masks = [m.astype(np.uint8) for m in masks]
    new = [False, True, True, False, False, True, False]
    # the tracker: 40 keypoints on the segment of label 3 in the last frame; model 2's stored view = those keypoints moved rigidly
    rng = np.random.default_rng(9)
    ys, xs = np.nonzero((masks[6] == 3) & (frames[6]["depth"] > 0))
    sel = rng.choice(len(ys), 40, replace=False)
    xy6 = np.stack([xs[sel], ys[sel]], 1).astype(np.int32)
    trk = DevicePointTracker(gpu_ctx, W, H, intr, capacity=128, max_keypoints=64)
    trk.addKeypointsPixels(xy6, unit_rows(rng, 40), 1006, dev(frames[6]["depth"]), 0.7, 30)
    vxy, vco, vde, _ = trk.visible()
    assert vxy.shape == (40, 2) and np.isfinite(vco).all()
    M = synth.make_pose((0.1, -0.2, 0.05), (0.3, -0.1, 0.2))
    views = [(vde.copy(), (vco.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32))]

    results = []
    for use_tracker in (False, True):
        g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
        g.setEnableRedetection(True)
        keep = []
        for i in range(n):
            ids_now = [m.id for m in g.getModels()]
            data = model_data(masks[i], frames[i]["depth"], ids_now + ([g.getNextModelID()] if new[i] else [])) if i > 0 else None
            if i == 4:
                assert ids_now == [0, 1] and [m.id for m in g.getInactiveModels()] == [2]
                assert g.storeViews(2, views) is True
            if i == 6:
                assert ids_now == [0, 1, 3]
                if use_tracker:
                    g.setTracker(trk, odom_init_kp=False)
                else:
                    g.setKeypoints(vxy, vco, vde)
            keep.append((dev(frames[i]["rgb"]), dev(frames[i]["depth"]), dev(masks[i])))
            g.processFrame(*keep[-1][:2], timestamp=1000 + i, mask=keep[-1][2], hasNewLabel=new[i], modelData=data)
        results.append(dict(ids=[m.id for m in g.getModels()], inactive=[m.id for m in g.getInactiveModels()],
                            events=[{**e, "transformation": e["transformation"].tobytes()} for e in g.getLastRedetections()], poses=[m.getPose().tobytes() for m in g.getModels()]))
        g.setTracker(None)
        g.close()
    a, b = results
    assert len(a["events"]) == 1 and a["events"][0]["activated"] and a["events"][0]["model_id"] == 2 and a["events"][0]["removed_id"] == 3
    assert a["ids"] == [0, 1, 2] and a["inactive"] == []
    assert b["events"] == a["events"] and b["ids"] == a["ids"] and b["inactive"] == a["inactive"] and b["poses"] == a["poses"]
    trk.close()
