"""-m gpu: the keypoint path that never leaves the device -- mmf_superpoint_get_features_device, the tracker add whose n is
on the device, and the front end inside processFrame (mmf_fusion_set_keypoint_frontend) -- against the oracle and against
the host-facing calls they stand beside.  Every comparison is bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

import tracker_oracle as to
from helpers import assert_bit_equal
from multimotionfusion_amd import synth
from multimotionfusion_amd._capi import MmfError

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit_rows(rng, n, dim=256):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def oracle_features(orc, img, weights, sp, limit=None):
    H, W = img.shape[:2]
    semi, cdesc = orc.sp_forward(orc.sp_input(img), weights)
    xy, conf = orc.sp_keypoints(orc.sp_heatmap(semi), sp.conf_thresh, sp.nms_dist, sp.border)
    if limit is not None:
        xy, conf = xy[:limit], conf[:limit]
    desc = orc.sp_sample_descriptors(cdesc, xy, H, W) if len(xy) else np.zeros((0, 256), np.float32)
    return xy, conf, desc


# ---- 1. selection ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(gpu_ctx, orc):
    from multimotionfusion_amd.superpoint import SuperPoint
    weights = orc.sp_random_weights(seed=4)
    sp = SuperPoint(gpu_ctx, weights, max_width=160, max_height=120, max_keypoints=2048)
    yield sp, weights
    sp.close()


@pytest.mark.parametrize("H,W,ch,seed", [(120, 160, 3, 21), (48, 64, 1, 48 + 64), (8, 8, 1, 16)])
def test_selection_equals_the_oracle_and_the_host_path(net, orc, H, W, ch, seed):
    sp, weights = net
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W) if ch == 1 else (H, W, ch), dtype=np.uint8)
    sp.getFeaturesDevice(img)
    xy, conf, desc, status = sp.lastFeatures()
    o_xy, o_conf, o_desc = oracle_features(orc, img, weights, sp)
    assert status == 0
    assert len(xy) == len(o_xy)
    assert_bit_equal(xy, o_xy, "keypoint pixels")
    assert_bit_equal(conf, o_conf, "keypoint confidences")
    assert_bit_equal(desc, o_desc, "sampled descriptors")
    h_xy, h_conf, h_desc = sp.keypoints(img)
    assert_bit_equal(xy, h_xy, "pixels, host path")
    assert_bit_equal(conf, h_conf, "confidences, host path")
    assert_bit_equal(desc, h_desc, "descriptors, host path")
    if (H, W) == (120, 160):
        assert len(xy) > 20
    if (H, W) == (8, 8):
        assert len(xy) == 0  # the border band removes everything
    cnt, st, pxy, pconf, pdesc = sp.deviceFeatures()
    assert pdesc % 16 == 0 and st not in (0, cnt)


# ---- 2. convergence worst cases ------------------------------------------------------------------------------------------------
def test_convergence_worst_cases_take_the_same_launches(gpu_ctx, net, orc):
    """the four heat maps of test_suppression_corner_cases (zero weights, the logits are the convPb bias), 40 x 56: the
    finisher workgroup reaches the fixed point on each, and the launches are those of a random image of that size"""
    from multimotionfusion_amd.superpoint import SuperPoint
    _, weights = net
    H, W = 40, 56
    launches = {}
    for case in ("flat", "ramp", "none", "radius0"):
        w = [(np.zeros_like(a), np.zeros_like(b)) for a, b in weights]
        bias = np.zeros(65, np.float32)
        if case == "ramp":
            bias[:64] = np.linspace(0.0, 3.0, 64, dtype=np.float32)
        elif case == "none":
            bias[64] = 20.0  # the dustbin takes all the mass
        w[9] = (w[9][0], bias)
        sp2 = SuperPoint(gpu_ctx, w, max_width=W, max_height=H, max_keypoints=H * W)
        sp2.nms_dist = 0 if case == "radius0" else 4
        img = np.zeros((H, W), np.uint8)
        sp2.getFeaturesDevice(img)
        launches[case] = sp2.lastLaunches()
        xy, conf, desc, status = sp2.lastFeatures()
        o_xy, o_conf, o_desc = oracle_features(orc, img, w, sp2)
        assert status == 0, case
        assert_bit_equal(xy, o_xy, f"{case}: keypoint pixels")
        assert_bit_equal(conf, o_conf, f"{case}: keypoint confidences")
        assert_bit_equal(desc, o_desc, f"{case}: descriptors")
        if case == "none":
            assert len(xy) == 0
        if case == "radius0":
            assert len(xy) == (H - 8) * (W - 8)  # the ranking at kept = candidates
        if case == "flat":
            assert len(xy) > 0 and np.all(conf == conf[0])
        sp2.close()
    sp3 = SuperPoint(gpu_ctx, weights, max_width=W, max_height=H, max_keypoints=H * W)
    img = np.random.default_rng(3).integers(0, 256, (H, W), dtype=np.uint8)
    sp3.getFeaturesDevice(img)
    launches["random"] = sp3.lastLaunches()
    xy, conf, desc, status = sp3.lastFeatures()
    o_xy, o_conf, o_desc = oracle_features(orc, img, weights, sp3)
    assert status == 0 and len(xy) > 0
    assert_bit_equal(xy, o_xy, "random: keypoint pixels")
    assert_bit_equal(desc, o_desc, "random: descriptors")
    sp3.close()
    assert len(set(launches.values())) == 1 and launches["flat"] > 0, launches


# ---- 3. limit ----------------------------------------------------------------------------------------------------------------
def test_limit_keeps_the_strongest_in_order(gpu_ctx, orc):
    from multimotionfusion_amd.superpoint import SuperPoint
    weights = orc.sp_random_weights(seed=4)
    sp = SuperPoint(gpu_ctx, weights, max_width=160, max_height=120, max_keypoints=16)
    img = np.random.default_rng(21).integers(0, 256, (120, 160, 3), dtype=np.uint8)
    sp.getFeaturesDevice(img)
    xy, conf, desc, status = sp.lastFeatures()
    o_xy, o_conf, o_desc = oracle_features(orc, img, weights, sp, limit=16)
    assert status == 0 and len(xy) == 16
    assert_bit_equal(xy, o_xy, "strongest 16")
    assert_bit_equal(conf, o_conf, "their confidences")
    assert_bit_equal(desc, o_desc, "their descriptors")
    sp.close()


# ---- 4. no hidden host state ---------------------------------------------------------------------------------------------------
def test_two_calls_back_to_back_share_no_host_state(gpu_ctx, orc):
    """two networks of one context on two images, one device add each into two trackers, ONE wait at the end"""
    from multimotionfusion_amd.superpoint import SuperPoint
    from multimotionfusion_amd.tracker import DevicePointTracker
    H, W = 48, 64
    intr = (52.0, 51.5, 31.5, 23.25)
    weights = orc.sp_random_weights(seed=4)
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2)]
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    sps = [SuperPoint(gpu_ctx, weights, max_width=W, max_height=H, max_keypoints=256) for _ in range(2)]
    trks = [DevicePointTracker(gpu_ctx, W, H, intr, capacity=512, max_keypoints=256) for _ in range(2)]
    d_imgs, d_depth = [dev(i) for i in imgs], dev(depth)
    for sp, im in zip(sps, d_imgs):
        sp.getFeaturesDevice(im)
    for sp, trk in zip(sps, trks):
        cnt, st, pxy, _, pdesc = sp.deviceFeatures()
        trk.setKeypointStatus(st)
        trk.addKeypointsDevice(cnt, pxy, pdesc, 1000, d_depth)
    gpu_ctx.synchronize()
    counts = []
    for sp, trk, im in zip(sps, trks, imgs):
        xy, conf, desc, status = sp.lastFeatures()
        o_xy, o_conf, o_desc = oracle_features(orc, im, weights, sp)
        assert status == 0
        assert_bit_equal(xy, o_xy, "keypoint pixels")
        assert_bit_equal(conf, o_conf, "keypoint confidences")
        assert_bit_equal(desc, o_desc, "descriptors")
        ora = to.OracleTracker(W, H, intr, capacity=512)
        ora.add(o_xy, o_desc, 1000, depth, 0.7, 30)
        diff = to.same_table(trk.download(), ora.flatten())
        assert diff is None, diff
        assert trk.keypointFailures() == 0
        counts.append(len(o_xy))
    assert min(counts) > 5 and not np.array_equal(imgs[0], imgs[1])
    for o in sps + trks:
        o.close()


# ---- 5. stale rows -------------------------------------------------------------------------------------------------------------
TW, TH = 64, 48
TK = (52.0, 51.5, 31.5, 23.25)
MAXKP = 100
STALE_N = [100, 37, 0, 100, 64, 37]


def stale_frames(seed):
    """six frames of keypoints out of one pool of descriptors, so that every frame's rows match live tracks exactly"""
    rng = np.random.default_rng(seed)
    pool = unit_rows(rng, 160)
    out = []
    for n in STALE_N:
        pick = rng.choice(pool.shape[0], n, replace=False) if n else np.zeros(0, np.int64)
        xy = np.stack([rng.integers(0, TW, n), rng.integers(0, TH, n)], 1).astype(np.int32)
        depth = rng.uniform(0.5, 4.0, (TH, TW)).astype(np.float32)
        depth[rng.random((TH, TW)) < 0.2] = 0.0
        out.append((xy, pool[pick].copy(), depth))
    return out


def same_tables(a, b, what):
    diff = to.same_table(a.download(), b.download())
    assert diff is None, (what, diff)


@pytest.mark.parametrize("view_log", [0, 4])
@pytest.mark.parametrize("capacity", [256, 128])
def test_stale_rows_never_enter_the_table(gpu_ctx, capacity, view_log):
    """n = 100, 37, 0, 100, 64, 37 in the SAME xy / descriptor buffers: the rows from n on are the previous frame's
    keypoints, which are live tracks now.  After every frame the table is that of a tracker given the host n and fresh
    arrays of n rows.  Capacity 128: appends drop, equally.  (Every download here waits and so resets both trackers'
    bound of the track count to the exact one: the looser bound of the device add is the next test's.)"""
    from multimotionfusion_amd.tracker import DevicePointTracker
    a = DevicePointTracker(gpu_ctx, TW, TH, TK, capacity=capacity, max_keypoints=MAXKP)
    b = DevicePointTracker(gpu_ctx, TW, TH, TK, capacity=capacity, max_keypoints=MAXKP)
    a.setViewLog(view_log), b.setViewLog(view_log)
    xy_buf = torch.zeros((MAXKP, 2), dtype=torch.int32, device="cuda")
    de_buf = torch.zeros((MAXKP, 256), dtype=torch.float32, device="cuda")
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    dropped = 0
    for i, (xy, de, depth) in enumerate(stale_frames(5)):
        n, ts = len(xy), 1000 + 33_000_000 * i
        if n:
            xy_buf[:n], de_buf[:n] = dev(xy), dev(de)
        n_dev.fill_(n)
        d_depth = dev(depth)
        a.addKeypointsDevice(n_dev, xy_buf, de_buf, ts, d_depth, 0.7, 30)
        assert a.lastLaunches() == (9 if view_log else 7)
        b.addKeypointsPixels(xy, de, ts, d_depth, 0.7, 30)
        assert b.lastLaunches() == a.lastLaunches()
        if i == 0:
            a.associateAll([1]), b.associateAll([1])
        same_tables(a, b, ("add", i, n))
        dropped = a.status()[2]
        print("frame", i, "n", n, "tracks", a.status()[0], "dropped", dropped)
    assert (dropped > 0) == (capacity == 128)
    if view_log:
        stamps = [3, 4, 5, 6]
        poses = np.stack([synth.make_pose((0.01 * k, 0.02, -0.01), (0.1, 0.02 * k, 0.3)).astype(np.float32) for k in range(4)])
        va, ma = a.modelViews(1, stamps, poses)
        vb, mb = b.modelViews(1, stamps, poses)
        assert ma == mb == 0 and sum(d.shape[0] for d, _ in va) > 0
        for (da, ca), (db, cb) in zip(va, vb):
            assert da.shape == db.shape and np.array_equal(bits(da), bits(db)) and np.array_equal(bits(ca), bits(cb))
    # the count is clamped to [0, max_keypoints]
    frames = stale_frames(6)
    xy, de, depth = frames[0]
    xy_buf[:], de_buf[:] = dev(xy), dev(de)
    d_depth = dev(depth)
    n_dev.fill_(1000)
    a.addKeypointsDevice(n_dev, xy_buf, de_buf, 5_000_000_000, d_depth, 0.7, 30)
    b.addKeypointsPixels(xy, de, 5_000_000_000, d_depth, 0.7, 30)
    same_tables(a, b, "n = 1000 is clamped to 100")
    n_dev.fill_(-3)
    a.addKeypointsDevice(n_dev, xy_buf, de_buf, 5_100_000_000, d_depth, 0.7, 30)
    b.addKeypointsPixels(np.zeros((0, 2), np.int32), np.zeros((0, 256), np.float32), 5_100_000_000, d_depth, 0.7, 30)
    same_tables(a, b, "n = -3 adds nothing")
    # a keypoint source that did not converge: a frame without keypoints, and the tracker says so
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    a.setKeypointStatus(status)
    n_dev.fill_(100)
    assert a.keypointFailures() == 0
    a.addKeypointsDevice(n_dev, xy_buf, de_buf, 5_200_000_000, d_depth, 0.7, 30)
    b.addKeypointsPixels(np.zeros((0, 2), np.int32), np.zeros((0, 256), np.float32), 5_200_000_000, d_depth, 0.7, 30)
    same_tables(a, b, "status 1 is a frame without keypoints")
    assert a.keypointFailures() == 1
    status.zero_()
    a.addKeypointsDevice(n_dev, xy_buf, de_buf, 5_300_000_000, d_depth, 0.7, 30)
    b.addKeypointsPixels(xy, de, 5_300_000_000, d_depth, 0.7, 30)
    same_tables(a, b, "status 0 again")
    assert a.keypointFailures() == 1
    a.setKeypointStatus(None)
    a.close(), b.close()


def search_rows(bound, capacity):
    """the train rows an add searches on for a host bound of the track count (tracker_host.hpp: nt_pad)"""
    return min((capacity + 63) // 64 * 64, max(64, (bound + 63) // 64 * 64))


@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("capacity", [256, 512])
def test_the_looser_bound_of_the_device_add_changes_no_bit(gpu_ctx, capacity, prune):
    """The six stale-row frames through the device add (and the front end's prune) with NO waiting call in between, as in
    a frame without -init kp: the host's bound of the track count is never refreshed and grows by max_keypoints per add
    -- 0, 100, 200, 256 (saturated at capacity 256) or 300, 400, 500 -- so the searches run on up to the whole capacity of
    padding rows.  The other tracker is given the host n and is waited for after every call, so its bound is the exact
    track count.  ONE comparison at the end: the table and the view log are bit-equal."""
    from multimotionfusion_amd.tracker import DevicePointTracker
    a = DevicePointTracker(gpu_ctx, TW, TH, TK, capacity=capacity, max_keypoints=MAXKP)
    b = DevicePointTracker(gpu_ctx, TW, TH, TK, capacity=capacity, max_keypoints=MAXKP)
    a.setViewLog(4), b.setViewLog(4)
    frames = stale_frames(5)
    stamps = [1000 + 33_000_000 * i for i in range(len(frames))]
    window = 40_000_000  # tracks last seen two frames ago or earlier go (none has 30 keypoints)
    # everything a reads is on the device before its first call: its loop below holds no copy from the host
    d_frames = [(len(xy), dev(xy) if len(xy) else None, dev(de) if len(xy) else None, dev(depth)) for xy, de, depth in frames]
    d_n = [torch.full((1,), n, dtype=torch.int32, device="cuda") for n, _, _, _ in d_frames]
    xy_buf = torch.zeros((MAXKP, 2), dtype=torch.int32, device="cuda")
    de_buf = torch.zeros((MAXKP, 256), dtype=torch.float32, device="cuda")
    bound_a, rows_a = 0, []
    for i, (n, d_xy, d_de, d_depth) in enumerate(d_frames):
        if n:
            xy_buf[:n].copy_(d_xy), de_buf[:n].copy_(d_de)
        rows_a.append(search_rows(bound_a, capacity))
        a.addKeypointsDevice(d_n[i], xy_buf, de_buf, stamps[i], d_depth, 0.7, 30)
        bound_a = min(capacity, bound_a + MAXKP)
        if i == 0:
            a.associateAll([1])
        if prune:
            a.prune(30, max(stamps[i] - window, 0))
    rows_b = []
    for i, ((xy, de, _), (_, _, _, d_depth)) in enumerate(zip(frames, d_frames)):
        rows_b.append(search_rows(b.status()[0], capacity))
        b.addKeypointsPixels(xy, de, stamps[i], d_depth, 0.7, 30)
        if i == 0:
            b.associateAll([1])
        if prune:
            b.prune(30, max(stamps[i] - window, 0))
    print("searched train rows, device add", rows_a, "host add", rows_b)
    assert all(x >= y for x, y in zip(rows_a, rows_b)) and sum(x > y for x, y in zip(rows_a, rows_b)) >= 2
    assert rows_a[-1] == (capacity + 63) // 64 * 64  # saturated: the whole capacity is searched
    same_tables(a, b, ("six adds, one wait", capacity, prune))
    assert a.status()[0] > 30 and a.status() == b.status()
    view_stamps = [3, 4, 5, 6]
    poses = np.stack([synth.make_pose((0.01 * k, 0.02, -0.01), (0.1, 0.02 * k, 0.3)).astype(np.float32) for k in range(4)])
    va, ma = a.modelViews(1, view_stamps, poses)
    vb, mb = b.modelViews(1, view_stamps, poses)
    assert ma == mb == 0 and sum(d.shape[0] for d, _ in va) > 0
    for (da, ca), (db, cb) in zip(va, vb):
        assert da.shape == db.shape and np.array_equal(bits(da), bits(db)) and np.array_equal(bits(ca), bits(cb))
    a.close(), b.close()


# ---- 6. the front end inside processFrame -----------------------------------------------------------------------------------
FW, FH = 160, 120
FMAX = 512
RAW = np.zeros(256, np.uint8)
RAW[1], RAW[2] = 37, 200


@pytest.fixture(scope="module")
def frontend_weights(orc):
    return orc.sp_random_weights(seed=4)


def choose_threshold(orc, weights, rgb, nms_dist=4, border=4):
    """a conf_thresh for which the oracle keeps between 50 and FMAX keypoints on this frame"""
    heat = orc.sp_heatmap(orc.sp_forward(orc.sp_input(rgb), weights)[0])
    for q in (0.0, 0.5, 0.8, 0.9, 0.95):
        thresh = max(0.015, float(np.quantile(heat, q)))
        n = len(orc.sp_keypoints(heat, thresh, nms_dist, border)[0])
        if 50 <= n <= FMAX:
            print("conf_thresh", thresh, "keeps", n)
            return thresh, n
    raise AssertionError("no threshold keeps between 50 and max_keypoints keypoints")


def run_front_end(gpu_ctx, weights, thresh, K, frames, on_device, icp_refine, masks=None):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import MaskConfig
    from multimotionfusion_amd.superpoint import SuperPoint
    from multimotionfusion_amd.tracker import NativeKeypointFrontEnd
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    if masks is None:
        g = MultiMotionFusion(gpu_ctx, FW, FH, K["cx"], K["cy"], K["fx"], K["fy"])
    else:
        g = MultiMotionFusion(gpu_ctx, FW, FH, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=2)
        g.setMaskSegmentation(MaskConfig(model_spawn_offset=1))
    sp = SuperPoint(gpu_ctx, weights, max_width=FW, max_height=FH, max_keypoints=FMAX, conf_thresh=thresh)
    fe = NativeKeypointFrontEnd(gpu_ctx, g, sp, intr, icp_refine=icp_refine, capacity=2048, max_keypoints=FMAX, on_device=on_device)
    out, keep = [], []
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"]), dev(masks[i]) if masks is not None else None))
        extra = dict(mask=keep[-1][2]) if masks is not None else {}
        fe.processFrame(keep[-1][0], keep[-1][1], timestamp=1000 + 33_000_000 * i, **extra)
        out.append(dict(pose=g.getCurrPose().copy(), T=g.getLastTrackTransforms().copy(), ids=[m.id for m in g.getModels()],
                        poses=[m.getPose().copy() for m in g.getModels()]))
    table = fe.tracker.download()
    failures = fe.tracker.keypointFailures()
    fe.close()
    sp.close()
    g.close()
    return out, table, failures


def assert_same_runs(a, b):
    (fa, ta, _), (fb, tb, failures) = a, b
    assert failures == 0
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert np.array_equal(bits(x["pose"]), bits(y["pose"])), (i, x["pose"], y["pose"])
        assert x["T"].shape == y["T"].shape and np.array_equal(bits(x["T"]), bits(y["T"])), (i, "track transforms")
        assert x["ids"] == y["ids"], i
        for p, q in zip(x["poses"], y["poses"]):
            assert np.array_equal(bits(p), bits(q)), (i, "model poses")
    diff = to.same_table(tb, ta)
    assert diff is None, diff
    print("tracks", ta["n_tracks"], "models", fa[-1]["ids"], "transforms per frame", [f["T"].shape[0] for f in fa])
    assert ta["n_tracks"] > 50


@pytest.fixture(scope="module")
def landmark_frames():
    K = synth.intrinsics(FW, FH)
    poses = synth.trajectory(5, seed=5)
    return K, [synth.render(p, FW, FH, seed=i) for i, p in enumerate(poses)]


@pytest.mark.parametrize("icp_refine", [True, False])
def test_in_frame_front_end_equals_the_caller_driven_one(gpu_ctx, orc, frontend_weights, landmark_frames, icp_refine):
    K, frames = landmark_frames
    thresh, n0 = choose_threshold(orc, frontend_weights, frames[0]["rgb"])
    assert 50 <= n0 <= FMAX
    a = run_front_end(gpu_ctx, frontend_weights, thresh, K, frames, False, icp_refine)
    b = run_front_end(gpu_ctx, frontend_weights, thresh, K, frames, True, icp_refine)
    assert_same_runs(a, b)
    assert any(f["T"].shape[0] == 1 for f in a[0][1:])


def test_in_frame_front_end_with_moving_objects(gpu_ctx, orc, frontend_weights):
    """the two-box scene of tests/test_gpu_tracker_fusion.py segmented from its label images: spawns, associate and forget
    come in the same order whichever front end adds the keypoints"""
    seed, n = 21, 6
    K = synth.intrinsics(FW, FH)
    poses = synth.trajectory(n, seed=seed)
    objs = synth.make_objects(2, seed=seed)
    traj = synth.object_trajectories(objs, n, seed=seed)
    frames = [synth.render(p, FW, FH, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    masks = [RAW[f["ids"].astype(np.uint8)] for f in frames]
    thresh, n0 = choose_threshold(orc, frontend_weights, frames[0]["rgb"])
    assert 50 <= n0 <= FMAX
    a = run_front_end(gpu_ctx, frontend_weights, thresh, K, frames, False, True, masks)
    b = run_front_end(gpu_ctx, frontend_weights, thresh, K, frames, True, True, masks)
    assert_same_runs(a, b)
    assert len(a[0][-1]["ids"]) > 1  # object models were spawned and tracked


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, frontend_weights, landmark_frames):
    from multimotionfusion_amd._capi import mmf_keypoint_frontend_config
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.superpoint import SuperPoint
    from multimotionfusion_amd.tracker import DevicePointTracker
    import ctypes as C
    K, frames = landmark_frames
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    sp = SuperPoint(gpu_ctx, frontend_weights, max_width=FW, max_height=FH, max_keypoints=64)
    small = SuperPoint(gpu_ctx, frontend_weights, max_width=FW - 8, max_height=FH - 8, max_keypoints=64)
    many = SuperPoint(gpu_ctx, frontend_weights, max_width=FW, max_height=FH, max_keypoints=128)
    trk = DevicePointTracker(gpu_ctx, FW, FH, intr, capacity=256, max_keypoints=64)
    g = MultiMotionFusion(gpu_ctx, FW, FH, K["cx"], K["cy"], K["fx"], K["fy"])
    with pytest.raises(MmfError) as e:  # no tracker
        g.setKeypointFrontEnd(sp)
    assert e.value.status == -4
    g.setShard(0, 2)
    with pytest.raises(MmfError) as e:  # not on a shard
        g.setKeypointFrontEnd(sp)
    assert e.value.status == -4
    g.close()
    g = MultiMotionFusion(gpu_ctx, FW, FH, K["cx"], K["cy"], K["fx"], K["fy"])
    g.setTracker(trk)
    with pytest.raises(MmfError) as e:  # the frame is larger than the network serves
        g.setKeypointFrontEnd(small)
    assert e.value.status == -1
    with pytest.raises(MmfError) as e:  # more keypoints than the tracker takes
        g.setKeypointFrontEnd(many)
    assert e.value.status == -1
    assert gpu_ctx.lib.mmf_fusion_set_keypoint_frontend(g.handle, sp.handle, None) == -1  # null configuration
    assert gpu_ctx.lib.mmf_keypoint_frontend_default_config(None) == -1
    big = dev(np.zeros((FH * 2, FW * 2, 3), np.uint8))
    with pytest.raises(MmfError) as e:  # an image larger than max_width x max_height
        sp.getFeaturesDevice(big)
    assert e.value.status == -1
    g.setKeypointFrontEnd(sp)
    rgb, depth = dev(frames[0]["rgb"]), dev(frames[0]["depth"])
    g.processFrame(rgb, depth, timestamp=1000)
    assert g.getTick() == 2 and trk.frame() == 1
    trk.addKeypointsPixels(np.zeros((0, 2), np.int32), np.zeros((0, 256), np.float32), 2000, depth)
    with pytest.raises(MmfError) as e:  # the caller added this frame's keypoints itself
        g.processFrame(rgb, depth, timestamp=2000)
    assert e.value.status == -1 and "keypoint front end" in str(e.value)
    assert g.getTick() == 2 and trk.frame() == 2
    g.processFrame(rgb, depth, timestamp=3000)  # the next frame is the front end's again
    assert g.getTick() == 3 and trk.frame() == 3
    g.setKeypointFrontEnd(None)
    g.processFrame(rgb, depth, timestamp=4000)  # off: nothing is added
    assert trk.frame() == 3
    g.setKeypointFrontEnd(sp)
    assert g._kp_predictor is sp
    g.setTracker(trk, icp_refine=False)  # any setTracker switches the front end off, and the object says so
    assert g._kp_predictor is None
    g.processFrame(rgb, depth, timestamp=5000)
    assert trk.frame() == 3
    cfg = mmf_keypoint_frontend_config()
    assert gpu_ctx.lib.mmf_keypoint_frontend_default_config(C.byref(cfg)) == 0 and cfg.history == 30
    g.setTracker(None)
    g.close()
    for o in (sp, small, many, trk):
        o.close()


# ---- 8. the C++ shim ---------------------------------------------------------------------------------------------------------
def test_shim_front_end_on_device(gpu_ctx, tmp_path):
    """cpp/MultiMotionFusion.h with setKeypointFrontEndOnDevice(true) against (false): three frames, the same poses and
    track counts (tests/cpp/keypoint_device_check.cpp, built with -Wall -Wextra -Werror like the other shim programs)"""
    from multimotionfusion_amd import build
    from multimotionfusion_amd.superpoint import random_weights
    build.build(verbose=False)
    n = 3
    K = synth.intrinsics(FW, FH)
    frames = [synth.render(p, FW, FH, seed=i) for i, p in enumerate(synth.trajectory(n, seed=5))]
    data, wfile = tmp_path / "frames.bin", tmp_path / "weights.bin"
    with open(data, "wb") as fp:
        for f in frames:
            fp.write(np.ascontiguousarray(f["rgb"], np.uint8).tobytes())
            fp.write(np.ascontiguousarray(f["depth"], np.float32).tobytes())
    with open(wfile, "wb") as fp:
        for w, b in random_weights(3):
            fp.write(np.ascontiguousarray(w, np.float32).tobytes())
            fp.write(np.ascontiguousarray(b, np.float32).tobytes())
    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "keypoint_device_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "keypoint_device_check.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    k = [np.float32(K[name]) for name in ("cx", "cy", "fx", "fy")]
    r = subprocess.run([str(exe), str(data), str(wfile), str(FW), str(FH), str(n)] + [f"{float(v):.9g}" for v in k],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "poses agree: 1" in r.stdout and "tracks agree: 1" in r.stdout, r.stdout
