"""-m gpu: the device track table (multimotionfusion_amd/tracker.py, csrc/tracker_kernels.hpp) against tests/tracker_oracle.py,
bit for bit after every step of random sequences on a 64 x 48 depth image with a capacity of 256 tracks."""
import numpy as np
import pytest
import torch

import tracker_oracle as to

pytestmark = pytest.mark.gpu

W, H = 64, 48
K = (52.0, 51.5, 31.5, 23.25)
CAP = 256
IDS = [0, 1, 2, 31, 32, 63, 64, 200, 254]  # 9 model ids up to 254: every word of the set, both ends of a word
SIZES = [64, 200, 0, 65, 1, 63, 200, 64, 200, 0, 65, 200]  # n of the steps: 0, 1, 63, 64, 65, 200


def unit_rows(rng, n, dim=256):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def make_pool(rng, n=320):
    """base descriptors; rows 2k and 2k + 1 are the same row for k < 24: ties in the search (the smallest index wins)"""
    pool = unit_rows(rng, n)
    pool[1:48:2] = pool[0:48:2]
    return pool


def make_step(rng, pool, n, step):
    """keypoints of one frame: descriptors = pool rows, exact or disturbed (distances on both sides of 0.7); pixels anywhere
    in the image, the last row / column and the corner included, one outside; a depth image with zero pixels"""
    pick = rng.choice(pool.shape[0], n, replace=False) if n else np.zeros(0, np.int64)
    if n >= 63:
        pick[:16] = rng.permutation(32)[:16]  # from the duplicated rows
    desc = pool[pick].copy()
    scale = rng.choice([0.0, 0.0, 0.02, 0.6, 1.5], n).astype(np.float32)[:, None]
    desc = desc + scale * unit_rows(rng, n) if n else desc
    desc = (desc / np.maximum(np.linalg.norm(desc, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    desc[scale[:, 0] == 0.0] = pool[pick][scale[:, 0] == 0.0]  # exactly the pool's rows
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32)
    if n >= 1:
        xy[0] = (W - 1, H - 1)
    if n >= 63:
        xy[1], xy[2], xy[3] = (W - 1, 5), (7, H - 1), (0, 0)
        xy[4] = (W, 3) if step % 2 else (-1, H)  # outside: NaN coordinates, no label
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.2] = 0.0
    return xy, desc, depth


def make_mask(rng):
    mask = rng.choice(np.array(IDS + [7, 255], np.uint8), (H // 8, W // 8)).repeat(8, 0).repeat(8, 1)
    return np.ascontiguousarray(mask)


def check_table(dev, ora, what):
    diff = to.same_table(dev.download(), ora.flatten())
    assert diff is None, (what, diff)


def check_pairs(dev, ora, ids, what):
    got = dev.lastPairs(ids)
    assert len(got) == len(ids)
    for m, (p0, p1) in zip(ids, got):
        w0, w1 = ora.last_pairs(m)
        assert p0.shape == w0.shape and np.array_equal(p0.view(np.uint32), w0.view(np.uint32)), (what, m)
        assert np.array_equal(p1.view(np.uint32), w1.view(np.uint32)), (what, m)


@pytest.mark.parametrize("min_feature_distance", [0.0, 0.7])
@pytest.mark.parametrize("history", [0, 1, 2, 30])
def test_random_sequences_match_the_oracle_after_every_step(gpu_ctx, orc, history, min_feature_distance):
    from multimotionfusion_amd.tracker import DevicePointTracker
    rng = np.random.default_rng(100 + 10 * history + int(min_feature_distance > 0))
    pool = make_pool(rng)
    dev = DevicePointTracker(gpu_ctx, W, H, K, capacity=CAP, max_keypoints=200)
    ora = to.OracleTracker(W, H, K, capacity=CAP)
    launches = {"add": set(), "prune": set(), "pairs1": set(), "pairs9": set()}
    full = False
    for step, n in enumerate(SIZES):
        ts = 1_000_000 + 33_000 * step
        xy, desc, depth = make_step(rng, pool, n, step)
        dev.addKeypointsPixels(xy, desc, ts, torch.from_numpy(depth).cuda(), min_feature_distance, history)
        launches["add"].add(dev.lastLaunches())
        ora.add(xy, desc, ts, depth, min_feature_distance, history)
        check_table(dev, ora, ("add", step, n))
        full = full or len(ora.tracks) == CAP
        if step == 0:
            dev.associateAll([0])
            ora.associate_all([0])
        elif step % 3 == 1:
            dev.associateAll(IDS[:2])
            ora.associate_all(IDS[:2])
        else:
            mask = make_mask(rng)
            dev.associate(torch.from_numpy(mask).cuda(), IDS)
            ora.associate(mask, IDS)
        check_table(dev, ora, ("associate", step))
        check_pairs(dev, ora, [0], ("pairs 1", step))
        launches["pairs1"].add(dev.lastLaunches())
        check_pairs(dev, ora, IDS, ("pairs 9", step))
        launches["pairs9"].add(dev.lastLaunches())
        vis_d, vis_o = dev.visible(), ora.visible()
        for g, w in zip(vis_d, vis_o):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                                         w.view(np.uint32) if w.dtype == np.float32 else w), ("visible", step)
        if step in (5, 9):
            dev.forgetModel(IDS[step % 9])
            ora.forget(IDS[step % 9])
        if step in (4, 7, 10):  # tracks seen once, last more than two frames ago, go; the rest close up
            dev.prune(2, ts - 2 * 33_000)
            launches["prune"].add(dev.lastLaunches())
            ora.prune(2, ts - 2 * 33_000)
            check_table(dev, ora, ("prune", step))
    assert full and ora.dropped > 0  # the sequence reached the capacity and went past it
    assert dev.status() == (len(ora.tracks), len(ora.tracks[0]), ora.dropped)
    assert all(len(v) == 1 for v in launches.values()), launches  # the same launches for every size
    # a prune that empties the table, then an add: the length restarts at 1, uids go on
    dev.prune(1 << 30, 1 << 60)
    ora.prune(1 << 30, 1 << 60)
    check_table(dev, ora, "emptied")
    assert dev.status()[:2] == (0, 0)
    dev.addKeypointsPixels(np.zeros((0, 2), np.int32), np.zeros((0, 256), np.float32), 1, torch.zeros((H, W)).cuda())
    ora.add(np.zeros((0, 2)), np.zeros((0, 256)), 1, np.zeros((H, W), np.float32))
    check_table(dev, ora, "n == 0 into an empty table")
    xy, desc, depth = make_step(rng, pool, 65, 1)
    dev.addKeypointsPixels(xy, desc, 5_000_000, torch.from_numpy(depth).cuda(), min_feature_distance, history)
    ora.add(xy, desc, 5_000_000, depth, min_feature_distance, history)
    check_table(dev, ora, "restart")
    assert dev.status()[:2] == (65, 1)
    dev.close()


def test_full_table_is_left_alone_and_drops_are_counted(gpu_ctx, orc):
    """every keypoint far from every track at the capacity: nothing is appended, every row of the table is what it was
    except for the shift by one null keypoint, and `dropped` grows by n"""
    from multimotionfusion_amd.tracker import DevicePointTracker
    rng = np.random.default_rng(7)
    dev = DevicePointTracker(gpu_ctx, W, H, K, capacity=CAP, max_keypoints=200)
    ora = to.OracleTracker(W, H, K, capacity=CAP)
    for step, n in enumerate([200, 200, 65]):
        xy, _, depth = make_step(rng, make_pool(rng), n, step)
        desc = unit_rows(rng, n)  # random unit rows: distance ~ 1.41 > 0.7 to everything
        dev.addKeypointsPixels(xy, desc, 10 + step, torch.from_numpy(depth).cuda(), 0.7, 30)
        ora.add(xy, desc, 10 + step, depth, 0.7, 30)
        check_table(dev, ora, step)
    assert dev.status() == (CAP, 3, 200 + 200 + 65 - CAP)
    f = dev.download()
    assert np.array_equal(f["uid"], np.arange(CAP)) and not f["nonnull"][0].any()
    assert not f["nonnull"][1, :200].any() and f["nonnull"][1, 200:].all()  # rows 200 .. 255 were born one frame ago
    dev.close()


def test_more_tracks_than_one_pass_of_the_workgroup(gpu_ctx, orc):
    """2500 tracks, 1100 keypoints a frame: the bookkeeping workgroup (1024 lanes) takes several passes over tracks and
    keypoints, ranks carry over from pass to pass, and prune closes up across them"""
    from multimotionfusion_amd.tracker import DevicePointTracker
    rng = np.random.default_rng(21)
    cap, n = 2500, 1100
    dev = DevicePointTracker(gpu_ctx, W, H, K, capacity=cap, max_keypoints=n)
    ora = to.OracleTracker(W, H, K, capacity=cap)
    base = unit_rows(rng, 3 * n)
    for step in range(4):
        desc = base[rng.permutation(3 * n)[:n]]  # about a third of them continue a track
        xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32)
        depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
        depth[rng.random((H, W)) < 0.2] = 0.0
        dev.addKeypointsPixels(xy, desc, 100 + step, torch.from_numpy(depth).cuda(), 0.7, 2)
        ora.add(xy, desc, 100 + step, depth, 0.7, 2)
        check_table(dev, ora, ("add", step))
        mask = make_mask(rng)
        dev.associate(torch.from_numpy(mask).cuda(), IDS)
        ora.associate(mask, IDS)
        check_table(dev, ora, ("associate", step))
        check_pairs(dev, ora, IDS, ("pairs", step))
        peak = len(ora.tracks)
        if step == 3:
            dev.prune(2, 103)
            ora.prune(2, 103)
            check_table(dev, ora, "prune")
    assert peak == cap and ora.dropped > 0 and 1024 < len(ora.tracks) < peak
    for g, w in zip(dev.visible(), ora.visible()):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                                     w.view(np.uint32) if w.dtype == np.float32 else w)
    dev.close()


def test_last_track_transform_equals_the_oracles(gpu_ctx, orc):
    """a rigid motion of 60 keypoints, four of them without depth: the transformation, error and inlier set of a fresh
    RigidRANSAC on the table's pairs; a model without tracks: identity and no inliers"""
    from multimotionfusion_amd.tracker import DevicePointTracker
    rng = np.random.default_rng(11)
    dev = DevicePointTracker(gpu_ctx, W, H, K, capacity=CAP, max_keypoints=200)
    ora = to.OracleTracker(W, H, K, capacity=CAP)
    n = 60
    flat = rng.choice(W * H, n, replace=False)
    xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
    desc = unit_rows(rng, n)
    for step in range(2):
        depth = (2.0 + 0.01 * np.arange(W)[None, :] + 0.02 * np.arange(H)[:, None] + 0.1 * step).astype(np.float32)
        if step:
            depth[xy[:4, 1], xy[:4, 0]] = 0.0
        dev.addKeypointsPixels(xy, desc, step, torch.from_numpy(depth).cuda(), 0.7, 30)
        ora.add(xy, desc, step, depth, 0.7, 30)
        dev.associateAll([0, 5])
        ora.associate_all([0, 5])
    for m in (0, 5, 9):
        T, err, inl = dev.getLastTrackTransform(m)
        Tw, errw, inlw = ora.last_track_transform(m)
        assert np.array_equal(T.view(np.uint32), Tw.view(np.uint32)), m
        assert (inl is None) == (inlw is None) and (err == errw or (np.isinf(err) and np.isinf(errw)))
        if inlw is not None:
            assert np.array_equal(inl[:inlw.size], inlw) and not inl[inlw.size:].any()
    assert ora.last_pairs(0)[0].shape == (n - 4, 3) and ora.last_pairs(9)[0].shape == (0, 3)
    dev.close()


def test_bad_arguments_are_refused(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.tracker import DevicePointTracker
    dev = DevicePointTracker(gpu_ctx, W, H, K, capacity=CAP, max_keypoints=8)
    depth = torch.ones((H, W), device="cuda")
    with pytest.raises(MmfError):  # more keypoints than max_keypoints
        dev.addKeypointsPixels(np.zeros((9, 2), np.int32), np.zeros((9, 256), np.float32), 0, depth)
    with pytest.raises(MmfError):  # model ids are 0 .. 255
        dev.associateAll([256])
    with pytest.raises(MmfError):
        dev.lastPairs([-1])
    assert dev.status() == (0, 0, 0)
    dev.close()
