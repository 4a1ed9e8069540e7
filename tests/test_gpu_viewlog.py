"""-m gpu: the tracker's view log, the views built from it on the device (mmf_tracker_set_view_log, mmf_tracker_model_views;
csrc/tracker_kernels.hpp) and their way into the view store without the host (mmf_viewstore_store_device) against
tests/viewlog_oracle.py and mmf_viewstore_store, bit for bit, on a 64 x 48 depth image."""
import numpy as np
import pytest
import torch

import tracker_oracle as to
import viewlog_oracle as vo

pytestmark = pytest.mark.gpu

W, H = 64, 48
K = (52.0, 51.5, 31.5, 23.25)
IDS = [1, 31, 32, 37, 254]  # both sides of a word of `member`, the last id


def make_mask(rng, ids=IDS):
    return np.ascontiguousarray(rng.choice(np.array(ids + [7, 0], np.uint8), (H // 8, W // 8)).repeat(8, 0).repeat(8, 1))


class Pair:
    """the device tracker and the oracle, driven together"""

    def __init__(self, ctx, capacity, max_keypoints, log_frames):
        from multimotionfusion_amd.tracker import DevicePointTracker
        self.dev = DevicePointTracker(ctx, W, H, K, capacity=capacity, max_keypoints=max_keypoints)
        self.ora = vo.ViewLogOracle(to.OracleTracker(W, H, K, capacity=capacity), 0)
        self.launches = {"add": set(), "views": set()}
        self.set_view_log(log_frames)

    def set_view_log(self, frames):
        self.dev.setViewLog(frames)
        self.ora.set_view_log(frames)

    def add(self, xy, desc, ts, depth, history=30):
        self.dev.addKeypointsPixels(xy, desc, ts, torch.from_numpy(depth).cuda(), 0.7, history)
        self.launches["add"].add(self.dev.lastLaunches())
        self.ora.add(xy, desc, ts, depth, 0.7, history)
        assert self.dev.frame() == self.ora.stamp

    def associate(self, mask, ids):
        self.dev.associate(torch.from_numpy(mask).cuda(), ids)
        self.ora.t.associate(mask, ids)

    def associate_all(self, ids):
        self.dev.associateAll(ids)
        self.ora.t.associate_all(ids)

    def prune(self, min_kps, min_time):
        self.dev.prune(min_kps, min_time)
        self.ora.t.prune(min_kps, min_time)

    def forget(self, m):
        self.dev.forgetModel(m)
        self.ora.t.forget(m)

    def reset(self):
        self.dev.reset()
        self.ora.reset()

    def check(self, model_id, stamps, poses, what):
        got, missing = self.dev.modelViews(model_id, stamps, poses)
        self.launches["views"].add(self.dev.lastLaunches())
        want, missing_w = self.ora.model_views(model_id, stamps, poses)
        assert missing == missing_w, (what, model_id)
        diff = vo.same_views(got, want)
        assert diff is None, (what, model_id, diff)
        return want


def window(pair, rng):
    """the stamps around the ring: two that have left it, the ones in it, one in the future; a pose for each"""
    hi = pair.ora.stamp
    stamps = list(range(max(hi - pair.ora.frames - 1, -1), hi + 2))
    return stamps, [vo.random_pose(rng) for _ in stamps]


@pytest.mark.parametrize("capacity,max_kp,log_frames,n_frames", [(128, 16, 4, 20), (256, 64, 5, 24), (512, 256, 8, 30)])
def test_random_sequences_match_the_oracle_after_every_step(gpu_ctx, orc, capacity, max_kp, log_frames, n_frames):
    """adds of 0 .. max_keypoints keypoints, associations, prunes and forgotten models; the ring wraps several times.  After
    every step the views of two of the models over the whole window, at the end those of all models and of one without tracks"""
    rng = np.random.default_rng(capacity + max_kp)
    pool = vo.unit_rows(rng, 2 * max_kp)
    p = Pair(gpu_ctx, capacity, max_kp, log_frames)
    seen = dict(pruned=False, nan=False, rows=0, left=False)
    for step in range(n_frames):
        ts = 1_000_000 + 33_000 * step
        n = [max_kp, max_kp // 2, 0, 1, max_kp - 1][step % 5] if step else max_kp
        xy, desc, depth = vo.make_step(rng, pool, n, W, H)
        p.add(xy, desc, ts, depth)
        two = [IDS[step % 5], IDS[(step + 2) % 5]]
        stamps, poses = window(p, rng)
        if step % 4 == 0:
            p.associate_all(IDS[:2])
        else:
            p.associate(make_mask(rng), IDS)
        for m in two:
            want = p.check(m, stamps, poses, ("associate", step))
            seen["rows"] += sum(d.shape[0] for d, _ in want)
        if step % 7 == 6:
            p.forget(IDS[step % 5])
            p.check(IDS[step % 5], stamps, poses, ("forget", step))
        if step % 6 == 5:  # tracks seen once, last more than two frames ago, go: they leave the views with the table
            before = {t.uid for t in p.ora.t.tracks}
            p.prune(2, ts - 2 * 33_000)
            gone = before - {t.uid for t in p.ora.t.tracks}
            logged = {int(u) for s in p.ora.ring if s is not None for u in s["uid"]}
            seen["pruned"] = seen["pruned"] or bool(gone & logged)
            for m in two:
                p.check(m, stamps, poses, ("prune", step))
        seen["nan"] = seen["nan"] or any(s is not None and not np.all(np.isfinite(s["coordinate"])) for s in p.ora.ring)
        seen["left"] = seen["left"] or p.ora.stamp > log_frames
    stamps, poses = window(p, rng)
    for m in IDS + [9]:
        p.check(m, stamps, poses, "end")
    assert p.check(9, stamps, poses, "no tracks")[2][0].shape[0] == 0
    assert seen["pruned"] and seen["nan"] and seen["left"] and seen["rows"] > 50, seen
    assert p.launches["add"] == {9} and p.launches["views"] == {2}, p.launches
    # n_views == 0, the same launches
    got, missing = p.dev.modelViews(1, [], np.zeros((0, 4, 4), np.float32))
    assert got == [] and missing == 0 and p.dev.lastLaunches() == 2
    # a pose with an Inf entry drops the whole view; the others stay
    bad = [P.copy() for P in poses]
    bad[-2][1, 3] = np.inf
    want = p.check(1, stamps, bad, "inf pose")
    assert want[-2][0].shape[0] == 0
    # after a reset nothing is in the ring and the stamps restart
    p.reset()
    assert p.dev.frame() == 0
    p.check(1, stamps, poses, "reset")
    assert p.dev.modelViews(1, stamps, poses)[1] == len(stamps)
    xy, desc, depth = vo.make_step(rng, pool, max_kp, W, H)
    p.add(xy, desc, 5_000_000, depth)
    p.associate_all([1])
    want = p.check(1, [0, 1, 2], poses[:3], "after reset")
    assert want[1][0].shape[0] > 0 and want[0][0].shape[0] == 0
    # off and on again starts empty; off: an add is the parent's 7 launches
    p.set_view_log(0)
    p.add(xy, desc, 5_033_000, depth)
    assert p.dev.lastLaunches() == 7
    p.check(1, [1, 2], poses[:2], "off")
    p.set_view_log(log_frames)
    p.check(1, [1, 2], poses[:2], "on again")
    assert p.dev.modelViews(1, [1, 2], poses[:2])[1] == 2
    p.add(xy, desc, 5_066_000, depth)
    assert p.dev.lastLaunches() == 9
    p.associate_all([1])
    want = p.check(1, [1, 2, 3], poses[:3], "logged again")
    assert want[2][0].shape[0] > 0 and want[1][0].shape[0] == 0
    p.dev.close()


def test_the_log_is_off_by_default(gpu_ctx, orc):
    """a tracker nobody switched the log on for: the parent's 7 launches per add, every requested frame missing"""
    rng = np.random.default_rng(3)
    p = Pair(gpu_ctx, 128, 32, 0)
    pool = vo.unit_rows(rng, 64)
    for step in range(3):
        xy, desc, depth = vo.make_step(rng, pool, 32, W, H)
        p.add(xy, desc, 10 + step, depth)
    p.associate_all([1])
    assert p.launches["add"] == {7}
    stamps, poses = [1, 2, 3], [vo.random_pose(rng) for _ in range(3)]
    want = p.check(1, stamps, poses, "off")
    assert p.dev.modelViews(1, stamps, poses)[1] == 3 and all(d.shape[0] == 0 for d, _ in want)
    assert to.same_table(p.dev.download(), p.ora.t.flatten()) is None
    p.dev.close()


def test_more_rows_than_one_pass_of_the_workgroup(gpu_ctx, orc):
    """1100 keypoints a frame, a table of 2304 tracks: a view's walk over its slot and the table the uids are looked up in
    both exceed one pass of the 1024 lanes"""
    rng = np.random.default_rng(21)
    cap, n = 2304, 1100
    p = Pair(gpu_ctx, cap, n, 4)
    base = vo.unit_rows(rng, 3 * n)
    for step in range(5):
        # rows 0 .. n, the next n, a mix (a third of it new), rows 0 .. n again -- all of them continue their tracks --, a mix
        desc = base[[np.arange(n), np.arange(n, 2 * n), None, np.arange(n), None][step]] if step not in (2, 4) else base[rng.permutation(3 * n)[:n]]
        xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32)
        depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)  # (no holes: every keypoint of frame 4 makes a row)
        p.add(xy, desc, 100 + step, depth, history=0)
        p.associate(make_mask(rng, [1, 37]), [1, 37])
    p.associate_all([254])
    p.prune(2, 103)
    assert 1024 < len(p.ora.t.tracks) <= cap
    stamps, poses = window(p, rng)
    rows = [d.shape[0] for d, _ in p.check(254, stamps, poses, "all tracks")]
    assert max(rows) > 1024, rows
    for m in (1, 37):
        p.check(m, stamps, poses, "by mask")
    p.dev.close()


@pytest.fixture()
def row_views(gpu_ctx, orc):
    """one tracker whose frames 1 .. 5 hold 0, 1, 31, 32 and 33 keypoints, all with depth, all in models 1 and 2"""
    rng = np.random.default_rng(5)
    p = Pair(gpu_ctx, 256, 64, 8)
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    for step, n in enumerate([0, 1, 31, 32, 33]):
        flat = rng.choice(W * H, n, replace=False)
        xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
        p.add(xy, vo.unit_rows(rng, n), 100 + step, depth)  # random unit rows: far from every track, all of them new
    p.associate_all([1, 2])
    yield p, rng
    p.dev.close()


def same_store(ctx, a, b, rng, models):
    """two stores answer alike: the views, the matches of 3 random query sets and the best match of every model, bit for bit"""
    assert a.views() == b.views()
    for nq in (40, 7, 33):
        q = torch.from_numpy(vo.unit_rows(rng, nq)).cuda()
        (ia, da), (ib, db) = a.match(q), b.match(q)
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    return True


def test_store_device_leaves_the_store_the_host_path_leaves(gpu_ctx, row_views):
    """views of 0, 1, 31, 32 and 33 rows through mmf_viewstore_store_device against mmf_viewstore_store with the same views
    downloaded; a second store of the model changes nothing; a second model whose 70 views make the buffers grow leaves the
    first model's rows as they are"""
    from multimotionfusion_amd.redetection import ViewStore
    p, rng = row_views
    stamps = [1, 2, 3, 4, 5, 9]  # (9: not in the ring)
    poses = [vo.random_pose(rng) for _ in stamps]
    want = p.check(1, stamps, poses, "rows")
    assert [d.shape[0] for d, _ in want] == [0, 1, 31, 32, 33, 0]
    dev_store, host_store = ViewStore(gpu_ctx), ViewStore(gpu_ctx)
    counts, de, co, missing = p.dev.modelViewsDevice(1, stamps, poses)
    assert list(counts) == [0, 1, 31, 32, 33, 0] and missing == 1
    assert dev_store.storeDevice(1, counts, de, co)
    assert host_store.store(1, want)
    assert not dev_store.storeDevice(1, counts, de, co)  # Model::store: stored before, nothing changes
    assert dev_store.views() == [(1, v, n) for v, n in enumerate([0, 1, 31, 32, 33, 0])]
    assert same_store(gpu_ctx, dev_store, host_store, rng, [1])
    # the best match finds the view a query set was taken from, with the same transformation, error and inliers
    P = poses[4]
    query, coord = want[4]
    moved = (coord.astype(np.float64) @ P[:3, :3].T.astype(np.float64)).astype(np.float32)  # some rigid motion of the view
    q = torch.from_numpy(query.copy()).cuda()
    ba, bb = dev_store.bestMatch(1, q, moved), host_store.bestMatch(1, q, moved)
    assert ba["found"] and ba["view"] == 4 and ba["n_matches"] == 33 and ba["inliers"] > 5 and ba["error"] < 0.01
    for key in ("found", "view", "n_matches", "inliers"):
        assert ba[key] == bb[key]
    assert np.float32(ba["error"]).view(np.uint32) == np.float32(bb["error"]).view(np.uint32)
    assert np.array_equal(ba["transformation"].view(np.uint32), bb["transformation"].view(np.uint32))
    assert np.array_equal(ba["inlier"], bb["inlier"])
    # a second model: 70 views of 33 rows = 4480 padded rows behind the first model's 160, past the first 4096
    q_first = torch.from_numpy(vo.unit_rows(rng, 20)).cuda()
    first_before = dev_store.match(q_first)
    stamps2 = [5] * 70
    poses2 = [vo.random_pose(rng) for _ in stamps2]
    want2 = p.check(2, stamps2, poses2, "second model")
    counts2, de2, co2, _ = p.dev.modelViewsDevice(2, stamps2, poses2)
    assert dev_store.storeDevice(2, counts2, de2, co2) and host_store.store(2, want2)
    first_after = dev_store.match(q_first)
    assert np.array_equal(first_before[0], first_after[0][:6]) and np.array_equal(first_before[1].view(np.uint32), first_after[1][:6].view(np.uint32))
    assert same_store(gpu_ctx, dev_store, host_store, rng, [1, 2])
    bb2, ba2 = host_store.bestMatch(2, q, moved), dev_store.bestMatch(2, q, moved)
    assert ba2["found"] == bb2["found"] and ba2["view"] == bb2["view"] and ba2["inliers"] == bb2["inliers"]
    assert np.array_equal(ba2["transformation"].view(np.uint32), bb2["transformation"].view(np.uint32))
    ba, bb = dev_store.bestMatch(1, q, moved), host_store.bestMatch(1, q, moved)
    assert ba["found"] and ba["view"] == 4 and np.array_equal(ba["transformation"].view(np.uint32), bb["transformation"].view(np.uint32))
    dev_store.close(), host_store.close()


def test_a_store_of_empty_views_and_bad_arguments(gpu_ctx, row_views):
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.redetection import ViewStore
    p, rng = row_views
    vs = ViewStore(gpu_ctx)
    counts, de, co, missing = p.dev.modelViewsDevice(1, [1, 40], [vo.random_pose(rng)] * 2)  # no keypoints; not in the ring
    assert list(counts) == [0, 0] and missing == 1 and de.shape == (0, 256)
    assert vs.storeDevice(3, counts, de, co) and vs.views() == [(3, 0, 0), (3, 1, 0)]
    assert not vs.storeDevice(3, counts, de, co)
    with pytest.raises(MmfError):
        p.dev.modelViews(256, [1], [np.eye(4, dtype=np.float32)])
    with pytest.raises(MmfError):
        p.dev.setViewLog(-1)
    vs.close()
