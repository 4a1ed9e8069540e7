"""CPU: tests/viewlog_oracle.py (the restatement the tracker's view log and mmf_tracker_model_views are compared with) against
point_tracker.ModelTracks, the host-side mirror of Model::store / computeTrackProjectionFirstFrame / getBestMatch's view
building (Core/Model/Model.cpp:1617-1644, 508-522, 798-816), fed the same tracks.  No device: the search is the CPU oracle's."""
import numpy as np
import pytest

import tracker_oracle as to
import viewlog_oracle as vo

W, H = 64, 48
K = (52.0, 51.5, 31.5, 23.25)
IDS = [1, 31, 32, 200]


def make_mask(rng):
    return np.ascontiguousarray(rng.choice(np.array(IDS + [7, 0], np.uint8), (H // 8, W // 8)).repeat(8, 0).repeat(8, 1))


def run(seed, n_frames, log_frames, n_kp=48):
    """a random sequence of adds, associations and prunes -> the oracle; no prune empties the table"""
    rng = np.random.default_rng(seed)
    pool = vo.unit_rows(rng, 96)
    ora = vo.ViewLogOracle(to.OracleTracker(W, H, K, capacity=256), log_frames)
    for step in range(n_frames):
        ts = 1_000_000 + 33_000 * step
        xy, desc, depth = vo.make_step(rng, pool, n_kp if step % 5 != 3 else 7, W, H)
        ora.add(xy, desc, ts, depth, 0.7, 30)
        if step % 4 == 0:
            ora.t.associate_all(IDS[:1])
        else:
            ora.t.associate(make_mask(rng), IDS)
        if step % 6 == 5:
            ora.t.prune(2, ts - 2 * 33_000)
    assert ora.t.tracks and len(ora.t.tracks[0]) == n_frames
    return ora


def model_tracks_views(ora, model_id, poses):
    """point_tracker.ModelTracks fed the model's tracks (insertion = uid order) and the poses of the last len(poses) frames"""
    from multimotionfusion_amd.point_tracker import ModelTracks
    mt = ModelTracks(model_id)
    mine = ora.t.models.get(model_id, set())
    mt.tracks = {id(t): t for t in ora.t.tracks if t.uid in mine}
    for k, P in enumerate(poses):
        mt.addPose(P, k)
    assert mt.store() and (not mt.tracks or not mt.store())  # (a second store changes nothing)
    views = mt.views()
    return views if views else [(np.zeros((0, 256), np.float32), np.zeros((0, 3), np.float32))] * len(poses)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_long_log_gives_the_views_of_model_tracks(orc, seed):
    """a log longer than the sequence, stamps = the last len(poses) frames: descriptors bit for bit, coordinates within one
    float32 ulp (the two sums differ only in float64 rounding -- numpy's matrix product may contract or reorder -- before the
    cast to float32).  Measured here: 0 of the 1 644 components of the three seeds differ."""
    n_frames, n_poses = 12, 9
    ora = run(seed, n_frames, 16)
    rng = np.random.default_rng(50 + seed)
    poses = [vo.random_pose(rng) for _ in range(n_poses)]
    stamps = list(range(n_frames - n_poses + 1, n_frames + 1))
    rows = differ = 0
    for m in IDS + [9]:  # (9: a model without tracks)
        got, missing = ora.model_views(m, stamps, poses)
        want = model_tracks_views(ora, m, poses)
        assert missing == 0 and len(got) == len(want) == n_poses
        for (gd, gc), (wd, wc) in zip(got, want):
            assert gd.shape == wd.shape and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), m
            assert gc.shape == wc.shape
            d = vo.ulp_distance(gc, wc)
            assert d.size == 0 or d.max() <= 1, (m, d.max())
            rows += gc.shape[0]
            differ += int((d > 0).sum())
    assert rows > 100
    print(f"seed {seed}: {differ} of {3 * rows} coordinate components differ by one ulp")
    assert not ora.model_views(9, stamps, poses)[0][0][0].size


def test_a_short_log_gives_the_last_frames_and_counts_the_rest(orc):
    n_frames, n_poses = 12, 9
    rng = np.random.default_rng(77)
    poses = [vo.random_pose(rng) for _ in range(n_poses)]
    stamps = list(range(n_frames - n_poses + 1, n_frames + 1))
    long = run(3, n_frames, 16)
    for log_frames in (1, 4, 5):
        short = run(3, n_frames, log_frames)
        for m in IDS:
            want, _ = long.model_views(m, stamps, poses)
            got, missing = short.model_views(m, stamps, poses)
            assert missing == n_poses - log_frames
            assert all(d.size == 0 and c.size == 0 for d, c in got[:missing])
            assert vo.same_views(got[missing:], want[missing:]) is None
            assert sum(d.shape[0] for d, _ in want[missing:]) > 0 or m != 1
    # a stamp in the future, stamp 0 and a frame from before a reset are not in the ring
    got, missing = long.model_views(1, [n_frames + 1, 0, -3], poses[:3])
    assert missing == 3 and all(d.size == 0 for d, _ in got)
    long.reset()
    assert long.model_views(1, stamps, poses)[1] == n_poses
    off = run(3, 4, 0)
    assert off.model_views(1, [1, 2, 3, 4], poses[:4])[1] == 4


def test_the_projection_rounds_every_operation_on_its_own():
    """((r0 x + r1 y) + r2 z) + t in float64, then float32: a case where a fused or reordered sum gives another float32"""
    P = np.eye(4, dtype=np.float32)
    P[0, :] = [1.0, 1.0, 1.0, 0.0]
    c = np.array([1.0, 2.0 ** -53, 2.0 ** -53], np.float32)
    # (1 + 2^-53) rounds to 1 in float64, twice; x + (y + z) would be 1 + 2^-52
    assert vo.project(P, c)[0] == np.float32(1.0)
    big = np.array([3e38, 3e38, 0.0], np.float32)
    assert not np.isfinite(vo.project(P, big)[0])  # finite in float64, +inf in float32: the keypoint is dropped
    P[1, 3] = np.inf
    assert not np.all(np.isfinite(vo.project(P, c)))
    # the array form the oracle's views use is the scalar form, bit for bit, non-finite values included
    rng = np.random.default_rng(4)
    co = (rng.standard_normal((200, 3)) * 10.0 ** rng.uniform(-3, 3, (200, 1))).astype(np.float32)
    co[5], co[6, 1], co[7] = np.nan, np.inf, 3e38
    for pose in (vo.random_pose(rng), P, (vo.random_pose(rng) * np.float32(1e3)).astype(np.float32)):
        want = np.stack([vo.project(pose, c) for c in co])
        assert np.array_equal(vo.project_rows(pose, co).view(np.uint32), want.view(np.uint32))
