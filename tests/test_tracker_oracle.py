"""CPU: tests/tracker_oracle.py (the restatement the device track table is compared with) against cases worked out by hand
from the reference's code (Core/Utils/PointTracker.cpp, Core/Model/Model.cpp:739-775, Core/MultiMotionFusion.cpp:425-436,
584-604).  No device: the search is the CPU oracle's, the fit the library's host code."""
import numpy as np
import pytest

import tracker_oracle as to

W, H = 320, 240
FX = FY = 264.0
CX, CY = 160.0, 120.0
K = (FX, FY, CX, CY)


def unit_rows(rng, n, dim=256):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def scene(rng, n):
    px = np.stack([rng.choice(np.arange(10, W - 10), n, replace=False), rng.integers(10, H - 10, n)], 1)
    z = rng.uniform(1.0, 3.0, n).astype(np.float32)
    depth = np.zeros((H, W), np.float32)
    depth[px[:, 1], px[:, 0]] = z
    return px, depth


@pytest.fixture()
def tracker(orc):
    return to.OracleTracker(W, H, K)


def test_grow_match_and_prune_40_45_48_33(tracker):
    """the scenario of tests/test_gpu_point_tracker.py::test_tracks_grow_match_and_prune, with the table's derived state"""
    rng = np.random.default_rng(0)
    tr = tracker
    px, depth = scene(rng, 40)
    desc = unit_rows(rng, 40)
    tr.add(px, desc, 1_000_000_000, depth)
    f = tr.flatten()
    assert f["n_tracks"] == 40 and f["length"] == 1 and np.all(f["age"] == 0) and np.all(f["nvalid"] == 1)
    assert np.array_equal(f["uid"], np.arange(40)) and not f["nonnull"][1].any() and f["nonnull"][0].all()
    z = depth[px[7, 1], px[7, 0]]
    assert np.allclose(f["coordinate"][0, 7], [z * (px[7, 0] - CX) / FX, z * (px[7, 1] - CY) / FY, z], atol=1e-5)

    order = rng.permutation(30)
    desc2 = np.concatenate([desc[order] + 0.01 * rng.standard_normal((30, 256)).astype(np.float32), unit_rows(rng, 5)])
    px2, depth2 = scene(rng, 35)
    tr.add(px2, desc2, 1_033_000_000, depth2)
    f = tr.flatten()
    assert f["n_tracks"] == 45 and f["length"] == 2
    for q, src in enumerate(order):  # the query keypoint q continues track src
        assert f["nonnull"][0, src] and tuple(f["xy"][0, src]) == tuple(px2[q]) and f["nvalid"][src] == 2
        assert np.array_equal(f["desc"][src], desc2[q]) and tuple(f["xy"][1, src]) == tuple(px[src])
    assert not f["nonnull"][0, 30:40].any() and np.all(f["age"][30:40] == 1) and np.all(f["nvalid"][30:40] == 1)
    assert np.array_equal(f["desc"][30:40], desc[30:40])  # the descriptor of the last non-null keypoint
    assert f["nonnull"][0, 40:].all() and not f["nonnull"][1, 40:].any() and np.array_equal(f["uid"][40:], np.arange(40, 45))

    tr.add(np.zeros((0, 2)), np.zeros((0, 256), np.float32), 1_066_000_000, depth2)  # n == 0: a null keypoint everywhere
    f = tr.flatten()
    assert f["length"] == 3 and not f["nonnull"][0].any() and f["n_tracks"] == 45
    assert np.all(f["age"][:30] == 1) and np.all(f["age"][30:40] == 2) and np.all(f["age"][40:] == 1)
    assert all(a is None for a in tr.last_active(1))
    assert sum(a is not None for a in tr.last_active(2)) == 35
    assert sum(a is not None for a in tr.last_active(0)) == 45

    tr.add(px2[:3], unit_rows(rng, 3), 1_100_000_000, depth2, min_feature_distance=0.7)  # too far: new tracks
    assert len(tr.tracks) == 48
    tr.prune(2, 1_050_000_000)
    f = tr.flatten()
    assert f["n_tracks"] == 33 and np.array_equal(f["uid"], np.r_[np.arange(30), np.arange(45, 48)])  # order kept
    tr.prune(30, 0)
    assert len(tr.tracks) == 33


@pytest.mark.parametrize("history,expect_tracks", [(1, 4), (2, 2), (0, 2)])
def test_history_bounds_the_active_set(tracker, history, expect_tracks):
    """two tracks, one frame without keypoints, then the same two descriptors again: with history 1 the tracks' last
    keypoint lies 1 step from the end (:214 `d >= history` breaks) and both keypoints start tracks; with 2 or 0 they match"""
    rng = np.random.default_rng(1)
    px, depth = scene(rng, 2)
    desc = unit_rows(rng, 2)
    tracker.add(px, desc, 10, depth)
    tracker.add(np.zeros((0, 2)), np.zeros((0, 256)), 20, depth)
    tracker.add(px, desc, 30, depth, 0.7, history)
    f = tracker.flatten()
    assert f["n_tracks"] == expect_tracks and f["length"] == 3
    if expect_tracks == 2:
        assert np.all(f["nvalid"] == 2) and np.all(f["age"] == 0) and not f["nonnull"][1].any()
    else:
        assert list(f["age"]) == [2, 2, 0, 0] and list(f["nvalid"]) == [1, 1, 1, 1]


def test_prune_that_empties_the_table_restarts_the_length(tracker):
    rng = np.random.default_rng(2)
    px, depth = scene(rng, 5)
    tracker.add(px, unit_rows(rng, 5), 10, depth)
    tracker.add(px[:2], unit_rows(rng, 2), 20, depth)
    assert tracker.flatten()["length"] == 2 and len(tracker.tracks) == 7
    tracker.prune(5, 1000)
    f = tracker.flatten()
    assert f["n_tracks"] == 0 and f["length"] == 0
    tracker.add(px[:3], unit_rows(rng, 3), 2000, depth)  # :61-66: added without matching, tracks of length 1
    f = tracker.flatten()
    assert f["n_tracks"] == 3 and f["length"] == 1 and np.array_equal(f["uid"], [7, 8, 9])  # uids are never reused


def test_zero_depth_and_outside_keypoints_have_nan_coordinates(tracker):
    depth = np.ones((H, W), np.float32)
    depth[5, 7] = 0.0
    tracker.add([[7, 5], [W, 3], [W - 1, H - 1], [-1, 0]], unit_rows(np.random.default_rng(3), 4), 1, depth)
    f = tracker.flatten()
    assert np.isnan(f["coordinate"][0, [0, 1, 3]]).all() and f["nonnull"][0].all()
    assert np.array_equal(f["coordinate"][0, 2], np.array([(W - 1 - CX) / FX, (H - 1 - CY) / FY, 1.0], np.float32))
    assert np.array_equal(f["xy"][0, 1], [W, 3])  # the pixel is kept


def test_capacity_drops_appends_and_counts_them(orc):
    tr = to.OracleTracker(W, H, K, capacity=6)
    rng = np.random.default_rng(4)
    px, depth = scene(rng, 8)
    tr.add(px[:4], unit_rows(rng, 4), 1, depth)
    tr.add(px[4:], unit_rows(rng, 4), 2, depth, 0.7)
    f = tr.flatten()
    assert f["n_tracks"] == 6 and f["dropped"] == 2 and np.array_equal(f["uid"], np.arange(6))


def association_fixture(tracker):
    """six tracks at x = 10, 20, ... on row 4; a mask with labels by column band"""
    rng = np.random.default_rng(5)
    px = np.stack([np.arange(1, 7) * 10, np.full(6, 4)], 1)
    depth = np.ones((H, W), np.float32)
    desc = unit_rows(rng, 6)
    tracker.add(px, desc, 1, depth)
    tracker.associate_all([0])
    return px, depth, desc


def members(f, m):
    return [int(i) for i in np.nonzero((f["member"][:, m >> 5] >> np.uint32(m & 31)) & 1)[0]]


def test_association_with_a_label_no_active_model_carries(tracker):
    px, depth, desc = association_fixture(tracker)
    mask = np.zeros((H, W), np.uint8)
    mask[:, 25:45] = 3   # tracks 2, 3
    mask[:, 45:] = 7     # tracks 4, 5: label 7 belongs to no active model
    tracker.associate(mask, [0, 3])
    f = tracker.flatten()
    assert list(f["label"]) == [0, 0, 3, 3, 7, 7]
    assert members(f, 0) == [0, 1]  # model 0 is visible: the other segments' tracks leave it, 7's included (:590-595)
    assert members(f, 3) == [2, 3] and members(f, 7) == []
    mask[:] = 7  # no listed model is visible: nothing changes (:587)
    tracker.associate(mask, [0, 3])
    f = tracker.flatten()
    assert members(f, 0) == [0, 1] and members(f, 3) == [2, 3] and list(f["label"]) == [7] * 6


def test_a_track_moves_from_model_0_to_model_3_and_back(tracker):
    px, depth, desc = association_fixture(tracker)
    mask = np.zeros((H, W), np.uint8)
    mask[:, 15:25] = 3  # track 1
    tracker.associate(mask, [0, 3])
    f = tracker.flatten()
    assert members(f, 0) == [0, 2, 3, 4, 5] and members(f, 3) == [1]
    tracker.add(px, desc, 2, depth)  # every track continues
    mask[:] = 0
    mask[:, 45:55] = 3  # now track 4 carries 3, track 1 is background again
    tracker.associate(mask, [0, 3])
    f = tracker.flatten()
    assert members(f, 0) == [0, 1, 2, 3, 5] and members(f, 3) == [4]
    tracker.add(px[:4], desc[:4], 3, depth)  # tracks 4, 5 invisible: unlabelled, they keep their sets
    mask[:] = 3
    tracker.associate(mask, [0, 3])
    f = tracker.flatten()
    assert list(f["label"]) == [3, 3, 3, 3, -1, -1]
    assert members(f, 0) == [0, 1, 2, 3, 5]  # model 0 is not visible: untouched
    assert members(f, 3) == [0, 1, 2, 3, 4]
    tracker.forget(3)
    assert members(tracker.flatten(), 3) == []


def test_pairs_skip_a_nan_on_either_side(tracker):
    rng = np.random.default_rng(6)
    px = np.stack([np.arange(1, 7) * 10, np.array([4, 9, 30, 7, 50, 21])], 1)
    desc = unit_rows(rng, 6)
    d0 = np.full((H, W), 2.0, np.float32)
    d0[9, 20] = 0.0  # track 1: NaN in prev
    tracker.add(px, desc, 1, d0)
    assert tracker.last_pairs(0)[0].shape == (0, 3)  # no model yet
    tracker.associate_all([0])
    p0, p1 = tracker.last_pairs(0)
    assert p0.shape == (0, 3)  # tracks of length 1 (the reference reads end()[-2] out of bounds there)
    T, err, inl = tracker.last_track_transform(0)
    assert np.array_equal(T, np.eye(4, dtype=np.float32)) and inl is None
    d1 = np.full((H, W), 2.5, np.float32)
    d1[7, 40] = 0.0  # track 3: NaN in cur
    tracker.add(px[[0, 1, 2, 3, 5]], desc[[0, 1, 2, 3, 5]], 2, d1)  # track 4 has no keypoint this frame
    p0, p1 = tracker.last_pairs(0)
    f = tracker.flatten()
    assert p0.shape == (3, 3)  # tracks 0, 2, 5 in table order
    assert np.array_equal(p0, f["coordinate"][1, [0, 2, 5]]) and np.array_equal(p1, f["coordinate"][0, [0, 2, 5]])
    assert np.all(p0[:, 2] == 2.0) and np.all(p1[:, 2] == 2.5)
    T, err, inl = tracker.last_track_transform(0)
    assert T.shape == (4, 4) and np.all(np.isfinite(T))
    assert tracker.last_pairs(9)[0].shape == (0, 3)
