"""CPU: the redetection oracle (tests/redetect_oracle.py) on its seeded fixture, and the host mirror's track bookkeeping
(multimotionfusion_amd/point_tracker.py: ModelTracks) against it.  The assertions here are what shows that the GPU tests
(tests/test_gpu_redetect.py: same generator, same seeds) run on inputs on which redetection really fires."""
import numpy as np
import pytest

import redetect_oracle as ro
from multimotionfusion_amd import synth

SEEDS = [3, 11, 29]


def fixture(seed, n_views=7):
    obj = ro.make_object(seed)
    tracks, poses = ro.make_tracks(obj, n_views, seed + 100)
    views = ro.views_of(ro.project_first_frame(tracks, poses))
    qd, qc, motion, is_obj = ro.make_query(obj, seed + 200)
    return obj, tracks, poses, views, qd, qc, motion, is_obj


@pytest.mark.parametrize("seed", SEEDS)
def test_projection_recovers_the_model_frame(seed):
    obj, tracks, poses, views, *_ = fixture(seed)
    assert len(views) == 7
    local = ro.project_first_frame(tracks, poses)
    for j, row in enumerate(local):
        for kp in row:
            if kp is not None:
                assert np.linalg.norm(kp.coordinate - obj["points"][j]) < 5e-3  # (0.5 mm noise per axis + float32 poses)
    dropped = sum(kp is None for row in local for kp in row)
    assert 0 < dropped < 7 * len(obj["points"])
    assert all(len(d) == len(c) and d.dtype == np.float32 for d, c in views)
    assert sum(len(d) for d, _ in views) == 7 * len(obj["points"]) - dropped


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_redetects_the_right_model_and_recovers_the_motion(orc, seed):
    obj, _, _, views, qd, qc, motion, is_obj = fixture(seed)
    best = ro.get_best_match(orc, qd, qc, views)
    assert best["found"] and best["error"] < 0.01 and best["inliers"] > 5, best
    # query ~ T train: T is the motion model -> camera
    T = best["transformation"].astype(np.float64)
    assert np.abs(T[:3, 3] - motion[:3, 3]).max() < 5e-3, (T, motion)
    assert synth.rotation_angle(T[:3, :3], motion[:3, :3]) < 0.02
    assert best["inliers"] <= best["n_matches"] <= int(is_obj.sum()) + 3
    P = ro.inverse_isometry(best["transformation"])
    assert np.abs(P.astype(np.float64) @ T - np.eye(4)).max() < 1e-5
    # an unrelated model (other descriptors, same geometry) is refused
    other = ro.make_object(seed + 1000)
    tracks, poses = ro.make_tracks(other, 7, seed + 1100)
    far = ro.get_best_match(orc, qd, qc, ro.views_of(ro.project_first_frame(tracks, poses)))
    assert not (far["found"] and far["error"] < 0.01 and far["inliers"] > 5), far


def decision_inputs(seed, label, n_kp=None):
    obj, _, _, views, qd, qc, _, _ = fixture(seed)
    if n_kp is not None:
        qd, qc = qd[:n_kp], qc[:n_kp]
    mask = np.zeros((48, 64), np.uint8)
    mask[10:40, 10:50] = label
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(10, 50, len(qd)), rng.integers(10, 40, len(qd))], 1)
    return mask, xy, qc, qd, views


@pytest.mark.parametrize("seed", SEEDS)
def test_decision_block(orc, seed):
    # a new label (2) whose keypoints match the inactive model 1: re-activated, the new label cancelled
    mask, xy, qc, qd, views = decision_inputs(seed, 2)
    other = ro.make_object(seed + 1000)
    tr, po = ro.make_tracks(other, 7, seed + 1100)
    views_other = ro.views_of(ro.project_first_frame(tr, po))
    r = ro.redetect(orc, mask, xy, qc, qd, [0], [(3, views_other), (1, views)], True)
    assert r["active_ids"] == [0, 1] and r["inactive_ids"] == [3] and r["has_new_label"] is False
    assert len(r["events"]) == 1 and r["events"][0]["model_id"] == 1 and r["events"][0]["removed_id"] == -1
    # keypoints outside the image and non-finite ones are dropped; with 2 keypoints left the segment is skipped
    mask, xy, qc, qd, views = decision_inputs(seed, 2)
    xy2, qc2 = xy.copy(), qc.copy()
    xy2[2:5] = [[-1, 5], [64, 5], [5, 48]]
    qc2[5:] = np.nan
    r = ro.redetect(orc, mask, xy2, qc2, qd, [0], [(1, views)], True)
    assert r["active_ids"] == [0] and r["inactive_ids"] == [1] and r["has_new_label"] is True and not r["events"]
    # an active model carries the label: a NEWER one (5 > 1) is replaced ...
    mask, xy, qc, qd, views = decision_inputs(seed, 5)
    r = ro.redetect(orc, mask, xy, qc, qd, [0, 5], [(1, views)], False)
    assert r["active_ids"] == [0, 1] and r["inactive_ids"] == [] and r["events"][0]["removed_id"] == 5
    # ... an OLDER one (1 < 4) is not: nothing happens for the pair
    mask, xy, qc, qd, views = decision_inputs(seed, 1)
    r = ro.redetect(orc, mask, xy, qc, qd, [0, 1], [(4, views)], False)
    assert r["active_ids"] == [0, 1] and r["inactive_ids"] == [4]
    assert len(r["events"]) == 1 and not r["events"][0]["activated"]
    # labels 0 and 255 are never searched
    for label in (0, 255):
        mask, xy, qc, qd, views = decision_inputs(seed, label)
        r = ro.redetect(orc, mask, xy, qc, qd, [0], [(1, views)], True)
        assert not r["events"] and r["has_new_label"] is True


def two_label_inputs(seed_a, seed_b, second_shows_a):
    """labels 3 and 4 side by side; the keypoints on label 3 show object A, those on label 4 object B (or A once more)"""
    _, _, _, views_a, qd_a, qc_a, _, _ = fixture(seed_a)
    _, _, _, views_b, qd_b, qc_b, _, _ = fixture(seed_b)
    if second_shows_a:
        qd_b, qc_b, _, _ = ro.make_query(ro.make_object(seed_a), seed_a + 250)
    mask = np.zeros((48, 64), np.uint8)
    mask[10:40, 5:30], mask[10:40, 35:60] = 3, 4
    rng = np.random.default_rng(seed_a)
    xy = np.concatenate([np.stack([rng.integers(5, 30, len(qd_a)), rng.integers(10, 40, len(qd_a))], 1),
                         np.stack([rng.integers(35, 60, len(qd_b)), rng.integers(10, 40, len(qd_b))], 1)])
    order = rng.permutation(len(xy))  # the two segments' keypoints interleaved, as a tracker hands them over
    on_a = (np.arange(len(xy)) < len(qd_a))[order]
    return mask, xy[order], np.concatenate([qc_a, qc_b])[order], np.concatenate([qd_a, qd_b])[order], views_a, views_b, on_a


@pytest.mark.parametrize("rule", ["one engine", "per view"])
def test_decision_block_two_labels_two_inactive_models(orc, rule):
    """Active [0, 3], inactive [1, 2] (views of A, views of B), a new label 4.  Expectations written out by hand, for the
    one-engine oracle and for the per-view one (tests/verify_oracle.py) the device tests lean on."""
    import verify_oracle as vo
    oracle = ro if rule == "one engine" else vo
    # label 3 shows A, label 4 shows B: label 3 drops the newer model 3 for model 1; label 4, not carried by any model,
    # brings model 2 back although it is by then the FIRST of the inactive list; the new label is cancelled
    mask, xy, qc, qd, views_a, views_b, on_a = two_label_inputs(3, 11, False)
    r = oracle.redetect(orc, mask, xy, qc, qd, [0, 3], [(1, views_a), (2, views_b)], True)
    assert r["active_ids"] == [0, 1, 2] and r["inactive_ids"] == [] and r["has_new_label"] is False
    assert [(e["label"], e["model_id"], e["removed_id"], e["activated"]) for e in r["events"]] == [(3, 1, 3, True), (4, 2, -1, True)]
    for ev, sel, views in ((r["events"][0], on_a, views_a), (r["events"][1], ~on_a, views_b)):
        alone = oracle.get_best_match(orc, qd[sel], qc[sel], views)  # the segment's keypoints in their order, that model's views
        assert alone["found"] and alone["view"] == ev["best"]["view"] and alone["inliers"] == ev["best"]["inliers"]
        assert np.array_equal(np.asarray(alone["transformation"], np.float32), np.asarray(ev["best"]["transformation"], np.float32))
        assert np.array_equal(ev["pose"], ro.inverse_isometry(alone["transformation"]))
    # the same with the inactive list the other way round: the events keep the labels' order
    r = oracle.redetect(orc, mask, xy, qc, qd, [0, 3], [(2, views_b), (1, views_a)], True)
    assert r["active_ids"] == [0, 1, 2] and r["inactive_ids"] == []
    assert [(e["label"], e["model_id"], e["removed_id"]) for e in r["events"]] == [(3, 1, 3), (4, 2, -1)]
    # both labels show A: label 3 takes model 1 out of the list label 4 iterates, so label 4 -- whose keypoints would match
    # model 1 -- has only model 2 left to ask and finds nothing; model 2 stays inactive
    mask, xy, qc, qd, views_a, views_b, on_a = two_label_inputs(3, 11, True)
    assert oracle.get_best_match(orc, qd[~on_a], qc[~on_a], views_a)["found"]
    r = oracle.redetect(orc, mask, xy, qc, qd, [0, 3], [(1, views_a), (2, views_b)], True)
    assert r["active_ids"] == [0, 1] and r["inactive_ids"] == [2] and r["has_new_label"] is False
    assert [(e["label"], e["model_id"], e["removed_id"], e["activated"]) for e in r["events"]] == [(3, 1, 3, True)]
    # ... and with model 1 still there (nothing on label 3) label 4 does take it
    r = oracle.redetect(orc, mask, xy[~on_a], qc[~on_a], qd[~on_a], [0, 3], [(1, views_a), (2, views_b)], True)
    assert r["active_ids"] == [0, 3, 1] and r["inactive_ids"] == [2]
    assert [(e["label"], e["model_id"], e["removed_id"], e["activated"]) for e in r["events"]] == [(4, 1, -1, True)]


def test_the_batch_cases_are_what_their_gpu_tests_need(orc):
    """tests/redetect_batch_cases.py under the oracle alone: found and not-found pairs, both models found, the set too large
    for a verifier of 40 points found, and the three 70-view layouts won by the view each is built for"""
    import redetect_batch_cases as bc
    bc.check_batch_conditions(orc)
    assert sorted(bc.chunk_layouts(orc)) == ["a", "b", "c"]


@pytest.mark.parametrize("seed", SEEDS)
def test_host_mirror_bookkeeping(seed):
    """ModelTracks: updateTracks, the pose list, computeTrackProjectionFirstFrame, store-once, activate"""
    from multimotionfusion_amd.point_tracker import Keypoint, ModelTracks
    obj, tracks, poses, views, *_ = fixture(seed)
    mine = [[None if kp is None else Keypoint(kp.timestamp, kp.xy, kp.coordinate, kp.descriptor) for kp in t] for t in tracks]
    mt = ModelTracks(1)
    mt.initGlobalTracks(mine[:5], poses[0], 1000)
    for i, P in enumerate(poses[1:]):
        mt.addPose(P, 1001 + i)
    extra = [[None] * 7]
    mt.updateTracks(mine[5:] + extra, [mine[0]])  # add the rest and one outlier track, remove the first again
    mt.updateTracks([mine[0]], extra)
    assert len(mt.tracks) == len(mine)
    assert mt.store() is True
    got = mt.views()
    want = ro.views_of(ro.project_first_frame(tracks[1:5] + tracks[5:] + tracks[:1], poses))  # (insertion order)
    assert len(got) == len(want) == 7
    for (gd, gc), (wd, wc) in zip(got, want):
        assert np.array_equal(gd, wd) and np.array_equal(gc.view(np.uint32), wc.view(np.uint32))
    # a second store changes nothing (Model.cpp:1618-1621)
    local_before = mt.tracks_local
    mt.updateTracks([], mine[:10])
    assert mt.store() is False and mt.tracks_local is local_before
    # activate: the stored tracks come back, one pose
    P = np.eye(4, dtype=np.float32)
    P[0, 3] = 0.5
    mt.activate(P, 2000)
    assert len(mt.tracks) == len(local_before) and len(mt.poses) == 1 and mt.timestamp_ns == [2000]
    assert np.array_equal(mt.poses[0], P)
