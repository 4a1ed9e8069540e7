"""-m gpu: keypoint redetection inside processFrame with the device verifier (mmf_fusion_set_redetection_verifier, mode 1)
on the gap scene of tests/test_gpu_redetect_fusion.py (its helpers imported), against the decision-block oracle run with the
per-view rule (tests/verify_oracle.py) on the same inputs."""
import numpy as np
import pytest

import redetect_oracle as ro
import test_gpu_redetect_fusion as rf
import verify_oracle as vo
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu
W, H, SPAWN, LAST_SEEN, BACK = rf.W, rf.H, rf.SPAWN, rf.LAST_SEEN, rf.BACK


def run_gap(gpu_ctx, orc, seed, max_points=None):
    """the "gap+redetect" run of test_gpu_redetect_fusion.run up to the frame the object comes back in, verifier on the
    device; max_points: the verifier's capacity (None = the default, 1024)"""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.point_tracker import Keypoint, ModelTracks
    K, poses, objs, traj, with_obj, without = rf.gap_scene(seed)
    kps, desc = rf.physical_keypoints(seed, K, poses, traj, with_obj)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setEnableRedetection(True)
    if max_points is not None:
        assert gpu_ctx.lib.mmf_debug_set_redetect_max_points(max_points) == 0
    try:
        g.setRedetectionVerifier(1)
    finally:
        gpu_ctx.lib.mmf_debug_set_redetect_max_points(1024)
    mt = ModelTracks(1)
    tracks = [[] for _ in range(len(desc))]
    out, keep = {}, []
    for i in range(BACK + 1):
        hidden = LAST_SEEN < i < BACK
        f = without[i] if hidden else with_obj[i]
        ids_now = [m.id for m in g.getModels()]
        new_label = i in (SPAWN, BACK)
        label = g.getNextModelID() if new_label else 1
        mask = np.zeros((H, W), np.uint8)
        if i >= SPAWN and not hidden:
            mask[f["ids"] == 1] = label
        data = rf.model_data(mask, f["depth"], ids_now + ([label] if new_label else [])) if i > 0 else None
        idx, xy, coord = kps[i]
        if not hidden and i >= SPAWN:
            g.setKeypoints(xy, coord, desc[idx])
        keep.append((rf.dev(f["rgb"]), rf.dev(f["depth"]), rf.dev(mask)))
        if i == BACK:
            inactive = g.getInactiveModels()
            assert [m.id for m in inactive] == [1] and ids_now == [0]
            out["count_inactive"], out["n_keypoints"] = inactive[0].lastCount(), len(idx)
            out["oracle"] = vo.redetect(orc, mask, xy, coord, desc[idx], [0], [(1, out["views"])], True)
            out["oracle_one_engine"] = ro.redetect(orc, mask, xy, coord, desc[idx], [0], [(1, out["views"])], True)
        g.processFrame(*keep[-1][:2], timestamp=1000 + i, mask=keep[-1][2], hasNewLabel=new_label, modelData=data)
        models = g.getModels()
        if SPAWN <= i <= LAST_SEEN:
            P = models[1].getPose()
            for j in range(len(desc)):
                hit = np.flatnonzero(idx == j)
                tracks[j].append(Keypoint(1000 + i, tuple(xy[hit[0]]), coord[hit[0]].astype(np.float64), desc[j]) if len(hit) else None)
            if i == SPAWN:
                mt.initGlobalTracks(tracks, P, 1000 + i)
            else:
                mt.addPose(P, 1000 + i)
        if i == LAST_SEEN + 1:
            assert mt.store() is True
            out["views"] = mt.views()
            assert g.storeViews(1, out["views"]) is True
    out["ids_back"], out["inactive_back"] = [m.id for m in models], [m.id for m in g.getInactiveModels()]
    out["events"], out["next_id"] = g.getLastRedetections(), g.getNextModelID()
    out["pose_back"], out["count_back"] = models[-1].getPose(), models[-1].lastCount()
    out["launches"], out["host_verified"] = g.getViewStore().lastLaunches(), g.redetectionHostVerified()
    g.close()
    return out


def check_against_oracle(a):
    o = a["oracle"]
    assert a["ids_back"] == o["active_ids"] == [0, 1] and a["inactive_back"] == o["inactive_ids"] == [] and a["next_id"] == 2
    assert o["has_new_label"] is False and len(a["events"]) == len(o["events"]) == 1
    for ev, want in zip(a["events"], o["events"]):
        best = want["best"]
        assert (ev["label"], ev["model_id"], ev["removed_id"], ev["activated"]) == (want["label"], want["model_id"], want["removed_id"], want["activated"])
        assert ev["view"] == best["view"] and ev["inliers"] == best["inliers"], (ev, best)
        assert np.float32(ev["error"]).view(np.uint32) == np.float32(best["error"]).view(np.uint32), (ev["error"], best["error"])
        assert np.array_equal(ev["transformation"].view(np.uint32), np.asarray(best["transformation"], np.float32).view(np.uint32))
    assert np.array_equal(a["pose_back"].view(np.uint32), o["events"][0]["pose"].view(np.uint32)), (a["pose_back"], o["events"][0]["pose"])
    assert a["count_back"] == a["count_inactive"] and a["count_back"] > 500  # its map and its id, as at inactivation


@pytest.mark.parametrize("seed", [21, 22])
def test_object_comes_back_verified_on_the_device(gpu_ctx, orc, seed):
    """Events (label, model, removed id, activated, view, inliers, error), the re-activated model's pose, its surfel count and
    its id equal the decision-block oracle under the per-view rule.  One segment: 3 match launches and 2 for the verification."""
    a = run_gap(gpu_ctx, orc, seed)
    check_against_oracle(a)
    assert a["launches"] == 5 and a["host_verified"] == 0


def test_a_segment_too_large_for_the_verifier_goes_to_the_host_core(gpu_ctx, orc):
    """a verifier of 20 points and a segment of more keypoints: verified by the host core under the same rule, and counted"""
    a = run_gap(gpu_ctx, orc, 21, max_points=20)
    assert a["n_keypoints"] > 20
    check_against_oracle(a)
    assert a["launches"] == 5 and a["host_verified"] == 1


def test_older_newer_rule_on_the_device(gpu_ctx, orc):
    """test_gpu_redetect_fusion.test_older_newer_rule_and_small_segments with the device verifier: a match inside the segment
    of an OLDER model is refused, two usable keypoints are too few, a NEWER model is dropped for the inactive one."""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(7, seed=21)
    objs = synth.make_objects(2, seed=21)
    traj = synth.object_trajectories(objs, 7, seed=21)
    frames = [synth.render(p, W, H, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    obj = ro.make_object(3)
    tr, po = ro.make_tracks(obj, 7, 103)
    views = ro.views_of(ro.project_first_frame(tr, po))
    qd, qc, _, _ = ro.make_query(obj, 203)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setEnableRedetection(True)
    g.setRedetectionVerifier(1)
    keep = []

    def xy_on(mask, label, count):
        ys, xs = np.nonzero(mask == label)
        sel = np.random.default_rng(5).choice(len(ys), count, replace=False)
        return np.stack([xs[sel], ys[sel]], 1).astype(np.int32)

    def step(i, mask, new, kp=None):
        ids_now = [m.id for m in g.getModels()]
        data = rf.model_data(mask, frames[i]["depth"], ids_now + ([g.getNextModelID()] if new else [])) if i > 0 else None
        if kp is not None:
            g.setKeypoints(*kp)
        keep.append((rf.dev(frames[i]["rgb"]), rf.dev(frames[i]["depth"]), rf.dev(mask)))
        g.processFrame(*keep[-1][:2], timestamp=1000 + i, mask=keep[-1][2], hasNewLabel=new, modelData=data)
        return [m.id for m in g.getModels()], [m.id for m in g.getInactiveModels()]

    assert step(0, np.zeros((H, W), np.uint8), False) == ([0], [])
    assert step(1, np.where(frames[1]["ids"] == 1, 1, 0).astype(np.uint8), True) == ([0, 1], [])
    assert step(2, np.where(np.isin(frames[2]["ids"], [1, 2]), frames[2]["ids"], 0).astype(np.uint8), True) == ([0, 1, 2], [])
    assert step(3, np.where(frames[3]["ids"] == 1, 1, 0).astype(np.uint8), False) == ([0, 1], [2])
    assert g.storeViews(2, views) is True
    m4 = np.where(frames[4]["ids"] == 1, 1, 0).astype(np.uint8)
    want = vo.redetect(orc, m4, xy_on(m4, 1, len(qd)), qc, qd, [0, 1], [(2, views)], False)
    assert step(4, m4, False, (xy_on(m4, 1, len(qd)), qc, qd)) == ([0, 1], [2])
    ev = g.getLastRedetections()
    assert len(ev) == len(want["events"]) == 1 and not ev[0]["activated"] and ev[0]["model_id"] == 2 and ev[0]["label"] == 1
    assert ev[0]["view"] == want["events"][0]["best"]["view"] and ev[0]["inliers"] == want["events"][0]["best"]["inliers"]
    m5 = np.where(frames[5]["ids"] == 1, 1, np.where(frames[5]["ids"] == 2, 3, 0)).astype(np.uint8)
    xy5, qc5 = xy_on(m5, 3, len(qd)), qc.copy()
    xy5[2] = [-4, 10]
    qc5[3:] = np.nan
    assert step(5, m5, True, (xy5, qc5, qd)) == ([0, 1, 3], [2])
    assert g.getLastRedetections() == []
    m6 = np.where(frames[6]["ids"] == 1, 1, np.where(frames[6]["ids"] == 2, 3, 0)).astype(np.uint8)
    xy6 = xy_on(m6, 3, len(qd))
    want = vo.redetect(orc, m6, xy6, qc, qd, [0, 1, 3], [(2, views)], False)
    assert want["active_ids"] == [0, 1, 2] and want["events"][0]["removed_id"] == 3
    assert step(6, m6, False, (xy6, qc, qd)) == ([0, 1, 2], [])
    ev = g.getLastRedetections()
    assert len(ev) == 1 and ev[0]["activated"] and ev[0]["removed_id"] == 3 and ev[0]["model_id"] == 2
    assert np.array_equal(g.getModels()[2].getPose().view(np.uint32), want["events"][0]["pose"].view(np.uint32))
    assert g.redetectionHostVerified() == 0
    g.close()


def test_two_segments_and_two_inactive_models_in_one_frame_on_the_device(gpu_ctx, orc):
    """test_gpu_redetect_fusion.run_two_segments with the device verifier: segment 3 activates model 1 -- asked[0] -- and
    segment 4 then reads model 2's record at asked[1] although model 2 is inactive[0] by then.  Events, lists, poses and the
    cancelled label equal the per-view oracle; two segments are 3 * 2 match launches and 2 for the verification of all pairs."""
    assert rf.run_two_segments(gpu_ctx, orc, vo, True) == (3 * 2 + 2, 0)


def test_one_segment_on_the_host_core_and_one_on_the_device_in_one_frame(gpu_ctx, orc):
    """a verifier of 32 points: segment 3 (30 keypoints) is verified on the device, segment 4 (35) by the host core"""
    assert rf.N_A <= 32 < len(rf.two_segment_inputs()[5][0]) - rf.N_A
    assert rf.run_two_segments(gpu_ctx, orc, vo, True, max_points=32) == (3 * 2 + 2, 1)


def test_the_verifier_is_refused_on_a_shard_and_off_by_default(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = synth.intrinsics(W, H)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    assert g.redetectionHostVerified() == 0
    g.setRedetectionVerifier(0)
    with pytest.raises(MmfError):
        g.setRedetectionVerifier(2)
    g.setShard(0, 2)
    with pytest.raises(MmfError):
        g.setRedetectionVerifier(1)
    g.setShard(0, 1)
    g.setRedetectionVerifier(1)
    with pytest.raises(MmfError):
        g.setShard(0, 2)
    g.setRedetectionVerifier(0)
    g.setShard(0, 2)
    g.close()
