"""-m gpu: MultiMotionFusion::savePly and loadModels (Core/MultiMotionFusion.cpp:1001-1018, :131-145) on the fusion: the files
of a fusion with one inactive object model, a fresh fusion restored from them, the restored model redetected when the object
returns, and savePly leaving a running sequence as it was.  Scene and keypoints: tests/test_gpu_redetect_fusion.py."""
import os

import numpy as np
import pytest
import torch

import modeldb_oracle as mo
from test_gpu_redetect_fusion import BACK, H, LAST_SEEN, SPAWN, W, dev, gap_scene, model_data, physical_keypoints

pytestmark = pytest.mark.gpu
SEED = 21


def translation(x, y, z):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = [x, y, z]
    return P


def step(g, keep, f, mask, new_label, kp=None):
    ids_now = [m.id for m in g.getModels()]
    data = model_data(mask, f["depth"], ids_now + ([g.getNextModelID()] if new_label else [])) if g.getTick() > 1 else None
    if kp is not None:
        g.setKeypoints(*kp)
    keep.append((dev(f["rgb"]), dev(f["depth"]), dev(mask)))
    g.processFrame(*keep[-1][:2], timestamp=1000 + len(keep), mask=keep[-1][2], hasNewLabel=new_label, modelData=data)


@pytest.fixture(scope="module")
def saved(gpu_ctx, tmp_path_factory):
    """Fusion A: the camera model and the object model 1, tracked while it is seen (frames 1..5) and inactive from frame 6 on,
    its keypoint views stored as tests/test_gpu_redetect_fusion.py stores them.  Then exact poses (translations by
    representable numbers: P = global * model^-1 has one answer) and savePly."""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.point_tracker import Keypoint, ModelTracks
    K, poses, objs, traj, with_obj, without = gap_scene(SEED)
    kps, desc = physical_keypoints(SEED, K, poses, traj, with_obj)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setEnableRedetection(True)
    mt = ModelTracks(1)
    tracks = [[] for _ in range(len(desc))]
    keep = []
    for i in range(LAST_SEEN + 2):
        hidden = i > LAST_SEEN
        f = without[i] if hidden else with_obj[i]
        mask = np.zeros((H, W), np.uint8)
        if i >= SPAWN and not hidden:
            mask[f["ids"] == 1] = 1
        step(g, keep, f, mask, i == SPAWN)
        if SPAWN <= i <= LAST_SEEN:
            idx, xy, coord = kps[i]
            P = g.getModels()[1].getPose()
            for j in range(len(desc)):
                hit = np.flatnonzero(idx == j)
                tracks[j].append(Keypoint(1000 + i, tuple(xy[hit[0]]), coord[hit[0]].astype(np.float64), desc[j]) if len(hit) else None)
            if i == SPAWN:
                mt.initGlobalTracks(tracks, P, 1000 + i)
            else:
                mt.addPose(P, 1000 + i)
    assert [m.id for m in g.getModels()] == [0] and [m.id for m in g.getInactiveModels()] == [1]
    assert mt.store() is True
    views = mt.views()
    assert g.storeViews(1, views) is True
    G, M = translation(0.5, -0.25, 1.0), translation(0.125, 2.0, -0.75)
    g.getModels()[0].overridePose(G)
    g.getInactiveModels()[0].overridePose(M)
    out = tmp_path_factory.mktemp("export")
    g.savePly(out)
    yield dict(g=g, dir=out, views=views, P={0: translation(0, 0, 0), 1: translation(0.375, -2.25, 1.75)}, scene=(K, poses, traj, with_obj, without),
               kps=kps, desc=desc)
    g.close()


def test_save_writes_the_clouds_and_the_tracks(saved):
    g, out = saved["g"], saved["dir"]
    files = sorted(os.path.relpath(os.path.join(r, f), out) for r, _, fs in os.walk(out) for f in fs)
    assert files == ["cloud-0.ply", "cloud-1.ply", "model_db/model-0/cloud.ply", "model_db/model-1/cloud.ply",
                     "model_db/model-1/tracks.ply"]  # the camera model has no views: no tracks.ply
    for m in g.getModels() + g.getInactiveModels():
        want = mo.cloud_bytes(m.exportCloud(saved["P"][m.id], m.confidenceThreshold()))
        assert (out / f"cloud-{m.id}.ply").read_bytes() == want
        assert (out / "model_db" / f"model-{m.id}" / "cloud.ply").read_bytes() == want
        print(f"model {m.id}: {m.lastCount()} surfels, {(len(want) - len(mo.cloud_header(0))) // 31} stable")
    assert g.getInactiveModels()[0].lastCount() > 500
    assert (out / "model_db" / "model-1" / "tracks.ply").read_bytes() == mo.tracks_bytes(saved["views"], saved["P"][1])


def test_load_restores_the_model_and_it_is_redetected(gpu_ctx, saved):
    from multimotionfusion_amd import modeldb
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K, poses, traj, with_obj, without = saved["scene"]
    b = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    b.setEnableRedetection(True)
    assert b.getNextModelID() == 1
    assert b.loadModels(saved["dir"]) == 1
    inactive = b.getInactiveModels()
    assert len(inactive) == 1 and inactive[0].id == 1 and b.getNextModelID() == 2 and [m.id for m in b.getModels()] == [0]
    assert inactive[0].lastCount() == 0  # no dense surfels, as in the reference
    from_file = modeldb.readTracks(saved["dir"] / "model_db" / "model-1" / "tracks.ply")
    vs = b.getViewStore()
    assert vs.views() == [(1, i, len(d)) for i, (d, _) in enumerate(from_file)] and len(from_file) == len(saved["views"])
    for v, (d, c) in enumerate(from_file):
        gd, gc = vs.downloadView(v)
        assert np.array_equal(gd.view(np.uint32), d.view(np.uint32)) and np.array_equal(gc.view(np.uint32), c.view(np.uint32))
    # one stored view's own keypoints against the loaded model: that view, under the redetection gate (error < 0.01)
    k = 2
    d, c = saved["views"][k]
    best = vs.bestMatch(1, torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda(), c)
    print("best match of view", k, ":", {x: best[x] for x in ("found", "view", "error", "inliers", "n_matches")})
    assert best["found"] and best["view"] == k and best["error"] < 0.01 and best["inliers"] > 5
    # the object is out of sight (frames 6..8), then returns under a new label: the loaded model is activated
    keep = []
    for i in range(LAST_SEEN + 1, BACK):
        step(b, keep, without[i], np.zeros((H, W), np.uint8), False)
        assert b.getLastRedetections() == []
    f = with_obj[BACK]
    mask = np.zeros((H, W), np.uint8)
    mask[f["ids"] == 1] = b.getNextModelID()
    idx, xy, coord = saved["kps"][BACK]
    step(b, keep, f, mask, True, (xy, coord, saved["desc"][idx]))
    ev = b.getLastRedetections()
    assert len(ev) == 1 and ev[0]["activated"] and ev[0]["model_id"] == 1 and ev[0]["label"] == 2 and ev[0]["removed_id"] == -1
    assert ev[0]["error"] < 0.01 and ev[0]["inliers"] > 5
    assert [m.id for m in b.getModels()] == [0, 1] and b.getInactiveModels() == [] and b.getNextModelID() == 2
    b.close()


def test_load_skips_a_broken_file_and_refuses_a_shard(gpu_ctx, saved, tmp_path):
    import shutil
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = saved["scene"][0]
    src = saved["dir"] / "model_db" / "model-1" / "tracks.ply"
    for id_ in (3, 7, 200):
        os.makedirs(tmp_path / "model_db" / f"model-{id_}")
        shutil.copy(src, tmp_path / "model_db" / f"model-{id_}" / "tracks.ply")
    (tmp_path / "model_db" / "model-7" / "tracks.ply").write_bytes(src.read_bytes()[:-3])
    os.makedirs(tmp_path / "model_db" / "model-9")  # a directory without tracks.ply is no model
    b = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    assert b.loadModels(tmp_path) == 2
    assert [m.id for m in b.getInactiveModels()] == [1, 2] and b.getNextModelID() == 3
    err = gpu_ctx.lib.mmf_last_error()
    assert b"model-7" in err and b"mmf_tracks_ply_read" in err
    assert sorted(set(v[0] for v in b.getViewStore().views())) == [1, 2]
    b.close()
    s = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    s.setShard(0, 2)
    with pytest.raises(MmfError) as e:
        s.loadModels(tmp_path)
    assert e.value.status == -4
    s.close()


def test_save_is_observational(gpu_ctx, tmp_path):
    """the same five frames (the object spawns in the second) with and without a savePly behind the third: equal poses and maps"""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K, poses, objs, traj, with_obj, without = gap_scene(SEED)
    result = []
    for save_at in (None, 2):
        g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
        keep = []
        for i in range(5):
            mask = np.zeros((H, W), np.uint8)
            if i >= SPAWN:
                mask[with_obj[i]["ids"] == 1] = 1
            step(g, keep, with_obj[i], mask, i == SPAWN)
            if i == save_at:
                g.savePly(tmp_path)
                assert (tmp_path / "cloud-1.ply").exists() and not (tmp_path / "model_db" / "model-1" / "tracks.ply").exists()
        result.append([(m.id, m.getPose().copy(), m.downloadMap().copy()) for m in g.getModels()])
        g.close()
    a, b = result
    assert [x[0] for x in a] == [x[0] for x in b] == [0, 1]
    for (_, pa, ma), (_, pb, mb) in zip(a, b):
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
        assert ma.shape == mb.shape and np.array_equal(ma.view(np.uint32), mb.view(np.uint32))
