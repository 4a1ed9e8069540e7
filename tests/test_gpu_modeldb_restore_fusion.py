"""-m gpu: loadModels(dir, dense=True) on the fusion: the restored model's surfels against the oracle's import
of its cloud.ply, the activating frame bringing them into its window, the flag leaving the camera model alone, and the files
that cannot be used.  Scene, keypoints and stepping: tests/test_gpu_redetect_fusion.py and tests/test_gpu_modeldb_fusion.py."""
import os
import shutil

import numpy as np
import pytest

import modeldb_import_oracle as io
import modeldb_oracle as mo
from test_gpu_modeldb_fusion import SEED, step, translation
from test_gpu_redetect_fusion import BACK, H, LAST_SEEN, SPAWN, W, gap_scene, physical_keypoints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def saved_db(gpu_ctx, tmp_path_factory):
    """A fusion with the camera model and the object model 1 (seen in frames 1..5, inactive from frame 6 on, its keypoint
    views stored), exact poses, savePly: the directory a later run restores from."""
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
    assert mt.store() is True and g.storeViews(1, mt.views()) is True
    g.getModels()[0].overridePose(translation(0.5, -0.25, 1.0))
    g.getInactiveModels()[0].overridePose(translation(0.125, 2.0, -0.75))
    out = tmp_path_factory.mktemp("restore")
    g.savePly(out)
    g.close()
    return dict(dir=out, cloud=out / "model_db" / "model-1" / "cloud.ply", K=K, with_obj=with_obj, without=without, kps=kps, desc=desc)


def new_fusion(gpu_ctx, K, **overrides):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, **overrides)
    g.setEnableRedetection(True)
    return g


def test_dense_load_gives_the_model_the_files_surfels(gpu_ctx, saved_db):
    from multimotionfusion_amd import modeldb
    records = modeldb.readCloud(saved_db["cloud"])
    assert len(records) > 500
    b = new_fusion(gpu_ctx, saved_db["K"])
    tick = b.getTick()
    assert b.loadModels(saved_db["dir"], dense=True) == 1
    inactive = b.getInactiveModels()
    assert len(inactive) == 1 and inactive[0].id == 1 and [m.id for m in b.getModels()] == [0] and b.getNextModelID() == 2
    want = io.import_cloud(records, io.IDENTITY, np.float32(inactive[0].confidenceThreshold()) + np.float32(1), tick)
    assert inactive[0].lastCount() == len(records)
    assert io.surfels_equal(inactive[0].downloadMap(), want)
    assert b.getLastDenseRestores() == [dict(model_id=1, surfels=len(records), status="restored")]
    assert gpu_ctx.lib.mmf_last_error() == b""
    # stable for the model: every surfel is exported again
    again = inactive[0].exportCloud(io.IDENTITY, inactive[0].confidenceThreshold())
    assert len(again) == len(records) and mo.records_equal(again, mo.export_cloud(want, io.IDENTITY, inactive[0].confidenceThreshold()))
    b.close()
    c = new_fusion(gpu_ctx, saved_db["K"])
    assert c.loadModels(saved_db["dir"], dense=False) == 1
    assert c.getInactiveModels()[0].lastCount() == 0 and c.getLastDenseRestores() == []  # as in the reference
    c.close()


def run_restored(gpu_ctx, saved_db, dense, frames_after=2):
    """a fresh fusion restored from the directory; the object is out of sight (frames 6..8), returns under a new label (frame
    9) and is tracked for `frames_after` more frames -> what the activating frame left, and the end state"""
    b = new_fusion(gpu_ctx, saved_db["K"])
    load_tick = b.getTick()
    assert b.loadModels(saved_db["dir"], dense=dense) == 1
    with_obj, without = saved_db["with_obj"], saved_db["without"]
    keep = []
    for i in range(LAST_SEEN + 1, BACK):
        step(b, keep, without[i], np.zeros((H, W), np.uint8), False)
        assert b.getLastRedetections() == []
    f = with_obj[BACK]
    mask = np.zeros((H, W), np.uint8)
    mask[f["ids"] == 1] = b.getNextModelID()
    idx, xy, coord = saved_db["kps"][BACK]
    act_tick = b.getTick()
    step(b, keep, f, mask, True, (xy, coord, saved_db["desc"][idx]))
    ev = b.getLastRedetections()
    assert len(ev) == 1 and ev[0]["activated"] and ev[0]["model_id"] == 1 and ev[0]["label"] == 2 and ev[0]["removed_id"] == -1
    assert ev[0]["error"] < 0.01 and ev[0]["inliers"] > 5
    assert [m.id for m in b.getModels()] == [0, 1] and b.getInactiveModels() == [] and b.getNextModelID() == 2
    out = dict(load_tick=load_tick, act_tick=act_tick, map_at_activation=b.getModels()[1].downloadMap().copy(), timings=b.lastTimings())
    for i in range(BACK + 1, BACK + 1 + frames_after):
        f = with_obj[i]
        mask = np.zeros((H, W), np.uint8)
        mask[f["ids"] == 1] = 1
        step(b, keep, f, mask, False)
    cam = b.getModels()[0]
    out["camera"] = (cam.getPose().copy(), cam.downloadMap().copy())
    b.close()
    return out


@pytest.fixture(scope="module")
def restored_runs(gpu_ctx, saved_db):
    return {dense: run_restored(gpu_ctx, saved_db, dense) for dense in (False, True)}  # the control first


def test_activation_brings_the_restored_surfels_into_the_window(saved_db, restored_runs):
    from multimotionfusion_amd import modeldb
    n_file = len(modeldb.readCloud(saved_db["cloud"]))
    off, on = restored_runs[False], restored_runs[True]
    assert off["load_tick"] == on["load_tick"] and off["act_tick"] == on["act_tick"] > on["load_tick"]
    # the control: without the flag nothing the model holds after the activating frame carries the load's tick (on this scene it
    # holds nothing at all then: the frame's mask carries the new label, so nothing is fused into the model before the next frame)
    assert not (off["map_at_activation"][:, 6] == off["load_tick"]).any()
    s = on["map_at_activation"]
    from_file = s[:, 6] == on["load_tick"]
    assert from_file.any()
    assert (s[from_file, 7] == on["act_tick"]).all()  # none was left outside the window
    print(f"restored surfels after the activating frame's clean: {int(from_file.sum())} of {n_file} in the file; the model holds {len(s)} "
          f"(without the flag {len(off['map_at_activation'])})")
    print(f"activating frame, host wall clock (tracking phase, whole call): dense {on['timings']}, not dense {off['timings']}")


def test_the_flag_leaves_the_camera_model_alone(restored_runs):
    (pa, ma), (pb, mb) = restored_runs[False]["camera"], restored_runs[True]["camera"]
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert ma.shape == mb.shape and len(ma) > 1000 and np.array_equal(ma.view(np.uint32), mb.view(np.uint32))


def test_files_that_cannot_be_used_leave_the_model_without_surfels(gpu_ctx, saved_db, tmp_path):
    from multimotionfusion_amd import modeldb
    from multimotionfusion_amd._capi import MmfError
    src = saved_db["dir"] / "model_db" / "model-1"
    cap = 300
    records = modeldb.readCloud(saved_db["cloud"])
    assert len(records) > cap + 1
    for id_ in (3, 7, 9, 200):
        os.makedirs(tmp_path / "model_db" / f"model-{id_}")
        shutil.copy(src / "tracks.ply", tmp_path / "model_db" / f"model-{id_}" / "tracks.ply")
    modeldb.writeCloud(tmp_path / "model_db" / "model-3" / "cloud.ply", records[:cap])  # exactly what the model holds
    (tmp_path / "model_db" / "model-7" / "cloud.ply").write_bytes(mo.cloud_bytes(records[:cap])[:-3])  # cut short
    # model-9: no cloud.ply
    modeldb.writeCloud(tmp_path / "model_db" / "model-200" / "cloud.ply", records[:cap + 1])  # one more than the model holds
    b = new_fusion(gpu_ctx, saved_db["K"], max_object_surfels=cap)
    assert b.loadModels(tmp_path, dense=True) == 4
    err = gpu_ctx.lib.mmf_last_error()
    assert b"model-200" in err and b"cloud.ply" in err and b"mmf_model_import_ply" in err  # the last file that was skipped
    inactive = b.getInactiveModels()
    assert [m.id for m in inactive] == [1, 2, 3, 4] and [m.lastCount() for m in inactive] == [cap, 0, 0, 0]
    assert b.getLastDenseRestores() == [dict(model_id=1, surfels=cap, status="restored"), dict(model_id=2, surfels=0, status="does not parse"),
                                        dict(model_id=3, surfels=0, status="no file"), dict(model_id=4, surfels=0, status="too large")]
    assert sorted(set(v[0] for v in b.getViewStore().views())) == [1, 2, 3, 4]  # every model has its views all the same
    b.close()
    # each kind alone: mmf_last_error names that file
    for id_, what in ((7, b"mmf_ply_read_cloud"), (9, b"no such file")):
        one = tmp_path / f"only-{id_}"
        shutil.copytree(tmp_path / "model_db" / f"model-{id_}", one / "model_db" / f"model-{id_}")
        b = new_fusion(gpu_ctx, saved_db["K"], max_object_surfels=cap)
        assert b.loadModels(one, dense=True) == 1 and b.getInactiveModels()[0].lastCount() == 0
        err = gpu_ctx.lib.mmf_last_error()
        assert f"model-{id_}".encode() in err and b"cloud.ply" in err and what in err, err
        b.close()
    s = new_fusion(gpu_ctx, saved_db["K"])
    s.setEnableRedetection(False)
    s.setShard(0, 2)
    with pytest.raises(MmfError) as e:
        s.loadModels(tmp_path, dense=True)
    assert e.value.status == -4
    s.close()
