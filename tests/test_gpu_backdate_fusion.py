"""-m gpu: back-dating inside MultiMotionFusion::processFrame (mmf_fusion_set_track_backdating; refineTrackSubset(segm_tracks[uid],
globalModel, 2), MultiMotionFusion.cpp:596-599) on the scene of tests/backdate_scene.py, frames 0 .. LOST.

Run A: back-dating on.  Run B: off.  The frames are the same bit for bit; A reports the oracle's pose list in the spawn frame
and nothing elsewhere; at the lost frame A stores B's views plus len - 1 more, in front, built from the back-dated poses."""
import numpy as np
import pytest
import torch

import backdate_oracle as bo
import backdate_scene as bs
import tracker_oracle as to
import viewlog_oracle as vo
from backdate_scene import H, LOST, SPAWN, W
from test_gpu_redetect_fusion import model_data

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scene():
    return bs.build()


def snapshot(g):
    act, ina = g.getModels(), g.getInactiveModels()
    return dict(ids=[m.id for m in act], inactive=[m.id for m in ina], next_id=g.getNextModelID(),
                poses=[m.getPose().tobytes() for m in act + ina], counts=[m.lastCount() for m in act + ina],
                events=[{**e, "transformation": e["transformation"].tobytes()} for e in g.getLastRedetections()])


def run(gpu_ctx, scene, history):
    """history None: the setter is never called; 0: called with 0; else back-dating with that history.  -> per frame the
    snapshot, getLastBackdatedPoses(), getLastStoredViews(); the oracle's pose list of the spawn frame, the model's
    (stamp, pose) list, the stored views' rows and the maps"""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.tracker import DevicePointTracker
    K, frames, kps = scene
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setEnableRedetection(True)
    trk = DevicePointTracker(gpu_ctx, W, H, intr, capacity=512, max_keypoints=256)
    trk.setViewLog(16)
    g.setTracker(trk, odom_init_kp=False)
    if history is not None:
        g.setTrackBackdating(history)
    ora = bo.BackdateOracle(to.OracleTracker(W, H, intr, capacity=512), 16)
    out = dict(frames=[], backdated=[], stored=[], model_poses=[], launches=None)
    keep = []
    for i in range(LOST + 1):
        f = frames[i]
        ids_now = [m.id for m in g.getModels()]
        new_label = i == SPAWN
        mask = bs.frame_mask(frames, i)
        data = model_data(mask, f["depth"], ids_now + ([1] if new_label else [])) if i > 0 else None
        ts = 1000 + i
        xy, desc = kps[i]
        keep.append((dev(f["rgb"]), dev(f["depth"]), dev(mask)))
        trk.addKeypointsPixels(xy, desc, ts, keep[-1][1], 0.7, 30)
        trk.prune(30, max(ts - int(1e9), 0))
        ora.add(xy, desc, ts, f["depth"], 0.7, 30)
        ora.t.prune(30, max(ts - int(1e9), 0))
        g.processFrame(*keep[-1][:2], timestamp=ts, mask=keep[-1][2], hasNewLabel=new_label, modelData=data)
        if i == SPAWN:
            out["launches"] = trk.lastLaunches()
        snap = snapshot(g)
        out["frames"].append(snap)
        out["backdated"].append(g.getLastBackdatedPoses())
        out["stored"].append(g.getLastStoredViews())
        if 1 in snap["ids"]:
            out["model_poses"].append((i + 1, g.getModels()[snap["ids"].index(1)].getPose().copy()))
        if 1 in snap["inactive"] and 1 in ids_now:  # found lost: Model::appendPoses ran before
            out["model_poses"].append((i + 1, g.getInactiveModels()[0].getPose().copy()))
            # (the oracle's views before this frame's forget / association: Model::store runs before them)
            stamps, poses = zip(*out["model_poses"])
            out["own_views"] = ora.model_views(1, stamps, poses)[0]
            if "want" in out:
                e = out["want"][:-1]
                out["front_views"] = ora.model_views(1, [x["stamp"] for x in e], [x["pose"] for x in e])[0]
        for m in ids_now:
            if m not in snap["ids"]:
                ora.t.forget(m)
        if i == 0:
            ora.t.associate_all([0])
        else:
            ora.t.associate(g.getTexture("MASK").cpu().numpy(), snap["ids"])
        assert to.same_table(trk.download(), ora.t.flatten()) is None, i
        if i == SPAWN and history:
            out["want"] = ora.backdate(1, history)[0]
    vs = g.getViewStore()
    out["store_views"] = vs.views()
    out["views"] = [vs.downloadView(v) for v in range(len(out["store_views"]))]
    out["maps"] = [m.downloadMap().tobytes() for m in g.getModels()]
    g.setTracker(None)
    trk.close()
    g.close()
    return out


@pytest.fixture(scope="module")
def runs(gpu_ctx, orc, scene):
    return {h: run(gpu_ctx, scene, h) for h in (4, 2, 0, None)}


def test_the_frames_do_not_depend_on_the_feature(runs):
    """ids, poses, counts, events at every frame up to the lost one, and the maps: on (history 4, 2), switched off, never called"""
    b = runs[None]
    assert b["frames"][SPAWN]["ids"] == [0, 1] and b["frames"][LOST]["ids"] == [0] and b["frames"][LOST]["inactive"] == [1]
    for h in (4, 2, 0):
        for i, (fa, fb) in enumerate(zip(runs[h]["frames"], b["frames"])):
            assert fa == fb, (h, i)
        assert runs[h]["maps"] == b["maps"], h
    assert runs[0]["views"] and vo.same_views(runs[0]["views"], b["views"]) is None and runs[0]["stored"] == b["stored"]
    assert all(x == (-1, []) for r in (runs[0], b) for x in r["backdated"])


@pytest.mark.parametrize("history", [4, 2])
def test_the_spawn_frame_reports_the_oracles_pose_list_and_no_other_frame_does(runs, history):
    a = runs[history]
    for i, (mid, entries) in enumerate(a["backdated"]):
        if i != SPAWN:
            assert (mid, entries) == (-1, []), i
    mid, entries = a["backdated"][SPAWN]
    assert mid == 1 and bo.same_entries(entries, a["want"]) is None, bo.same_entries(entries, a["want"])
    # two frames since the table was empty: len 2 whatever the history, one pair, estimated on the device
    assert len(entries) == min(SPAWN + 1, history) == 2 and entries[1]["nvalid"] >= 3 and entries[1]["status"] == bo.OK
    assert entries[1]["host_estimated"] == 0 and a["launches"] == 3


@pytest.mark.parametrize("history", [4, 2])
def test_the_lost_model_stores_its_back_dated_views_in_front_of_the_others(runs, history):
    a, b = runs[history], runs[None]
    n_front = len(a["want"]) - 1
    assert n_front == 1  # (history 2 and 4 alike: exactly one more view)
    nb = len(b["views"])
    assert nb == LOST - SPAWN + 1 and b["store_views"] == [(1, v, d.shape[0]) for v, (d, _) in enumerate(b["views"])]
    assert len(a["views"]) == nb + n_front and [m for m, _, _ in a["store_views"]] == [1] * (nb + n_front)
    assert a["stored"][LOST] == [dict(model_id=1, n_views=nb + n_front, rows=sum(d.shape[0] for d, _ in a["views"]))]
    assert all(s == [] for i, s in enumerate(a["stored"]) if i != LOST)
    # the common views are the same bytes, and the oracle's
    assert vo.same_views(a["views"][n_front:], b["views"]) is None
    assert vo.same_views(b["views"], b["own_views"]) is None
    # the added ones are the oracle's views of the earlier frames under the back-dated poses
    assert vo.same_views(a["views"][:n_front], a["front_views"]) is None
    assert a["views"][0][0].shape[0] >= 3


def test_what_the_setter_refuses(gpu_ctx, scene):
    """history 0 (off), 2 .. 256; MMF_ERR_STATE on a shard, and a shard is refused while it is on; without a tracker the feature does
    nothing"""
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = scene[0]
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    assert g.getLastBackdatedPoses() == (-1, [])
    for bad in (1, -1, 257):
        with pytest.raises(MmfError):
            g.setTrackBackdating(bad)
    g.setShard(0, 2)
    with pytest.raises(MmfError):
        g.setTrackBackdating(2)
    assert gpu_ctx.lib.mmf_fusion_set_track_backdating(g.handle, 2) == -4  # MMF_ERR_STATE
    g.setTrackBackdating(0)  # (off is always allowed)
    g.setShard(0, 1)
    g.setTrackBackdating(256)
    with pytest.raises(MmfError):
        g.setShard(0, 2)
    g.setTrackBackdating(0)
    g.setTrackBackdating(2)
    # on, but no tracker attached: two frames, the second spawns a model, nothing is back-dated
    _, frames, _ = scene
    for i in range(SPAWN + 1):
        f = frames[i]
        mask = bs.frame_mask(frames, i)
        data = model_data(mask, f["depth"], [0] + ([1] if i == SPAWN else [])) if i > 0 else None
        g.processFrame(dev(f["rgb"]), dev(f["depth"]), timestamp=1000 + i, mask=dev(mask), hasNewLabel=i == SPAWN, modelData=data)
    assert [m.id for m in g.getModels()] == [0, 1] and g.getLastBackdatedPoses() == (-1, [])
    g.close()
