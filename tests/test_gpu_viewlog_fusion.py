"""-m gpu: the models' keypoint views inside MultiMotionFusion::processFrame (Model::store on deactivation, Core/Model/Model.cpp:
1617-1644; mmf_tracker_set_view_log, mmf_tracker_model_views, mmf_viewstore_store_device): the scene and the object's keypoints
of tests/test_gpu_redetect_fusion.py (320 x 240, 14 frames, the object leaves for three frames and comes back under a new label)
plus 100 static landmarks, all of them through DevicePointTracker.addKeypointsPixels + prune.

Run A: a tracker with a view log, redetection on, nobody stores views.  Run B: no log; when model 1 turns up inactive the test
builds its views with tests/viewlog_oracle.py (poses from getPose() after each frame, stamps from the frames) and stores them
with storeViews.  A must be B, bit for bit, at every frame."""
import numpy as np
import pytest
import torch

import tracker_oracle as to
import viewlog_oracle as vo
from test_gpu_redetect_fusion import BACK, H, LAST_SEEN, N_FRAMES, SPAWN, W, gap_scene, model_data, physical_keypoints

pytestmark = pytest.mark.gpu
SEED = 21
LOST = LAST_SEEN + 1  # the frame in which model 1 is found lost


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scene():
    """-> K, per frame (rgb, depth, ids of the rendering the frame shows), per frame the keypoints (xy [m,2], descriptor [m,256])"""
    K, poses, objs, traj, with_obj, without = gap_scene(SEED)
    obj_kps, obj_desc = physical_keypoints(SEED, K, poses, traj, with_obj)
    rng = np.random.default_rng(SEED)
    f0 = with_obj[0]
    ys, xs = np.nonzero((f0["ids"] == 0) & (f0["depth"] > 0))
    pick = rng.choice(len(ys), 100, replace=False)
    cam = f0["vertex"][ys[pick], xs[pick], :3].astype(np.float64)
    world = cam @ poses[0][:3, :3].T + poses[0][:3, 3]
    land_desc = vo.unit_rows(rng, 100)
    frames, kps = [], []
    for i in range(N_FRAMES):
        hidden = LAST_SEEN < i < BACK
        frames.append(without[i] if hidden else with_obj[i])
        Pi = np.linalg.inv(poses[i])
        x = world @ Pi[:3, :3].T + Pi[:3, 3]
        u = np.rint(x[:, 0] / x[:, 2] * K["fx"] + K["cx"]).astype(np.int64)
        v = np.rint(x[:, 1] / x[:, 2] * K["fy"] + K["cy"]).astype(np.int64)
        ok = (x[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        xy, desc = np.stack([u[ok], v[ok]], 1).astype(np.int32), land_desc[ok]
        if not hidden and i >= SPAWN:
            idx, oxy, _ = obj_kps[i]
            xy, desc = np.concatenate([xy, oxy]), np.concatenate([desc, obj_desc[idx]])
        kps.append((xy, desc))
    return K, frames, kps


def snapshot(g):
    """what a frame left behind, as bytes and integers"""
    act, ina = g.getModels(), g.getInactiveModels()
    return dict(ids=[m.id for m in act], inactive=[m.id for m in ina], next_id=g.getNextModelID(),
                poses=[m.getPose().tobytes() for m in act + ina], counts=[m.lastCount() for m in act + ina],
                events=[{**e, "transformation": e["transformation"].tobytes()} for e in g.getLastRedetections()])


def run(gpu_ctx, scene, log_frames, redetect=True, with_oracle=False, last=N_FRAMES, schedule_at=None, set_log_off=False, reuse=None):
    """-> per frame the snapshot and getLastStoredViews(); with_oracle: the oracle beside the tracker, the views of a model that
    turns up inactive built by it (before the frame's forget / association: Model::store runs before them) and stored by hand"""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.tracker import DevicePointTracker
    K, frames, kps = scene
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    if reuse:  # a fusion and its tracker after their reset
        g, trk = reuse
    else:
        g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
        if redetect:
            g.setEnableRedetection(True)
        trk = DevicePointTracker(gpu_ctx, W, H, intr, capacity=512, max_keypoints=256)
        if log_frames or set_log_off:
            trk.setViewLog(log_frames)
        g.setTracker(trk, odom_init_kp=False)
    ora = vo.ViewLogOracle(to.OracleTracker(W, H, intr, capacity=512), 16) if with_oracle else None
    out = dict(frames=[], stored=[], oracle_views={}, maps=None)
    model_poses = {}  # model id -> [(stamp, pose)]
    keep, obj_id = [], 1
    for i in range(last):
        f = frames[i]
        hidden = LAST_SEEN < i < BACK
        ids_now = [m.id for m in g.getModels()]
        if schedule_at == i:
            g.scheduleDeactivation(1)
        new_label = i == SPAWN or i == BACK
        label = g.getNextModelID() if new_label else obj_id
        mask = np.zeros((H, W), np.uint8)
        if i >= SPAWN and (not hidden if schedule_at is None else i < schedule_at):
            mask[f["ids"] == 1] = label
        data = model_data(mask, f["depth"], ids_now + ([label] if new_label else [])) if i > 0 else None
        ts = 1000 + i
        xy, desc = kps[i]
        keep.append((dev(f["rgb"]), dev(f["depth"]), dev(mask)))
        trk.addKeypointsPixels(xy, desc, ts, keep[-1][1], 0.7, 30)
        trk.prune(30, max(ts - int(1e9), 0))
        assert trk.frame() == i + 1
        if ora:
            ora.add(xy, desc, ts, f["depth"], 0.7, 30)
            ora.t.prune(30, max(ts - int(1e9), 0))
        g.processFrame(*keep[-1][:2], timestamp=ts, mask=keep[-1][2], hasNewLabel=new_label, modelData=data)
        snap = snapshot(g)
        out["frames"].append(snap)
        out["stored"].append(g.getLastStoredViews())
        if i == BACK:
            obj_id = snap["ids"][-1]
        activated = {e["model_id"] for e in snap["events"] if e["activated"]}
        for m in g.getModels()[1:] + g.getInactiveModels():  # Model::appendPoses; a re-activated model restarts (Model::activate)
            lost_now = m.id in snap["inactive"] and m.id in ids_now
            if m.id in snap["ids"] or lost_now:
                if m.id in activated:
                    model_poses[m.id] = []
                if not (lost_now and schedule_at == i):  # (a scheduled model left before the frame's tracking)
                    model_poses.setdefault(m.id, []).append((i + 1, m.getPose().copy()))
            if lost_now and ora:
                stamps, poses = zip(*model_poses[m.id])
                views, missing = ora.model_views(m.id, stamps, poses)
                assert missing == 0
                out["oracle_views"][m.id] = views
                if not log_frames:
                    assert g.storeViews(m.id, views) is True
        if ora:
            for m in ids_now:
                if m not in snap["ids"]:
                    ora.t.forget(m)
            mask_now = g.getTexture("MASK").cpu().numpy()
            if i == 0:
                ora.t.associate_all([0])
            else:
                ora.t.associate(mask_now, snap["ids"])
            assert to.same_table(trk.download(), ora.t.flatten()) is None, i
    out["maps"] = [m.downloadMap().tobytes() for m in g.getModels()]
    out["store_views"] = g.getViewStore().views() if redetect else []
    out["fusion"], out["tracker"] = g, trk
    return out


def finish(r):
    r["fusion"].setTracker(None)
    r["tracker"].close()
    r["fusion"].close()


def test_an_object_that_leaves_and_comes_back_keeps_its_id_without_a_caller_kept_history(gpu_ctx, orc, scene):
    """A (16-frame log, nobody calls storeViews) against B (no log, the oracle's views stored by hand): events, active and
    inactive ids, the next id, every model's pose and surfel count, bit for bit at every frame.  On the parent commit A fails:
    nothing stores the views and the object comes back with a new id."""
    b = run(gpu_ctx, scene, 0, with_oracle=True)
    ev = b["frames"][BACK]["events"]
    assert len(ev) == 1 and ev[0]["activated"] and ev[0]["model_id"] == 1 and ev[0]["error"] < 0.01 and ev[0]["inliers"] > 5
    assert b["frames"][BACK]["ids"] == [0, 1] and b["frames"][BACK]["inactive"] == [] and b["frames"][BACK]["next_id"] == 2
    assert b["frames"][LOST]["ids"] == [0] and b["frames"][LOST]["inactive"] == [1]
    assert all(s == [] for s in b["stored"])  # no log: the fusion stores nothing
    views = b["oracle_views"][1]
    rows = [d.shape[0] for d, _ in views]
    assert len(views) == LOST - SPAWN + 1 and min(rows[:-1]) >= 20, rows  # (the last view: the frame without the object)
    a = run(gpu_ctx, scene, 16)
    for i, (fa, fb) in enumerate(zip(a["frames"], b["frames"])):
        assert fa == fb, (i, {k: (fa[k], fb[k]) for k in fa if fa[k] != fb[k] and k not in ("poses",)})
    for i, s in enumerate(a["stored"]):
        assert s == ([dict(model_id=1, n_views=len(views), rows=sum(rows))] if i == LOST else []), (i, s)
    assert a["store_views"] == b["store_views"] == [(1, v, n) for v, n in enumerate(rows)]
    assert a["maps"] == b["maps"]
    # mmf_fusion_reset clears the lists: the same sequence again stores the same views, not the old entries' as well
    a["fusion"].reset()
    a["tracker"].reset()
    again = run(gpu_ctx, scene, 16, last=LOST + 1, reuse=(a["fusion"], a["tracker"]))
    assert again["stored"] == a["stored"][:LOST + 1]
    assert again["store_views"] == [(-1, v, n) for _, v, n in a["store_views"]] + a["store_views"]  # (the old map's views belong to nobody)
    for fa, fb in zip(again["frames"], a["frames"]):
        assert (fa["ids"], fa["inactive"], fa["next_id"], fa["events"]) == (fb["ids"], fb["inactive"], fb["next_id"], fb["events"])
    finish(a)
    finish(b)


def test_a_short_log_stores_its_last_frames(gpu_ctx, orc, scene):
    """a log of 3 frames: 3 views, the oracle's last 3"""
    b = run(gpu_ctx, scene, 16, with_oracle=True, last=LOST + 1)  # (log on: the fusion stores; the oracle's views for comparison)
    rows = [d.shape[0] for d, _ in b["oracle_views"][1]]
    a = run(gpu_ctx, scene, 3, last=LOST + 1)
    assert a["stored"][LOST] == [dict(model_id=1, n_views=3, rows=sum(rows[-3:]))]
    assert a["store_views"] == [(1, v, n) for v, n in enumerate(rows[-3:])] and sum(rows[-3:]) > 40
    assert b["store_views"] == [(1, v, n) for v, n in enumerate(rows)]
    # the rows themselves: both stores answer a query made of the oracle's views alike, view by view
    q = torch.from_numpy(np.concatenate([d for d, _ in b["oracle_views"][1][-3:]])).cuda()
    ia, da = a["fusion"].getViewStore().match(q)
    ib, db = b["fusion"].getViewStore().match(q)
    assert np.array_equal(ia, ib[-3:]) and np.array_equal(da.view(np.uint32), db[-3:].view(np.uint32))
    finish(a)
    finish(b)


def test_a_scheduled_deactivation_stores_too(gpu_ctx, orc, scene):
    """model 1 is scheduled at frame 4 and leaves before that frame's tracking: the views of frames 1 .. 3, paired by stamp"""
    a = run(gpu_ctx, scene, 16, with_oracle=True, last=5, schedule_at=4)
    assert a["frames"][4]["ids"] == [0] and a["frames"][4]["inactive"] == [1]
    views = a["oracle_views"][1]
    rows = [d.shape[0] for d, _ in views]
    assert len(views) == 3 and min(rows) >= 20
    assert a["stored"][4] == [dict(model_id=1, n_views=3, rows=sum(rows))] and all(s == [] for s in a["stored"][:4])
    assert a["store_views"] == [(1, v, n) for v, n in enumerate(rows)]
    from multimotionfusion_amd.redetection import ViewStore
    host = ViewStore(gpu_ctx)
    assert host.store(1, views)
    q = torch.from_numpy(np.concatenate([d for d, _ in views])[::2].copy()).cuda()
    (ia, da), (ib, db) = a["fusion"].getViewStore().match(q), host.match(q)
    assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    host.close()
    finish(a)


def test_nothing_is_stored_without_redetection_and_the_log_changes_no_frame(gpu_ctx, scene):
    """redetection off with a log: getLastStoredViews stays empty.  Log off and redetection off: six frames with the tracker
    attached give the same poses and maps whether or not setViewLog(0) was called -- and the same as with a log nobody reads"""
    runs = [run(gpu_ctx, scene, 0, redetect=False, last=6), run(gpu_ctx, scene, 0, redetect=False, last=6, set_log_off=True),
            run(gpu_ctx, scene, 16, redetect=False, last=LOST + 1)]
    for r in runs:
        assert all(s == [] for s in r["stored"])
    assert runs[0]["frames"] == runs[1]["frames"] and runs[0]["maps"] == runs[1]["maps"]
    assert runs[2]["frames"][:6] == runs[0]["frames"]
    assert runs[2]["frames"][LOST]["inactive"] == [1]
    for r in runs:
        finish(r)
