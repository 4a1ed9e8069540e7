"""-m gpu: processFrame with the segmentation from the frame's own label image switched on
(mmf_fusion_set_mask_segmentation; Segmentation.cpp:89-147 and what MultiMotionFusion.cpp:410-415, 469-487, 585-620 do
with its result): 320x240, seven frames, two moving boxes from synth, raw labels {0 -> 0, 1 -> 37, 2 -> 200}.

Run A (mode on, model_spawn_offset 1) is checked against the rule itself -- which frame spawns which label under which id,
the table, the 0.4 confidence threshold, a model leaving the list when its label is missing for a frame, inhibit_new, the
maskless frame, reset -- and against run B: the mode off and the pre-mapped path fed A's id image, model data and
has_new_label.  B must reproduce A bit for bit after every frame: nothing downstream of the segmentation result may differ."""
import numpy as np
import pytest
import torch

import mask_oracle as mo
from multimotionfusion_amd import synth
from multimotionfusion_amd._capi import MmfError
from multimotionfusion_amd.segmentation import MaskConfig

pytestmark = pytest.mark.gpu
W, H, N_FRAMES = 320, 240, 7
RAW = np.zeros(256, np.uint8)
RAW[1], RAW[2] = 37, 200


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scene():
    seed = 21
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(N_FRAMES, seed=seed)
    objs = synth.make_objects(2, seed=seed)
    traj = synth.object_trajectories(objs, N_FRAMES, seed=seed)
    frames = [synth.render(p, W, H, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    labels = [RAW[f["ids"].astype(np.uint8)] for f in frames]
    for lab in labels:
        assert (lab == 37).sum() > 512 and (lab == 200).sum() > 512, "both boxes are visible in every frame"
    return K, frames, labels


def fusion(gpu_ctx, K, **kw):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    return MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=2, **kw)


def state(g):
    """what the frame left: per model id, pose, confidence threshold and the surfel store in its order"""
    return [(m.id, m.getPose().tobytes(), np.float32(m.confidenceThreshold()).tobytes(), m.downloadMap().tobytes()) for m in g.getModels()]


def rule(labels, spawn_after, inhibit=False, next_id=1):
    """MultiMotionFusion.cpp:410-415, 484 + Segmentation.cpp:106-123 over the sequence: per tracked frame (allow_new,
    new label or -1, spawned id or -1, table)"""
    table, so, out = np.zeros(256, np.uint8), 0, []
    for lab in labels[1:]:
        if so < spawn_after:
            so += 1
        allow = so >= spawn_after
        present, first = np.unique(lab.ravel(), return_index=True)
        unmapped = sorted((i, l) for l, i in zip(present, first) if l != 0 and table[l] == 0)
        new, spawned = -1, -1
        if allow and unmapped:
            new = int(unmapped[0][1])
            table[new] = next_id
            if not inhibit:
                spawned, so, next_id = next_id, 0, next_id + 1
        out.append((allow, new, spawned, table.copy()))
    return out


def run_a(gpu_ctx, scene, labels=None, cfg=None, host=False):
    K, frames, raw = scene
    labels = raw if labels is None else labels
    g = fusion(gpu_ctx, K)
    g.setMaskSegmentation(cfg or MaskConfig(model_spawn_offset=1))
    out, keep = [], []
    for i, f in enumerate(frames):
        if host:
            g.processFrameHost(f["rgb"], f["depth"], timestamp=1000 + i, mask=labels[i], hasNewLabel=True)  # (ignored)
        else:
            keep.append((dev(f["rgb"]), dev(f["depth"]), dev(labels[i])))  # predict() re-reads the frame: keep it alive
            g.processFrame(*keep[-1][:2], timestamp=1000 + i, mask=keep[-1][2], hasNewLabel=(i % 2 == 0))  # (ignored)
        out.append(dict(state=state(g), mask=g.getTexture("MASK").clone(), mapping=g.maskMapping(),
                        seg=g.lastMaskSegmentation() if i > 0 else None, ids=[m.id for m in g.getModels()],
                        inactive=[m.id for m in g.getInactiveModels()], conf=[m.confidenceThreshold() for m in g.getModels()]))
    return g, out


def test_spawns_table_thresholds_and_the_premapped_path_agree(gpu_ctx, scene):
    K, frames, raw = scene
    g, a = run_a(gpu_ctx, scene)
    expect = rule(raw, 1)
    # 37 and 200 spawn in the first two tracked frames, one per frame, ids 1 and 2 in raster-first order
    assert [e[2] for e in expect] == [1, 2] + [-1] * (N_FRAMES - 3)
    ids = [0]
    for i in range(1, N_FRAMES):
        allow, new, spawned, table = expect[i - 1]
        if spawned >= 0:
            ids.append(spawned)
        r = a[i]
        assert r["ids"] == ids and r["inactive"] == [], (i, r["ids"])
        assert r["seg"]["allow_new"] == allow and r["seg"]["new_label"] == new and r["seg"]["has_new_label"] == (spawned >= 0)
        assert np.array_equal(r["mapping"], table), i
        # the id image and the model data are the oracle's for the table and the list the frame found
        before = expect[i - 2][3] if i >= 2 else np.zeros(256, np.uint8)
        o = mo.segment(raw[i], frames[i]["depth"], a[i - 1]["ids"], len(a[i - 1]["ids"]), allow, before)
        assert np.array_equal(r["mask"].cpu().numpy(), o["mask"])
        assert [(e["id"], e["super_pixel_count"]) for e in r["seg"]["model_data"]] == [(e["id"], e["super_pixel_count"]) for e in o["model_data"]]
        for e, x in zip(r["seg"]["model_data"], o["model_data"]):
            assert mo.ulp_distance(np.float32(e["depth_mean"]), x["depth_mean"]) <= 1 and np.float32(e["avg_confidence"]) == np.float32(0.4)
        # object thresholds: 0.4 from the model data (:616-620), at the latest after the model's first tracked frame
        for k, m_id in enumerate(r["ids"]):
            if m_id != 0 and m_id in a[i - 1]["ids"]:
                assert np.float32(r["conf"][k]) == np.float32(0.4), (i, m_id, r["conf"][k])
    first = int(raw[1].ravel()[np.flatnonzero(raw[1].ravel())[0]])  # the label met first in raster order
    assert a[-1]["mapping"][first] == 1 and a[-1]["mapping"][37 + 200 - first] == 2 and a[-1]["mapping"].sum() == 3
    # a maskless frame falls through to the callback / the CRF: none is set
    with pytest.raises(MmfError) as e:
        g.processFrame(dev(frames[-1]["rgb"]), dev(frames[-1]["depth"]), timestamp=2000)
    assert e.value.status == -1 and "needs a segmentation" in str(e.value)
    g.reset()
    assert not g.maskMapping().any() and [m.id for m in g.getModels()] == [0]
    with pytest.raises(MmfError) as e:
        g.lastMaskSegmentation()
    assert e.value.status == -4
    g.close()

    # run B: the mode off, the pre-mapped path with A's id image, model data and has_new_label
    b = fusion(gpu_ctx, K)
    keep = []
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"]), a[i]["mask"]))
        seg = a[i]["seg"]
        b.processFrame(*keep[-1][:2], timestamp=1000 + i, mask=keep[-1][2], hasNewLabel=bool(seg and seg["has_new_label"]),
                       modelData=seg["model_data"] if seg else None)
        sb = state(b)
        assert [s[0] for s in sb] == [s[0] for s in a[i]["state"]], i
        for x, y in zip(sb, a[i]["state"]):
            assert x[1] == y[1], ("pose", i, x[0])
            assert x[2] == y[2], ("confidence threshold", i, x[0])
            assert x[3] == y[3], ("surfels", i, x[0], len(x[3]), len(y[3]))
    assert not b.maskMapping().any()  # the mode off touches nothing of it
    b.close()

    # the host hand-over (mmf_fusion_process_frame_host: FrameData::mask = raw labels) is the same frame step
    gh, ah = run_a(gpu_ctx, scene, host=True)
    for i in range(N_FRAMES):
        assert ah[i]["ids"] == a[i]["ids"] and np.array_equal(ah[i]["mapping"], a[i]["mapping"])
        assert torch.equal(ah[i]["mask"], a[i]["mask"]) and ah[i]["seg"] == a[i]["seg"]
        assert [s[:3] for s in ah[i]["state"]] == [s[:3] for s in a[i]["state"]], i
    gh.close()


def test_a_model_whose_label_is_missing_for_a_frame_leaves_the_list(gpu_ctx, scene):
    K, frames, raw = scene
    first = int(raw[1].ravel()[np.flatnonzero(raw[1].ravel())[0]])  # the label that became model 1
    labels = [l.copy() for l in raw]
    labels[4][labels[4] == first] = 0
    g, a = run_a(gpu_ctx, scene, labels=labels)
    assert a[3]["ids"] == [0, 1, 2] and a[3]["inactive"] == []
    assert a[4]["seg"]["model_data"][1] == dict(id=1, super_pixel_count=0, avg_confidence=a[4]["seg"]["model_data"][1]["avg_confidence"],
                                                depth_mean=0.0, depth_std=0.0)
    assert a[4]["ids"] == [0, 2] and a[4]["inactive"] == [1]  # (:606-613)
    # the label is back and still mapped to the model that left: its pixels keep the id, no entry counts them (B7)
    assert a[5]["ids"] == [0, 2] and a[5]["mapping"][first] == 1 and not a[5]["seg"]["has_new_label"]
    m5 = a[5]["mask"].cpu().numpy()
    assert np.array_equal(m5 == 1, labels[5] == first) and [e["id"] for e in a[5]["seg"]["model_data"]] == [0, 2]
    g.close()


def test_inhibit_new_spawns_nothing_and_records_the_table_entry(gpu_ctx, scene):
    K, frames, raw = scene
    g, a = run_a(gpu_ctx, scene, cfg=MaskConfig(model_spawn_offset=1, inhibit_new=1))
    expect = rule(raw, 1, inhibit=True)
    first = expect[0][1]
    for i in range(1, N_FRAMES):
        assert a[i]["ids"] == [0] and not a[i]["seg"]["has_new_label"]
        assert np.array_equal(a[i]["mapping"], expect[i - 1][3])
    # both labels end up on the id that never came (the mask and the entry stay, MultiMotionFusion.cpp:413-415)
    assert a[1]["seg"]["new_label"] == first and a[1]["mapping"][first] == 1 and a[2]["mapping"][37 + 200 - first] == 1
    assert (a[1]["mask"].cpu().numpy() == 1).sum() == (raw[1] == first).sum()
    g.close()


def test_setter_is_refused_on_a_shard(gpu_ctx, scene):
    K = scene[0]
    g = fusion(gpu_ctx, K)
    g.setShard(0, 2)
    with pytest.raises(MmfError) as e:
        g.setMaskSegmentation(True)
    assert e.value.status == -4  # MMF_ERR_STATE
    g.close()
