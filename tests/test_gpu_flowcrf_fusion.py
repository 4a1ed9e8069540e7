"""-m gpu: the flow-CRF inference hook of processFrame (mmf_fusion_set_flow_inference).  The sequence of
test_gpu_flow_fusion.py (320 x 240, one moving box that the built-in segmentation spawns: two models) with the optical-flow hook
on, once without and once with the inference hook: poses, surfel counts, masks and model lists are the same bits; every tracked
frame's id image equals the stand-alone engine's on the same inputs (the models' predictions as the frame met them, the frame's
depth, the hook's flow; no tracker is attached, so every unary is log L); the first frame of a sequence has no result; the two
MMF_ERR_STATE refusals."""
import numpy as np
import pytest
import torch

import crf_oracle as co
from test_gpu_crf_fusion import dev, scene

pytestmark = pytest.mark.gpu
W, H, N, REPLAY = 320, 240, 7, 3


def make(gpu_ctx, K):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, batch_tracking=1,
                          conf_global_init=1.0)
    g.setCrfSegmentation(CrfConfig(**co.config(model_spawn_offset=2)))
    g.setOpticalFlow(True)
    return g


def state(g):
    ms = g.getModels()
    return dict(mask=g.getTexture("MASK").cpu().numpy(), poses=[np.asarray(m.getPose()).tobytes() for m in ms],
                counts=[m.lastCount() for m in ms], ids=[m.id for m in ms])


def sequence(gpu_ctx, K, keep, hook):
    """N frames, a reset, REPLAY frames.  -> the state behind every frame, and with the hook per frame what the inference
    was given (model ids, next id, the models' predictions before the frame) and what it and the flow hook handed out"""
    g = make(gpu_ctx, K)
    if hook:
        g.setFlowInference(True)
    states, seen = [], []
    for k, i in enumerate(list(range(N)) + list(range(REPLAY))):
        if k == N:
            g.reset()
        before = None
        if hook:
            torch.cuda.synchronize()
            ms = g.getModels()
            before = dict(ids=[m.id for m in ms], new_id=g.getNextModelID(), vertex=[m.texture("vertexConf").clone() for m in ms])
        g.processFrame(*keep[i], timestamp=(1000 if k < N else 2000) + 33 * i)
        states.append(state(g))
        if hook:
            before["flow"], before["result"] = g.getLastFlow(), g.getLastFlowInference()
            seen.append(before)
    g.close()
    return states, seen


def test_the_hook_changes_nothing_and_its_ids_are_the_engines(gpu_ctx):
    from multimotionfusion_amd.flowcrf import FlowCrf
    K, frames = scene(W, H, N, 60.0)
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames]
    base, _ = sequence(gpu_ctx, K, keep, False)
    got, seen = sequence(gpu_ctx, K, keep, True)
    assert any(len(s["ids"]) > 1 for s in base[:N]), "the sequence must reach two models"
    for i, (a, b) in enumerate(zip(base, got)):
        assert a["ids"] == b["ids"] and a["counts"] == b["counts"], (i, a["counts"], b["counts"])
        assert a["poses"] == b["poses"], i
        assert np.array_equal(a["mask"], b["mask"]), i
    # no result behind the first frame of a sequence: frame 0, and the first frame after the reset
    assert seen[0]["result"] is None and seen[N]["result"] is None
    e = FlowCrf(gpu_ctx, W, H, (K["fx"], K["fy"], K["cx"], K["cy"]), max_labels=4, max_tracks=0)
    order = list(range(N)) + list(range(REPLAY))
    checked, two = 0, 0
    for k, i in enumerate(order):
        if i == 0:
            continue
        s = seen[k]
        assert s["result"] is not None and s["flow"] is not None, k
        M = len(s["ids"])
        eye = [np.eye(4, dtype=np.float32)] * M  # (without tracks the transformations are not read)
        ids, full = e.infer(s["ids"], eye, eye, s["vertex"], keep[i][1], s["flow"][0], s["flow"][2], tracks=None, allow_new=True,
                            new_id=s["new_id"])
        assert tuple(ids.shape) == (H // 4, W // 4) and tuple(full.shape) == (H, W)
        assert torch.equal(s["result"][0], ids) and torch.equal(s["result"][1], full), (k, i)
        assert set(np.unique(ids.cpu().numpy())) <= set(s["ids"] + [s["new_id"]])
        checked += 1
        two += M > 1
    assert checked == N - 1 + REPLAY - 1 and two >= 1
    e.close()


def test_the_setter_refuses_without_the_flow_and_on_a_shard(gpu_ctx):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.flowcrf import FlowCrfConfig
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K, frames = scene(W, H, 2, 60.0)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"])
    with pytest.raises(MmfError, match="mmf_fusion_last_flow_inference") as err:
        g.getLastFlowInference()
    assert err.value.status == -4  # MMF_ERR_STATE
    with pytest.raises(MmfError, match="optical-flow hook is off") as err:
        g.setFlowInference(True)
    assert err.value.status == -4
    g.setOpticalFlow(True)
    with pytest.raises(MmfError, match="iterations") as err:
        g.setFlowInference(FlowCrfConfig(iterations=51))
    assert err.value.status == -1  # MMF_ERR_INVALID, as mmf_flowcrf_create
    g.setFlowInference(True)
    g.processFrame(dev(frames[0]["rgb"]), dev(frames[0]["depth"]), timestamp=0)
    assert g.getLastFlowInference() is None
    g.processFrame(dev(frames[1]["rgb"]), dev(frames[1]["depth"]), timestamp=33)
    ids, full = g.getLastFlowInference()
    assert (ids == 0).all() and (full == 0).all()  # one model, no new label: its id everywhere
    g.setOpticalFlow(False)  # ... takes the inference with it
    with pytest.raises(MmfError, match="mmf_fusion_last_flow_inference"):
        g.getLastFlowInference()
    g.close()
    # a sharded fusion refuses the optical-flow hook, and the inference hook with it
    s = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    s.setShard(0, 2)
    with pytest.raises(MmfError, match="mmf_fusion_set_flow_inference") as err:
        s.setFlowInference(True)
    assert err.value.status == -4
    s.close()
