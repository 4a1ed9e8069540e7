"""-m gpu: the flow_crf mode inside processFrame (mmf_fusion_set_flow_segmentation) on the sequence of
tests/flowseg_scene.py at 160 x 120 and 172 x 124 (43 x 31 cells), five frames, with a tracker attached.

Per frame the mask and the entries must equal tests/flowseg_oracle.py applied to that frame's downloaded inference ids and its
depth, bit for bit; the first frame has a zero mask and no segmentation.  The whole run must equal, bit for bit in poses,
maps and model list, a second run without any hook in which the caller hands the same masks and entries in through
mmf_frame::segmentation.  The scene and the inference's weights (0.3 / 0.3: flowseg_scene.predict shows on the CPU that the
reference's 40 / 40 lets the camera's label swallow the patch) make frame 2 spawn a model from the new label's blob; that
is asserted.  Then the switches and the refusals."""
import numpy as np
import pytest
import torch

import flowseg_oracle as fo
import flowseg_scene as scene
from helpers import bits

pytestmark = pytest.mark.gpu
CRF = dict(weight_smoothness=0.3, weight_appearance=0.3)
SIZES = [(160, 120), (172, 124)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def state(g):
    ms = g.getModels()
    return [(m.id, np.array(m.getPose(), np.float32).tobytes(), m.downloadMap().tobytes()) for m in ms]


def play(gpu_ctx, W, H, mode, handed=None, before=None):
    """one run over the scene.  mode "flow": the flow_crf mode; "handed": the masks and entries of `handed` go in with the
    frames; before(g): called on the fresh fusion.  Returns per frame: state, mask, and for mode "flow" what the mode did"""
    from multimotionfusion_amd.flowcrf import FlowCrfConfig
    from multimotionfusion_amd.flowseg import FlowSegConfig
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.tracker import DevicePointTracker
    K, frames, kps = scene.make(W, H)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=2)
    if before:
        before(g)
    if mode == "flow":
        g.setOpticalFlow(True)
        g.setFlowInference(FlowCrfConfig(**CRF))
        g.setFlowSegmentation(FlowSegConfig(model_spawn_offset=1))
    trk = DevicePointTracker(gpu_ctx, W, H, (K["fx"], K["fy"], K["cx"], K["cy"]), capacity=512, max_keypoints=256)
    g.setTracker(trk, odom_init_kp=False, icp_refine=True)
    out, keep = [], []
    for i, f in enumerate(frames):
        ts = 1000 + scene.DT * i
        rgb, depth = dev(f["rgb"]), dev(f["depth"])
        keep.append((rgb, depth))
        trk.addKeypointsPixels(kps[i][0], kps[i][1], ts, depth, 0.7, 30)
        torch.cuda.synchronize()
        rec = dict(ids_before=[m.id for m in g.getModels()], next_id=g.getNextModelID())
        if mode == "handed" and i > 0:
            h = handed[i]
            g.processFrame(rgb, depth, timestamp=ts, mask=h["mask"], hasNewLabel=h["seg"]["has_new_label"], modelData=h["seg"]["model_data"])
        else:
            g.processFrame(rgb, depth, timestamp=ts)
        rec["state"], rec["mask"] = state(g), g.getTexture("MASK").clone()
        if mode == "flow" and i > 0:
            rec["seg"] = g.getLastFlowSegmentation()
            rec["ids"] = g.downloadFlowInference("ids") if rec["seg"]["has_result"] else None
        out.append(rec)
    g.setTracker(None)
    trk.close()
    g.close()
    return out, frames


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def runs(request, gpu_ctx):
    W, H = request.param
    flow, frames = play(gpu_ctx, W, H, "flow")
    return W, H, frames, flow


def test_every_frame_equals_the_oracle_on_its_inference(runs):
    W, H, frames, flow = runs
    assert not flow[0]["mask"].any().item() and "seg" not in flow[0]  # the first frame: a zero mask, nothing segmented
    spawned = 0
    for i in range(1, len(frames)):
        rec, seg = flow[i], flow[i]["seg"]
        assert seg["has_result"], i
        # model_spawn_offset 1: the counter is 1 again on the frame after a spawn (MultiMotionFusion.cpp:148, :410, :484)
        assert seg["allow_new"], i
        want = fo.segment(rec["ids"], frames[i]["depth"], rec["ids_before"], True, rec["next_id"])
        assert np.array_equal(rec["mask"].cpu().numpy(), want["full"]), i
        assert seg["has_new_label"] == want["has_new_label"] and seg["new_cells"] == want["new_cells"], i
        assert seg["area2"] == want["entry_area2"] and seg["first_cell"] == want["entry_first"], i
        assert len(seg["model_data"]) == len(want["models"]) == want["n_entries"], i
        for got, (mid, spc, conf, mean, std) in zip(seg["model_data"], want["models"]):
            assert (got["id"], got["super_pixel_count"]) == (mid, spc), (i, got)
            for key, v in (("avg_confidence", conf), ("depth_mean", mean), ("depth_std", std)):
                assert bits(np.float32(got[key])) == bits(np.float32(v)), (i, mid, key, got[key], v)
        if seg["has_new_label"]:
            spawned += 1
            assert seg["new_cells"] > 0.05 * (W // 4) * (H // 4) and (rec["mask"] == rec["next_id"]).any().item()
            assert rec["state"][-1][0] == rec["next_id"] and rec["next_id"] not in rec["ids_before"], i
    # the scene is not vacuous: the new label's blob spawned a model, and it has surfels
    assert spawned >= 1 and len(flow[-1]["state"]) >= 2, [r["seg"]["new_cells"] for r in flow[1:]]
    assert flow[2]["seg"]["has_new_label"], flow[2]["seg"]
    assert len(flow[2]["state"][-1][2]) > 0


def test_the_run_equals_one_that_is_handed_the_same_segmentation(gpu_ctx, runs):
    W, H, frames, flow = runs
    handed, _ = play(gpu_ctx, W, H, "handed", handed=flow)

    def switched(g):  # everything on and off again before the first frame: as if it had never been on
        from multimotionfusion_amd.flowseg import FlowSegConfig
        g.setOpticalFlow(True)
        g.setFlowInference(True)
        g.setFlowSegmentation(FlowSegConfig(model_spawn_offset=1))
        g.setFlowSegmentation(None)
        g.setOpticalFlow(None)
    again, _ = play(gpu_ctx, W, H, "handed", handed=flow, before=switched)
    for i, (a, b, c) in enumerate(zip(flow, handed, again)):
        assert [s[0] for s in a["state"]] == [s[0] for s in b["state"]], i
        for (mid, pose_a, map_a), (_, pose_b, map_b), (_, pose_c, map_c) in zip(a["state"], b["state"], c["state"]):
            assert pose_a == pose_b and map_a == map_b, (i, mid)
            assert pose_b == pose_c and map_b == map_c, (i, mid)
        assert torch.equal(a["mask"], b["mask"]) and torch.equal(b["mask"], c["mask"]), i


def test_switches_and_refusals(gpu_ctx):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.flowseg import FlowSegConfig
    from multimotionfusion_amd.fusion import MultiMotionFusion
    W, H = SIZES[0]
    K, frames, _ = scene.make(W, H)
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)

    def refused(status, fn):
        with pytest.raises(MmfError) as err:
            fn()
        assert err.value.status == status, err.value

    refused(-4, lambda: g.setFlowSegmentation(True))  # MMF_ERR_STATE: the inference hook is off
    refused(-1, lambda: g.setFlowSegmentation(FlowSegConfig(div=2)))  # MMF_ERR_INVALID comes first
    g.setOpticalFlow(True)
    refused(-4, lambda: g.setFlowSegmentation(True))
    g.setFlowInference(True)
    for bad in (dict(div=2), dict(new_model_size=1.5), dict(model_spawn_offset=-1)):
        refused(-1, lambda: g.setFlowSegmentation(FlowSegConfig(**bad)))
    g.setFlowSegmentation(True)
    refused(-4, g.getLastFlowSegmentation)  # no frame yet
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames[:2]]
    g.processFrame(*keep[0], timestamp=1000)
    refused(-4, g.getLastFlowSegmentation)  # the first frame is not segmented
    g.processFrame(*keep[1], timestamp=1000 + scene.DT)
    assert g.getLastFlowSegmentation()["has_result"]
    g.setFlowInference(None)  # takes the mode with it
    refused(-4, g.getLastFlowSegmentation)
    g.setFlowInference(True)
    g.setFlowSegmentation(True)
    g.setOpticalFlow(None)  # ... and so does the flow hook
    refused(-4, g.getLastFlowSegmentation)
    refused(-4, lambda: g.setFlowSegmentation(True))
    g.close()
