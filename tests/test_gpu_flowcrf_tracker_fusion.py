"""-m gpu: the flow-CRF inference hook of processFrame with an attached tracker (mmf_fusion_set_flow_inference beside
mmf_fusion_set_tracker; DESIGN.md 4.9 "Inside processFrame").  The two-box scene of tests/test_gpu_tracker_fusion.py (320 x 240,
six frames, segmented from its label images: three models), without the keypoint initialisation, with it, and with it and
icp_refine off.

What the hook hands its engine is T_start = prev pose^-1 and T_end = pose pose^-1 per model, prev being the pose the frame
before left the model with (the reference's poses[-2]) -- not Model::lastPose, which the keypoint initialisation overrides with
this frame's initial pose -- and the tracker's table.  E and U depend on exactly these, so the hook's E and U
(mmf_fusion_flow_inference_download) must be, bit for bit, those of the stand-alone engine given the same table and the two
transformations built from the poses read before and after the call with the float arithmetic of the library (the oracle's
inverse4f / matmul4f restate it).  Without the initialisation the predictions the frame was tracked against are the ones read
before the call, so the id images are compared as well; with it they are re-predicted inside the call at the initial pose.
The scene must be able to tell: on some frame the engine given T_start = identity (what lastPose gives once it is overridden)
computes another E."""
import numpy as np
import pytest
import torch

from test_gpu_tracker_fusion import H, N_FRAMES, W, dev, object_scene  # noqa: F401 (object_scene: a fixture)

pytestmark = pytest.mark.gpu
SLOTS = ("xy", "coordinate", "timestamp", "nonnull")  # what the inference reads of the table


@pytest.mark.parametrize("init_kp,icp_refine", [(False, True), (True, True), (True, False)])
def test_the_hook_hands_its_engine_the_previous_pose_and_the_table(gpu_ctx, orc, object_scene, init_kp, icp_refine):
    from multimotionfusion_amd.flowcrf import FlowCrf
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import MaskConfig
    from multimotionfusion_amd.tracker import DevicePointTracker
    K, frames, labels, kps = object_scene
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=2)
    g.setMaskSegmentation(MaskConfig(model_spawn_offset=1))
    g.setOpticalFlow(True)
    g.setFlowInference(True)
    trk = DevicePointTracker(gpu_ctx, W, H, intr, capacity=512, max_keypoints=256)
    g.setTracker(trk, odom_init_kp=init_kp, icp_refine=icp_refine)
    e = FlowCrf(gpu_ctx, W, H, intr, max_labels=4, max_tracks=512)
    keep, checked, told, sampled, most = [], 0, 0, 0, 0
    for i, f in enumerate(frames):
        ts = 1000 + 33_000_000 * i
        xy, de, _ = kps[i]
        keep.append((dev(f["rgb"]), dev(f["depth"]), dev(labels[i])))
        trk.addKeypointsPixels(xy, de, ts, keep[-1][1], 0.7, 30)
        trk.prune(30, max(ts - int(1e9), 0))
        torch.cuda.synchronize()
        ms = g.getModels()
        ids, new_id = [m.id for m in ms], g.getNextModelID()
        prev = [np.array(m.getPose(), np.float32) for m in ms]
        vertex = [m.texture("vertexConf").clone() for m in ms]
        table = trk.download()
        g.processFrame(*keep[-1][:2], timestamp=ts, mask=keep[-1][2])
        got = g.getLastFlowInference()
        if i == 0:
            assert got is None
            continue
        assert got is not None, i
        after = {m.id: np.array(m.getPose(), np.float32) for m in g.getModels()}
        assert all(m in after for m in ids), (i, ids, list(after))
        now = trk.download()  # (the association behind the inference leaves the slots alone: the engine below reads them in place)
        assert all(table[k].tobytes() == now[k].tobytes() for k in SLOTS), i
        Ts, Te = [], []
        for m, p in zip(ids, prev):
            inv = orc.inverse4f(after[m])
            Ts.append(orc.matmul4f(p, inv)), Te.append(orc.matmul4f(after[m], inv))
        flow, _, motion = g.getLastFlow()
        hook = {k: g.downloadFlowInference(k) for k in ("E", "U")}
        assert hook["E"].shape == (len(ids) + 1, H // 4, W // 4)
        eids, efull = e.infer(ids, Ts, Te, vertex, keep[-1][1], flow, motion, tracks=trk, allow_new=True, new_id=new_id)
        E = e.download("E")
        assert hook["E"].tobytes() == E.tobytes(), (i, ids, int((hook["E"] != E).sum()))
        assert hook["U"].tobytes() == e.download("U").tobytes(), i
        if not init_kp:
            assert torch.equal(got[0], eids) and torch.equal(got[1], efull), i
        sampled += int(np.isfinite(E[0]).sum())
        most = max(most, len(ids))
        eye = [np.eye(4, dtype=np.float32)] * len(ids)
        e.infer(ids, eye, Te, vertex, keep[-1][1], flow, motion, tracks=trk, allow_new=True, new_id=new_id)
        told += e.download("E").tobytes() != E.tobytes()
        checked += 1
    assert checked == N_FRAMES - 1 and most == 3
    assert sampled >= 20 * checked, sampled  # (the camera model's row carries the tracks' samples on every frame)
    assert told >= 1, "no frame's E depends on T_start: the scene cannot tell the previous pose from the identity"
    e.close()
    g.setTracker(None)
    trk.close()
    g.close()


def test_replacing_the_flow_engine_keeps_the_hook_on(gpu_ctx, object_scene):
    """a second setOpticalFlow(True) replaces the flow engine (a new sequence) and leaves the inference hook on: no result on
    the next frame, one on the frame after it; setOpticalFlow(False) takes the hook with it"""
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K, frames, _, _ = object_scene
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"])
    g.setOpticalFlow(True)
    g.setFlowInference(True)
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames[:4]]
    seen = []
    for i, (rgb, depth) in enumerate(keep):
        if i == 2:
            g.setOpticalFlow(True)
            assert g.getLastFlowInference() is None  # (on, without a result: not MMF_ERR_STATE)
        g.processFrame(rgb, depth, timestamp=1000 + 33_000_000 * i)
        seen.append(g.getLastFlowInference() is not None)
    assert seen == [False, True, False, True]
    assert g.downloadFlowInference("ids").shape == (H // 4, W // 4)
    g.setOpticalFlow(False)
    with pytest.raises(MmfError, match="hook is off") as err:
        g.downloadFlowInference("E")
    assert err.value.status == -4  # MMF_ERR_STATE
    g.close()
