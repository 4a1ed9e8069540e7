"""-m gpu: an f16 SuperPoint as the keypoint predictor of processFrame (-init kp).  The in-frame front end
(mmf_fusion_set_keypoint_frontend) reads the object's device features only, so with an f16 object it must give the track
table and the poses of the caller-driven front end bit for bit, as tests/test_gpu_keypoint_device.py shows for f32."""
import numpy as np
import pytest
import torch

import tracker_oracle as to
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu

FW, FH, FMAX = 160, 120, 512


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(gpu_ctx, weights, thresh, K, frames, on_device):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.superpoint import SuperPoint
    from multimotionfusion_amd.tracker import NativeKeypointFrontEnd
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    g = MultiMotionFusion(gpu_ctx, FW, FH, K["cx"], K["cy"], K["fx"], K["fy"])
    sp = SuperPoint(gpu_ctx, weights, max_width=FW, max_height=FH, max_keypoints=FMAX, conf_thresh=thresh, precision="f16")
    assert sp.precision == "f16"
    fe = NativeKeypointFrontEnd(gpu_ctx, g, sp, intr, icp_refine=True, capacity=2048, max_keypoints=FMAX, on_device=on_device)
    out, keep = [], []
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"])))
        fe.processFrame(keep[-1][0], keep[-1][1], timestamp=1000 + 33_000_000 * i)
        out.append(dict(pose=g.getCurrPose().copy(), T=g.getLastTrackTransforms().copy(), ids=[m.id for m in g.getModels()],
                        poses=[m.getPose().copy() for m in g.getModels()]))
    table = fe.tracker.download()
    failures = fe.tracker.keypointFailures()
    fe.close()
    sp.close()
    g.close()
    return out, table, failures


def test_in_frame_front_end_with_an_f16_predictor(gpu_ctx, orc):
    from multimotionfusion_amd.superpoint import SuperPoint
    weights = orc.sp_random_weights(seed=4)
    K = synth.intrinsics(FW, FH)
    frames = [synth.render(p, FW, FH, seed=i) for i, p in enumerate(synth.trajectory(4, seed=5))]
    # a threshold at which the f16 network keeps between 50 and FMAX keypoints on the first frame
    probe = SuperPoint(gpu_ctx, weights, max_width=FW, max_height=FH, max_keypoints=FW * FH, precision="f16")
    heat = probe.forward(frames[0]["rgb"])[2]
    thresh = None
    for q in (0.0, 0.5, 0.8, 0.9, 0.95):
        probe.conf_thresh = max(0.015, float(np.quantile(heat, q)))
        n = len(probe.keypoints(frames[0]["rgb"])[0])
        if 50 <= n <= FMAX:
            thresh = probe.conf_thresh
            break
    probe.close()
    assert thresh is not None
    (fa, ta, _), (fb, tb, failures) = run(gpu_ctx, weights, thresh, K, frames, False), run(gpu_ctx, weights, thresh, K, frames, True)
    assert failures == 0
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert np.array_equal(bits(x["pose"]), bits(y["pose"])), (i, x["pose"], y["pose"])
        assert x["T"].shape == y["T"].shape and np.array_equal(bits(x["T"]), bits(y["T"])), (i, "track transforms")
        assert x["ids"] == y["ids"] and len(x["ids"]) == 1, i
        for p, q in zip(x["poses"], y["poses"]):
            assert np.array_equal(bits(p), bits(q)), (i, "model poses")
    diff = to.same_table(tb, ta)
    assert diff is None, diff
    assert ta["n_tracks"] > 50
    assert any(f["T"].shape[0] == 1 for f in fa[1:])  # -init kp produced a transform from the tracks
