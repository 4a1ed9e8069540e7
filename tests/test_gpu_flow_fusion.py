"""-m gpu: the optical-flow hook of processFrame (mmf_fusion_set_optical_flow).  The sequence of
test_gpu_crf_fusion.py (320 x 240, one moving box that the built-in segmentation spawns: two models) once with the hook off
and once with it on: poses, surfel counts, masks and model lists are the same bits; every frame's flow equals the stand-alone
engine on that frame pair bit for bit; frame 1 and the first frame after a reset report no flow; switching the hook off frees
the engine and the frames after it run as before."""
import numpy as np
import pytest

import crf_oracle as co
from helpers import assert_bit_equal
from test_gpu_crf_fusion import dev, scene

pytestmark = pytest.mark.gpu
W, H, N, REPLAY = 320, 240, 7, 4


def make(gpu_ctx, K):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    g = MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, batch_tracking=1,
                          conf_global_init=1.0)
    g.setCrfSegmentation(CrfConfig(**co.config(model_spawn_offset=2)))
    return g


def state(g):
    ms = g.getModels()
    return dict(mask=g.getTexture("MASK").cpu().numpy(), poses=[np.asarray(m.getPose()).tobytes() for m in ms],
                counts=[m.lastCount() for m in ms], ids=[m.id for m in ms])


def sequence(gpu_ctx, K, keep, hook):
    """N frames, a reset, REPLAY frames; with the hook: on from the start, off before the last frame.  -> (the state behind
    every frame, the flow behind every frame or None)"""
    from multimotionfusion_amd import MmfError
    g = make(gpu_ctx, K)
    if hook:
        g.setOpticalFlow(True)
    else:
        with pytest.raises(MmfError, match="mmf_fusion_last_flow"):
            g.getLastFlow()
    states, flows = [], []
    for i in range(N):
        g.processFrame(*keep[i], timestamp=1000 + i)
        states.append(state(g))
        flows.append(g.getLastFlow() if hook else None)
    g.reset()
    for i in range(REPLAY):
        if hook and i == REPLAY - 1:
            g.setOpticalFlow(False)
            with pytest.raises(MmfError, match="mmf_fusion_last_flow"):
                g.getLastFlow()
        g.processFrame(*keep[i], timestamp=2000 + i)
        states.append(state(g))
        flows.append(g.getLastFlow() if hook and i < REPLAY - 1 else None)
    g.close()
    return states, flows


def test_the_hook_changes_nothing_and_its_flow_is_the_engines(gpu_ctx):
    from multimotionfusion_amd.flow import FarnebackFlow
    K, frames = scene(W, H, N, 60.0)
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames]
    base, _ = sequence(gpu_ctx, K, keep, False)
    got, flows = sequence(gpu_ctx, K, keep, True)
    assert any(len(s["ids"]) > 1 for s in base[:N]), "the sequence must reach two models"
    for i, (a, b) in enumerate(zip(base, got)):
        assert a["ids"] == b["ids"] and a["counts"] == b["counts"], (i, a["counts"], b["counts"])
        assert a["poses"] == b["poses"], i
        assert np.array_equal(a["mask"], b["mask"]), i
    # no flow behind the first frame of a sequence: frame 0, and the first frame after the reset; none once the hook is off
    order = list(range(N)) + list(range(REPLAY))
    assert flows[0] is None and flows[N] is None and flows[-1] is None
    e = FarnebackFlow(gpu_ctx, W, H)
    checked = 0
    for k, i in enumerate(order):
        if i == 0 or k == len(order) - 1:
            continue
        assert flows[k] is not None, k
        want = e.compute(keep[i - 1][0], keep[i][0])
        for x, y, name in zip(flows[k], want, ("flow", "magnitude", "motion")):
            assert tuple(x.shape[:2]) == (H // 4, W // 4)
            assert_bit_equal(x.cpu().numpy(), y.cpu().numpy(), f"call {k} (frame {i}): {name}")
        checked += 1
    assert checked == N - 1 + REPLAY - 2
    e.close()


def test_the_setter_refuses_what_the_engine_refuses(gpu_ctx):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.flow import FlowConfig
    K, frames = scene(W, H, 2, 60.0)
    g = make(gpu_ctx, K)
    for over in (dict(levels=2), dict(div=3), dict(winsize=40), dict(poly_n=9), dict(iterations=0), dict(poly_sigma=0.0)):
        with pytest.raises(MmfError, match="mmf_fusion_set_optical_flow"):
            g.setOpticalFlow(FlowConfig(**over))
    # ... and stays off: the frame runs, there is no flow to ask for
    g.processFrame(dev(frames[0]["rgb"]), dev(frames[0]["depth"]), timestamp=0)
    with pytest.raises(MmfError, match="mmf_fusion_last_flow"):
        g.getLastFlow()
    # another configuration than the reference's: div 2, replaced while on (a new sequence)
    g.setOpticalFlow(FlowConfig(div=2, winsize=9))
    g.processFrame(dev(frames[1]["rgb"]), dev(frames[1]["depth"]), timestamp=1)
    assert g.getLastFlow() is None
    g.close()
