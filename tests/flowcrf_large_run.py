"""One inference of the flow-CRF engine at a large frame size, as a program of its own (tests/test_gpu_flowcrf.py runs it as a
child process with a time limit): status, ranges and the launch count only.  Usage: flowcrf_large_run.py WIDTH HEIGHT"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flowcrf_oracle as fo  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.flowcrf import FlowCrf  # noqa: E402

F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def main():
    W, H = int(sys.argv[1]), int(sys.argv[2])
    w, h = W // 4, H // 4
    rng = np.random.default_rng(W)
    depth = rng.uniform(1.0, 2.0, (H, W)).astype(F32)
    vert = []
    for _ in range(2):
        v = np.zeros((H, W, 4), F32)
        v[..., 2] = depth + rng.uniform(0, 0.05, (H, W)).astype(F32)
        vert.append(dev(v))
    flow = rng.normal(0, 1.5, (h, w, 2)).astype(F32)
    tracks = {k: dev(v) for k, v in fo.make_scene(16, 12, 2, False, 1)["tracks"].items()}
    ctx = Context(0)
    e = FlowCrf(ctx, W, H, fo.camera(W, H), max_labels=2, max_tracks=256, iterations=1)
    eye = [np.eye(4, dtype=F32)] * 2
    e.infer([0, 4], eye, eye, vert, dev(depth), dev(flow), dev(fo.motion_of(flow)), tracks=tracks)
    Q, prob, ids = e.download("Q"), e.download("prob"), e.download("ids")
    assert np.abs(Q.sum(0) - 1).max() <= 1e-5 and Q.min() >= 0
    assert prob.min() >= 0 and prob.max() <= 1
    assert e.last_launches() == 8
    assert np.array_equal(e.download("ids_full"), fo.upscale4(ids))
    assert set(np.unique(ids)) <= {0, 4}
    e.close()
    ctx.close()
    print(f"flowcrf large run {W}x{H}: ok")


if __name__ == "__main__":
    main()
