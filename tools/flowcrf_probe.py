"""The flow-CRF inference engine on the device, measured (profiles/r17_flowcrf_probe.txt):

1. mmf_flowcrf_infer at 640x480 (160 x 120 = 19 200 cells) with 2, 3 and 5 labels, 10 mean-field iterations: device-event
   time of the whole inference on the context's stream, after a warm-up.
2. mmf_crf_segment at its largest size (2048x2048, S = 16: 16 384 cells) with the same numbers of labels, the same way, in
   the same session: the yardstick of the pair kernels.

The pair launches alone come from a separate `rocprofv3 --kernel-trace --stats -- python tools/flowcrf_probe.py` summarised by
tools/kstats.py with the patterns fcrf_pair and crf_pair: fcrf_pair_kernel<LP, .> evaluates N^2 = 3.686e8 pairs per launch
(one kernel value each), crf_pair_kernel<LP> 16 384^2 = 2.684e8 pairs (two kernel values each)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimotionfusion_amd import segmentation  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.flowcrf import FlowCrf  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def timed(stream, call, reps, warm=5):
    for _ in range(warm):
        call()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return np.median(times), np.min(times)


def flowcrf_times(ctx, stream, W, H, L, iterations, reps):
    w, h, M = W // 4, H // 4, L - 1
    rng = np.random.default_rng(L)
    depth = (1.0 + rng.random((H, W), dtype=np.float32)).astype(np.float32)
    vert = []
    for m in range(M):
        v = np.zeros((H, W, 4), np.float32)
        v[..., 2] = depth + 0.04 * rng.random((H, W), dtype=np.float32)
        vert.append(dev(v))
    flow = rng.normal(0, 1.0, (h, w, 2)).astype(np.float32)
    mag = np.sqrt((flow ** 2).sum(-1))
    motion = np.clip((mag - 0.2) / 4.8, 0, 1).astype(np.float32)
    n = 1000
    px = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    co = np.stack([(px[:, 0] - W / 2) / W * 1.5, (px[:, 1] - H / 2) / W * 1.5, np.full(n, 1.5)], 1).astype(np.float32)
    tr = dict(xy_cur=dev(px.astype(np.int32)), xy_prev=dev(px.astype(np.int32)), co_cur=dev(co), co_prev=dev(co + np.float32(0.002)),
              ts_cur=dev(np.full(n, 1_033_000_000, np.int64)), ts_prev=dev(np.full(n, 1_000_000_000, np.int64)),
              ok_cur=dev(np.ones(n, np.int32)), ok_prev=dev(np.ones(n, np.int32)))
    e = FlowCrf(ctx, W, H, (W, W, W / 2, H / 2), max_labels=L, max_tracks=n, iterations=iterations)
    eye = [np.eye(4, dtype=np.float32)] * M
    a_depth, a_flow, a_motion = dev(depth), dev(flow), dev(motion)

    def call():
        e.infer_async(list(range(M)), eye, eye, vert, a_depth, a_flow, a_motion, tracks=tr, allow_new=True, new_id=M)
    out = timed(stream, call, reps)
    e.close()
    return out


def crf_times(ctx, stream, W, H, L, reps):
    S, M = 16, L - 1
    N = (W // S) * (H // S)
    rng = np.random.default_rng(L)
    maps = np.empty((M, 2, N), np.float32)
    maps[:, 0] = rng.random((M, N), dtype=np.float32) * 0.05
    maps[:, 1] = 1.0 + rng.random((M, N), dtype=np.float32)
    a_rgb = dev(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
    a_depth, a_maps = dev((1.0 + 2.0 * rng.random((H, W), dtype=np.float32)).astype(np.float32)), dev(maps)
    return timed(stream, lambda: segmentation.segment(ctx, a_rgb, a_depth, a_maps, list(range(M)), M, True), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--iterations", type=int, default=10)
    a = ap.parse_args()
    ctx = Context(0)
    print(f"device {ctx.device_name()}")
    ptr = ctx.lib.mmf_ctx_stream(ctx.handle)  # (NULL: the context runs on the default stream)
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    for L in (2, 3, 5):
        med, mn = flowcrf_times(ctx, stream, 640, 480, L, a.iterations, a.reps)
        print(f"mmf_flowcrf_infer 640x480 (19200 cells) L={L} iterations={a.iterations}: median {med:.1f} us, min {mn:.1f} us "
              f"(device events, {a.reps} calls)")
    for L in (2, 3, 5):
        med, mn = crf_times(ctx, stream, 2048, 2048, L, a.reps)
        print(f"mmf_crf_segment 2048x2048 S16 (16384 cells) L={L}: median {med:.1f} us, min {mn:.1f} us (device events, {a.reps} calls)")
    ctx.close()


if __name__ == "__main__":
    main()
