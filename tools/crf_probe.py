"""The built-in dense-CRF segmentation on the device, measured (profiles/r06_crf_probe.txt):

1. mmf_crf_segment (stages 1-14 of DESIGN.md section 4.4, stage 1 of the depth only: the models' maps come in) at
   640x480 and 1280x960 (S = 16: 1 200 / 4 800 super-pixels) with 2, 4 and 8 labels, 10 mean-field iterations:
   device-event time on the context's stream (events before and after the call, which ends in one pinned read).
2. processFrame of a two-model sequence (camera + one box, spawned from a ground-truth id image) with the rest of the
   frames segmented by the built-in CRF against the same frames with ground-truth masks: frames/s over the same frames.

Kernel statistics come from a separate `rocprofv3 --kernel-trace --stats -- python tools/crf_probe.py --segment-only`."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimotionfusion_amd import segmentation, synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def segment_times(ctx, W, H, L, reps):
    S, M = 16, L - 1
    N = (W // S) * (H // S)
    rng = np.random.default_rng(L)
    maps = np.empty((M, 2, N), np.float32)
    maps[:, 0] = rng.random((M, N), dtype=np.float32) * 0.05
    maps[:, 1] = 1.0 + rng.random((M, N), dtype=np.float32)
    depth = (1.0 + 2.0 * rng.random((H, W), dtype=np.float32)).astype(np.float32)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    a_rgb, a_depth, a_maps = dev(rgb), dev(depth), dev(maps)
    ptr = ctx.lib.mmf_ctx_stream(ctx.handle)  # (NULL: the context runs on the default stream)
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    for _ in range(5):
        segmentation.segment(ctx, a_rgb, a_depth, a_maps, list(range(M)), M, True)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        segmentation.segment(ctx, a_rgb, a_depth, a_maps, list(range(M)), M, True)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return np.median(times), np.min(times)


def sequence_fps(ctx, use_crf, n_frames, w=640, h=480):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = synth.intrinsics(w, h)
    poses = synth.trajectory(n_frames, seed=21)
    objs = synth.make_objects(1, seed=21)
    traj = synth.object_trajectories(objs, n_frames, seed=21)
    frames = [synth.render(p, w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    dframes = [(dev(f["rgb"]), dev(f["depth"]), dev(np.where(f["ids"] == 1, 1, 0).astype(np.uint8))) for f in frames]
    g = MultiMotionFusion(ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    if use_crf:
        g.setCrfSegmentation(segmentation.CrfConfig())
    zero = dev(np.zeros((h, w), np.uint8))
    g.processFrame(*dframes[0][:2], timestamp=0, mask=zero)
    g.processFrame(*dframes[1][:2], timestamp=1, mask=dframes[1][2], hasNewLabel=True)  # the box's model
    for i in range(2, 6):  # warm-up
        g.processFrame(*dframes[i][:2], timestamp=i, mask=None if use_crf else dframes[i][2])
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(6, n_frames):
        g.processFrame(*dframes[i][:2], timestamp=i, mask=None if use_crf else dframes[i][2])
    ctx.synchronize()
    dt = time.perf_counter() - t0
    n_models = len(g.getModels())
    g.close()
    return (n_frames - 6) / dt, n_models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--segment-only", action="store_true")
    a = ap.parse_args()
    ctx = Context(0)
    print(f"device {ctx.device_name()}")
    for W, H in ((640, 480), (1280, 960)):
        for L in (2, 4, 8):
            med, mn = segment_times(ctx, W, H, L, a.reps)
            print(f"mmf_crf_segment {W}x{H} S16 ({(W // 16) * (H // 16)} cells) L={L}: median {med:.1f} us, min {mn:.1f} us "
                  f"(device events, {a.reps} calls)")
    if not a.segment_only:
        for use_crf in (False, True, False, True):
            fps, n = sequence_fps(ctx, use_crf, a.frames)
            print(f"processFrame 640x480, camera + 1 box, {'built-in CRF' if use_crf else 'ground-truth masks'}: "
                  f"{fps:.0f} frames/s ({n} models at the end)")
    ctx.close()


if __name__ == "__main__":
    main()
