"""The super-pixel engine on the device, measured (profiles/r07_slic_probe.txt):

1. mmf_slic_segment (initialise, 5 x (associate, update), associate = 12 launches) at 640x480 / S 16 and
   1280x960 / S 16 and 32 on a synthetic frame: device-event time on the context's stream (events before and after the
   call, warm, min and median over --reps calls), and the same with 0 iterations (2 launches) for the cost of one
   association.
2. processFrame of the two-model sequence of tools/crf_probe.py (camera + one box, the frames after the spawn segmented by
   the built-in CRF) with the engine on against the same frames with it off (the regular grid), alternating: frames/s.
   A third arm hands the same label images in (computed before the clock starts): what the segmentation itself costs
   more on real super-pixels than on the grid.  The engine runs on a stream of its own beside the tracking chains; what
   remains between the second and the third arm did not overlap.

Kernel statistics come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/slic_probe.py --segment-only --size 640x480x16`."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimotionfusion_amd import segmentation, slic, synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def segment_times(ctx, W, H, S, iterations, reps):
    rgb = dev(synth.render(synth.trajectory(2, seed=21)[1], W, H, seed=3)["rgb"])
    ptr = ctx.lib.mmf_ctx_stream(ctx.handle)  # (NULL: the context runs on the default stream)
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    for _ in range(10):
        slic.segment(ctx, rgb, S, iterations)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        slic.segment(ctx, rgb, S, iterations)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return np.median(times), np.min(times)


_SCENES = {}


def scene(n_frames, w, h):
    if (n_frames, w, h) not in _SCENES:
        poses = synth.trajectory(n_frames, seed=21)
        objs = synth.make_objects(1, seed=21)
        traj = synth.object_trajectories(objs, n_frames, seed=21)
        frames = [synth.render(p, w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
        _SCENES[(n_frames, w, h)] = [(dev(f["rgb"]), dev(f["depth"]), dev(np.where(f["ids"] == 1, 1, 0).astype(np.uint8))) for f in frames]
    return _SCENES[(n_frames, w, h)]


def sequence_fps(ctx, mode, n_frames, w=640, h=480):
    """mode: "grid" (engine off), "engine", or "given": the engine's labels of every frame computed beforehand and handed in
    through setSuperpixels (one device copy per frame) -- the segmentation's cost on real super-pixels without the engine"""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = synth.intrinsics(w, h)
    dframes = scene(n_frames, w, h)
    cfg = segmentation.CrfConfig()
    g = MultiMotionFusion(ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setCrfSegmentation(cfg)
    g.setSuperpixelEngine(mode == "engine")
    given = [slic.segment(ctx, f[0], cfg.spixel_size) for f in dframes] if mode == "given" else None
    zero = dev(np.zeros((h, w), np.uint8))

    def step(i):
        if given is not None:
            g.setSuperpixels(given[i])
        g.processFrame(*dframes[i][:2], timestamp=i)
    g.processFrame(*dframes[0][:2], timestamp=0, mask=zero)
    g.processFrame(*dframes[1][:2], timestamp=1, mask=dframes[1][2], hasNewLabel=True)  # the box's model
    for i in range(2, 6):  # warm-up
        step(i)
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(6, n_frames):
        step(i)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    n_models = len(g.getModels())
    g.close()
    return (n_frames - 6) / dt, n_models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--segment-only", action="store_true")
    ap.add_argument("--size", default=None, help="WxHxS: only this shape, 5 iterations (for a kernel trace)")
    a = ap.parse_args()
    ctx = Context(0)
    print(f"device {ctx.device_name()}")
    shapes = ((640, 480, 16), (1280, 960, 16), (1280, 960, 32)) if a.size is None else (tuple(int(v) for v in a.size.split("x")),)
    for W, H, S in shapes:
        for it in ((5, 0) if a.size is None else (5,)):
            med, mn = segment_times(ctx, W, H, S, it, a.reps)
            print(f"mmf_slic_segment {W}x{H} S{S} ({(W // S) * (H // S)} centres) iterations={it} ({2 + 2 * it} launches): "
                  f"median {med:.1f} us, min {mn:.1f} us (device events, {a.reps} calls)")
    if not a.segment_only:
        names = {"grid": "the grid", "engine": "the engine", "given": "the engine, computed beforehand and handed in"}
        for mode in ("grid", "engine", "given") * 3:
            fps, n = sequence_fps(ctx, mode, a.frames)
            print(f"processFrame 640x480, camera + 1 box, built-in CRF, super-pixels from {names[mode]}: "
                  f"{fps:.0f} frames/s ({1e6 / fps:.0f} us per frame, {n} models at the end)")
    ctx.close()


if __name__ == "__main__":
    main()
