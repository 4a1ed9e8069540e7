"""The optical-flow engine on the device, measured (LABNOTES.md):

1. mmf_flow_next at 640x480 / div 4 (flow image 160x120, the reference's settings: 1 + 2 * 2 = 5 launches) on a sliding
   synthetic sequence: device-event time on the context's stream (events before and after the call, warm, median and min
   over --reps calls), the stateless pair (mmf_flow_compute) beside it.
2. processFrame of a one-model 640x480 sequence with the hook on against the same frames with it off, alternating: host
   wall clock per call with the stream drained at the end of the loop -- what the hook adds to a frame."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.flow import FarnebackFlow  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def engine_times(ctx, W, H, reps):
    frames = [dev(synth.render(p, W, H, seed=i)["rgb"]) for i, p in enumerate(synth.trajectory(4, seed=21))]
    ptr = ctx.lib.mmf_ctx_stream(ctx.handle)  # (NULL: the context runs on the default stream)
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    e = FarnebackFlow(ctx, W, H)
    has = C.c_int()
    out = {}
    for name in ("next", "compute"):
        def call(i):
            if name == "next":
                ctx.lib.mmf_flow_next(e.handle, C.c_void_p(frames[i % 4].data_ptr()), C.byref(has))
            else:
                ctx.lib.mmf_flow_compute(e.handle, C.c_void_p(frames[i % 4].data_ptr()), C.c_void_p(frames[(i + 1) % 4].data_ptr()))
        for i in range(20):
            call(i)
        times = []
        for i in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(i)
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        out[name] = (float(np.median(times)), float(np.min(times)), e.last_launches())
    e.close()
    return out


def sequence_us(ctx, hook, dframes, K, w, h):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    g = MultiMotionFusion(ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"])
    if hook:
        g.setOpticalFlow(True)
    for i in range(10):  # warm-up
        g.processFrame(*dframes[i], timestamp=i)
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(10, len(dframes)):
        g.processFrame(*dframes[i], timestamp=i)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    g.close()
    return 1e6 * dt / (len(dframes) - 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--engine-only", action="store_true", help="part 1 only (for a kernel trace)")
    a = ap.parse_args()
    ctx = Context(0)
    print(f"device {ctx.device_name()}")
    W, H = 640, 480
    for name, (med, mn, launches) in engine_times(ctx, W, H, a.reps).items():
        print(f"mmf_flow_{name} {W}x{H} div 4 (flow image {W // 4}x{H // 4}, {launches} launches): median {med:.1f} us, min {mn:.1f} us "
              f"(device events, {a.reps} calls)")
    if a.engine_only:
        ctx.close()
        return
    K = synth.intrinsics(W, H)
    dframes = [(dev(f["rgb"]), dev(f["depth"])) for f in (synth.render(p, W, H, seed=i) for i, p in enumerate(synth.trajectory(a.frames, seed=21)))]
    for hook in (False, True) * 3:
        print(f"processFrame {W}x{H}, one model, optical-flow hook {'on' if hook else 'off'}: {sequence_us(ctx, hook, dframes, K, W, H):.1f} us per frame")
    ctx.close()


if __name__ == "__main__":
    main()
