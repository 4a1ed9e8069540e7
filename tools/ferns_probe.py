"""The fern keyframe database on the device, measured (LABNOTES.md):

1. mmf_ferns_process(FIND | ADD) at 640x480 with 500 ferns against databases of 1, 256 and 1 024 keyframes (capacity 1 024):
   device-event time on the context's stream around a window of --reps back-to-back calls, warm, per call (the larger of
   enqueue and execution); median and min over --windows
   windows.  The frame is one the database holds, so the add rule rejects it and the database keeps its size; a window of
   calls that ARE added (threshold -1) beside it.
2. bench.py's headline loop (640x480, one model, the 30-frame sequence played forwards and backwards with the next frame
   handed in) with the hook off and on, alternating, --pairs times in one process: host wall clock per frame with the device
   drained at the end of each run."""
import argparse
import gc
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.ferns import FernDatabase  # noqa: E402
from multimotionfusion_amd.fusion import MultiMotionFusion  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fill_images(W, H, seed):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    vert = rng.normal(size=(H, W, 4)).astype(np.float32)
    vert[..., 2] = rng.uniform(0.4, 6.0, (H, W)).astype(np.float32)
    return dev(image), dev(vert), dev(rng.normal(size=(H, W, 4)).astype(np.float32))


def engine_times(ctx, W, H, reps, windows):
    pose = np.eye(4, dtype=np.float32)
    frame = fill_images(W, H, 1)
    e = FernDatabase(ctx, W, H, threshold=-1.0)
    out = {}
    n = 0

    import ctypes as C
    args = [C.c_void_p(t.data_ptr()) for t in frame] + [pose.ctypes.data_as(C.POINTER(C.c_float))]

    def process(time_):  # (the C ABI directly: the window is meant to hold launches, not the wrapper's checks)
        assert ctx.lib.mmf_ferns_process(e.handle, *args, time_, 3) == 0

    def window(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(k):
            process(5000 + i)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / k

    for target in (1, 256, 1024):
        e.set_threshold(-1.0)  # every frame is kept: fill up to the target
        while n < target:
            process(n)
            n += 1
        assert e.result()["count"] == target, e.result()
        e.set_threshold(0.3095)  # the frame is in the database: rejected, the size stays
        window(reps)
        t = [window(reps) for _ in range(windows)]
        assert e.result()["count"] == n and e.result()["added"] == 0
        out[f"n_{n}"] = dict(median_us=round(float(np.median(t)), 2), min_us=round(min(t), 2))
        if target == 256:  # ... and a window of frames that are added (172 800 bytes copied into the slot each)
            e.set_threshold(-1.0)
            out["adding_from_256"] = round(window(reps), 2)
            n += reps
            assert e.result()["count"] == n
    e.close()
    return out


def hook_cost(ctx, W, H, steps, warmup, pairs):
    K = synth.intrinsics(W, H)
    frames = [synth.render(p, W, H, seed=i) for i, p in enumerate(synth.trajectory(bench.N_FRAMES, seed=1))]
    d_rgb, d_depth = [dev(f["rgb"]) for f in frames], [dev(f["depth"]) for f in frames]

    def run(hook):
        mmf = MultiMotionFusion(ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], icp_weight=bench.ICP_WEIGHT)
        if hook:
            mmf.setFernDatabase(True)
        state = [0]

        def step(i):
            k = bench.pingpong(state[0], len(frames))
            state[0] += 1
            kn = bench.pingpong(state[0], len(frames))
            mmf.processFrame(d_rgb[k], d_depth[k], timestamp=i, next=(d_rgb[kn], d_depth[kn]))
            return mmf.getCurrPose()
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        gc.collect()
        gc.disable()
        t0 = time.perf_counter()
        for i in range(steps):
            step(warmup + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        gc.enable()
        rec = mmf.getLastFernResult() if hook else None
        mmf.close()
        return dt / steps * 1e6, rec

    off, on, rec = [], [], None
    for _ in range(pairs):
        off.append(round(run(False)[0], 1))
        t, rec = run(True)
        on.append(round(t, 1))
    return dict(frame_us_hook_off=off, frame_us_hook_on=on, keyframes=rec["count"], dropped=rec["dropped_total"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3)
    args = ap.parse_args()
    ctx = Context(0)
    print("[ferns probe] process(FIND | ADD), 640x480, 500 ferns, us per call:", engine_times(ctx, 640, 480, args.reps, args.windows), flush=True)
    print("[ferns probe] headline loop, us per frame:", hook_cost(ctx, 640, 480, args.steps, args.warmup, args.pairs), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
