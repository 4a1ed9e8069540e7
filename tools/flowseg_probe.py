"""The blob stage of the flow_crf segmentation on the device, measured (LABNOTES):

1. mmf_flowseg_run at 640x480 (160 x 120 cells) with 2 and 4 labels on a blobby id image, and on the two extremes (one id
   everywhere; a one-cell-wide serpentine): device-event time of the whole run on the context's stream, median over --reps
   calls after a warm-up.  Beside it mmf_flowcrf_infer with the same numbers of labels (tools/flowcrf_probe.py's set-up).
2. processFrame at 640x480 on one rendered frame shown again and again (a static camera: one model, with the new label two
   labels): wall-clock time per call, stream drained, median over --reps calls after a warm-up -- with no hook and a zero
   mask handed in, with the flow and inference hooks and the same mask, and with the flow_crf mode segmenting the frame."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from flowcrf_probe import dev, flowcrf_times, timed  # noqa: E402
from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.flowseg import FlowSegConfig, FlowSegmentation  # noqa: E402
from multimotionfusion_amd.fusion import MultiMotionFusion  # noqa: E402

W, H = 640, 480


def id_images(L):
    w, h = W // 4, H // 4
    rng = np.random.default_rng(L)
    table = list(range(L))
    blobs = np.repeat(np.repeat(rng.integers(0, L, (h // 8, w // 8)), 8, axis=0), 8, axis=1)
    noise = rng.random((h, w)) < 0.03
    blobs = np.where(noise, rng.integers(0, L, (h, w)), blobs).astype(np.uint8)
    snake = np.zeros((h, w), np.uint8)
    snake[0::2, :] = 1
    snake[1::4, w - 1] = 1
    snake[3::4, 0] = 1
    return table, dict(blobs=blobs, uniform=np.zeros((h, w), np.uint8), serpentine=snake)


def stage_times(ctx, stream, reps):
    depth = dev((1.0 + np.random.default_rng(0).random((H, W), dtype=np.float32)).astype(np.float32))
    e = FlowSegmentation(ctx, W, H)
    for L in (2, 4):
        table, images = id_images(L)
        for name, ids in images.items():
            a = dev(ids)
            med, mn = timed(stream, lambda: e.run_async(a, depth, table[:-1], True, table[-1]), reps)
            print(f"mmf_flowseg_run 640x480 (19200 cells) L={L} {name}: median {med:.1f} us, min {mn:.1f} us (device events, {reps} calls, "
                  f"{e.last_launches()} launches)")
    e.close()


def frame_times(ctx, reps, warm=20):
    K = synth.intrinsics(W, H)
    f = synth.render(synth.trajectory(1, seed=1)[0], W, H, seed=0)
    rgb, depth = dev(f["rgb"]), dev(f["depth"])
    zero = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    entry = [dict(id=0, super_pixel_count=1, avg_confidence=0.4, depth_mean=2.0, depth_std=0.5)]
    for name in ("no hook, mask handed in", "flow + inference hooks, mask handed in", "flow_crf mode"):
        g = MultiMotionFusion(ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
        if name != "no hook, mask handed in":
            g.setOpticalFlow(True)
            g.setFlowInference(True)
        if name == "flow_crf mode":
            g.setFlowSegmentation(FlowSegConfig(model_spawn_offset=1))
        times = []
        for i in range(warm + reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            if name == "flow_crf mode":
                g.processFrame(rgb, depth, timestamp=1000 + 33_000_000 * i)
            else:
                g.processFrame(rgb, depth, timestamp=1000 + 33_000_000 * i, mask=zero, modelData=entry)
            ctx.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        t = np.array(times[warm:])
        extra = ""
        if name == "flow_crf mode":
            s = g.getLastFlowSegmentation()
            extra = f"; last frame: has_result {s['has_result']}, allow_new {s['allow_new']}, entries {s['n_entries']}"
        print(f"processFrame 640x480, {name}: median {np.median(t):.3f} ms, min {t.min():.3f} ms ({reps} calls{extra})")
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    ctx = Context(0)
    print(f"device {ctx.device_name()}")
    ptr = ctx.lib.mmf_ctx_stream(ctx.handle)  # (NULL: the context runs on the default stream)
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    stage_times(ctx, stream, a.reps)
    for L in (2, 4):
        med, mn = flowcrf_times(ctx, stream, W, H, L, 10, a.reps)
        print(f"mmf_flowcrf_infer 640x480 (19200 cells) L={L} iterations=10: median {med:.1f} us, min {mn:.1f} us (device events, {a.reps} calls)")
    frame_times(ctx, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
