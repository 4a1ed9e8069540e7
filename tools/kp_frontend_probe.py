"""What the keypoint front end costs per frame, caller-driven against in-frame.

640 x 480, the bench's synthetic sequence (30 frames played forwards and backwards), SuperPoint with random weights,
max_keypoints = 1024, `-init kp -icp_refine`.  Per row -- the default threshold 0.015, and the 97th percentile of frame 0's heat
map (random weights put about half of all pixels above 0.015, far denser than a trained network) -- wall time per frame of

    (a) tracker.NativeKeypointFrontEnd as it was: getFeatures (host), addKeypoints, prune, processFrame
    (b) NativeKeypointFrontEnd(on_device=True): everything inside processFrame, nothing awaited before the pairs call

plus the stream time of the features alone (forward pass; forward pass + selection on the device; the host-facing call) and,
per frame of the sequence, candidates (heat >= threshold), kept (after suppression and border) and count (min(kept, 1024)).

    python tools/kp_frontend_probe.py [--frames 200] [--warmup 20] [--precision f32|f16] > profiles/r14_kp_frontend_probe.txt

--precision f16 runs every SuperPoint object of the probe with the f16 forward pass.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.fusion import MultiMotionFusion  # noqa: E402
from multimotionfusion_amd.superpoint import SuperPoint, random_weights  # noqa: E402
from multimotionfusion_amd.tracker import NativeKeypointFrontEnd  # noqa: E402

W, H, N_FRAMES, MAX_KP, ICP_WEIGHT = 640, 480, 30, 1024, 10.0


def pingpong(i, n):
    p = i % (2 * n - 2)
    return p if p < n else 2 * n - 2 - p


def run(ctx, K, d_rgb, d_depth, weights, thresh, on_device, warmup, frames, precision):
    g = MultiMotionFusion(ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], icp_weight=ICP_WEIGHT)
    sp = SuperPoint(ctx, weights, max_width=W, max_height=H, max_keypoints=MAX_KP, conf_thresh=thresh, precision=precision)
    fe = NativeKeypointFrontEnd(ctx, g, sp, (K["fx"], K["fy"], K["cx"], K["cy"]), icp_refine=True, max_keypoints=MAX_KP, on_device=on_device)
    t0 = None
    for i in range(warmup + frames):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        k = pingpong(i, len(d_rgb))
        fe.processFrame(d_rgb[k], d_depth[k], timestamp=1000 + 33_000_000 * i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / frames
    tracks, _, dropped = fe.tracker.status()
    pose = g.getCurrPose().copy()
    failures = fe.tracker.keypointFailures()
    fe.close()
    sp.close()
    g.close()
    return ms, tracks, dropped, pose, failures


def stream_ms(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", choices=("f32", "f16"), default="f32")
    args = ap.parse_args()
    ctx = Context(0)
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(N_FRAMES, seed=1)
    seq = [synth.render(p, W, H, seed=i) for i, p in enumerate(poses)]
    d_rgb = [torch.from_numpy(f["rgb"]).cuda() for f in seq]
    d_depth = [torch.from_numpy(f["depth"]).cuda() for f in seq]
    weights = random_weights(0)
    big = SuperPoint(ctx, weights, max_width=W, max_height=H, max_keypoints=16384, precision=args.precision)
    heat0 = big.forward(d_rgb[0])[2]
    rows = [("default threshold", 0.015), ("97th percentile of frame 0's heat map", float(np.quantile(heat0, 0.97)))]
    print(f"device {ctx.device_name()}  {W}x{H}  SuperPoint precision {args.precision}  max_keypoints {MAX_KP}  {args.frames} timed frames after {args.warmup}")
    for name, thresh in rows:
        print(f"\n== {name}: conf_thresh = {thresh:.6g}")
        big.conf_thresh = thresh
        stats = []
        for k in range(N_FRAMES):
            heat = big.forward(d_rgb[k])[2]
            kept = len(big.keypoints(d_rgb[k])[0])
            stats.append((int((heat >= np.float32(thresh)).sum()), kept, min(kept, MAX_KP)))
        print("frame: candidates kept count")
        for k, s in enumerate(stats):
            print(f"  {k:2d}: {s[0]:6d} {s[1]:5d} {s[2]:4d}")
        sp = SuperPoint(ctx, weights, max_width=W, max_height=H, max_keypoints=MAX_KP, conf_thresh=thresh, precision=args.precision)
        t_fwd = stream_ms(lambda: sp.enqueue(d_rgb[0]))
        t_dev = stream_ms(lambda: sp.getFeaturesDevice(d_rgb[0]))
        t_host = stream_ms(lambda: sp.keypoints(d_rgb[0]))
        print(f"features of frame 0, ms: forward pass {t_fwd:.3f}, forward + selection on the device {t_dev:.3f} "
              f"({sp.lastLaunches()} launches, status {sp.lastFeatures()[3]}), host-facing get_features {t_host:.3f}")
        sp.close()
        res = {}
        for label, on_device in (("(a) caller-driven", False), ("(b) in-frame, on the device", True)):
            ms, tracks, dropped, pose, failures = run(ctx, K, d_rgb, d_depth, weights, thresh, on_device, args.warmup, args.frames, args.precision)
            res[on_device] = (ms, pose)
            print(f"{label}: {ms:.3f} ms per frame  (tracks {tracks}, dropped appends {dropped}, failed adds {failures})")
        same = np.array_equal(res[False][1].view(np.uint32), res[True][1].view(np.uint32))
        print(f"(b) / (a) = {res[True][0] / res[False][0]:.3f}; last pose bit-equal: {same}")
    big.close()
    ctx.close()


if __name__ == "__main__":
    main()
