"""The SuperPoint forward pass in f16 against f32.

One process, an f32 and an f16 object on the same random weights, `forward` enqueued on them alternately with device
events around each call: median and minimum of --calls calls per precision after a warm-up, at 640x480, 320x240 and
1280x960.  Then, recorded and not a criterion (the weights are random): on 20 frames of the bench's synthetic sequence at
the 97th-percentile threshold of tools/kp_frontend_probe.py's second row, the largest |heat_f16 - heat_f32|, the share of
the f32 path's keypoints the f16 path finds within one pixel, and the largest distance between the descriptors of such
pairs.  Last, what the matrix cores do with f16 subnormal operands: a 1x1 layer whose activations are 2^-20 and whose
weights are 2^10 (every product 2^-10, 32 of them, exact) -- the f32 output is 2^-5 if subnormal operands are honoured and
0 if they are flushed.

    python tools/sp_f16_probe.py > profiles/r20_sp_f16_probe.txt
    python tools/sp_f16_probe.py --trace 30      # 30 forwards per precision and nothing else: the run to put under
                                                 # rocprofv3 --kernel-trace --stats
    python tools/sp_f16_probe.py --summarise x_results.db 30 > profiles/r20_sp_f16_kernel_stats.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.superpoint import SuperPoint, conv_f16, forward_flops, random_weights  # noqa: E402


def timed(objs, img, calls, warmup):
    """per-object lists of event times (ms) of `calls` alternating forward passes"""
    for _ in range(warmup):
        for o in objs:
            o.enqueue(img)
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for _ in objs]
    for k in range(calls):
        for j, o in enumerate(objs):
            ev[j][k][0].record()
            o.enqueue(img)
            ev[j][k][1].record()
    torch.cuda.synchronize()
    return [np.array([a.elapsed_time(b) for a, b in row]) for row in ev]


def summarise(path, forwards):
    """per (kernel, grid) times of a rocprofv3 --kernel-trace database of `--trace forwards`: one line per layer launch"""
    import re
    import sqlite3
    db = sqlite3.connect(path)
    rows = db.execute("select name, grid_x, grid_y, grid_z, count(*), avg(end-start), min(end-start), min(start) from kernels "
                      "where name like '%sp_%' group by name, grid_x, grid_y, grid_z order by 8").fetchall()
    for prec, pick in (("f32", lambda n: "f16" not in n), ("f16", lambda n: "f16" in n)):
        mine = [r for r in rows if pick(r[0]) and ("conv" in r[0])]
        print(f"== {prec} convolutions, {forwards} forwards at 640x480: launches per forward, avg us, min us")
        total = 0.0
        for name, gx, gy, gz, n, avg, mn, _ in mine:
            short = re.sub(r"\(.*", "", name).replace("void mmf::", "").replace("mmf::", "")
            total += n * avg / forwards / 1e3
            print(f"{short:52s} grid {gx // 256:5d} x {gy:3d} x {gz:2d}  n/fwd {n / forwards:4.1f}  "
                  f"avg {avg / 1e3:7.2f}  min {mn / 1e3:7.2f}")
        print(f"sum of the averages per forward: {total:.1f} us")
    tail = [r for r in rows if "conv" not in r[0]]
    for name, gx, gy, gz, n, avg, mn, _ in tail:
        short = re.sub(r"\(.*", "", name).replace("void mmf::", "").replace("mmf::", "")
        print(f"(both) {short:45s} n {n:4d}  avg {avg / 1e3:7.2f}  min {mn / 1e3:7.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", nargs=2, metavar=("DB", "FORWARDS"), help="summarise the kernel trace of a --trace run")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0, help="only this many forwards per precision at 640x480 (for a kernel trace)")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise[0], int(args.summarise[1]))
        return
    ctx = Context(0)
    weights = random_weights(0)
    rng = np.random.default_rng(0)
    if args.trace:
        img = torch.from_numpy(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)).cuda()
        for prec in ("f32", "f16"):
            sp = SuperPoint(ctx, weights, max_width=640, max_height=480, precision=prec)
            for _ in range(args.trace):
                sp.enqueue(img)
            torch.cuda.synchronize()
            sp.close()
        ctx.close()
        return
    import bench
    print(f"device {ctx.device_name()}  source_stamp {bench.source_stamp()}")
    print(f"forward pass, device events around each call, {args.calls} alternating calls per precision after {args.warmup}")
    for W, H in ((640, 480), (320, 240), (1280, 960)):
        img = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        objs = [SuperPoint(ctx, weights, max_width=W, max_height=H, precision=p) for p in ("f32", "f16")]
        t32, t16 = timed(objs, img, args.calls, args.warmup)
        gf = forward_flops(W, H) / 1e9
        print(f"{W}x{H}: f32 median {np.median(t32):.4f} ms min {t32.min():.4f} ms ({gf / np.median(t32):.1f} TFLOP/s) | "
              f"f16 median {np.median(t16):.4f} ms min {t16.min():.4f} ms ({gf / np.median(t16):.1f} TFLOP/s) | "
              f"f16 / f32 medians = {np.median(t16) / np.median(t32):.3f}")
        for o in objs:
            o.close()

    # recorded, not a criterion
    W, H, n = 640, 480, 20
    seq = [synth.render(p, W, H, seed=i) for i, p in enumerate(synth.trajectory(n, seed=1))]
    a = SuperPoint(ctx, weights, max_width=W, max_height=H, max_keypoints=16384)
    b = SuperPoint(ctx, weights, max_width=W, max_height=H, max_keypoints=16384, precision="f16")
    thresh = float(np.quantile(a.forward(seq[0]["rgb"])[2], 0.97))
    a.conf_thresh = b.conf_thresh = thresh
    dheat, found, total, ddesc = 0.0, 0, 0, 0.0
    for f in seq:
        dheat = max(dheat, float(np.abs(a.forward(f["rgb"])[2] - b.forward(f["rgb"])[2]).max()))
        xa, _, da = a.keypoints(f["rgb"])
        xb, _, db = b.keypoints(f["rgb"])
        grid = -np.ones((H + 2, W + 2), np.int64)
        grid[xb[:, 1] + 1, xb[:, 0] + 1] = np.arange(len(xb))
        for k, (x, y) in enumerate(xa):
            near = grid[y:y + 3, x:x + 3].ravel()
            near = near[near >= 0]
            total += 1
            if len(near):
                found += 1
                ddesc = max(ddesc, float(min(np.linalg.norm(da[k] - db[j]) for j in near)))
    print(f"\n{n} frames of the synthetic sequence at {W}x{H}, conf_thresh {thresh:.6g} (random weights; recorded, not a criterion):")
    print(f"largest |heat_f16 - heat_f32| {dheat:.3e}; f32 keypoints found by f16 within one pixel {found} of {total} "
          f"({100.0 * found / max(total, 1):.2f} %); largest descriptor distance of such pairs {ddesc:.3e}")
    a.close(), b.close()

    # f16 subnormal operands on the matrix cores (observed, not pinned)
    x = torch.full((8, 16, 32), 2.0 ** -20, dtype=torch.float16, device="cuda")
    w = np.full((32, 32, 1, 1), 2.0 ** 10, np.float32)
    y = conv_f16(ctx, x, w, np.zeros(32, np.float32), relu=False, out_f32=True).cpu().numpy()
    print(f"\nsubnormal f16 operands: 32 products 2^-20 * 2^10 give {np.unique(y)} (2^-5 = {2.0 ** -5}: honoured; 0: flushed)")
    ctx.close()


if __name__ == "__main__":
    main()
