"""The geometric verification of the redetection candidates: one segment of 64 keypoints against the store of
tools/redetect_probe.py (4 inactive models x N views x 50-70 keypoints), as the four mmf_viewstore_best_match calls of the
host path (match on the device, one RigidRANSAC per call on the host) and as four mmf_viewstore_best_match_device calls
(match + verification on the device, a fresh RigidRANSAC per view), alternating; wall clock of the calls with their waits.
The views of model 1 show the segment's object (a rigid motion plus 0.5 mm noise and 20 unrelated keypoints), so that both
paths have real estimates to refit; the other models are unrelated.

    python tools/verify_probe.py [both|host|device] [views per model: 200] [repeats: 20]
    rocprofv3 --kernel-trace --stats -- python tools/verify_probe.py device 200     (kernel times, in a run of its own)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimotionfusion_amd import synth
from multimotionfusion_amd.cudafuncs import Context
from multimotionfusion_amd.ransac import RansacBatch
from multimotionfusion_amd.redetection import ViewStore


def unit_rows(rng, n):
    d = rng.normal(size=(n, 256)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


mode = sys.argv[1] if len(sys.argv) > 1 else "both"
n_views = int(sys.argv[2]) if len(sys.argv) > 2 else 200
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = Context(0)
rng = np.random.default_rng(1)
obj_desc, obj_pts = unit_rows(rng, 64), rng.uniform(-0.15, 0.15, (64, 3)) + np.array([0.0, 0.0, 1.5])
vs = ViewStore(ctx)
n_models = 4 if n_views > 1 else 1
for m in range(n_models):
    views = []
    for v in range(n_views):
        n = int(rng.integers(50, 71))
        d, c = unit_rows(rng, n), rng.normal(size=(n, 3)).astype(np.float32)
        if m == 0:  # the object, seen under another pose: 44 of its keypoints, the rest unrelated
            sel = rng.permutation(64)[:44]
            P = synth.make_pose(rng.normal(size=3) * 0.4, rng.normal(size=3) * 0.3)
            d[:44] = obj_desc[sel]
            c[:44] = ((obj_pts[sel] + rng.normal(size=(44, 3)) * 5e-4) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)
        views.append((d, c))
    vs.store(m + 1, views)
batch = RansacBatch(ctx, 10, 0.03, 0.8, max_points=1024)
vs.setVerifier(batch)
q = torch.from_numpy(obj_desc).cuda()
qc_host = obj_pts.astype(np.float32)
qc = torch.from_numpy(qc_host).cuda()
idx, _ = vs.match(q)
per_view = (idx >= 0).sum(1)
print(f"views {idx.shape[0]}, matches per view: model 1 mean {per_view[:n_views].mean():.1f}, others mean {per_view[n_views:].mean() if n_models > 1 else 0:.1f}, "
      f"views with at least 3 matches {(per_view >= 3).sum()}")


def host():
    t = time.perf_counter()
    r = [vs.bestMatch(m + 1, q, qc_host) for m in range(n_models)]
    return (time.perf_counter() - t) * 1e6, r


def device():
    t = time.perf_counter()
    r = [vs.bestMatchDevice(m + 1, q, qc) for m in range(n_models)]
    return (time.perf_counter() - t) * 1e6, r


a, b, ra, rb = [], [], None, None
for i in range(repeats + 5):
    if mode in ("both", "host"):
        t, ra = host()
        a.append(t)
    if mode in ("both", "device"):
        t, rb = device()
        b.append(t)
stats = {}
for name, x, r in (("host path (4 x best_match)", a, ra), ("device path (4 x best_match_device)", b, rb)):
    if x:
        x = np.array(x[5:])
        stats[name] = (x.min(), x.max())
        print(f"{name}: median of {len(x)} {np.median(x):.1f} us, min {x.min():.1f}, max {x.max():.1f}; launches per call {vs.lastLaunches() if r is rb else 3}; "
              f"model 1: found {r[0]['found']} view {r[0]['view']} inliers {r[0]['inliers']} error {r[0]['error']:.6f}; others found {[x_['found'] for x_ in r[1:]]}")
if len(stats) == 2:
    (h0, h1), (d0, d1) = stats.values()
    print("device path faster with disjoint min-max ranges:", bool(d1 < h0), f"(host {h0:.1f} .. {h1:.1f} us, device {d0:.1f} .. {d1:.1f} us)")
vs.close()
batch.close()
ctx.close()
