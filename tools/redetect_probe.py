"""The redetection search: one segment of 64 keypoints against 4 inactive models x N views x 50-70 keypoints (unit
descriptors), as ONE batched match (redetection.ViewStore.match: 3 launches) and as one mmf_match_descriptors call per view
(what the library offered before), alternating; wall clock of the call including the host's wait for the results.

    python tools/redetect_probe.py [both|batched|perview] [views per model: 200]
    rocprofv3 --kernel-trace --stats -- python tools/redetect_probe.py batched 200     (kernel times, launches per query set)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class ro:
    @staticmethod
    def unit_rows(rng, n):
        d = rng.normal(size=(n, 256)).astype(np.float32)
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


from multimotionfusion_amd.cudafuncs import Context
from multimotionfusion_amd.redetection import ViewStore
from multimotionfusion_amd.matcher import matchDescriptors

mode = sys.argv[1] if len(sys.argv) > 1 else "both"
n_views = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ctx = Context(0)
rng = np.random.default_rng(1)
vs = ViewStore(ctx)
train_dev = []
rows = 0
for m in range(4 if n_views > 1 else 1):
    views = []
    for v in range(n_views):
        n = int(rng.integers(50, 71))
        d = ro.unit_rows(rng, n)
        views.append((d, rng.normal(size=(n, 3)).astype(np.float32)))
        train_dev.append(torch.from_numpy(d).cuda())
        rows += n
    vs.store(m + 1, views)
q = torch.from_numpy(ro.unit_rows(rng, 64)).cuda()
torch.cuda.synchronize()
print("views", len(train_dev), "rows", rows, "padded rows", sum((t.shape[0] + 31) // 32 * 32 for t in train_dev))

def batched():
    t = time.perf_counter(); vs.match(q); return (time.perf_counter() - t) * 1e6

def per_view():
    t = time.perf_counter()
    for tr in train_dev:
        matchDescriptors(ctx, q, tr, 0.0)
    ctx.synchronize()
    return (time.perf_counter() - t) * 1e6

a, b = [], []
for i in range(25):
    if mode in ("both", "batched"): a.append(batched())
    if mode in ("both", "perview"): b.append(per_view())
for name, x in (("batched", a), ("per-view", b)):
    if x:
        x = np.array(x[5:])
        print(f"{name}: median {np.median(x):.1f} us, min {x.min():.1f}, max {x.max():.1f}, launches/query set {vs.lastLaunches() if name == 'batched' else 3 * len(train_dev)}")
