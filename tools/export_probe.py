"""GPU box: mmf_model_export_cloud on the headline loop's steady map (640x480, the bench's sequence played forwards and backwards)
and on a mature store (that map + three occluded copies, all stable), against what the library offered before for the same
records: mmf_model_download_map followed by the numpy filter and packing.  HIP events around each call after a warm-up, median
of 15; both calls wait for their result, so the events span the kernels and the copy to the host.

    python tools/export_probe.py [WxH] [frames]
"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.fusion import MultiMotionFusion  # noqa: E402
from multimotionfusion_amd.model import Model  # noqa: E402
from multimotionfusion_amd.modeldb import CLOUD_DTYPE  # noqa: E402

W, H = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "640x480").split("x"))
N = int(sys.argv[2]) if len(sys.argv) > 2 else 90
CONF, HBM_PEAK = 10.0, 8.0e12  # MI355X: 8 TB/s
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def numpy_export(s, pose, thr):
    """the same records from a downloaded map: filter, transform, pack (float32, the order of csrc/export_kernels.hpp)"""
    s = s[s[:, 3] > np.float32(thr)]
    P = np.asarray(pose, np.float32).reshape(4, 4)
    out = np.zeros(len(s), CLOUD_DTYPE)
    for r, (a, b) in enumerate((("x", "nx"), ("y", "ny"), ("z", "nz"))):
        out[a] = ((P[r, 0] * s[:, 0] + P[r, 1] * s[:, 1]) + P[r, 2] * s[:, 2]) + P[r, 3]
        out[b] = -((P[r, 0] * s[:, 8] + P[r, 1] * s[:, 9]) + P[r, 2] * s[:, 10])
    c = s[:, 4].astype(np.int32)
    out["red"], out["green"], out["blue"], out["radius"] = (c >> 16) & 255, (c >> 8) & 255, c & 255, s[:, 11]
    return out


def timed(fn, reps=18, skip=3):
    ev, wall, res = [], [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ev.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ev[skip:])), float(np.median(wall[skip:])), res


K = synth.intrinsics(W, H)
poses = synth.trajectory(30, seed=1)
frames = [synth.render(p, W, H, seed=i) for i, p in enumerate(poses)]
ctx = Context(0)
g = MultiMotionFusion(ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"])
for i in range(N):  # 0 .. 29, 28 .. 1, 0 .. as bench.py plays it
    k = i % 58
    k = k if k < 30 else 58 - k
    g.processFrame(up(frames[k]["rgb"]), up(frames[k]["depth"]), timestamp=i)
steady = g.getModels()[0].downloadMap()
pose = np.asarray(g.getCurrPose(), np.float32)
g.close()
layers = []
for step in (0.0, 0.02, 0.04, 0.06):
    cp = steady.copy()
    cp[:, :3] += step * cp[:, :3] / np.maximum(np.linalg.norm(cp[:, :3], axis=1, keepdims=True), 1e-6)
    cp[:, 3] = np.maximum(cp[:, 3], 20.0)
    layers.append(cp)
mature = np.concatenate(layers)[: 1024 * 1024 - 310000]
m = Model(ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], 0, CONF)
for name, surfels in (("steady", steady), ("mature", mature)):
    m.uploadMap(surfels)
    ev_new, wall_new, got = timed(lambda: m.exportCloud(pose, CONF))

    def old():
        return numpy_export(m.downloadMap(), pose, CONF)
    ev_old, wall_old, want = timed(old, reps=8, skip=2)
    ev_dl, wall_dl, _ = timed(m.downloadMap, reps=8, skip=2)
    count, kept = len(surfels), len(got)
    same = got.tobytes() == want.tobytes()
    read, written = 16 * count + 32 * kept, 31 * kept
    print(f"{name}: {count} surfels, {kept} stable; export_cloud {ev_new:.0f} us by events ({wall_new:.0f} us wall, {m.exportLastLaunches()} launches); "
          f"download_map alone {ev_dl:.0f} us by events ({wall_dl:.0f} us wall), with the numpy filter and packing {wall_old:.0f} us wall; "
          f"records equal: {same}")
    print(f"{name}: device traffic {read / 1e6:.2f} MB read + {written / 1e6:.2f} MB written = {(read + written) / 1e6:.2f} MB: "
          f"{(read + written) / HBM_PEAK * 1e6:.1f} us at the HBM peak, {100 * (read + written) / HBM_PEAK / (ev_new * 1e-6):.2f} % of it over the "
          f"whole call (the call ends with {written / 1e6:.2f} MB copied to pageable host memory)")
m.close()
ctx.close()
