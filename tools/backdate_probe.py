"""What back-dating a spawned model's poses costs (mmf_tracker_backdate; LABNOTES.md).  One process,
640 x 480, a full table of 4 096 tracks that are all seen in every frame, of which 64 or 1 024 carry the new model's label,
a view log of 64 frames.  The whole call -- three launches, the wait for the counts, the batch object's launch, the wait for
the estimates, the chain of products -- between device events and on the wall clock (time.perf_counter, the stream idle
before it), medians of 25 calls after 10 warm-up calls, for history 2, 16 and 64.  Beside it the same pose list built on
the host from point_tracker histories (lists of Keypoint per track): the pairs gathered in Python, one fresh RigidRANSAC per
pair, the same 4 x 4 products.

    python tools/backdate_probe.py
"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

W, H, CAP, LOG, WARM, CALLS = 640, 480, 4096, 64, 10, 25


def unit_rows(rng, n):
    x = rng.standard_normal((n, 256)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def median_us(samples):
    return statistics.median(samples) * 1e6


def host_backdate(tracks, history):
    """Model::refineTrackSubset over full histories on the host, a fresh engine per pair"""
    from multimotionfusion_amd.ransac import RigidRANSAC
    n = min(len(tracks[0]), history)
    rel = [np.eye(4, dtype=np.float32)]
    ik = 0
    for jk in range(1, n):
        p0, p1 = [], []
        for t in tracks:
            a, b = t[len(t) - n + ik], t[len(t) - n + jk]
            if a is not None and b is not None and np.all(np.isfinite(a.coordinate)) and np.all(np.isfinite(b.coordinate)):
                p0.append(a.coordinate), p1.append(b.coordinate)
        if len(p0) < 3:
            rel.append(rel[ik])
            continue
        T = RigidRANSAC(10, 0.03, 0.6).estimate(np.array(p0, np.float32), np.array(p1, np.float32))[0]
        rel.append(rel[ik] @ T)
        ik = jk
    E = np.linalg.inv(rel[-1])
    return [E @ r for r in rel]


def main():
    from multimotionfusion_amd.cudafuncs import Context
    from multimotionfusion_amd.point_tracker import Keypoint
    from multimotionfusion_amd.ransac import RansacBatch
    from multimotionfusion_amd.tracker import DevicePointTracker
    ctx = Context(0)
    rng = np.random.default_rng(0)
    K = (528.0, 528.0, 320.0, 240.0)
    desc = torch.from_numpy(unit_rows(rng, CAP)).cuda()
    flat = rng.choice(W * H, CAP, replace=False)
    xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
    xy_dev = torch.from_numpy(xy).cuda()
    batch = RansacBatch(ctx, 10, 0.03, 0.6, max_points=1024)
    trk = DevicePointTracker(ctx, W, H, K, capacity=CAP, max_keypoints=CAP)
    trk.setViewLog(LOG)
    trk.reserveBackdate(LOG)
    tracks = [[] for _ in range(CAP)]
    for step in range(LOG):  # a plane that comes closer by 2 mm a frame: every track has a finite keypoint in every frame
        depth = torch.full((H, W), 2.0 - 0.002 * step, device="cuda")
        trk.addKeypointsPixels(xy_dev, desc, 1000 + step, depth, 0.7, 30)
        _, co, _, _ = trk.visible()
        for j in range(CAP):
            tracks[j].append(Keypoint(1000 + step, tuple(xy[j]), co[j].astype(np.float64), None))
    assert trk.status()[:2] == (CAP, LOG)
    for segment in (64, 1024):
        mask = np.zeros((H, W), np.uint8)
        mask[xy[:segment, 1], xy[:segment, 0]] = 1
        trk.associate(torch.from_numpy(mask).cuda(), [0, 1])
        for history in (2, 16, 64):
            host, device, mirror = [], [], []
            for rep in range(WARM + CALLS):
                ctx.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                entries = trk.backdate(1, history, batch)
                e1.record()
                ctx.synchronize()
                t1 = time.perf_counter()
                assert len(entries) == history and all(e["nvalid"] == segment and e["status"] == 0 for e in entries[1:])
                if rep >= WARM:
                    host.append(t1 - t0), device.append(e0.elapsed_time(e1) * 1e-3)
            for rep in range(3):
                t2 = time.perf_counter()
                poses = host_backdate(tracks[:segment], history)
                mirror.append(time.perf_counter() - t2)
            worst = max(float(np.abs(p - e["pose"]).max()) for p, e in zip(poses, entries))
            print(f"{segment} tracks of {CAP}, history {history}: backdate {median_us(host):.0f} us on the wall clock, "
                  f"{median_us(device):.0f} us between the events around it ({trk.lastLaunches()} + {batch.last_launches()} launches, "
                  f"{history - 1} problems); on the host from full histories {median_us(mirror):.0f} us (median of 3); "
                  f"largest pose difference {worst:.2e}")
    trk.close()
    batch.close()
    ctx.close()


if __name__ == "__main__":
    main()
