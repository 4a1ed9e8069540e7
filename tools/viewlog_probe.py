"""What the tracker's view log costs and what it saves (LABNOTES.md).  One process, 640 x 480, a full
table of 4 096 tracks of which every fourth continues, 1 024 keypoints per frame with slightly disturbed descriptors so that
all of them match -- the set-up of the track table's own figures.  time.perf_counter around the calls with the stream idle
before them, medians of 25 frames after 10 warm-up frames; device time from events around the enqueued work.

  add + prune with the log off, then with a log of 64 frames, in the same process
  modelViews + storeDevice for one model of 64 keypoints over 16 and 64 views: device time, and with the host's waits
  the same views built by point_tracker.ModelTracks on the host from full histories and stored with mmf_viewstore_store

    python tools/viewlog_probe.py
"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

W, H, CAP, N, WARM, FRAMES = 640, 480, 4096, 1024, 10, 25


def unit_rows(rng, n):
    x = rng.standard_normal((n, 256)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def median_us(samples):
    return statistics.median(samples) * 1e6


def main():
    from multimotionfusion_amd.cudafuncs import Context
    from multimotionfusion_amd.point_tracker import Keypoint, ModelTracks
    from multimotionfusion_amd.redetection import ViewStore
    from multimotionfusion_amd.tracker import DevicePointTracker
    ctx = Context(0)
    rng = np.random.default_rng(0)
    K = (528.0, 528.0, 320.0, 240.0)
    base = unit_rows(rng, CAP)
    depth = torch.full((H, W), 2.0, device="cuda")

    def frame(step):
        rows = (np.arange(N) * 4 + step % 4) % CAP
        desc = base[rows] + 0.01 * unit_rows(rng, N)
        xy = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], 1).astype(np.int32)
        return torch.from_numpy(xy).cuda(), torch.from_numpy(desc.astype(np.float32)).cuda()

    for log in (0, 64):
        trk = DevicePointTracker(ctx, W, H, K, capacity=CAP, max_keypoints=N)
        trk.setViewLog(log)
        for step in range(4):  # fill the table
            xy, de = frame(step)
            trk.addKeypointsPixels(xy, torch.from_numpy(base[step * N:(step + 1) * N]).cuda(), step, depth, 0.7, 0)
        assert trk.status()[0] == CAP
        host, device = [], []
        for step in range(WARM + FRAMES):
            xy, de = frame(step)
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            trk.addKeypointsPixels(xy, de, 10 + step, depth, 0.7, 0)
            trk.prune(30, 0)
            e1.record()
            ctx.synchronize()
            t1 = time.perf_counter()
            if step >= WARM:
                host.append(t1 - t0)
                device.append(e0.elapsed_time(e1) * 1e-3)
        print(f"add + prune, log {'off' if not log else f'of {log} frames'}: {median_us(host):.0f} us with the wait, "
              f"{median_us(device):.0f} us on the device, {trk.status()[0]} tracks, add = {7 if not log else 9} launches")
        trk.close()

    # one model of 64 keypoints seen in every frame, over 16 and 64 views
    kp = 64
    desc = unit_rows(rng, kp)
    flat = rng.choice(W * H, kp, replace=False)
    xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
    for n_views in (16, 64):
        trk = DevicePointTracker(ctx, W, H, K, capacity=CAP, max_keypoints=N)
        trk.setViewLog(n_views)
        tracks = [[] for _ in range(kp)]
        for step in range(n_views):
            trk.addKeypointsPixels(xy, desc, step, depth, 0.7, 30)
            _, co, _, _ = trk.visible()
            for j in range(kp):
                tracks[j].append(Keypoint(step, tuple(xy[j]), co[j].astype(np.float64), desc[j]))
        trk.associateAll([1])
        stamps = list(range(1, n_views + 1))
        poses = np.stack([np.eye(4, dtype=np.float32)] * n_views)
        poses[:, :3, 3] = rng.standard_normal((n_views, 3)).astype(np.float32)
        host, device, mirror = [], [], []
        for rep in range(WARM + FRAMES):
            vs = ViewStore(ctx)
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            counts, de, co, missing = trk.modelViewsDevice(1, stamps, poses)
            assert vs.storeDevice(1, counts, de, co) and missing == 0 and int(counts.sum()) == kp * n_views
            e1.record()
            ctx.synchronize()
            t1 = time.perf_counter()
            vs.close()
            vs = ViewStore(ctx)
            ctx.synchronize()
            t2 = time.perf_counter()
            mt = ModelTracks(1)
            mt.tracks = {id(t): t for t in tracks}
            for v in range(n_views):
                mt.addPose(poses[v], v)
            mt.store()
            assert vs.store(1, mt.views())
            t3 = time.perf_counter()
            vs.close()
            if rep >= WARM:
                host.append(t1 - t0)
                device.append(e0.elapsed_time(e1) * 1e-3)
                mirror.append(t3 - t2)
        print(f"{n_views} views of {kp} keypoints: modelViews + storeDevice {median_us(host):.0f} us with the host's waits, "
              f"{median_us(device):.0f} us between the events around them; ModelTracks.store + views + mmf_viewstore_store on the "
              f"host {median_us(mirror):.0f} us (a store's first use allocates its buffers in both)")
        trk.close()
    ctx.close()


if __name__ == "__main__":
    main()
