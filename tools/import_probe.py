"""GPU box: mmf_model_import_cloud on the records of the headline loop's steady map (640x480, the bench's sequence played
forwards and backwards) and of a mature store (that map + three occluded copies, all stable), against what a caller had to do
before for the same records: unpack them with numpy into the 48-byte AoS and call mmf_model_upload_map.  The records are in
host memory before either clock starts.  HIP events around each call after a warm-up, median of 15; both calls wait for their
result, so the events span the copy to the device and the kernel.  Then the frame that activates a model restored from disk, with
and without its dense surfels (the redetection scene of tests/test_gpu_redetect_fusion.py).

    python tools/import_probe.py [WxH] [frames]
"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context  # noqa: E402
from multimotionfusion_amd.fusion import MultiMotionFusion  # noqa: E402
from multimotionfusion_amd.model import Model  # noqa: E402

W, H = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "640x480").split("x"))
N = int(sys.argv[2]) if len(sys.argv) > 2 else 90
CONF, HBM_PEAK = 10.0, 8.0e12  # MI355X: 8 TB/s
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def numpy_import(r, confidence, t):
    """the same surfels on the host: unpack the records into the 48-byte AoS (identity pose: x * 1 + 0 ... = x, -(n))"""
    s = np.zeros((len(r), 12), np.float32)
    s[:, 0], s[:, 1], s[:, 2], s[:, 3] = r["x"] + 0.0, r["y"] + 0.0, r["z"] + 0.0, confidence
    s[:, 4] = (r["red"].astype(np.uint32) << 16 | r["green"].astype(np.uint32) << 8 | r["blue"]).astype(np.float32)
    s[:, 6] = s[:, 7] = t
    s[:, 8], s[:, 9], s[:, 10], s[:, 11] = -r["nx"], -r["ny"], -r["nz"], r["radius"]
    return s


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
g.close()
layers = []
for step in (0.0, 0.02, 0.04, 0.06):
    cp = steady.copy()
    cp[:, :3] += step * cp[:, :3] / np.maximum(np.linalg.norm(cp[:, :3], axis=1, keepdims=True), 1e-6)
    cp[:, 3] = np.maximum(cp[:, 3], 20.0)
    layers.append(cp)
mature = np.concatenate(layers)[: 1024 * 1024 - 310000]
m = Model(ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"], 0, CONF)
eye = np.eye(4, dtype=np.float32)
for name, surfels in (("steady", steady), ("mature", mature)):
    m.uploadMap(surfels)
    records = m.exportCloud(eye, CONF).copy()  # the stable surfels, as savePly writes them
    n = len(records)
    ev_new, wall_new, _ = timed(lambda: m.importCloud(records, None, CONF + 1, 7))
    launches, got = m.importLastLaunches(), m.downloadMap()

    def old():
        m.uploadMap(numpy_import(records, CONF + 1, 7))
    ev_old, wall_old, _ = timed(old, reps=8, skip=2)
    want = m.downloadMap()
    aos = numpy_import(records, CONF + 1, 7)
    ev_up, wall_up, _ = timed(lambda: m.uploadMap(aos), reps=8, skip=2)
    same = np.array_equal(got, want)  # (as values: the host shortcut above does not reproduce the signs of zeros)
    read, written = 31 * n, 48 * n
    print(f"{name}: {len(surfels)} surfels, {n} records; import_cloud {ev_new:.0f} us by events ({wall_new:.0f} us wall, {launches} launch); "
          f"numpy unpack + upload_map {wall_old:.0f} us wall, upload_map alone {ev_up:.0f} us by events ({wall_up:.0f} us wall); "
          f"maps equal: {same}")
    print(f"{name}: device traffic {read / 1e6:.2f} MB read + {written / 1e6:.2f} MB written = {(read + written) / 1e6:.2f} MB: "
          f"{(read + written) / HBM_PEAK * 1e6:.2f} us at the HBM peak, {100 * (read + written) / HBM_PEAK / (ev_new * 1e-6):.2f} % of it over the "
          f"whole call (the call begins with {read / 1e6:.2f} MB copied from pageable host memory and ends with a wait)")
    ev_ts, wall_ts, _ = timed(lambda: m.setTimestamps(9))
    print(f"{name}: set_timestamps {ev_ts:.0f} us by events ({wall_ts:.0f} us wall), {16 * n / 1e6:.2f} MB of colour vectors touched")
m.close()

# ---- the activating frame of a model restored from disk, with and without its dense surfels ----
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_gpu_redetect_fusion as rf  # noqa: E402
from test_gpu_modeldb_fusion import SEED, step, translation  # noqa: E402
from multimotionfusion_amd.point_tracker import Keypoint, ModelTracks  # noqa: E402

Kr, rposes, objs, traj, with_obj, without = rf.gap_scene(SEED)
kps, desc = rf.physical_keypoints(SEED, Kr, rposes, traj, with_obj)


def fusion():
    f = MultiMotionFusion(ctx, rf.W, rf.H, Kr["cx"], Kr["cy"], Kr["fx"], Kr["fy"], enable_multiple_models=1)
    f.setEnableRedetection(True)
    return f


a = fusion()
mt, tracks, keep = ModelTracks(1), [[] for _ in range(len(desc))], []
for i in range(rf.LAST_SEEN + 2):
    hidden = i > rf.LAST_SEEN
    f = without[i] if hidden else with_obj[i]
    mask = np.zeros((rf.H, rf.W), np.uint8)
    if i >= rf.SPAWN and not hidden:
        mask[f["ids"] == 1] = 1
    step(a, keep, f, mask, i == rf.SPAWN)
    if rf.SPAWN <= i <= rf.LAST_SEEN:
        idx, xy, coord = kps[i]
        P = a.getModels()[1].getPose()
        for j in range(len(desc)):
            hit = np.flatnonzero(idx == j)
            tracks[j].append(Keypoint(1000 + i, tuple(xy[hit[0]]), coord[hit[0]].astype(np.float64), desc[j]) if len(hit) else None)
        if i == rf.SPAWN:
            mt.initGlobalTracks(tracks, P, 1000 + i)
        else:
            mt.addPose(P, 1000 + i)
assert mt.store() and a.storeViews(1, mt.views())
a.getModels()[0].overridePose(translation(0.5, -0.25, 1.0))
a.getInactiveModels()[0].overridePose(translation(0.125, 2.0, -0.75))
out = tempfile.mkdtemp(prefix="import_probe_")
a.savePly(out)
a.close()
for rep in range(3):
    for dense in (False, True):  # alternating, same process
        b = fusion()
        b.loadModels(out, dense=dense)
        restored = b.getInactiveModels()[0].lastCount()
        keep = []
        for i in range(rf.LAST_SEEN + 1, rf.BACK):
            step(b, keep, without[i], np.zeros((rf.H, rf.W), np.uint8), False)
        f = with_obj[rf.BACK]
        mask = np.zeros((rf.H, rf.W), np.uint8)
        mask[f["ids"] == 1] = b.getNextModelID()
        idx, xy, coord = kps[rf.BACK]
        step(b, keep, f, mask, True, (xy, coord, desc[idx]))
        ctx.synchronize()
        t_track, t_frame = b.lastTimings()
        ev = b.getLastRedetections()
        print(f"activating frame (run {rep}, dense={dense}): {restored} surfels restored, activated={bool(ev and ev[0]['activated'])}, "
              f"processFrame {t_frame * 1e6:.0f} us host wall clock ({t_track * 1e6:.0f} us of it tracking); the model holds "
              f"{b.getModels()[-1].lastCount()} surfels after the frame; one added launch (import_stamp_kernel) is expected with dense=True")
        b.close()
shutil.rmtree(out, ignore_errors=True)
ctx.close()
