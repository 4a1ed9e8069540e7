"""Times of the segmentation from a frame's label image (csrc/mask_kernels.hpp):
  1. one synchronous mmf_mask_segment call between two HIP events on the context's stream, median / min over --reps calls,
     at 640x480 and 1280x960.  The call waits for its summary before it returns, so the second event is recorded after the
     host has woken up: the figure is the two passes, the two one-workgroup launches and the summary's copy PLUS that
     wake-up and the record -- an upper bound of the device work, not the kernels alone.  The call's wall clock beside it;
  2. the same frame through tools/mask_host_loop.cpp (-O2, one thread): what a front end pays on the host today;
  3. processFrame per frame with two objects at 640x480: the mode on (raw labels) against the pre-mapped path fed the
     same id image and model data.
python tools/mask_probe.py [--reps 200] [--frames 20]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from multimotionfusion_amd import synth  # noqa: E402
from multimotionfusion_amd._capi import mmf_segmentation_model  # noqa: E402
from multimotionfusion_amd.cudafuncs import Context, _p  # noqa: E402
from multimotionfusion_amd.fusion import MultiMotionFusion  # noqa: E402
from multimotionfusion_amd.segmentation import MaskConfig  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frame(w, h, i=1):
    objs = synth.make_objects(2, seed=21)
    poses = synth.trajectory(i + 1, seed=21)
    traj = synth.object_trajectories(objs, i + 1, seed=21)
    return synth.render(poses[i], w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj])


def host_loop():
    with tempfile.TemporaryDirectory() as tmp:  # (the mapped library outlives its directory entry)
        so = os.path.join(tmp, "mask_host_loop.so")
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", os.path.join(REPO, "tools", "mask_host_loop.cpp"), "-o", so], check=True)
        fn = C.CDLL(so).mask_host_loop
    vp = C.c_void_p
    fn.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_uint, C.c_int, vp, vp, vp, vp, vp]
    fn.restype = C.c_int
    return fn


def kernel_and_host(ctx, loop, w, h, reps):
    f = frame(w, h)
    lab, depth = f["ids"].astype(np.uint8) * 37, np.ascontiguousarray(f["depth"], np.float32)
    tl, td, mask = dev(lab), dev(depth), torch.empty((h, w), dtype=torch.uint8, device="cuda")
    ids = (C.c_uint * 3)(0, 1, 2)
    table = np.zeros(256, np.uint8)
    table[37], table[74] = 1, 2
    out = (mmf_segmentation_model * 4)()
    n_out, has_new, new_label = C.c_int(), C.c_int(), C.c_int()
    stream = torch.cuda.current_stream()
    assert (ctx.lib.mmf_ctx_stream(ctx.handle) or 0) == stream.cuda_stream, "the context runs on torch's current stream"
    warm = 20
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warm + reps)]
    wall = []
    for k in range(warm + reps):
        t = table.copy()
        a, b = ev[k]
        a.record(stream)
        t0 = time.perf_counter()
        rc = ctx.lib.mmf_mask_segment(ctx.handle, w, h, _p(tl), _p(td), ids, 3, 3, 1, t.ctypes.data_as(C.POINTER(C.c_uint8)), _p(mask), out,
                                      C.byref(n_out), C.byref(has_new), C.byref(new_label))
        wall.append(time.perf_counter() - t0)
        b.record(stream)
        assert rc == 0
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev[warm:]])
    wall = np.array(wall[warm:]) * 1e6
    cnt, mean, std = np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros(4, np.float32)
    hm = np.zeros(w * h, np.uint8)
    host = []
    for _ in range(max(reps // 4, 20)):
        t = table.copy()
        t0 = time.perf_counter()
        loop(lab.ctypes.data, depth.ctypes.data, w * h, ids, 3, 3, 1, t.ctypes.data, hm.ctypes.data, cnt.ctypes.data, mean.ctypes.data,
             std.ctypes.data)
        host.append(time.perf_counter() - t0)
    host = np.array(host) * 1e6
    assert np.array_equal(hm.reshape(h, w), mask.cpu().numpy())
    print(f"{w}x{h}: synchronous call between two events ({reps} calls) median {np.median(us):.1f} us min {us.min():.1f} us; call wall median "
          f"{np.median(wall):.1f} us; host loop median {np.median(host):.1f} us min {host.min():.1f} us", flush=True)


def process_frame(ctx, n_frames):
    w, h = 640, 480
    K = synth.intrinsics(w, h)
    objs = synth.make_objects(2, seed=21)
    poses = synth.trajectory(n_frames, seed=21)
    traj = synth.object_trajectories(objs, n_frames, seed=21)
    frames = [synth.render(p, w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    rgb, depth = [dev(f["rgb"]) for f in frames], [dev(f["depth"]) for f in frames]
    raw = [dev(f["ids"].astype(np.uint8) * 37) for f in frames]

    def run(on, fed=None):
        g = MultiMotionFusion(ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=2)
        if on:
            g.setMaskSegmentation(MaskConfig(model_spawn_offset=1))
        times, rec = [], []
        for i in range(n_frames):
            if on:
                kw = dict(mask=raw[i])
            else:
                m, seg = fed[i]
                kw = dict(mask=m, hasNewLabel=bool(seg and seg["has_new_label"]), modelData=seg["model_data"] if seg else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.processFrame(rgb[i], depth[i], timestamp=i, **kw)
            times.append(time.perf_counter() - t0)
            if on:
                rec.append((g.getTexture("MASK").clone(), g.lastMaskSegmentation() if i > 0 else None))
        g.close()
        return np.array(times[5:]) * 1e3, rec

    res = {}
    _, fed = run(True)
    for rnd in range(3):
        for name, on in (("mode on", True), ("pre-mapped", False)):
            t, _ = run(on, fed)
            res.setdefault(name, []).append(float(np.median(t)))
    for name, v in res.items():
        print(f"processFrame 640x480, camera + two objects, {n_frames - 5} frames x 3 runs: {name}: median ms per run {['%.3f' % x for x in v]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=20)
    a = ap.parse_args()
    ctx = Context(0)
    loop = host_loop()
    for w, h in ((640, 480), (1280, 960)):
        kernel_and_host(ctx, loop, w, h, a.reps)
    process_frame(ctx, a.frames)
    ctx.close()
