"""-m gpu: back-dating through the C++ shims (setTrackBackdating / getLastBackdatedPoses of cpp/MultiMotionFusion.h,
PointTracker::backdate of cpp/PointTracker.h): tests/cpp/backdate_shim_sequence.cpp builds with g++ -Wall -Wextra -Werror
against libmmf_hip.so and runs three frames with a box that is labelled from the second one on.  It prints every entry with
its floats as bit patterns; the Python mirror's run over the same frames, id images and SuperPoint weights must print the
same lines."""
import os
import subprocess

import numpy as np
import pytest
import torch

from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, SPAWN = 320, 240, 3, 1


def lines_of(what, frame, model, entries):
    out = [f"{what} {frame} model {model} entries {len(entries)}"]
    hx = lambda a: " ".join(f"{int(v):08x}" for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32))
    for e in entries:
        out.append(f"entry {e['stamp']} {e['timestamp']} {e['from']} {e['both']} {e['nvalid']} {e['status']} {e['host_estimated']} "
                   f"{hx([e['error']])} {e['n_inliers']} {hx(e['T'])} {hx(e['pose'])}")
    return out


def test_shim_back_dates_like_the_python_mirror(gpu_ctx, tmp_path):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.ransac import RansacBatch
    from multimotionfusion_amd.superpoint import SuperPoint, random_weights
    from multimotionfusion_amd.tracker import DevicePointTracker
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(N, seed=5)
    objs = synth.make_objects(1, seed=5)
    frames = [synth.render(p, W, H, seed=i, objects=objs, object_poses=[np.eye(4)]) for i, p in enumerate(poses)]
    masks = [np.ascontiguousarray((f["ids"] == 1).astype(np.uint8)) for f in frames]
    assert all(m.sum() > 500 for m in masks)
    weights = random_weights(3)
    data, wfile = tmp_path / "frames.bin", tmp_path / "weights.bin"
    with open(data, "wb") as fp:
        for f, m in zip(frames, masks):
            fp.write(np.ascontiguousarray(f["rgb"], np.uint8).tobytes())
            fp.write(np.ascontiguousarray(f["depth"], np.float32).tobytes())
            fp.write(m.tobytes())
    with open(wfile, "wb") as fp:
        for w, b in weights:
            fp.write(np.ascontiguousarray(w, np.float32).tobytes())
            fp.write(np.ascontiguousarray(b, np.float32).tobytes())

    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "backdate_shim_sequence"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "backdate_shim_sequence.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    k = [np.float32(K[n]) for n in ("cx", "cy", "fx", "fy")]
    r = subprocess.run([str(exe), str(data), str(wfile), str(W), str(H), str(N), str(SPAWN)] + [f"{float(v):.9g}" for v in k],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "backdate shim sequence: ok" in r.stdout
    shim = [l for l in r.stdout.splitlines() if l.split()[0] in ("frame", "tracker", "entry")]

    cx, cy, fx, fy = (float(v) for v in k)
    g = MultiMotionFusion(gpu_ctx, W, H, cx, cy, fx, fy, enable_multiple_models=1)
    g.setEnableRedetection(True)
    kp = SuperPoint(gpu_ctx, weights, max_width=W, max_height=H, max_keypoints=1024)
    trk = DevicePointTracker(gpu_ctx, W, H, (fx, fy, cx, cy), capacity=4096, max_keypoints=1024)
    g.setTracker(trk, odom_init_kp=False)
    trk.setViewLog(8)
    g.setTrackBackdating(4)
    mine = []
    for i, f in enumerate(frames):
        ts = 1000 + 33_000_000 * i
        rgb, depth = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["depth"]).cuda()
        coordinates, descriptors = kp.getFeatures(rgb)
        trk.addKeypoints(coordinates, descriptors, ts, depth, 0.7, 30)
        trk.prune(30, max(ts - int(1e9), 0))
        g.processFrameHost(f["rgb"], f["depth"], timestamp=ts, mask=masks[i] if i > 0 else None, hasNewLabel=i == SPAWN)
        mid, entries = g.getLastBackdatedPoses()
        mine += lines_of("frame", i, mid, entries)
        if i == SPAWN:
            assert mid == 1 and len(entries) == 2 and entries[1]["both"] >= 3, entries  # (the box carries tracks of two frames)
    batch = RansacBatch(gpu_ctx, 10, 0.03, 0.6, max_points=1024)
    mine += lines_of("tracker", 2, 1, trk.backdate(1, 2, batch))
    mine += lines_of("tracker", 3, 0, trk.backdate(0, 3, batch))
    assert shim == mine, [(a, b) for a, b in zip(shim, mine) if a != b][:2]
    batch.close()
    g.setTracker(None)
    trk.close()
    kp.close()
    g.close()
