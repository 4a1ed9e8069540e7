"""-m gpu: the C++ shims of the keypoint front end (multimotionfusion_amd/cpp/PointTracker.h; setKeypointPredictor, setOdomInit,
setOdomRefine of cpp/MultiMotionFusion.h) build with g++ -Wall -Wextra -Werror against libmmf_hip.so and run three frames
(tests/cpp/tracker_shim_sequence.cpp).  The program prints tracks, poses and track transformations per frame; the Python
mirror's run over the same frames and SuperPoint weights must give the same numbers, bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 320, 240, 3


def test_shim_runs_the_keypoint_front_end(gpu_ctx, tmp_path):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.superpoint import SuperPoint, random_weights
    from multimotionfusion_amd.tracker import DevicePointTracker
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(N, seed=5)
    frames = [synth.render(p, W, H, seed=i) for i, p in enumerate(poses)]
    weights = random_weights(3)
    data, wfile = tmp_path / "frames.bin", tmp_path / "weights.bin"
    with open(data, "wb") as fp:
        for f in frames:
            fp.write(np.ascontiguousarray(f["rgb"], np.uint8).tobytes())
            fp.write(np.ascontiguousarray(f["depth"], np.float32).tobytes())
    with open(wfile, "wb") as fp:
        for w, b in weights:
            fp.write(np.ascontiguousarray(w, np.float32).tobytes())
            fp.write(np.ascontiguousarray(b, np.float32).tobytes())

    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "tracker_shim_sequence"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "tracker_shim_sequence.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    k = [np.float32(K[n]) for n in ("cx", "cy", "fx", "fy")]
    r = subprocess.run([str(exe), str(data), str(wfile), str(W), str(H), str(N)] + [f"{float(v):.9g}" for v in k],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "tracker shim sequence: ok" in r.stdout
    shim, transforms, last = {}, {}, None
    for line in r.stdout.splitlines():
        t = line.split()
        if t and t[0] == "frame":
            shim[int(t[1])] = (int(t[3]), int(t[5]), np.array(t[7:23], np.float32))
        elif t and t[0] == "transform":
            transforms[int(t[1])] = np.array(t[2:18], np.float32)
        elif t and t[0] == "last":
            last = np.array(t[1:17], np.float32)
    assert sorted(shim) == list(range(N)) and sorted(transforms) == list(range(1, N)) and last is not None

    cx, cy, fx, fy = (float(v) for v in k)
    g = MultiMotionFusion(gpu_ctx, W, H, cx, cy, fx, fy)
    kp = SuperPoint(gpu_ctx, weights, max_width=W, max_height=H, max_keypoints=1024)
    trk = DevicePointTracker(gpu_ctx, W, H, (fx, fy, cx, cy), capacity=4096, max_keypoints=1024)
    g.setTracker(trk, odom_init_kp=True, icp_refine=True)
    for i, f in enumerate(frames):
        ts = 1000 + 33_000_000 * i
        rgb, depth = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["depth"]).cuda()
        coordinates, descriptors = kp.getFeatures(rgb)
        trk.addKeypoints(coordinates, descriptors, ts, depth, 0.7, 30)
        trk.prune(30, max(ts - int(1e9), 0))
        g.processFrameHost(f["rgb"], f["depth"], timestamp=ts)  # (the shim's entry point)
        n_tracks, length, _ = trk.status()
        assert (n_tracks, length) == shim[i][:2], (i, n_tracks, length, shim[i][:2])
        assert shim[i][2].tobytes() == g.getCurrPose().astype(np.float32).tobytes(), (i, shim[i][2], g.getCurrPose())
        T = g.getLastTrackTransforms()
        assert T.shape[0] == (0 if i == 0 else 1)
        if i > 0:
            assert transforms[i].tobytes() == T[0].tobytes(), (i, transforms[i], T[0])
    assert n_tracks > 0 and np.all(np.isfinite(g.getCurrPose()))
    assert last.tobytes() == trk.getLastTrackTransform(0)[0].tobytes()
    g.setTracker(None)
    trk.close()
    kp.close()
    g.close()
