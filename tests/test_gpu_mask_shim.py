"""-m gpu: the C++ shim (multimotionfusion_amd/cpp/MultiMotionFusion.h) with setMaskSegmentation(true): FrameData::mask carries
raw labels and processFrame(const FrameData&) behaves like the reference's with frame.mask set (tests/cpp/
mask_shim_sequence.cpp, compiled with g++ against libmmf_hip.so).  The program prints model ids, confidence thresholds and
poses per frame; the Python mirror's run over the same frames (processFrameHost: the same C entry point) must give the same
numbers, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from multimotionfusion_amd import synth
from multimotionfusion_amd.segmentation import MaskConfig

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 320, 240, 5


def test_shim_segments_the_frames_labels(gpu_ctx, tmp_path):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    K = synth.intrinsics(W, H)
    poses = synth.trajectory(N, seed=21)
    objs = synth.make_objects(2, seed=21)
    traj = synth.object_trajectories(objs, N, seed=21)
    frames = [synth.render(p, W, H, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    raw = np.zeros(256, np.uint8)
    raw[1], raw[2] = 37, 200
    labels = [raw[f["ids"].astype(np.uint8)] for f in frames]
    data = tmp_path / "frames.bin"
    with open(data, "wb") as fp:
        for f, lab in zip(frames, labels):
            fp.write(np.ascontiguousarray(f["rgb"], np.uint8).tobytes())
            fp.write(np.ascontiguousarray(f["depth"], np.float32).tobytes())
            fp.write(np.ascontiguousarray(lab, np.uint8).tobytes())

    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "mask_shim_sequence"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "mask_shim_sequence.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    k = [np.float32(K[n]) for n in ("cx", "cy", "fx", "fy")]
    r = subprocess.run([str(exe), str(data), str(W), str(H), str(N)] + [f"{float(v):.9g}" for v in k], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "mask shim sequence: ok" in r.stdout
    shim = {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t and t[0] == "frame":
            shim[(int(t[1]), int(t[3]))] = (np.float32(t[5]), np.array(t[7:23], np.float32))
    table = {int(a): int(b) for a, b in (x.split(":") for x in next(l for l in r.stdout.splitlines() if l.startswith("table")).split()[1:])}

    g = MultiMotionFusion(gpu_ctx, W, H, *[float(v) for v in k], enable_multiple_models=1, preallocated_models=2)
    g.setMaskSegmentation(MaskConfig(model_spawn_offset=22))
    g.setModelSpawnOffset(1)  # (as the shim: pushed while the mode is on)
    seen = 0
    for i, (f, lab) in enumerate(zip(frames, labels)):
        g.processFrameHost(f["rgb"], f["depth"], timestamp=1000 + i, mask=lab)
        for m in g.getModels():
            conf, pose = shim[(i, m.id)]
            assert conf.tobytes() == np.float32(m.confidenceThreshold()).tobytes(), (i, m.id)
            assert pose.tobytes() == m.getPose().astype(np.float32).tobytes(), (i, m.id, pose, m.getPose())
            seen += 1
    assert seen == len(shim) == 1 + 2 + 3 * (N - 2)
    mapping = g.maskMapping()
    assert table == {int(l): int(mapping[l]) for l in np.flatnonzero(mapping)} and sorted(table.values()) == [1, 2]
    g.close()
