"""-m gpu: cpp/SuperPoint.h constructed with SuperPoint::F16 (tests/cpp/superpoint_f16_check.cpp, built with -Wall -Wextra
-Werror like the other shim programs): getFeatures against the C ABI's f16 object on the same image."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_f16_predictor(gpu_ctx, tmp_path):
    from multimotionfusion_amd import build
    from multimotionfusion_amd.superpoint import random_weights
    build.build(verbose=False)
    W, H = 160, 120
    img = np.random.default_rng(21).integers(0, 256, (H, W, 3), dtype=np.uint8)
    ifile, wfile = tmp_path / "image.bin", tmp_path / "weights.bin"
    ifile.write_bytes(img.tobytes())
    with open(wfile, "wb") as fp:
        for w, b in random_weights(3):
            fp.write(np.ascontiguousarray(w, np.float32).tobytes())
            fp.write(np.ascontiguousarray(b, np.float32).tobytes())
    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "superpoint_f16_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "superpoint_f16_check.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe), str(ifile), str(wfile), str(W), str(H)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "precision: f16" in r.stdout and "shim agrees: 1" in r.stdout, r.stdout
    n = int(r.stdout.split("keypoints:")[1].split()[0])
    assert n > 20
