"""-m gpu: the C++ shim on the fern keyframe database -- class Ferns (addFrame, findCandidate, frames, frame, blockHDAware,
lastClosest) on hand-made fill-in images, and MultiMotionFusion::setFernDatabase / setFernThresh / getFerns /
getLastFernResult over four frames against the C ABI's engine on the same fill-in images (tests/cpp/ferns_shim_sequence.cpp,
compiled with g++ -Wall -Wextra -Werror against libmmf_hip.so)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ferns_through_the_shims(tmp_path):
    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "ferns_shim_sequence"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "ferns_shim_sequence.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "ferns shim sequence: ok" in r.stdout
