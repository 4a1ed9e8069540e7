"""-m gpu: the C++ class of the flow-CRF inference engine (multimotionfusion_amd/cpp/FlowCrf.h) on a scene whose answer is
known (tests/cpp/flowcrf_engine_check.cpp, compiled with g++ -Wall -Wextra -Werror against libmmf_hip.so)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_engine_through_its_cpp_class(tmp_path):
    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "flowcrf_engine_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "flowcrf_engine_check.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "flowcrf engine check: ok" in r.stdout
