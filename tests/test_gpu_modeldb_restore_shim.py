"""-m gpu: restoring dense surfels through the C++ shim (Model::importCloud / importPly / setTimestamps,
MultiMotionFusion::setRestoreDense + loadModels) once (tests/cpp/modeldb_restore_shim_sequence.cpp, compiled with g++ against
libmmf_hip.so)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_restores_dense_surfels(tmp_path):
    pkg = os.path.join(REPO, "multimotionfusion_amd")
    exe = tmp_path / "modeldb_restore_shim_sequence"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "cpp", "modeldb_restore_shim_sequence.cpp"), "-o", str(exe), f"-L{pkg}", "-lmmf_hip",
                    "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "modeldb restore shim sequence: ok" in r.stdout
