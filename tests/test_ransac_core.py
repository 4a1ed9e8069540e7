"""CPU (host code in libmmf_hip.so): the RANSAC core that the host class and the device verifier share
(csrc/rigid_ransac.hpp): the restated std::hash<float>, and table + hash + sort + core against a fresh
RigidRANSAC object per problem, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import ransac_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rr():
    from multimotionfusion_amd import build
    build.build(verbose=False)
    from multimotionfusion_amd import ransac
    return ransac


def test_restated_hash_equals_std_hash(rr):
    """hash_float_bits against std::hash<float> of the C++ library the class used so far: 2 M random bit patterns (NaNs
    and denormals among them), every exponent with a zero and a full mantissa, and the special values."""
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2 ** 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    exps = (np.arange(256, dtype=np.uint32) << 23)
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff,
                        0x7f7fffff, 0xff7fffff, 0x7fc00000, 0xffc00000, 0x3f800000, 0xbf800000], np.uint32)
    x = np.concatenate([bits, exps, exps | 0x007fffff, exps | 0x80000000, special]).view(np.float32)
    mine, std = rr.hash_float(x)
    assert np.array_equal(mine, std), int((mine != std).sum())
    z, _ = rr.hash_float(np.array([0.0, -0.0], np.float32))
    assert z[0] == 0 and z[1] == 0
    assert len(np.unique(mine)) > 1_990_000  # it is a hash, not a constant


def test_core_equals_a_fresh_object_per_problem(rr):
    """mmf_debug_ransac_core_host against mmf_ransac_create / _estimate / _destroy per problem: T, error and the inlier
    flags over the hash-sorted rows, bit for bit, on 2142 problems of the device tests' sizes and kinds.  Both outcomes occur."""
    probs = rc.problems(14, seed=3)
    assert len(probs) >= 2000
    with_inliers = without = 0
    for k, (kind, p0, p1) in enumerate(probs):
        T, err, inl = rr.core_host(*rc.CONFIG, p0, p1)
        Tr, errr, inlr = rr.RigidRANSAC(*rc.CONFIG).estimate(p0, p1)
        assert rc.same_bits(T, Tr), (k, kind, len(p0), T, Tr)
        assert rc.same_bits(np.float32(err), np.float32(errr)), (k, kind, len(p0), err, errr)
        assert (inl is None) == (inlr is None) and (inl is None or np.array_equal(inl, inlr)), (k, kind, len(p0))
        if inl is None:
            without += 1
            assert np.isinf(err)
        else:
            with_inliers += 1
    assert with_inliers > 200 and without > 200, (with_inliers, without)


def test_core_with_other_configurations(rr):
    """Other iteration counts, thresholds and fractions (the tracker's {10, 0.03, 0.6} among them), 32 iterations at most."""
    rng = np.random.default_rng(5)
    for cfg in [(10, 0.03, 0.6), (1, 0.05, 0.5), (32, 0.01, 0.9), (7, 0.1, 0.1)]:
        for n in [3, 9, 64, 65, 200]:
            for kind in ["noise", "outliers30", "duplicates"]:
                p0, p1 = rc.make(kind, n, rng)
                T, err, inl = rr.core_host(*cfg, p0, p1)
                Tr, errr, inlr = rr.RigidRANSAC(*cfg).estimate(p0, p1)
                assert rc.same_bits(T, Tr) and rc.same_bits(np.float32(err), np.float32(errr)), (cfg, n, kind)
                assert (inl is None) == (inlr is None) and (inl is None or np.array_equal(inl, inlr)), (cfg, n, kind)


def test_core_refuses_what_it_cannot_run(rr):
    from multimotionfusion_amd._capi import MmfError
    p = np.zeros((5, 3), np.float32)
    with pytest.raises(MmfError):
        rr.core_host(0, 0.03, 0.8, p, p)
    with pytest.raises(MmfError):
        rr.core_host(33, 0.03, 0.8, p, p)
    with pytest.raises(MmfError):
        rr.core_host(10, 0.03, 0.8, p[:2], p[:2])


def test_core_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/ransac_core_sanitized.cpp: host code only, its own main, built with -fsanitize=address,undefined and run
    directly.  It runs the core and a fresh class object over the same kinds of problems and compares them itself."""
    exe = tmp_path / "ransac_core_sanitized"
    src = os.path.join(REPO, "tests", "cpp", "ransac_core_sanitized.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    assert out.stdout.strip().startswith("ok ") and out.stderr == "", (out.stdout, out.stderr)
