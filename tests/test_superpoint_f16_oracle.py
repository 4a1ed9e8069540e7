"""CPU: the host half of the f16 SuperPoint path and the oracle that judges the device half
(tests/superpoint_f16_oracle.py): the library's f16 rounding against numpy's on every f16 value, every midpoint and the
named edge values; the exact cases stay below 2^24; f32 sums in two orders stay within the tolerance T on every random
case; every random case can see a dropped term; the header's new symbols are bound."""
import ctypes

import numpy as np
import pytest

import superpoint_f16_oracle as so


@pytest.fixture(scope="module")
def lib():
    from multimotionfusion_amd import _capi, build
    build.build(verbose=False)
    return _capi.load()


def lib_round(lib, a):
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty(a.shape, np.uint16)
    assert lib.mmf_f16_round(a.ctypes.data, a.size, out.ctypes.data) == 0
    return out


def test_f16_round_equals_numpy_on_every_value_and_midpoint(lib):
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    got = lib_round(lib, every.astype(np.float32))
    assert np.array_equal(got, every.view(np.uint16))  # every f16 value, both zeros, infinities and every NaN payload
    finite = np.sort(every[np.isfinite(every)].astype(np.float32))
    finite = finite[np.concatenate([[True], np.diff(finite) > 0])]  # (-0 and +0 are one point)
    mid = (finite[:-1].astype(np.float64) + finite[1:].astype(np.float64)) / 2
    mid32 = mid.astype(np.float32)
    assert np.array_equal(mid32.astype(np.float64), mid)  # the midpoints are f32 values
    for m in (mid32, np.nextafter(mid32, np.float32(np.inf)), np.nextafter(mid32, np.float32(-np.inf))):
        assert np.array_equal(lib_round(lib, m), so.rne16(m).view(np.uint16))
    rng = np.random.default_rng(0)
    r = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    assert np.array_equal(lib_round(lib, r), so.rne16(r).view(np.uint16))


def test_f16_round_named_values(lib):
    inf = np.float32(np.inf)
    for x, want in [(2049.0, 2048.0), (2051.0, 2052.0), (65519.0, 65504.0), (65520.0, inf), (-65520.0, -inf),
                    (2.0 ** -25, 0.0), (1.5 * 2.0 ** -25, 2.0 ** -24), (-(2.0 ** -25), -0.0), (0.0, 0.0), (-0.0, -0.0), (1e5, inf)]:
        got = lib_round(lib, np.array([x], np.float32)).view(np.float16)[0]
        assert got.view(np.uint16) == np.float16(want).view(np.uint16), (x, got, want)
        assert got.view(np.uint16) == so.rne16(np.float32(x)).view(np.uint16)
    assert np.isnan(lib_round(lib, np.array([np.nan, -np.nan], np.float32)).view(np.float16)).all()
    assert lib.mmf_f16_round(None, 0, None) == 0 and lib.mmf_f16_round(None, 1, None) == -1


@pytest.mark.parametrize("case", so.CASES, ids=[str(i) for i in range(len(so.CASES))])
def test_exact_cases_stay_below_2_24_and_reach_the_rounding(case):
    x, w, b = so.exact_case(case)
    assert np.array_equal(so.rne16(w).astype(np.float32), w)  # the weights are f16 values
    assert so.abs_sum_max(x, w, b) < 2 ** 24
    ref, B, _ = so.layer(x, w, b, case[5], case[6], True)
    assert np.array_equal(ref, np.round(ref))
    if case[2] * case[4] ** 2 == 1152:  # sums that f16 cannot hold: above 2048 and odd
        big = ref[ref > 2048]
        assert big.size > 100 and (big % 2 == 1).sum() > 20, (big.size, (big % 2 == 1).sum())


def sampled_f32_sums(x, w, rows):
    """f32 sums of the layer's products on a sample of output pixels, accumulated sequentially (K ascending) and pairwise"""
    cout, cin, k, _ = w.shape
    a = so.patches(x.astype(np.float32), k).reshape(-1, k * k * cin)[rows]            # [P][tap*cin]
    wm = so.rne16(w).astype(np.float32).reshape(cout, cin, k * k).transpose(0, 2, 1).reshape(cout, -1)
    prod = a[:, None, :] * wm[None, :, :]                                             # exact in f32
    seq = np.cumsum(prod, axis=2, dtype=np.float32)[:, :, -1]
    pair = prod.sum(axis=2, dtype=np.float32)
    return seq, pair


@pytest.mark.parametrize("case", so.CASES, ids=[str(i) for i in range(len(so.CASES))])
def test_random_cases_f32_sums_within_tolerance_and_see_a_dropped_term(case):
    H, W, cin, cout, k, relu, pool, _ = case
    x, w, b = so.random_case(case)
    assert not np.any((x != 0) & (np.abs(x) < np.float16(2.0 ** -14)))  # no f16 subnormal operand
    ref, B, T = so.layer(x, w, b, False, False, True)  # the accumulation itself: before ReLU and pool, f32 out
    rng = np.random.default_rng(1)
    rows = rng.choice(H * W, min(H * W, 24), replace=False)
    seq, pair = sampled_f32_sums(x, w, rows)
    b32 = b.astype(np.float32)
    worst = 0.0
    for s in (seq, pair):
        got = (s + b32).astype(np.float64)
        ratio = np.abs(got - ref.reshape(H * W, cout)[rows]) / T.reshape(H * W, cout)[rows]
        worst = max(worst, float(ratio.max()))
    print("K", cin * k * k, "worst |f32 sum - ref| / T", worst)
    assert worst <= 0.30
    # a dropped term leaves T in at least 10 % of the outputs, in either output format
    for out_f32 in (True, False):
        ref, _, T = so.layer(x, w, b, relu, pool, out_f32)
        bad, _, _ = so.layer(x, w, b, relu, pool, out_f32, drop=so.dropped_term(case))
        share = float((np.abs(bad - ref) > T).mean())
        print("out_f32", out_f32, "share of outputs a dropped term moves out of T", share)
        assert share >= 0.10


def test_new_symbols_are_declared_and_bound(lib):
    from multimotionfusion_amd import _capi
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmf_hip.h")).read()
    for name in ("mmf_superpoint_create_ex", "mmf_superpoint_precision", "mmf_superpoint_conv_f16", "mmf_f16_round",
                 "mmf_debug_superpoint_forward_prefix"):
        assert name in _capi.SIGNATURES and name + "(" in header and hasattr(lib, name), name
    assert "MMF_SP_F32 = 0" in header and "MMF_SP_F16 = 1" in header
    assert lib.mmf_abi_version() == 3
    assert lib.mmf_superpoint_precision(None) == -1
    assert isinstance(lib, ctypes.CDLL)
