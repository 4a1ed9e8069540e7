"""The arithmetic of the f16 SuperPoint forward pass (MMF_SP_F16), stated in numpy.

* Weights of conv1b ... convDb are rounded to f16 once: to nearest, ties to even (`rne16`, which is numpy's float16
  conversion).  Biases stay f32.  conv1a keeps f32 weights and the f32 arithmetic of the f32 path (grey conversion, one
  fmaf chain over the taps, + bias, ReLU); its result is `rne16` of that f32 value.
* Every other layer: products of two f16 values are exact in f32; each output has ONE f32 accumulator that walks K in a
  fixed order (K blocks of 32 channels, taps, the two 16-channel halves of a block, each ascending); what the matrix
  instruction does inside its 16 products is not specified.  Then one f32 `+ bias`, ReLU where the layer has one, the
  2x2 maximum where it pools (NaN kept), and one rounding to nearest-even f16 (overflow to inf, NaN kept).  The two 1x1
  heads store the f32 value unrounded.
* Because the order inside an instruction is open, a layer is checked against the EXACT value with a bound:
      ref = sum(a_i w_i) + bias in float64 on the f16 operands (exact to 2^-53 relative),
      B   = (K + 1) 2^-23 (sum|a_i w_i| + |bias|)   -- K f32 additions in any order, doubled for a truncating adder,
      T   = B                                        for f32 outputs,
      T   = B + 2^-11 (|ref| + B) + 2^-25            for f16 outputs (one rounding of a value within B of ref; 2^-25 is
                                                     half the smallest subnormal's spacing).
  ReLU and the maximum do not expand a difference, so the pooled output's T takes the largest B of its window.
  On integer data whose sums stay below 2^24 every order gives the same f32 sum and the check is bit for bit.
"""
import numpy as np


def rne16(x):
    """f32 -> f16, round to nearest, ties to even, overflow to inf (numpy's conversion)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def patches(x, k):
    """[H,W,C] -> [H,W,k*k,C] with zero padding (k = 3) or the image itself (k = 1); tap = 3*dy + dx"""
    H, W, C = x.shape
    if k == 1:
        return x.reshape(H, W, 1, C)
    p = np.zeros((H + 2, W + 2, C), x.dtype)
    p[1:-1, 1:-1] = x
    return np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=2)


def pool_max(y):
    H, W, C = y.shape
    return y.reshape(H // 2, 2, W // 2, 2, C).max(axis=(1, 3))  # (numpy's max keeps NaN)


def layer(x16, w, b, relu, pool, out_f32, drop=None):
    """One layer on f16 activations x16 [H,W,Cin], f32 weights w [Cout,Cin,k,k] (rounded here) and f32 bias b.
    Returns (ref, B, T): the exact output [h,w,Cout] in float64, the accumulation bound and the tolerance, after ReLU
    and pooling.  drop = (tap, channel-or-None) leaves those terms out (the mistake the cases must be able to see)."""
    assert x16.dtype == np.float16
    cout, cin, k, _ = w.shape
    w16 = rne16(w).astype(np.float64).reshape(cout, cin, k * k).transpose(2, 1, 0)  # [tap][ci][co]
    if drop is not None:
        tap, ch = drop
        w16 = w16.copy()
        if ch is None:
            w16[tap] = 0.0
        else:
            w16[tap, ch] = 0.0
    a = patches(x16.astype(np.float64), k)  # [H,W,taps,Cin]
    K = cin * k * k
    s = np.tensordot(a, w16, axes=([2, 3], [0, 1]))
    sabs = np.tensordot(np.abs(a), np.abs(w16), axes=([2, 3], [0, 1]))
    b64 = np.asarray(b, np.float32).astype(np.float64)
    ref = s + b64
    B = (K + 1) * 2.0 ** -23 * (sabs + np.abs(b64))
    if relu:
        ref = np.maximum(ref, 0.0)
    if pool:
        ref, B = pool_max(ref), pool_max(B)
    T = B if out_f32 else B + 2.0 ** -11 * (np.abs(ref) + B) + 2.0 ** -25
    return ref, B, T


def layer_exact(x16, w, b, relu, pool, out_f32):
    """the layer's output where every order of addition gives the same f32 sum (integer data, sums below 2^24): f32, or
    its rne16"""
    ref, _, _ = layer(x16, w, b, relu, pool, True)
    y = ref.astype(np.float32)
    assert np.array_equal(y.astype(np.float64)[~np.isnan(ref)], ref[~np.isnan(ref)])
    return y if out_f32 else rne16(y)


def abs_sum_max(x16, w, b):
    """largest sum|a_i w_i| + |bias| of a layer: below 2^24, every partial sum of integers is exact in f32"""
    cout, cin, k, _ = w.shape
    a = patches(np.abs(x16.astype(np.float64)), k)
    wa = np.abs(rne16(w).astype(np.float64)).reshape(cout, cin, k * k).transpose(2, 1, 0)
    return float((np.tensordot(a, wa, axes=([2, 3], [0, 1])) + np.abs(np.asarray(b, np.float64))).max())


def conv1a_f16(y_f32):
    """conv1a of the f16 path from the f32 path's conv1a output"""
    return rne16(y_f32)


# ---- the cases of tests/test_gpu_superpoint_f16.py (the shapes of test_conv_layer_bit_exact) ---------------------------------
CASES = [
    (8, 16, 32, 32, 3, True, False, 1),      # exactly one tile, one K block
    (24, 40, 64, 64, 3, True, False, 2),     # ragged right edge, two K blocks
    (24, 40, 64, 64, 3, True, True, 2),      # fused 2x2 max pool
    (20, 36, 128, 128, 3, True, True, 4),    # ragged both ways, four K blocks, widest tile
    (20, 36, 128, 128, 3, True, False, 1),
    (6, 8, 128, 512, 3, True, False, 1),     # the fused detector | descriptor head
    (6, 8, 256, 65, 1, False, False, 1),     # 1x1, output channels not a multiple of 32, no ReLU
    (12, 20, 256, 256, 1, False, False, 4),
    (16, 16, 64, 96, 3, False, False, 0),    # automatic tile width, 96 channels
]
F32_OUT = {6, 7}  # the cases the issue lists with f32 output (the two 1x1 heads)


def case_seed(case):
    H, W, cin, cout = case[:4]
    return H * 1000 + W * 10 + cin + cout


def exact_case(case):
    """activations in {0,1,2} (mostly 2), weights in {-1,0,1}, integer biases in [-3,3].  Every fourth output channel has
    all weights +1, so that 3x3 layers of 128 channels reach sums above 2048, where f16 keeps even integers only."""
    H, W, cin, cout, k = case[:5]
    rng = np.random.default_rng(case_seed(case))
    x = rng.choice(np.array([0, 1, 2], np.float16), size=(H, W, cin), p=[0.03, 0.07, 0.9])
    w = rng.integers(-1, 2, (cout, cin, k, k)).astype(np.float32)
    w[::4] = 1.0
    b = rng.integers(-3, 4, cout).astype(np.float32)
    return x, w, b


def random_case(case):
    """normal(0,1) after ReLU, rounded to f16, f16 subnormals (below 2^-14) set to 0; He-scaled weights"""
    H, W, cin, cout, k = case[:5]
    rng = np.random.default_rng(case_seed(case) + 1)
    x = rne16(np.maximum(rng.normal(0, 1, (H, W, cin)), 0).astype(np.float32))
    x[x < np.float16(2.0 ** -14)] = 0
    w = rng.normal(0, np.sqrt(2.0 / (cin * k * k)), (cout, cin, k, k)).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    return x, w, b


def dropped_term(case):
    """the mistake a case must see: tap 7 of a 3x3 layer; a 1x1 layer has one tap, so input channel 7 of it"""
    return (7, None) if case[4] == 3 else (0, 7)
