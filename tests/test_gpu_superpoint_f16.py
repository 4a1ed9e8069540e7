"""-m gpu: the f16 forward pass of SuperPoint (precision="f16") against tests/superpoint_f16_oracle.py.

Layers on integer data must equal the oracle bit for bit (every order of addition gives the same f32 sum); on random data
every output must lie within the oracle's tolerance T of the exact value.  conv1a is rne16 of the f32 path's; the network
is the chain of its layers; everything behind the two 1x1 heads is the f32 path's code on the same buffers."""
import functools

import numpy as np
import pytest
import torch

import superpoint_f16_oracle as so
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

CASE_IDS = [str(i) for i in range(len(so.CASES))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_layer(ctx, x16, w, b, case, out_f32):
    from multimotionfusion_amd.superpoint import conv_f16
    relu, pool, nt = case[5:8]
    return conv_f16(ctx, dev(x16), w, b, relu=relu, pool=pool, nt=nt, out_f32=out_f32).cpu().numpy()


def assert_same_values(got, want, what):
    """bit for bit, except that any NaN equals any NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int(gn.sum()), int(wn.sum()))
    u = np.uint16 if got.dtype == np.float16 else np.uint32
    bad = (got.view(u) != want.view(u)) & ~gn
    assert not bad.any(), (what, int(bad.sum()), got[bad][:5], want[bad][:5])


# ---- 1. exact data --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_reference(i, out_f32):
    x, w, b = so.exact_case(so.CASES[i])
    return so.layer_exact(x, w, b, so.CASES[i][5], so.CASES[i][6], out_f32)


@pytest.mark.parametrize("i", range(len(so.CASES)), ids=CASE_IDS)
def test_exact_data_bit_for_bit(gpu_ctx, i):
    case = so.CASES[i]
    x, w, b = so.exact_case(case)
    out_f32 = i in so.F32_OUT
    got = run_layer(gpu_ctx, x, w, b, case, out_f32)
    assert_same_values(got, exact_reference(i, out_f32), f"case {case} out_f32={out_f32}")
    if i not in so.F32_OUT:  # the accumulators themselves, before the rounding to f16
        assert_same_values(run_layer(gpu_ctx, x, w, b, case, True), exact_reference(i, True), f"case {case} f32 out")


def test_exact_data_every_tile_width_gives_the_same_bits(gpu_ctx):
    case = so.CASES[3]  # 20 x 36, 128 -> 128, pooled
    x, w, b = so.exact_case(case)
    for nt in (0, 1, 2, 4):
        got = run_layer(gpu_ctx, x, w, b, case[:7] + (nt,), False)
        assert_same_values(got, exact_reference(3, False), f"nt {nt}")


# ---- 2. rounding and special values ---------------------------------------------------------------------------------------
def test_rounding_and_special_values(gpu_ctx):
    from multimotionfusion_amd.superpoint import conv_f16
    H, W, C = 8, 16, 32
    x = np.zeros((H, W, C), np.float16)
    x[0, 0, :2] = 2048, 1    # 2049 -> 2048 (tie to even)
    x[0, 1, :2] = 2048, 3    # 2051 -> 2052
    x[0, 2, :2] = 65504, 15  # 65519 -> 65504
    x[0, 3, :2] = 65504, 16  # 65520 -> inf
    x[5, 9, 5] = np.nan
    w = np.zeros((C, C, 1, 1), np.float32)
    w[0, :2] = 1
    w[1, :2] = -1  # the negative sums: 0 under ReLU
    b = np.zeros(C, np.float32)
    for relu in (True, False):
        for out_f32 in (False, True):
            got = conv_f16(gpu_ctx, dev(x), w, b, relu=relu, pool=False, nt=1, out_f32=out_f32).cpu().numpy()
            want = so.layer_exact(x, w, b, relu, False, out_f32)
            assert_same_values(got, want, f"1x1 relu={relu} out_f32={out_f32}")
            nan = np.isnan(got)
            assert nan[5, 9].all() and nan.sum() == C  # the one pixel whose window holds the NaN, every channel
            if not out_f32:
                assert list(got[0, :4, 0].astype(np.float64)) == [2048.0, 2052.0, 65504.0, np.inf]
                assert list(got[0, :4, 1].astype(np.float64)) == ([0.0] * 4 if relu else [-2048.0, -2052.0, -65504.0, -np.inf])
            else:
                assert list(got[0, :4, 0]) == [2049.0, 2051.0, 65519.0, 65520.0]
    # 3x3: the nine outputs around the NaN, and the pooled cells over them; the pool's maximum of four
    rng = np.random.default_rng(3)
    x = rng.permutation(np.arange(H * W * C) % 64).reshape(H, W, C).astype(np.float16)  # integers 0..63
    x[5, 9, 5] = np.nan
    w = np.zeros((C, C, 3, 3), np.float32)
    w[np.arange(C), np.arange(C), 1, 1] = 1  # the centre tap alone: the layer copies its input
    got = conv_f16(gpu_ctx, dev(x), w, b, relu=True, pool=False, nt=1).cpu().numpy()
    assert_same_values(got, so.layer_exact(x, w, b, True, False, False), "3x3 copy")
    nan = np.isnan(got)
    assert nan[4:7, 8:11].all() and nan.sum() == 9 * C
    got = conv_f16(gpu_ctx, dev(x), w, b, relu=True, pool=True, nt=1).cpu().numpy()
    assert_same_values(got, so.layer_exact(x, w, b, True, True, False), "3x3 copy, pooled")
    nan = np.isnan(got)
    assert nan[2:4, 4:6].all() and nan.sum() == 4 * C  # rows 4..6, columns 8..10 lie in pooled cells (2..3, 4..5)
    clean = np.nan_to_num(x.astype(np.float32), nan=0.0)
    pooled = clean.reshape(H // 2, 2, W // 2, 2, C).max(axis=(1, 3))
    where = clean.reshape(H // 2, 2, W // 2, 2, C).transpose(0, 2, 4, 1, 3).reshape(H // 2, W // 2, C, 4).argmax(axis=3)
    assert set(np.unique(where[~nan])) == {0, 1, 2, 3}  # the maximum sits at each of the four places somewhere
    assert np.array_equal(got[~nan].astype(np.float32), pooled[~nan])


# ---- 3. random data -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_reference(i, out_f32):
    x, w, b = so.random_case(so.CASES[i])
    ref, _, T = so.layer(x, w, b, so.CASES[i][5], so.CASES[i][6], out_f32)
    return ref, T


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32out", "f16out"])
@pytest.mark.parametrize("i", range(len(so.CASES)), ids=CASE_IDS)
def test_random_data_within_the_tolerance(gpu_ctx, i, out_f32):
    case = so.CASES[i]
    x, w, b = so.random_case(case)
    got = run_layer(gpu_ctx, x, w, b, case, out_f32).astype(np.float64)
    ref, T = random_reference(i, out_f32)
    err = np.abs(got - ref)
    print("case", case, "out_f32", out_f32, "worst |got - ref| / T", float((err / T).max()), "worst |got - ref|", float(err.max()))
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (err <= T).all(), (int((err > T).sum()), float((err / T).max()))


# ---- 4. / 5. the network ----------------------------------------------------------------------------------------------------
SIZES = [(8, 8, 1), (48, 64, 1), (72, 104, 3), (120, 160, 3)]


@pytest.fixture(scope="module")
def nets(gpu_ctx, orc):
    from multimotionfusion_amd.superpoint import SuperPoint
    weights = orc.sp_random_weights(seed=4)
    f32 = SuperPoint(gpu_ctx, weights, max_width=160, max_height=120, max_keypoints=2048)
    f16 = SuperPoint(gpu_ctx, weights, max_width=160, max_height=120, max_keypoints=2048, precision="f16")
    yield f32, f16, weights
    f32.close(), f16.close()


def image(H, W, ch):
    rng = np.random.default_rng(H + W)
    return rng.integers(0, 256, (H, W) if ch == 1 else (H, W, ch), dtype=np.uint8)


def test_precision_is_a_property_of_the_object(nets):
    f32, f16, _ = nets
    assert f32.precision == "f32" and f16.precision == "f16"


@pytest.mark.parametrize("H,W,ch", SIZES[:3])
def test_conv1a_is_the_f32_result_rounded(nets, H, W, ch):
    f32, f16, _ = nets
    img = image(H, W, ch)
    got = f16.forwardPrefix(img, 1)
    want = so.conv1a_f16(f32.forwardPrefix(img, 1))
    assert got.dtype == np.float16 and got.shape == (H, W, 64)
    assert_same_values(got, want, "conv1a")
    assert np.count_nonzero(got) > got.size // 10


@pytest.mark.parametrize("H,W,ch", SIZES)
def test_the_network_is_its_layers(gpu_ctx, nets, H, W, ch):
    from multimotionfusion_amd.superpoint import conv_f16
    f32, f16, weights = nets
    img = image(H, W, ch)
    x = dev(f16.forwardPrefix(img, 1))
    pools = [True, False, True, False, True, False, False]
    for k in range(2, 9):  # conv1b ... conv4b
        w, b = weights[k - 1]
        x = conv_f16(gpu_ctx, x, w, b, relu=True, pool=pools[k - 2])
        assert_same_values(f16.forwardPrefix(img, k), x.cpu().numpy(), f"launch {k}")
    wh = np.concatenate([weights[8][0], weights[10][0]])
    bh = np.concatenate([weights[8][1], weights[10][1]])
    head = conv_f16(gpu_ctx, x, wh, bh, relu=True, pool=False)
    assert_same_values(f16.forwardPrefix(img, 9), head.cpu().numpy(), "launch 9")
    semi = conv_f16(gpu_ctx, head[:, :, :256].contiguous(), weights[9][0], weights[9][1], relu=False, out_f32=True)
    desc = conv_f16(gpu_ctx, head[:, :, 256:].contiguous(), weights[11][0], weights[11][1], relu=False, out_f32=True)
    # the unchanged tail, run by the f32 object on these maps
    f32.setMaps(W, H, semi=semi, desc=desc, normalize_desc=True)
    want = [f32.download(which, W, H) for which in range(3)]
    got = f16.forward(img)
    again = f16.forward(img)
    for g, a, w_, what in zip(got, again, want, ("logits", "coarse descriptors", "heat map")):
        assert_bit_equal(g, w_, what)
        assert_bit_equal(a, g, what + ", second forward")
    assert_bit_equal(got[0], semi.cpu().numpy(), "logits = convPb's f32 output")


def test_create_ex_with_f32_is_create(gpu_ctx, nets):
    from multimotionfusion_amd.superpoint import SuperPoint
    f32, f16, weights = nets
    ex = SuperPoint(gpu_ctx, weights, max_width=160, max_height=120, max_keypoints=2048, precision=0)
    assert ex.precision == "f32"
    img = image(72, 104, 3)
    for g, w_ in zip(ex.forward(img), f32.forward(img)):
        assert_bit_equal(g, w_, "create_ex(..., MMF_SP_F32)")
    for k in (1, 5, 9):
        assert_bit_equal(ex.forwardPrefix(img, k), f32.forwardPrefix(img, k), f"prefix {k}")
    differs = any(not np.array_equal(a, b) for a, b in zip(f16.forward(img), f32.forward(img)))
    assert differs  # (and the f16 object is another computation)
    ex.close()


# ---- 6. post-processing untouched ---------------------------------------------------------------------------------------------
def test_post_processing_is_the_f32_path_on_the_same_maps(nets):
    f32, f16, _ = nets
    H, W = 120, 160
    img = image(H, W, 3)
    xy, conf, desc = f16.keypoints(img)
    semi, cdesc, heat = f16.forward(img)
    f16.getFeaturesDevice(img)
    d_xy, d_conf, d_desc, status = f16.lastFeatures()
    assert status == 0 and len(xy) > 20
    f32.setMaps(W, H, semi=semi, desc=cdesc)
    assert_bit_equal(f32.download(2, W, H), heat, "heat map")
    s_xy, s_conf, s_desc = f32.select()
    assert_bit_equal(xy, s_xy, "keypoints")
    assert_bit_equal(conf, s_conf, "confidences")
    assert_bit_equal(desc, s_desc, "descriptors")
    f32.selectDevice()
    e_xy, e_conf, e_desc, e_status = f32.lastFeatures()
    assert e_status == 0
    assert_bit_equal(d_xy, e_xy, "keypoints, device path")
    assert_bit_equal(d_conf, e_conf, "confidences, device path")
    assert_bit_equal(d_desc, e_desc, "descriptors, device path")
    assert_bit_equal(d_xy, xy, "device path = host path")


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, nets):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.superpoint import SuperPoint, conv_f16
    _, _, weights = nets
    with pytest.raises(MmfError) as e:
        SuperPoint(gpu_ctx, weights, max_width=64, max_height=48, precision=2)
    assert e.value.status == -1
    for bad in (1e5, np.inf, np.nan):
        w = [(a.copy(), b.copy()) for a, b in weights]
        w[5][0][3, 2, 1, 0] = bad
        with pytest.raises(MmfError) as e:
            SuperPoint(gpu_ctx, w, max_width=64, max_height=48, precision="f16")
        assert e.value.status == -1, bad
        if np.isfinite(bad):
            SuperPoint(gpu_ctx, w, max_width=64, max_height=48).close()  # an f32 object takes it, as before
    x = torch.zeros((8, 16, 48), device="cuda", dtype=torch.float16)
    with pytest.raises(MmfError):
        conv_f16(gpu_ctx, x, np.zeros((32, 48, 3, 3), np.float32), np.zeros(32, np.float32))  # cin % 32
    x = torch.zeros((7, 16, 32), device="cuda", dtype=torch.float16)
    with pytest.raises(MmfError):
        conv_f16(gpu_ctx, x, np.zeros((32, 32, 3, 3), np.float32), np.zeros(32, np.float32), pool=True)  # odd height
    x = torch.zeros((8, 16, 32), device="cuda", dtype=torch.float16)
    with pytest.raises(MmfError):
        conv_f16(gpu_ctx, x, np.full((32, 32, 1, 1), 1e5, np.float32), np.zeros(32, np.float32))  # rounds to inf
    _, f16, _ = nets
    with pytest.raises(IndexError):
        f16.forwardPrefix(image(8, 8, 1), 10)  # the mirror knows nine launches
    img, out = dev(image(8, 8, 1)), np.empty(8 * 8 * 64, np.float16)
    for layers, nbytes in ((0, out.nbytes), (10, out.nbytes), (1, out.nbytes - 2)):
        assert f16.lib.mmf_debug_superpoint_forward_prefix(f16.handle, img.data_ptr(), 8, 8, 1, layers, out.ctypes.data, nbytes) == -1
