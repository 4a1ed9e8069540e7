"""CPU: the optical-flow engine's host side and its oracle (tests/flow_oracle.py).  The library's tables
against Python's double computation, the configurations it refuses before it touches a device, and the oracle against the
truth: frames whose motion is known."""
import ctypes as C

import numpy as np
import pytest

import flow_oracle as fo

F32 = np.float32


def lib():
    from multimotionfusion_amd import _capi
    return _capi.load()


@pytest.mark.parametrize("n,sigma", [(5, 0.3), (5, 1.1), (7, 1.5)])
def test_the_librarys_tables_agree_with_the_double_computation_to_one_ulp(n, sigma):
    """g, xg, xxg and {ig11, ig03, ig33, ig55} as the kernels read them (float32) against tests/flow_oracle.tables (numpy
    float64, the 6 x 6 inverse by LAPACK; the library writes the inverse out): at most one float32 ulp apart, subnormal
    entries included (g[4] at sigma 0.3 is one; g[5] rounds to 0)."""
    from multimotionfusion_amd.flow import make_tables
    got = make_tables(n, sigma)
    want = fo.tables(n, sigma)
    for name, a, b in zip(("g", "xg", "xxg", "ig"), got, want):
        assert a.dtype == F32 and a.shape == b.shape, name
        r = b.astype(F32)
        ulp = np.maximum(np.spacing(np.abs(r)), np.spacing(F32(0)))
        assert np.all(np.abs(a.astype(np.float64) - b) <= ulp.astype(np.float64)), (name, a, b)
    assert got[0][0] > 0 and abs(float(got[0][0] + 2 * got[0][1:].sum()) - 1) < 1e-6
    assert got[3][0] > 0 and got[3][1] < 0 and got[3][2] > 0 and got[3][3] > 0


REFUSALS = [
    ("levels", dict(levels=2), 640, 480),
    ("levels 0", dict(levels=0), 640, 480),
    ("div 3", dict(div=3), 640, 480),
    ("div 0", dict(div=0), 640, 480),
    ("div 8", dict(div=8), 640, 480),
    ("width", dict(), 642, 480),
    ("height", dict(div=2), 640, 481),
    ("under 8 x 8: width", dict(), 28, 480),
    ("under 8 x 8: height", dict(div=2), 640, 14),
    ("winsize 1", dict(winsize=1), 640, 480),
    ("winsize 34", dict(winsize=34), 640, 480),
    ("poly_n 2", dict(poly_n=2), 640, 480),
    ("poly_n 8", dict(poly_n=8), 640, 480),
    ("iterations 0", dict(iterations=0), 640, 480),
    ("iterations 11", dict(iterations=11), 640, 480),
    ("poly_sigma 0", dict(poly_sigma=0.0), 640, 480),
    ("poly_sigma < 0", dict(poly_sigma=-1.0), 640, 480),
    ("poly_sigma nan", dict(poly_sigma=float("nan")), 640, 480),
]


@pytest.mark.parametrize("what,over,w,h", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_create_refuses_before_it_touches_a_device(what, over, w, h):
    """MMF_ERR_INVALID (-1) with the function's name in mmf_last_error; the check comes before the context is looked at, so
    it is the same on a machine without a device (the context here is NULL)."""
    from multimotionfusion_amd.flow import FlowConfig
    cfg = FlowConfig(**over)
    h_out = C.c_void_p()
    rc = lib().mmf_flow_create(None, w, h, C.byref(cfg.c), C.byref(h_out))
    assert rc == -1 and not h_out.value, what
    assert b"mmf_flow_create" in lib().mmf_last_error(), lib().mmf_last_error()


def test_defaults_are_the_references_and_pass_the_check():
    from multimotionfusion_amd.flow import FlowConfig
    cfg = FlowConfig()
    assert (cfg.div, cfg.levels, cfg.winsize, cfg.iterations, cfg.poly_n) == (4, 1, 20, 2, 5)
    assert F32(cfg.poly_sigma) == F32(0.3)
    h_out = C.c_void_p()
    # a valid configuration gets as far as the context: NULL is refused as a null argument, still without a device
    assert lib().mmf_flow_create(None, 640, 480, C.byref(cfg.c), C.byref(h_out)) == -1
    assert b"null argument" in lib().mmf_last_error()
    assert lib().mmf_flow_default_config(None) == -1 and b"mmf_flow_default_config" in lib().mmf_last_error()
    with pytest.raises(TypeError):
        FlowConfig(pyramid=3)


# ---- truth --------------------------------------------------------------------------------------------------------------
W_FLOW, H_FLOW = 72, 56  # the flow image; the interior (further than m + poly_n = 15 from an edge) is 42 x 26


def texture(X, Y, phase=0.0):
    """an analytic multi-sinusoid RGB texture at full-resolution coordinates (float64 arrays) -> uint8 [.., 3]; wavelengths of
    80 to 200 frame pixels (20 to 50 flow-image pixels at div 4), every direction present in every channel"""
    def ch(a, b, c):
        v = (np.sin(2 * np.pi * (X / a + Y / (1.7 * a)) + phase) + np.sin(2 * np.pi * (Y / b - X / (2.3 * b)) + 1.0 + phase)
             + 0.7 * np.sin(2 * np.pi * (X + Y) / c + 2.0))
        return 128.0 + 45.0 * v
    rgb = np.stack([ch(110.0, 90.0, 200.0), ch(130.0, 80.0, 170.0), ch(95.0, 120.0, 150.0)], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def shifted_pair(fx, fy, div=4):
    """prev(y, x) = next(y + fy, x + fx) in flow-image pixels: the texture evaluated at coordinates shifted by div * flow"""
    Y, X = np.mgrid[0:H_FLOW * div, 0:W_FLOW * div].astype(np.float64)
    return texture(X, Y), texture(X - div * fx, Y - div * fy)


def interior_error(flow, fx, fy, cfg):
    b = cfg["winsize"] // 2 + cfg["poly_n"]
    d = flow[b + 1:-(b + 1), b + 1:-(b + 1)].astype(np.float64) - np.array([fx, fy])
    return float(np.median(np.sqrt((d * d).sum(axis=-1))))


# median endpoint error of the float64 restatement on these inputs, measured; the bound is twice that, rounded up
TRUTH = [
    ((1.0, 0.0), 0.006),
    ((0.0, -0.75), 0.016),
    ((0.6, 0.4), 0.021),
]


@pytest.mark.parametrize("motion,bound", TRUTH, ids=[str(t[0]) for t in TRUTH])
def test_the_oracle_finds_a_known_translation(motion, bound):
    """The convention is prev(y, x) ~ next(y + flow.y, x + flow.x).  Median endpoint error over the interior (further than
    m + poly_n from an edge), reference settings (div 4, winsize 20, two iterations, poly_n 5, sigma 0.3), flow image 72 x 56.
    Measured (float64 restatement / float32 oracle with the library's tables), in flow-image pixels:
        (1.0, 0)    0.00255 / 0.00255
        (0, -0.75)  0.00780 / 0.00780
        (0.6, 0.4)  0.01042 / 0.01042
    The bound is twice the float64 figure rounded up to the next thousandth, and stays below half the motion's magnitude
    (0.5, 0.375, 0.36): a zero flow, a wrong sign or swapped axes miss it by far."""
    fx, fy = motion
    assert bound < 0.5 * float(np.hypot(fx, fy))
    cfg = fo.config()
    from multimotionfusion_amd.flow import make_tables
    prev, nxt = shifted_pair(fx, fy)
    out = fo.pair(prev, nxt, cfg, tab=make_tables(cfg["poly_n"], cfg["poly_sigma"]))
    err = interior_error(out["flow"], fx, fy, cfg)
    print(f"motion {motion}: median endpoint error {err:.4f} (bound {bound})")
    assert err <= bound, (motion, err)
    # and the flipped conventions do miss it
    for wrong in ((-fx, -fy), (fy, fx), (0.0, 0.0)):
        if wrong != (fx, fy):
            assert interior_error(out["flow"], wrong[0], wrong[1], cfg) > bound


def test_a_moving_rectangle_stands_out_of_a_static_ground():
    """a textured rectangle moving by (2, 1) flow-image pixels over a static textured ground: the mean `motion` inside the
    rectangle exceeds the mean outside"""
    div = 4
    Y, X = np.mgrid[0:H_FLOW * div, 0:W_FLOW * div].astype(np.float64)
    ground = texture(X, Y)
    x0, x1, y0, y1, sx, sy = 96, 192, 64, 152, 8, 4
    prev, nxt = ground.copy(), ground.copy()
    prev[y0:y1, x0:x1] = texture(1.9 * X, 1.9 * Y, 1.3)[y0:y1, x0:x1]
    nxt[y0 + sy:y1 + sy, x0 + sx:x1 + sx] = texture(1.9 * (X - sx), 1.9 * (Y - sy), 1.3)[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    out = fo.pair(prev, nxt, fo.config())
    inside = np.zeros((H_FLOW, W_FLOW), bool)
    inside[y0 // div:y1 // div, x0 // div:x1 // div] = True
    m_in, m_out = float(out["motion"][inside].mean()), float(out["motion"][~inside].mean())
    print(f"motion inside {m_in:.4f}, outside {m_out:.4f}")
    assert out["motion"].min() >= 0 and out["motion"].max() <= 1
    assert m_in > m_out and m_in > 0.05


def test_float32_and_float64_restatements_agree_on_a_frame_pair():
    """the same text at two precisions: the float32 oracle's flow stays within 1e-3 of the float64 one on a textured pair
    (the rounding, not the algorithm, is all that separates them)"""
    prev, nxt = shifted_pair(0.6, 0.4)
    cfg = fo.config()
    a = fo.pair(prev, nxt, cfg, dt=F32)["flow"]
    b = fo.pair(prev, nxt, cfg, dt=np.float64)["flow"]
    assert a.dtype == F32 and b.dtype == np.float64
    assert float(np.abs(a - b).max()) < 1e-3
