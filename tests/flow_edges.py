"""Edge cases of the optical-flow engine (csrc/flow_kernels.hpp), shared by tests/test_flow_edges_oracle.py
(CPU: every case reaches the edge it is named for, on the oracle alone) and tests/test_gpu_flow_edges.py (the device equals
the oracle bit for bit on every one of them).  numpy and tests/flow_oracle.py only.

A case is a `Case(name, prev, nxt, over, claim)`: two uint8 RGB frames, the configuration's overrides and a dict of what the
case promises beyond "the device equals the oracle" -- every number a lower bound on a pixel count, taken over all
iterations, that test_flow_edges_oracle.py asserts and whose observed value is written in that file:
  neg_det        pixels with det <= -1e-3: idet is negative
  small_neg_det  pixels with -1e-3 < det < 0
  det_zero       pixels with det == 0 exactly
  idet_1000      pixels with idet == 1000.0f (det == 0, or so small that the double sum rounds to it)
  neg_zero, pos_zero   flow components that are -0.0, +0.0
  beyond_int     components of the last flow with |value| > 2^31
  flow_above_1000   components of any iteration's flow with |value| > 1000
  subnormal      subnormal values in R0, R1, M and the flows
  all_zero       R0, R1, M, every flow, magnitude and motion are +0.0 everywhere
  tiny_M         M is not zero but below 1e-9 everywhere: the rounding residue of the expansion of a constant
  f64_bounded    the float64 restatement stays below F64_FACTOR image diagonals where the float32 one explodes
  corner, x_m1, x_w1, y_m1, y_h1   warp positions of iterations 2 and later: (x1f, y1f) == (W-2, H-2), the last inside
                 one, and the first outside ones x1f == -1, x1f == W-1, y1f == -1, y1f == H-1
  corner_moved   ... (W-2, H-2) reached by another pixel than (W-2, H-2) itself
  frac0          inside pixels of a non-zero flow whose two fractions are exactly 0, in iterations 2 and later
  tie_even, tie_odd, rem7, rem9, sum_max, sum_zero   div 4: channel sums s of a 4 x 4 block with s & 15 == 8 at even and odd
                 s >> 4, s & 15 == 7 and 9, s == 4080, s == 0
  rem2           div 2: the smallest count over the four values of s & 3
  gray_on, gray_under   grey sums c0*1868 + c1*9617 + c2*4899 + 8192 whose low 14 bits are 0 (a step just taken) and 16383
                 (one short of it)
  size           the flow image's (W, H)
Under div 1 a frame of three equal channels c has grey value c ((c*16384 + 8192) >> 14 == c): such a case draws its flow
image directly."""
from collections import namedtuple

import numpy as np

import flow_oracle as fo
from test_gpu_flow import frames

Case = namedtuple("Case", "name prev nxt over claim")
F32 = np.float32
SMALL = dict(div=1, winsize=4, poly_n=5, poly_sigma=1.1)   # the cancelling determinants: a 5 x 5 window
TINY = dict(div=1, winsize=2, poly_n=3, poly_sigma=1.1)    # the smallest window and expansion
WIDE = dict(poly_n=7, poly_sigma=1.5, winsize=33)          # the largest halo and the largest window
W1, H1 = 37, 23


def rgb_of(gray):
    """three equal channels: under div 1 the grey image is `gray` itself"""
    g = np.asarray(gray)
    assert g.dtype == np.uint8
    return np.repeat(g[..., None], 3, axis=-1)


def grid(w=W1, h=H1):
    y, x = np.mgrid[0:h, 0:w]
    return x, y


# ---- 1: a determinant that cancels ----------------------------------------------------------------------------------------
def sinusoid(u):
    return np.rint(127.5 + 127.5 * np.sin(0.5 * u)).astype(np.uint8)


def bands(u):
    return (((u // 4) % 2) * 255).astype(np.uint8)


def cancelling_cases():
    """one-dimensional structure along a diagonal: g11 g22 and g12^2 agree to rounding"""
    x, y = grid()
    out = []
    for tag, u in (("diag", x + y), ("anti", x - y + H1)):
        for it in (3, 10):
            # the sinusoid: det of either small sign, growth by about ten per iteration; the bands: det <= -1e-3 in the
            # first iteration (and the second of the anti-diagonal), flows above 1000 in the second, no small negative det
            sin = dict(neg_det=20, small_neg_det=50, neg_zero=4, f64_bounded=True)
            if it == 10:
                sin.update(neg_det=200, small_neg_det=150, beyond_int=1)
            out.append(Case(f"cancel_sin_{tag}_it{it}", rgb_of(sinusoid(u.astype(np.float64))), rgb_of(sinusoid(u - 1.5)),
                            dict(SMALL, iterations=it), sin))
            out.append(Case(f"cancel_bands_{tag}_it{it}", rgb_of(bands(u)), rgb_of(bands(u - 2)), dict(SMALL, iterations=it),
                            dict(neg_det=30, neg_zero=12, flow_above_1000=1, f64_bounded=True)))
    return out


F64_FACTOR = 8  # the float64 flows of this group reach 181 pixels = 4.2 diagonals of 43.6 at most (cancel_sin_anti)


# ---- 2: exact zeros -------------------------------------------------------------------------------------------------------
ZW, ZH = 40, 12  # two tiles wide: the step edge stands on the boundary between them


def zero_cases():
    x, y = grid(ZW, ZH)
    rng = np.random.default_rng(21)
    noisy = rng.integers(0, 256, (ZH, ZW), dtype=np.uint8)
    flat = np.full((ZH, ZW), 131, np.uint8)
    pow2 = np.full((ZH, ZW), 128, np.uint8)
    step = lambda at: np.where(x >= at, 156, 0).astype(np.uint8)
    dot = lambda px, py, ground: np.where((x == px) & (y == py), 255, ground).astype(np.uint8)
    ramp = lambda s: np.clip(7 * (x - s), 0, 255).astype(np.uint8)
    it2 = dict(TINY, iterations=2)
    n = 2 * ZW * ZH  # pixels times iterations
    return [
        # 128 is a power of two: the expansion of a constant leaves no rounding residue, every stage behind it is +0.0
        Case("zero_constant_128", rgb_of(pow2), rgb_of(pow2), it2, dict(all_zero=True, det_zero=n, idet_1000=n, pos_zero=2 * n)),
        # 131: R[2], R[3] keep a residue of 8e-6, M of 6e-11, det of 1e-21: idet still rounds to 1000.0f, the flow is +0.0
        Case("zero_constant_131", rgb_of(flat), rgb_of(flat), it2, dict(tiny_M=True, idet_1000=n, pos_zero=2 * n)),
        Case("zero_black_to_white", rgb_of(np.zeros((ZH, ZW), np.uint8)), rgb_of(np.full((ZH, ZW), 255, np.uint8)), it2,
             dict(tiny_M=True, idet_1000=n, pos_zero=2 * n)),
        Case("zero_identical_noise", rgb_of(noisy), rgb_of(noisy), it2, dict(pos_zero=700)),
        Case("zero_step", rgb_of(step(32)), rgb_of(step(33)), it2, dict(det_zero=700, neg_zero=6, frac0=20)),
        Case("zero_impulse", rgb_of(dot(17, 5, 0)), rgb_of(dot(19, 6, 0)), it2, dict(det_zero=600, frac0=6)),
        # the reference's sigma: g[2..4] are 2e-10, 2e-22 and a subnormal, the impulse's skirt underflows
        Case("zero_impulse_sigma03", rgb_of(dot(17, 5, 128)), rgb_of(dot(19, 6, 128)), dict(div=1, winsize=2), dict(neg_zero=25, subnormal=35)),
        Case("zero_ramp", rgb_of(ramp(0)), rgb_of(ramp(1)), it2, dict(det_zero=48, neg_zero=16, frac0=100)),
    ]


# ---- 3: the warp's boundaries ---------------------------------------------------------------------------------------------
def warp_cases():
    """noise that slides by 12 pixels: the 3 x 3 window follows whatever it finds, flows of several pixels either way"""
    rng = np.random.default_rng(48)  # (of the seeds 30..59 the one that sends most pixels to the last inside position)
    big = rng.integers(0, 256, (H1, W1 + 12), dtype=np.uint8)
    claim = dict(corner=3, corner_moved=3, x_m1=9, x_w1=20, y_m1=10, y_h1=20)
    return [Case("warp_noise_shift12", rgb_of(big[:, 12:]), rgb_of(big[:, :W1]), dict(TINY, iterations=3), claim)]


# ---- 4: the integer front end ---------------------------------------------------------------------------------------------
def blocks_of_sums(s, div):
    """a frame whose div x div block (by, bx) has channel sums s[by, bx, c]: every pixel sum // div^2, the first sum % div^2
    of a block (row-major) one more"""
    s = np.asarray(s, np.int64)
    n = div * div
    assert s.min() >= 0 and s.max() <= 255 * n
    k = np.arange(n).reshape(div, div)
    px = s[:, None, :, None, :] // n + (k[None, :, None, :, None] < (s[:, None, :, None, :] % n))
    return px.reshape(s.shape[0] * div, s.shape[1] * div, 3).astype(np.uint8)


def gray_step_triples(low, count, seed):
    """`count` channel triples whose grey sum has the low 14 bits `low`, drawn from all of them by a seeded choice"""
    c = np.arange(256, dtype=np.int32)
    v = c[:, None, None] * 1868 + c[None, :, None] * 9617 + c[None, None, :] * 4899 + 8192
    hit = np.argwhere((v & 16383) == low)
    return hit[np.random.default_rng(seed).choice(len(hit), count, replace=False)].astype(np.uint8)


FW, FH = 16, 12  # the front end's flow image


def front_end_cases():
    rng = np.random.default_rng(44)
    by, bx = np.mgrid[0:FH, 0:FW]
    # div 4, previous frame: every channel sum on a tie, s >> 4 even and odd in a checkerboard (the channels shifted against
    # each other); next frame: remainders 7 and 9, a row of 4080 and a row of 0
    q = 2 * rng.integers(0, 127, (FH, FW, 3)) + ((bx + by)[..., None] + np.arange(3)) % 2
    ties = blocks_of_sums(16 * q + 8, 4)
    s = 16 * rng.integers(0, 255, (FH, FW, 3)) + np.where((bx + by) % 2 == 0, 7, 9)[..., None]
    s[0], s[1] = 4080, 0
    near = blocks_of_sums(s, 4)
    # div 2: every remainder, in every channel
    s2 = 4 * rng.integers(0, 255, (FH, FW, 3)) + ((bx + 2 * by)[..., None] + np.arange(3)) % 4
    two_a, two_b = blocks_of_sums(s2, 2), blocks_of_sums((s2 + 1 + 4 * (s2 < 1000)) % 1021, 2)
    # div 1: grey sums on and one short of a rounding step; white and black among them
    on, under = gray_step_triples(0, FW * FH, 45), gray_step_triples(16383, FW * FH, 46)
    on[0], on[1] = 255, 0
    one = dict(iterations=1)
    return [
        Case("front_div4", ties, near, dict(one), dict(tie_even=200, tie_odd=200, rem7=150, rem9=150, sum_max=48, sum_zero=48)),
        Case("front_div2", two_a, two_b, dict(one, div=2), dict(rem2=200)),
        Case("front_gray", on.reshape(FH, FW, 3), under.reshape(FH, FW, 3), dict(one, div=1), dict(gray_on=150, gray_under=150)),
    ]


# ---- 5: geometry ----------------------------------------------------------------------------------------------------------
GEOMETRY = [
    ((8, 8), dict(WIDE)),
    ((8, 8), dict(div=1)),
    ((8, 8), dict(div=2)),
    ((32, 8), dict()),
    ((64, 16), dict()),
    ((8, 41), dict(WIDE)),
    ((70, 8), dict(WIDE)),
    ((37, 23), dict(iterations=10)),
]


def geometry_cases():
    """the blocky sliding texture of test_gpu_flow.py at the sizes and settings it leaves out"""
    out = []
    for (w, h), over in GEOMETRY:
        div = over.get("div", fo.DEFAULTS["div"])
        a, b = frames(w * div, h * div, 2, seed=w * 100 + h)
        tag = "-".join(f"{k}{v}" for k, v in over.items()) or "reference"
        out.append(Case(f"geometry_{w}x{h}_{tag}", a, b, over, dict(size=(w, h), moves=True)))
    return out


_cache = {}


def all_cases():
    """every case by name, built once and never modified"""
    if not _cache:
        cases = cancelling_cases() + zero_cases() + warp_cases() + front_end_cases() + geometry_cases()
        for c in cases:
            c.prev.setflags(write=False), c.nxt.setflags(write=False)
            cfg = fo.config(**c.over)
            assert c.prev.shape == c.nxt.shape and c.prev.dtype == c.nxt.dtype == np.uint8 and c.prev.shape[2] == 3, c.name
            assert c.prev.shape[0] % cfg["div"] == 0 and c.prev.shape[1] % cfg["div"] == 0, c.name
            assert c.prev.shape[1] // cfg["div"] <= 70 and c.prev.shape[0] // cfg["div"] <= 41, c.name
        assert len({c.name for c in cases}) == len(cases)
        _cache.update((c.name, c) for c in cases)
    return _cache


def case(name):
    return all_cases()[name]


def flow_size(c):
    div = fo.config(**c.over)["div"]
    return c.prev.shape[1] // div, c.prev.shape[0] // div


NAMES = list(all_cases())
SEQUENCE = ("cancel_sin_diag_it10", "zero_step")  # run as frames 0, 1, 0 through next()
CHAINED = "cancel_bands_diag_it3"  # the flow handed to the flow-CRF inference
CHAINED_SEED = 5


def chained_scene(flow, motion):
    """(scene, configuration, oracle result) of the flow-CRF inference (tests/flowcrf_oracle.py) on a two-model scene of the
    flow image's size whose flow and motion are replaced by the given ones"""
    import flowcrf_oracle as fc
    h, w = motion.shape
    sc = fc.make_scene(w, h, 2, False, CHAINED_SEED, edge_tracks=False)
    assert sc["flow"].shape == flow.shape and sc["flow"].dtype == flow.dtype == F32 and sc["motion"].shape == motion.shape
    sc["flow"], sc["motion"] = flow, motion
    cfg = fc.config()
    return sc, cfg, fc.run_scene(sc, cfg)
