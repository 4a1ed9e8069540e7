"""Edge cases of the photometric passes (csrc/track_kernels.hpp: residual_block4, rgb_step_kernel, so3_kernel;
csrc/gn_fused.hpp: gn_pixel_waves), shared by tests/test_photo_edges_oracle.py (CPU) and tests/test_gpu_photo_edges.py.
numpy and the oracle only.  A builder that needs a tie, an equality or a sign constructs it (or finds it by a seeded
search) with the oracle's own float32 arithmetic and asserts it, so a case never claims a property its inputs do not have.

The per-pixel decision is Core/Cuda/reduce.cu:773-812; `restate` below is a plain restatement of that text (explicit loops
over the clipped window, no bit tricks) and `VARIANTS` are deliberately wrong versions of it.

A stand-alone case is a `Case` of the inputs of cudafuncs.computeRgbResidual plus `claim`, a dict of what the case promises
beyond "the device equals the oracle":
  count      the number of correspondences          sumsq   the sum of diff^2
  valid      bool [rows, cols]: exactly these pixels have a correspondence (worked out from the geometry of the case)
  zero       {(x, y): (u0, v0)}: where these pixels land
  invalid    [(x, y)]: pixels without one           oob     the whole case has none because every warp leaves the image
  exact64    [(td1, d0, delta, side)]: td1 - d0 evaluated in float64 is <, == or > delta in magnitude as `side` says
  ties       [(x, y, qx, qy)]: the warp's quotients (float64, exact) of these pixels

All arrays are read-only and built once per session (functools.lru_cache).
"""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name family min_scale dIdx dIdy last_depth next_depth last_image next_image max_depth_delta kt krkinv claim")

f32 = np.float32
RECORD = np.dtype([("zero_x", "<i2"), ("zero_y", "<i2"), ("one_x", "<i2"), ("one_y", "<i2"), ("diff", "<f4"), ("valid", "u1"),
                   ("pad", "u1", 3)])  # mmf_dataterm / DataTerm, 16 bytes
assert RECORD.itemsize == 16
INT_MAX = 2 ** 31 - 1
DELTA = f32(0.0625)
DELTA_SHIPPED = f32(0.07)  # RGBDOdometry.cpp:33
CHAIN_MIN_SCALES = (1600.0, 576.0, 64.0)  # (minimumGradientMagnitudes / sobelScale)^2 of levels 0, 1, 2
EYE = np.eye(3, dtype=f32)
ZERO3 = np.zeros(3, f32)
FAMILIES = ("window", "border", "gate", "depth", "warp", "last")


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def textured(cols, rows, seed):
    """next and last image, both non-zero everywhere, |next - last| varied so that a wrong address shows in `diff`"""
    y, x = np.mgrid[0:rows, 0:cols]
    nxt = (1 + (x * 37 + y * 101 + seed * 7) % 255).astype(np.uint8)
    last = (1 + (x * 53 + y * 29 + seed * 11 + 5) % 255).astype(np.uint8)
    return nxt, last


def base(cols, rows, seed=0):
    """inputs under which every pixel of the band x < cols - 5, y < rows - 1 has a correspondence with itself"""
    nxt, last = textured(cols, rows, seed)
    return dict(min_scale=f32(25.0), dIdx=np.full((rows, cols), 3, np.int16), dIdy=np.full((rows, cols), 4, np.int16),
                last_depth=np.ones((rows, cols), f32), next_depth=np.ones((rows, cols), f32), last_image=last, next_image=nxt,
                max_depth_delta=DELTA, kt=ZERO3.copy(), krkinv=EYE.copy())


def make(name, family, d, claim):
    arrays = {k: frozen(np.asarray(d[k], {"dIdx": np.int16, "dIdy": np.int16, "last_image": np.uint8, "next_image": np.uint8}.get(k, f32)))
              for k in ("dIdx", "dIdy", "last_depth", "next_depth", "last_image", "next_image", "kt", "krkinv")}
    return Case(name=name, family=family, min_scale=f32(d["min_scale"]), max_depth_delta=f32(d["max_depth_delta"]), claim=claim, **arrays)


def band(cols, rows):
    m = np.zeros((rows, cols), bool)
    m[:max(rows - 1, 0), :max(cols - 5, 0)] = True
    return m


def inputs(case):
    """the positional arguments of orc.rgb_residual after min_scale ... in its order"""
    return (case.min_scale, case.dIdx, case.dIdy, case.last_depth, case.next_depth, case.last_image, case.next_image,
            case.max_depth_delta, case.kt, case.krkinv)


# ---- the restatement and its wrong variants ---------------------------------------------------------------------------------
VARIANTS = ("window 3x3", "window rows i-2..i+2", "window not clipped", "x < cols - 4", "y < rows", "mTwo > min_scale",
            "round half up", "truncate", "u0 <= cols", "v0 < rows - 1", "d0 >= 0", "|td1 - d0| < delta", "last_image test dropped",
            "NaN test on d1 dropped")
# `fabsf(NaN - d0) <= delta` is false whatever d0 is, and td1 = d1 * (...) + kt.z is NaN whenever d1 is: the reference's
# isnan(d1) test (reduce.cu:806) decides nothing that :816 would not decide.  No input tells this variant from the text.
UNOBSERVABLE = ("NaN test on d1 dropped",)


def rn(q):
    """__float2int_rn: nearest, ties to even; NaN -> 0; saturating"""
    if q != q:
        return 0
    if q >= 2.0 ** 31:
        return INT_MAX
    if q <= -2.0 ** 31:
        return -2 ** 31
    return int(np.rint(np.float64(q)))


def half_up(q):
    return 0 if q != q else int(np.clip(np.floor(np.float64(q) + 0.5), -2.0 ** 31, INT_MAX))


def trunc(q):
    return 0 if q != q else int(np.clip(np.trunc(np.float64(q)), -2.0 ** 31, INT_MAX))


def restate(case, variant=None):
    """reduce.cu:773-836 in plain loops: (records [rows, cols] of RECORD, count, sum of diff^2).  `variant`: one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    v = variant
    rows, cols = case.next_image.shape
    K, kt = case.krkinv.reshape(9), case.kt
    rec = np.zeros((rows, cols), RECORD)
    count = sumsq = 0
    rounding = half_up if v == "round half up" else trunc if v == "truncate" else rn
    with np.errstate(all="ignore"):
        for i in range(rows):
            for j0 in range(cols):
                if not (j0 < cols - (4 if v == "x < cols - 4" else 5) and i < rows - (0 if v == "y < rows" else 1)):  # :773
                    continue
                us = range(i - 1, i + 2) if v == "window 3x3" else range(i - 2, i + 3) if v == "window rows i-2..i+2" else range(i - 2, i + 2)
                vs = range(j0 - 1, j0 + 2) if v == "window 3x3" else range(j0 - 2, j0 + 2)
                ok = True
                for u in us:  # :777-787
                    for w in vs:
                        inside = 0 <= u < rows and 0 <= w < cols
                        if not inside:
                            ok = ok and v != "window not clipped"  # (unclipped: what lies outside the image is not > 0)
                        else:
                            ok = ok and case.next_image[u, w] > 0
                if not ok:
                    continue
                valx, valy = int(case.dIdx[i, j0]), int(case.dIdy[i, j0])
                mTwo = f32(valx * valx + valy * valy)  # :797
                if not (mTwo > case.min_scale if v == "mTwo > min_scale" else mTwo >= case.min_scale):
                    continue
                d1 = case.next_depth[i, j0]
                if d1 != d1 and v != "NaN test on d1 dropped":  # :806
                    continue
                x, y = f32(j0), f32(i)
                td1 = f32(d1 * f32(f32(f32(K[6] * x) + f32(K[7] * y)) + K[8])) + kt[2]  # :808
                u0 = rounding(f32(f32(d1 * f32(f32(f32(K[0] * x) + f32(K[1] * y)) + K[2])) + kt[0]) / td1)
                v0 = rounding(f32(f32(d1 * f32(f32(f32(K[3] * x) + f32(K[4] * y)) + K[5])) + kt[1]) / td1)
                if not (u0 >= 0 and v0 >= 0 and (u0 <= cols if v == "u0 <= cols" else u0 < cols) and
                        v0 < (rows - 1 if v == "v0 < rows - 1" else rows)):  # :812
                    continue
                ug = min(u0, cols - 1)  # (only the `u0 <= cols` variant ever reads beside the image)
                d0 = case.last_depth[v0, ug]
                li = int(case.last_image[v0, ug])
                if not ((d0 >= 0 if v == "d0 >= 0" else d0 > 0) and
                        (abs(f32(td1 - d0)) < case.max_depth_delta if v == "|td1 - d0| < delta" else abs(f32(td1 - d0)) <= case.max_depth_delta) and
                        (li != 0 or v == "last_image test dropped")):  # :816
                    continue
                diff = int(case.next_image[i, j0]) - li
                rec[i, j0] = (u0, v0, j0, i, f32(diff), 1, (0, 0, 0))
                count += 1
                sumsq += diff * diff
    return rec, count, sumsq


def record_bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(rec.shape + (16,))


# ---- window -------------------------------------------------------------------------------------------------------------------
def disabled_by(zeros, cols, rows):
    """a zero of the next image at (x0, y0) is in the window (columns x-2 .. x+1, rows y-2 .. y+1) of x0-1 .. x0+2, y0-1 .. y0+2"""
    m = np.zeros((rows, cols), bool)
    for x0, y0 in zeros:
        m[max(y0 - 1, 0):y0 + 3, max(x0 - 1, 0):x0 + 3] = True
    return m


def window_case(name, cols, rows, zeros, seed):
    d = base(cols, rows, seed)
    for a in range(len(zeros)):
        for b in range(a):  # isolated: no pixel is disabled by two of them
            assert abs(zeros[a][0] - zeros[b][0]) >= 4 or abs(zeros[a][1] - zeros[b][1]) >= 4, (zeros[a], zeros[b])
    for x0, y0 in zeros:
        d["next_image"][y0, x0] = 0
    valid = band(cols, rows) & ~disabled_by(zeros, cols, rows)
    return make(name, "window", d, dict(valid=valid, count=int(valid.sum()), zeros=tuple(zeros)))


def window_cases():
    cols, rows = 40, 16
    out, seen = [], set()
    for t in range(4):
        for s in range(4):  # one zero in every column; columns 4 apart share a row, neighbours are 4 or more rows apart
            zeros = [(x0, (4 * ((x0 + t) % 4) + s) % rows) for x0 in range(cols)]
            seen.update(zeros)
            out.append(window_case(f"window_lattice_t{t}s{s}", cols, rows, zeros, 4 * t + s))
    # every column (so every residue mod 20, 4, 5 and 2, the first five and the last eight) met every row
    assert seen == {(x, y) for x in range(cols) for y in range(rows)}
    # blocks of zeros across a boundary between two groups of four columns (their regions overlap: the union is claimed)
    d = base(cols, rows, 99)
    blocks = [(3, 5), (4, 5), (3, 6), (4, 6)] + [(x, 10) for x in (14, 15, 16, 17)] + [(x, 1) for x in (26, 27, 28, 29)] + \
             [(31, 12), (32, 12), (31, 13), (32, 13)]
    for x0, y0 in blocks:
        d["next_image"][y0, x0] = 0
    valid = band(cols, rows) & ~disabled_by(blocks, cols, rows)
    out.append(make("window_blocks", "window", d, dict(valid=valid, count=int(valid.sum()), zeros=tuple(blocks))))
    return out


# ---- border -------------------------------------------------------------------------------------------------------------------
BORDER_COLS = (4, 5, 6, 8, 9, 12, 13, 20, 24)
BORDER_ROWS = (1, 2, 3, 5)


def border_cases():
    out = []
    for cols in BORDER_COLS:
        for rows in BORDER_ROWS:
            valid = band(cols, rows)
            claim = dict(valid=valid, count=max(cols - 5, 0) * max(rows - 1, 0))
            assert int(valid.sum()) == claim["count"]
            out.append(make(f"border_{cols}x{rows}", "border", base(cols, rows, cols + rows), claim))
    return out


# ---- gate ---------------------------------------------------------------------------------------------------------------------
def gate_case(name, min_scale, pairs, seed):
    cols, rows = 24, 12
    d = base(cols, rows, seed)
    d["min_scale"] = f32(min_scale)
    k = (np.arange(rows)[:, None] * 7 + np.arange(cols)[None, :]) % len(pairs)
    gx, gy = np.array([p[0] for p in pairs], np.int16), np.array([p[1] for p in pairs], np.int16)
    d["dIdx"], d["dIdy"] = gx[k], gy[k]
    passes = np.array([p[0] * p[0] + p[1] * p[1] >= float(min_scale) for p in pairs])  # integers below 2^24: exact as floats
    valid = band(cols, rows) & passes[k]
    at_equality = [p for p in pairs if p[0] * p[0] + p[1] * p[1] == float(min_scale)]
    for p in range(len(pairs)):
        assert (band(cols, rows) & (k == p)).any(), p  # every pair sits on a pixel of the band
    return make(name, "gate", d, dict(valid=valid, count=int(valid.sum()), at_equality=at_equality, pairs=tuple(pairs)))


def gate_cases():
    out = [gate_case("gate_25", 25.0, [(3, 4), (4, 3), (5, 0), (0, -5), (-3, -4), (4, 2), (3, 3), (1020, 1020), (-1020, 1020),
                                       (1020, -1020), (-1020, -1020), (0, 0), (5, 1)], 1),
           gate_case("gate_0", 0.0, [(0, 0)], 2),
           gate_case("gate_1600", 1600.0, [(40, 0), (0, -40), (24, 32), (-32, 24), (39, 8), (28, 28), (40, 1), (0, 0)], 3),
           gate_case("gate_576", 576.0, [(24, 0), (0, 24), (-24, 0), (23, 6), (17, 17), (16, 18), (24, -1)], 4),
           gate_case("gate_64", 64.0, [(8, 0), (0, -8), (7, 3), (5, 6), (6, 6), (-8, 1)], 5)]
    assert [len(c.claim["at_equality"]) for c in out] == [5, 1, 4, 3, 2]
    return out


# ---- depth --------------------------------------------------------------------------------------------------------------------
def side_of(td1, d0, delta):
    """where |td1 - d0| lies against delta, in float64 (float32 inputs: the difference is exact there)"""
    a = abs(np.float64(td1) - np.float64(d0))
    return "==" if a == np.float64(delta) else "<" if a < np.float64(delta) else ">"


def shipped_delta_pairs(n=4, seed=20):
    """(td1, d0) with fl(td1 - d0) == 0.07f exactly, by a seeded search; both signs.  0.07f is a multiple of 2^-27 and no
    coarser power of two, so d0 has to lie below 1 / 8 for the sum to be a float at all, and wherever the difference does."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(10000):
        plus = len(out) % 2 == 0
        d0 = f32(rng.uniform(0.0625, 0.12)) if plus else f32(rng.uniform(0.14, 0.19))
        td1 = f32(d0 + DELTA_SHIPPED) if plus else f32(d0 - DELTA_SHIPPED)
        if abs(f32(td1 - d0)) == DELTA_SHIPPED and side_of(td1, d0, DELTA_SHIPPED) == "==":
            out.append((td1, d0))
            if len(out) == n:
                return out
    raise AssertionError("no pair with a difference of exactly 0.07f found")


def depth_cases():
    cols, rows = 24, 12
    out = []
    tiny = f32(2.0 ** -100)
    # (a) values of d1 (identity warp, kt = 0); a zero depth looks at (0, 0): 0 / 0 -> NaN -> 0 on both axes
    for name, d00 in (("depth_d1_origin_matches", f32(0.03125)), ("depth_d1_origin_differs", f32(1.0))):
        d = base(cols, rows, 30)
        spots = {(3, 2): f32(np.nan), (7, 2): f32(0.0), (11, 2): f32(-1.0), (15, 2): f32(np.inf), (5, 6): tiny, (9, 6): tiny, (13, 6): f32(0.0)}
        for (x, y), val in spots.items():
            d["next_depth"][y, x] = val
        d["last_depth"][6, 5] = tiny           # td1 == d0 == 2^-100: a correspondence
        d["last_depth"][0, 0] = d00            # what the zero depths find at (0, 0)
        valid = band(cols, rows)
        for p in ((3, 2), (11, 2), (15, 2), (9, 6)):
            valid[p[1], p[0]] = False
        valid[0, 0] = d00 == 1.0               # its own depth is 1
        zero = {(5, 6): (5, 6)}
        for p in ((7, 2), (13, 6)):
            valid[p[1], p[0]] = d00 != 1.0     # |0 - 0.03125| <= 0.0625, |0 - 1| is not
            if d00 != 1.0:
                zero[p] = (0, 0)
        out.append(make(name, "depth", d, dict(valid=valid, count=int(valid.sum()), zero=zero)))
    # (b) kt.z takes td1 to 0 and below it: x / 0 and y / 0 are infinite (out of the image) except at the origin, where
    #     0 / 0 looks at (0, 0) and finds |td1 - 1| > delta
    for name, ktz in (("depth_td1_zero", -1.0), ("depth_td1_negative", -2.0)):
        d = base(cols, rows, 31)
        d["kt"][2] = ktz
        out.append(make(name, "depth", d, dict(valid=np.zeros((rows, cols), bool), count=0)))
    # (c) values of d0
    d = base(cols, rows, 32)
    d["next_depth"][:] = f32(0.03125)
    d["last_depth"][:] = f32(0.03125)
    bad = {(2, 1): f32(0.0), (6, 1): f32(-0.0), (10, 1): f32(-0.03125), (14, 1): f32(np.nan), (4, 5): f32(np.inf), (8, 5): f32(-np.inf)}
    valid = band(cols, rows)
    for (x, y), val in bad.items():
        d["last_depth"][y, x] = val
        valid[y, x] = False
    assert all(side_of(0.03125, v, DELTA) != ">" for v in (bad[(2, 1)], bad[(6, 1)], bad[(10, 1)]))  # only `d0 > 0` refuses these
    out.append(make("depth_d0_values", "depth", d, dict(valid=valid, count=int(valid.sum()), invalid=list(bad))))
    # (d) |td1 - d0| at delta = 2^-4 and one ulp beyond, both signs
    d = base(cols, rows, 33)
    above, below = f32(1.0625), f32(0.9375)
    spots = {(2, 1): (above, "=="), (6, 1): (below, "=="), (10, 1): (np.nextafter(above, f32(2)), ">"), (14, 1): (np.nextafter(below, f32(0)), ">"),
             (4, 5): (np.nextafter(above, f32(0)), "<"), (8, 5): (np.nextafter(below, f32(2)), "<")}
    valid = band(cols, rows)
    exact = []
    for (x, y), (d0, side) in spots.items():
        d["last_depth"][y, x] = d0
        assert side_of(1.0, d0, DELTA) == side
        assert f32(abs(f32(f32(1.0) - d0))) == abs(np.float64(1.0) - np.float64(d0))  # the float32 difference is exact
        valid[y, x] = side != ">"
        exact.append((f32(1.0), f32(d0), DELTA, side))
    out.append(make("depth_delta_dyadic", "depth", d, dict(valid=valid, count=int(valid.sum()), exact64=exact)))
    # (e) the shipped 0.07f: pairs whose float32 difference is 0.07f exactly, and their neighbours one ulp of d0 either way
    d = base(cols, rows, 34)
    d["max_depth_delta"] = DELTA_SHIPPED
    valid = band(cols, rows)
    exact = []
    for k, (td1, d0) in enumerate(shipped_delta_pairs()):
        y = 1 + 2 * k
        for x, d0v in ((3, d0), (8, np.nextafter(d0, f32(0))), (13, np.nextafter(d0, f32(4)))):
            d["next_depth"][y, x] = td1
            d["last_depth"][y, x] = d0v
            side = side_of(td1, d0v, DELTA_SHIPPED)
            assert f32(abs(f32(td1 - d0v))) == abs(np.float64(td1) - np.float64(d0v))  # close operands: exact
            valid[y, x] = side != ">"
            exact.append((td1, f32(d0v), DELTA_SHIPPED, side))
    assert sorted(e[3] for e in exact) == ["<"] * 4 + ["=="] * 4 + [">"] * 4
    out.append(make("depth_delta_shipped", "depth", d, dict(valid=valid, count=int(valid.sum()), exact64=exact)))
    return out


# ---- warp ---------------------------------------------------------------------------------------------------------------------
def warp_case(name, cols, rows, kt, krkinv, seed, extra=None, exact=True):
    """depth 1 everywhere: td1 = K[6] x + K[7] y + K[8] + kt.z.  The claim is worked out in float64 with Python's round
    (ties to even) from quotients whose numerator is rounded to float32 once, as `d1 * (...) + kt` is with integer entries;
    exact: the builder asserts that not even that rounding happened, so a claimed tie is one."""
    d = base(cols, rows, seed)
    d["kt"] = np.asarray(kt, f32)
    d["krkinv"] = np.asarray(krkinv, f32)
    K, ktv = d["krkinv"].astype(np.float64).reshape(9), d["kt"].astype(np.float64)
    valid = np.zeros((rows, cols), bool)
    zero, ties = {}, []

    def nearest(q):
        return round(q) if abs(q) < 2 ** 31 else INT_MAX * int(np.sign(q))

    for y in range(rows - 1):
        for x in range(cols - 5):
            z = K[6] * x + K[7] * y + K[8] + ktv[2]
            nx, ny = K[0] * x + K[1] * y + K[2] + ktv[0], K[3] * x + K[4] * y + K[5] + ktv[1]
            qx, qy = float(f32(nx)) / z, float(f32(ny)) / z
            assert f32(z) == z and f32(qx) == qx and f32(qy) == qy, (name, x, y, qx, qy)
            if exact:
                assert f32(nx) == nx and f32(ny) == ny, (name, x, y, nx, ny)  # no rounding before the tie
            u0, v0 = nearest(qx), nearest(qy)
            if (qx % 1 == 0.5 or qy % 1 == 0.5) and f32(nx) == nx and f32(ny) == ny:  # (a tie the rounding made is not claimed as one)
                ties.append((x, y, qx, qy))
            if 0 <= u0 < cols and 0 <= v0 < rows:
                valid[y, x] = True
                zero[(x, y)] = (u0, v0)
    claim = dict(valid=valid, count=int(valid.sum()), zero=zero, ties=ties)
    claim.update(extra or {})
    return make(name, "warp", d, claim)


def warp_cases():
    out = []
    below_half = np.nextafter(f32(-0.5), f32(-1))
    for cols, rows in ((24, 12), (23, 11)):  # cols - 1 and rows - 1 odd and even: the ties beside the image go both ways
        tag = f"{cols}x{rows}"
        s = cols + rows
        out.append(warp_case(f"warp_tie_x_{tag}", cols, rows, (0.5, 0, 0), EYE, s))        # x + 0.5: to x (even) or x + 1 (odd)
        out.append(warp_case(f"warp_tie_y_{tag}", cols, rows, (0, 0.5, 0), EYE, s + 1))
        out.append(warp_case(f"warp_tie_xy_{tag}", cols, rows, (0.5, 0.5, 0), EYE, s + 2))
        out.append(warp_case(f"warp_minus_half_{tag}", cols, rows, (-0.5, -0.5, 0), EYE, s + 3))  # -0.5 -> 0: column 0 and row 0 stay inside
        out.append(warp_case(f"warp_below_minus_half_x_{tag}", cols, rows, (below_half, 0, 0), EYE, s + 4, exact=False))  # column 0 -> -1
        out.append(warp_case(f"warp_below_minus_half_y_{tag}", cols, rows, (0, below_half, 0), EYE, s + 5, exact=False))
        for k, shift in enumerate((4.5, 5.0, 5.5, 6.0, 6.5)):  # x = cols - 6 at cols - 1.5, cols - 1, cols - 0.5, cols, cols + 0.5
            out.append(warp_case(f"warp_right_{shift}_{tag}", cols, rows, (shift, 0, 0), EYE, s + 6 + k))
        for k, shift in enumerate((0.5, 1.0, 1.5, 2.0)):       # y = rows - 2 at rows - 1.5, rows - 1, rows - 0.5, rows
            out.append(warp_case(f"warp_bottom_{shift}_{tag}", cols, rows, (0, shift, 0), EYE, s + 11 + k))
        # shears: u0 = x + y + c puts a diagonal on cols - 1 and the next on cols; v0 = x + y + c the same with rows
        out.append(warp_case(f"warp_shear_x_{tag}", cols, rows, (0, 0, 0), [[1, 1, 3], [0, 1, 0], [0, 0, 1]], s + 15))
        out.append(warp_case(f"warp_shear_y_{tag}", cols, rows, (0, 0, 0), [[1, 0, 0], [1, 1, -4], [0, 0, 1]], s + 16))
        out.append(warp_case(f"warp_shear_row_x_{tag}", cols, rows, (0, 0, 0), [[0, 1, cols - rows + 2], [0, 1, 0], [0, 0, 1]], s + 17))
        out.append(warp_case(f"warp_shear_col_y_{tag}", cols, rows, (0, 0, 0), [[1, 0, 0], [1, 0, rows - cols + 6], [0, 0, 1]], s + 18))
        for k, far in enumerate((3.0e9, -3.0e9)):  # beyond 2^31: the device saturates at 2147483520, the oracle at INT_MAX
            out.append(warp_case(f"warp_far_x_{k}_{tag}", cols, rows, (far, 0, 0), EYE, s + 19, dict(oob=True), exact=False))
            out.append(warp_case(f"warp_far_y_{k}_{tag}", cols, rows, (0, far, 0), EYE, s + 20, dict(oob=True), exact=False))
    by = {c.name: c for c in out}
    for tag, cols, rows in (("24x12", 24, 12), ("23x11", 23, 11)):
        c = by[f"warp_tie_x_{tag}"].claim
        assert all(c["zero"][(x, 0)][0] == (x if x % 2 == 0 else x + 1) for x in range(cols - 5)) and len(c["ties"]) == c["count"]
        assert by[f"warp_minus_half_{tag}"].claim["zero"][(0, 0)] == (0, 0)
        assert not by[f"warp_below_minus_half_x_{tag}"].claim["valid"][:, 0].any() and by[f"warp_below_minus_half_x_{tag}"].claim["valid"][0, 1]
        assert not by[f"warp_below_minus_half_y_{tag}"].claim["valid"][0, :].any()
        x = cols - 6  # the last column of the band
        landed = {sh: by[f"warp_right_{sh}_{tag}"].claim["zero"].get((x, 0)) for sh in (4.5, 5.0, 5.5, 6.0, 6.5)}
        assert landed[5.0] == (cols - 1, 0) and landed[6.0] is None
        assert landed[4.5] == ((cols - 2, 0) if cols % 2 == 0 else (cols - 1, 0))     # cols - 1.5 -> the even neighbour
        assert landed[5.5] == (None if cols % 2 == 0 else (cols - 1, 0))              # cols - 0.5 -> cols or cols - 1
        y = rows - 2
        landed = {sh: by[f"warp_bottom_{sh}_{tag}"].claim["zero"].get((0, y)) for sh in (0.5, 1.0, 1.5, 2.0)}
        assert landed[1.0] == (0, rows - 1) and landed[2.0] is None
        assert landed[1.5] == (None if rows % 2 == 0 else (0, rows - 1))
        for name, axis, n in ((f"warp_shear_x_{tag}", 0, cols), (f"warp_shear_y_{tag}", 1, rows), (f"warp_shear_row_x_{tag}", 0, cols),
                              (f"warp_shear_col_y_{tag}", 1, rows)):
            c = by[name].claim
            hits = [p for p, z in c["zero"].items() if z[axis] == n - 1]
            assert len(hits) >= 2 and (band(cols, rows) & ~c["valid"]).any(), name  # some land on the last column / row, some beyond
        for k in (0, 1):
            assert by[f"warp_far_x_{k}_{tag}"].claim["count"] == 0 and by[f"warp_far_y_{k}_{tag}"].claim["count"] == 0
    return out


# ---- last ---------------------------------------------------------------------------------------------------------------------
def last_cases():
    """|diff| = 255 cannot occur: it needs a zero on one side, and a zero of the last image is refused (reduce.cu:816) while a
    zero of the next image fails the pixel's own window (:782).  254 is the extreme; the pixel with next = 255 over last = 0
    is what tells the dropped test apart (it would enter with diff = 255)."""
    cols, rows = 24, 12
    d = base(cols, rows, 40)
    d["next_image"][:] = 128
    d["last_image"][:] = 128
    spots = {(2, 1): (255, 1), (6, 1): (1, 255), (10, 1): (128, 128), (14, 1): (129, 128), (3, 5): (128, 129), (7, 5): (255, 0), (11, 5): (1, 0),
             (15, 5): (200, 0)}
    valid = band(cols, rows)
    sumsq = 0
    for (x, y), (n, l) in spots.items():
        d["next_image"][y, x], d["last_image"][y, x] = n, l
        valid[y, x] = l != 0
        sumsq += (n - l) ** 2 if l else 0
    assert sumsq == 254 ** 2 * 2 + 2
    out = [make("last_extremes", "last", d, dict(valid=valid, count=int(valid.sum()), sumsq=sumsq, invalid=[p for p, v in spots.items() if v[1] == 0]))]
    # the landing pixel, not the pixel's own, is what is tested: a shift by (2, 1)
    d = base(cols, rows, 41)
    d["kt"] = np.array([2, 1, 0], f32)
    holes = [(4, 3), (9, 7), (20, 10), (2, 1)]
    valid = band(cols, rows)
    for x, y in holes:
        d["last_image"][y, x] = 0
        if x - 2 >= 0 and y - 1 >= 0:
            valid[y - 1, x - 2] = False
    diff = d["next_image"].astype(np.int64)[:rows - 1, :cols - 2] - d["last_image"].astype(np.int64)[1:, 2:]
    sumsq = int((diff ** 2)[valid[:rows - 1, :cols - 2]].sum())
    out.append(make("last_shifted", "last", d, dict(valid=valid, count=int(valid.sum()), sumsq=sumsq)))
    return out


@functools.lru_cache(maxsize=None)
def standalone_cases():
    out = window_cases() + border_cases() + gate_cases() + depth_cases() + warp_cases() + last_cases()
    assert len({c.name for c in out}) == len(out)
    for c in out:
        rows, cols = c.next_image.shape
        assert c.family in FAMILIES
        assert cols <= 40 and rows <= 16 and (c.family == "window" or (cols <= 24 and rows <= 12))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_result(orc, name):
    """(records uint8 [rows, cols, 16], sum diff^2, count, error map) of the oracle on a case, computed once and read-only"""
    case = {c.name: c for c in standalone_cases()}[name]
    rec, sumsq, count, err = orc.rgb_residual(*inputs(case), want_err=True)
    return frozen(rec), sumsq, count, frozen(err)


# ---- rgbStep on records (reduce.cu:495-578) -------------------------------------------------------------------------------
StepCase = namedtuple("StepCase", "name corres sigma cloud fx fy dIdx dIdy sobel_scale claim")
FLT_EPSILON = f32(1.1920929e-7)
STEP_SIZES = ((1, 1), (3, 1), (2, 2), (15, 17), (16, 16), (257, 1), (41, 25))  # 1, 3, 4, 255, 256, 257 and 1025 records
SE3_PAIRS = tuple((i, j) for i in range(6) for j in range(i, 7))  # the 27 products that make A and b (reduce.cu:458-472)


def step_sigmas(count):
    return (f32(count), f32(1.0), f32(-1.0), f32(0.0), FLT_EPSILON, np.nextafter(FLT_EPSILON, f32(1)))


def plain_cloud(cols, rows):
    """points in front of the camera that have nothing to do with the case's depths (a landed pixel's own may be 2^-100)"""
    y, x = np.mgrid[0:rows, 0:cols]
    return frozen(np.stack([(x - cols / 2) * 0.05, (y - rows / 2) * 0.05, 1.0 + ((x + 2 * y) % 5) * 0.25], -1).astype(f32))


def plain_gradients(cols, rows):
    y, x = np.mgrid[0:rows, 0:cols]
    return frozen(((x * 29 + y * 13) % 401 - 200).astype(np.int16)), frozen(((x * 17 + y * 31) % 301 - 150).astype(np.int16))


def step_rows64(case):
    """rgbStep's rows (reduce.cu:504-535) for sigma = -1 (w = 1) in float64: [n, 7], zero where there is no record"""
    rec = case.corres.view(RECORD)[..., 0]
    rows, cols = rec.shape
    out = np.zeros((rows * cols, 7))
    with np.errstate(all="ignore"):
        for k, c in enumerate(rec.reshape(-1)):
            if not c["valid"]:
                continue
            X, Y, Z = (np.float64(v) for v in case.cloud[c["zero_y"], c["zero_x"]])
            invz = 1.0 / Z
            gx, gy = float(case.dIdx[c["one_y"], c["one_x"]]), float(case.dIdy[c["one_y"], c["one_x"]])
            v0, v1 = case.sobel_scale * gx * case.fx * invz, case.sobel_scale * gy * case.fy * invz
            v2 = -(v0 * X + v1 * Y) * invz
            out[k] = (v0, v1, v2, -Z * v1 + Y * v2, Z * v0 - X * v2, -Y * v0 + X * v1, -float(c["diff"]))
    return out


def exactly_summable(terms):
    """every float32 sum of these float64 terms, in any order, is exact: they share a quantum 2^-m and sum |term| < 2^24 quanta"""
    terms = np.asarray(terms, np.float64)
    for m in range(0, 60):
        if np.all(terms * 2.0 ** m == np.rint(terms * 2.0 ** m)):
            return float(np.abs(terms).sum()) * 2.0 ** m < 2.0 ** 24
    return False


def assert_exact_sums(products):
    """products [n, k]: each column's sum in float32, forwards and backwards, equals the float64 sum"""
    for col in products.T:
        assert exactly_summable(col)
        fwd, bwd = f32(0), f32(0)
        for v in col:
            fwd = f32(fwd + f32(v))
        for v in col[::-1]:
            bwd = f32(bwd + f32(v))
        assert np.float64(fwd) == np.float64(bwd) == col.sum()


def step_exact_case(cols, rows, kind, seed):
    """every entry of every row a small dyadic rational: X, Y in {-1, 0, 1}, Z in {1, 2, 4}, fx = fy = 8, sobel_scale = 1 / 8,
    sigma = -1, integer gradients and differences"""
    rng = np.random.default_rng(seed)
    n = cols * rows
    cloud = np.stack([rng.integers(-1, 2, (rows, cols)), rng.integers(-1, 2, (rows, cols)), 2 ** rng.integers(0, 3, (rows, cols))], -1).astype(f32)
    dIdx, dIdy = rng.integers(-2, 3, (rows, cols)).astype(np.int16), rng.integers(-2, 3, (rows, cols)).astype(np.int16)
    rec = np.zeros(n, RECORD)
    which = {"ends": sorted({0, n - 1}), "dense": range(n), "none": (), "z0": range(n)}[kind]
    for k in which:
        rec[k] = (rng.integers(0, cols), rng.integers(0, rows), k % cols, k // cols, f32(rng.integers(-8, 9)), 1, (0, 0, 0))
    claim = dict(kind=kind, valid=len(list(which)))
    if kind == "z0":  # the point under the first record lies in the camera's plane: 1 / Z is infinite
        cloud[rec[0]["zero_y"], rec[0]["zero_x"], 2] = 0.0
        dIdx[0, 0], dIdy[0, 0] = 2, -1
    case = StepCase(f"step_exact_{kind}_{cols}x{rows}", frozen(record_bytes(rec.reshape(rows, cols))), f32(-1.0), frozen(cloud), f32(8.0), f32(8.0),
                    frozen(dIdx), frozen(dIdy), f32(0.125), claim)
    if kind != "z0":
        r = step_rows64(case)
        assert_exact_sums(np.stack([r[:, i] * r[:, j] for i, j in SE3_PAIRS], 1))
    return case


@functools.lru_cache(maxsize=None)
def step_exact_cases():
    out = []
    for s, (cols, rows) in enumerate(STEP_SIZES):
        for kind in ("ends", "dense", "none"):
            out.append(step_exact_case(cols, rows, kind, 100 + s))
    out.append(step_exact_case(2, 2, "z0", 120))
    out.append(step_exact_case(15, 17, "z0", 121))
    return tuple(out)


# ---- so3Step (reduce.cu:981-1064) -------------------------------------------------------------------------------------------
So3Case = namedtuple("So3Case", "name last_image next_image B kinv krlr claim")
SO3_SIZES = ((3, 3), (4, 3), (5, 8), (20, 12))


def so3_rows64(case):
    """so3Step's rows in float64 with Python's round for the warp: ([n, 4], found count); for cases whose arithmetic is exact"""
    rows, cols = case.next_image.shape
    B, kinv, k = case.B.astype(np.float64), case.kinv.astype(np.float64), case.krlr.astype(np.float64).reshape(9)
    li, ni = case.last_image.astype(np.float64), case.next_image.astype(np.float64)
    out, found = [], 0

    def grad(img, x, y):
        return (img[y, x - 1] + img[y, x]) / 2 - (img[y, x + 1] + img[y, x]) / 2, (img[y - 1, x] + img[y, x]) / 2 - (img[y + 1, x] + img[y, x]) / 2

    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(cols):
                w = B @ np.array([x, y, 1.0])
                qx, qy = w[0] / w[2], w[1] / w[2]
                if not (np.isfinite(qx) and np.isfinite(qy)):
                    continue
                wx, wy = round(qx), round(qy)
                if not (1 <= wx < cols - 1 and 1 <= wy < rows - 1 and 1 <= x < cols - 1 and 1 <= y < rows - 1):
                    continue
                found += 1
                gnx, gny = grad(ni, wx, wy)
                glx, gly = grad(li, x, y)
                gx, gy = (gnx + glx) / 2, (gny + gly) / 2
                p = kinv @ np.array([x, y, 1.0])
                z2 = p[2] * p[2]
                left = np.array([(p[2] * (k[3 + c] * gy + k[c] * gx) - gy * k[6 + c] * y - gx * k[6 + c] * x) / z2 for c in range(3)])
                jac = np.cross(left, p)
                out.append((jac[0], jac[1], jac[2], -(ni[wy, wx] - li[y, x])))
    return np.array(out).reshape(-1, 4), found


def shifted_found(cols, rows, tx, ty):
    """pixels whose warp (x + tx, y + ty), rounded to even at a tie, stays inside the border of one pixel, as they do themselves"""
    return sum(1 for y in range(1, rows - 1) for x in range(1, cols - 1) if 1 <= round(x + tx) < cols - 1 and 1 <= round(y + ty) < rows - 1)


def stepped_images(cols, rows, seed):
    """0 / 255 steps between neighbours, some pixels in between"""
    rng = np.random.default_rng(seed)
    return [frozen(rng.choice(np.array([0, 255, 255, 0, 128, 1], np.uint8), (rows, cols))) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def so3_cases():
    out = []
    kinv_cam = np.array([[1 / 64, 0, -0.5], [0, 1 / 64, -0.25], [0, 0, 1]], f32)
    krlr_cam = np.array([[64, 0.5, 32], [-0.5, 64, 16], [0.001, -0.002, 1]], f32)
    for s, (cols, rows) in enumerate(SO3_SIZES):
        tag = f"{cols}x{rows}"
        last, nxt = stepped_images(cols, rows, 200 + s)
        for name, tx, ty in (("tie", 0.5, 0.5), ("tie_x", 0.5, 0.0), ("tie_y", 0.0, -0.5), ("left", -1.0, 0.0), ("right", 1.0, 0.0), ("up", 0.0, -1.0),
                             ("down", 0.0, 1.0), ("still", 0.0, 0.0)):
            B = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], f32)
            out.append(So3Case(f"so3_{name}_{tag}", last, nxt, frozen(B), frozen(kinv_cam), frozen(krlr_cam), dict(found=shifted_found(cols, rows, tx, ty))))
        # warped.z = y - 1: zero for the whole of row 1 (x / 0, and 0 / 0 at x = 0), negative above it
        B = np.array([[1, 0, 0], [0, 1, 0], [0, 1, -1]], f32)
        out.append(So3Case(f"so3_z0_{tag}", last, nxt, frozen(B), frozen(kinv_cam), frozen(krlr_cam), dict(z0_row=1)))
        # exact: images of a few grey levels (gradients are multiples of 1 / 2, up to 2), kinv and krlr powers of two
        rng = np.random.default_rng(300 + s)
        top = 105 if cols * rows < 100 else 102  # (two grey levels at 20 x 12: the rows grow with x and y, the sums with the pixels)
        el, en = frozen(rng.integers(100, top, (rows, cols)).astype(np.uint8)), frozen(rng.integers(100, top, (rows, cols)).astype(np.uint8))
        for name, tx in (("exact", 0.0), ("exact_tie", 0.5)):
            B = np.array([[1, 0, tx], [0, 1, 0], [0, 0, 1]], f32)
            c = So3Case(f"so3_{name}_{tag}", el, en, frozen(B), frozen(np.diag([0.25, 0.25, 1]).astype(f32)),
                        frozen(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0.125]], f32)), dict(found=shifted_found(cols, rows, tx, 0.0), exact=True))
            r, found = so3_rows64(c)
            assert found == c.claim["found"]
            if len(r):
                assert_exact_sums(np.stack([r[:, i] * r[:, j] for i in range(4) for j in range(i, 4)], 1))
            out.append(c)
    by = {c.name: c for c in out}
    assert by["so3_still_3x3"].claim["found"] == 1 and by["so3_left_3x3"].claim["found"] == 0 and by["so3_tie_3x3"].claim["found"] == 0
    assert by["so3_left_20x12"].claim["found"] == 17 * 10 and by["so3_tie_x_20x12"].claim["found"] == 18 * 10  # 1.5 -> 2 .. 17.5 -> 18, and 18.5 -> 18: half up would lose that column
    return tuple(out)


# ---- the chains: static cases ---------------------------------------------------------------------------------------------------
MODES = {"default": dict(rgbOnly=False, icpWeight=10.0, pyramid=True, fastOdom=False, so3=True),   # the GUI's
         "rgb_only": dict(rgbOnly=True, icpWeight=10.0, pyramid=True, fastOdom=False, so3=True),
         "level0": dict(rgbOnly=False, icpWeight=10.0, pyramid=False, fastOdom=False, so3=False)}  # what a truncated chain at level 0 is cut from
MODE_ITERATIONS = {"default": (19, 10), "rgb_only": (19, 10), "level0": (10, 0)}  # RGBDOdometry.cpp:312-314; the SO3 loop's 10
STATIC_DEPTH = 2.0
# mmf_odom_create takes no image below 32 x 32 (include/mmf_hip.h), so the chains' cases have 32 rows where 16 would do
FORCED_PX_SIZE = (40, 32)        # cols % 20 == 0: 1, 2, 4 and 5 pixels per lane are all allowed; level 2 is 10 x 8, ragged
ALIGNED_PYRAMID_SIZE = (32, 32)  # the smallest the odometry takes: level 2 (8 x 8) still has whole groups of four columns
NATURAL_PX_SIZES = {2: (328, 200), 4: (440, 300), 5: (460, 572)}  # just above 65 536, 131 072 and 262 144 pixels


class StaticCase:
    """name, w, h, K, fp / fc (the model's and the sensor's frame), model (the pose: identity), cutoff -- what gn_range.setup
    takes -- and modes (the names of MODES the builder asserted the case in), claim: count (the correspondences of a level-0
    pass), sumsq = 0."""


def plane_frame(orc, w, h, seed):
    """a textured plane facing the camera at 2 m: depth, the vertex and normal maps the oracle itself makes of it (so the ICP
    residual of the frame against itself is 0 exactly at every level), grey levels 2 .. 255 in blocks of 2 x 2"""
    from multimotionfusion_amd import synth
    K = synth.intrinsics(w, h)
    depth = np.full((h, w), STATIC_DEPTH, f32)
    vm = orc.create_vmap(depth, K["fx"], K["fy"], K["cx"], K["cy"], 15.0)
    nm = orc.create_nmap(vm)
    vertex, normal = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32)
    for p in range(3):
        vertex[..., p], normal[..., p] = vm[p * h:(p + 1) * h], nm[p * h:(p + 1) * h]
    vertex[..., 3], normal[..., 3] = 1.0, 0.01
    g = np.random.default_rng(seed).integers(2, 256, (h // 2 + 1, w // 2 + 1)).astype(np.uint8)
    gray = np.repeat(np.repeat(g, 2, 0), 2, 1)[:h, :w]
    return K, dict(depth=depth, vertex=vertex, normal=normal, rgb=np.ascontiguousarray(np.stack([gray] * 3, -1)))


def lattice_tiled(w, h, parity):
    """the window lattice of every second column, repeated every 16 rows"""
    return [(x0, y0 + 16 * j) for x0 in range(parity, w, 2) for y0 in [(4 * (x0 % 4) + 1) % 16] for j in range((h + 15) // 16) if y0 + 16 * j < h]


def level0_pass(orc, case):
    """the oracle's correspondence pass at level 0 from the identity: (valid [h, w], count, sum diff^2)"""
    import gn_range as gr
    o = gr.oracle_odometry(orc, case)
    dIdx, dIdy = orc.derivative_images(o.buffer("next_image", 0))
    rec, sumsq, count, _ = orc.rgb_residual(f32(CHAIN_MIN_SCALES[0]), dIdx, dIdy, o.buffer("last_depth", 0), o.buffer("next_depth", 0),
                                            o.buffer("last_image", 0), o.buffer("next_image", 0), DELTA_SHIPPED, ZERO3, EYE)
    zeros = (o.buffer("next_image", 0) == 0, o.buffer("last_image", 0) == 0)
    o.close()
    return rec.view(RECORD)[..., 0]["valid"] == 1, count, sumsq, zeros


def oracle_chain(orc, case, mode):
    """the oracle's whole tracking call from the identity: (t, R, stats, rgb error image)"""
    import gn_range as gr
    o = gr.oracle_odometry(orc, case)
    t, R = o.getIncrementalTransformation(case.model[:3, 3], case.model[:3, :3], want_err=True, **MODES[mode])
    st, err = o.stats(), o.rgb_err.copy()
    o.close()
    return t, R, st, err


def assert_static(orc, case):
    from helpers import assert_bit_equal
    for mode in case.modes:
        t, R, st, err = oracle_chain(orc, case, mode)
        assert_bit_equal(t, case.model[:3, 3], f"{case.name} {mode}: translation")
        assert_bit_equal(R, case.model[:3, :3], f"{case.name} {mode}: rotation")
        assert (st.iterations_run, st.so3_iterations_run) == MODE_ITERATIONS[mode], (case.name, mode, st.iterations_run, st.so3_iterations_run)
        assert st.lastRGBCount == case.claim["count"] and st.lastRGBError == 0.0, (case.name, mode, st.lastRGBCount, st.lastRGBError)
        assert not err.any()


def static_case(orc, name, w, h, seed, modes, rgb_zeros=(), model_holes=(), last_zeros=()):
    """rgb_zeros: pixels black in both frames (a zero in the 4 x 4 window, at every level alike); model_holes: {(x, y): z} put
    into the model's vertex map (RGBDOdometry.cpp:177-204 takes BOTH depth pyramids of the photometric term from the
    prediction, so this is d1 and d0 at once: NaN for z <= 0, z beyond the cut-off or NaN); last_zeros: black in the model's
    image alone (level 0 only: the coarser levels would see a difference)."""
    K, f = plane_frame(orc, w, h, seed)
    c = StaticCase()
    c.name, c.w, c.h, c.K, c.cutoff, c.modes = name, w, h, K, 15.0, tuple(modes)
    c.model = np.eye(4, dtype=f32)
    clean = StaticCase()
    clean.__dict__.update(c.__dict__)
    clean.fp = clean.fc = f
    valid_clean, _, _, _ = level0_pass(orc, clean)
    fp, fc = {k: v.copy() for k, v in f.items()}, {k: v.copy() for k, v in f.items()}
    gone = np.zeros((h, w), bool)
    for x, y in rgb_zeros:
        fp["rgb"][y, x] = fc["rgb"][y, x] = 0
    gone |= disabled_by(rgb_zeros, w, h)
    for (x, y), z in dict(model_holes).items():
        fp["vertex"][y, x, 2] = z
        gone[y, x] = True
    for x, y in last_zeros:
        fp["rgb"][y, x] = 0
        gone[y, x] = True
    for d in (fp, fc):
        for v in d.values():
            v.setflags(write=False)
    c.fp, c.fc = fp, fc
    valid, count, sumsq, (next0, last0) = level0_pass(orc, c)
    # the features are where they were put and do what they were put there for, and nothing else
    want_next0 = np.zeros((h, w), bool)
    for x, y in rgb_zeros:
        want_next0[y, x] = True
    want_last0 = want_next0.copy()
    for x, y in last_zeros:
        want_last0[y, x] = True
    assert np.array_equal(next0, want_next0) and np.array_equal(last0, want_last0), name
    assert np.array_equal(valid, valid_clean & ~gone) and sumsq == 0, name
    c.claim = dict(count=int((valid_clean & ~gone).sum()), sumsq=0, clean=int(valid_clean.sum()), removed=int((valid_clean & gone).sum()))
    assert count == c.claim["count"] and (c.claim["removed"] > 0) == bool(len(rgb_zeros) or len(model_holes) or len(last_zeros)), name
    assert_static(orc, c)
    return c


MODEL_HOLES = {(5, 3): 0.0, (9, 3): np.nan, (12, 8): 20.0, (13, 8): 20.0, (14, 8): 20.0, (15, 8): 20.0, (16, 8): 20.0, (30, 12): -1.0, (0, 0): 0.0,
               (19, 5): np.inf, (20, 5): -0.0, (24, 10): 0.0, (25, 10): 0.0}
LAST_ZEROS = ((3, 2), (10, 7), (33, 13), (0, 0), (4, 2), (16, 7), (17, 7), (18, 7), (19, 7))


@functools.lru_cache(maxsize=None)
def static_cases(orc):
    """the 40 x 32 cases of the forced pixels-per-lane runs (and the pyramid whose level 2 is ragged) and the 32 x 32 ones"""
    out = []
    for (w, h), seed in ((FORCED_PX_SIZE, 1), (ALIGNED_PYRAMID_SIZE, 2)):
        tag = f"{w}x{h}"
        every = ("default", "rgb_only", "level0")
        out.append(static_case(orc, f"static_clean_{tag}", w, h, seed, every))
        out.append(static_case(orc, f"static_window_even_{tag}", w, h, seed, every, rgb_zeros=lattice_tiled(w, h, 0)))
        out.append(static_case(orc, f"static_window_odd_{tag}", w, h, seed, every, rgb_zeros=lattice_tiled(w, h, 1)))
        out.append(static_case(orc, f"static_holes_{tag}", w, h, seed, every, model_holes={p: z for p, z in MODEL_HOLES.items() if p[0] < w}))
        out.append(static_case(orc, f"static_last0_{tag}", w, h, seed, ("level0",), last_zeros=[p for p in LAST_ZEROS if p[0] < w]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def natural_case(orc, px):
    """the window lattice tiled over the smallest image at which the launch geometry itself picks `px` pixels per lane"""
    w, h = NATURAL_PX_SIZES[px]
    return static_case(orc, f"static_window_px{px}_{w}x{h}", w, h, 10 + px, ("level0",), rgb_zeros=lattice_tiled(w, h, px % 2))


def geometry_px(cols, rows, max_groups=256, lanes=256):
    """csrc/chain_host.hpp, gn_geometry's first loop restated: the fewest pixels per lane of 1, 2, 4, 5 that the width allows
    and that need no more than 256 workgroups of 256 pixel lanes"""
    for px in (1, 2, 4, 5):
        if cols % px == 0 and cols % 4 == 0 and (cols * rows // px + lanes - 1) // lanes <= max_groups:
            return px
    return None


for _px, (_w, _h) in NATURAL_PX_SIZES.items():
    assert geometry_px(_w, _h) == _px and _w % 4 == 0 and _h % 4 == 0
assert NATURAL_PX_SIZES[5][0] % 20 == 0 and geometry_px(*FORCED_PX_SIZE) == 1
