"""CPU restatement of the optical-flow engine's specification (csrc/flow_kernels.hpp): Farneback's dense
flow, one level, box window, on a frame pair scaled down by `div`.  numpy, float32 in the written order -- vectorised over
pixels, a Python loop over taps, so every sum adds its terms in the order the text gives -- or float64 (`dt`), the same
restatement at a precision that shows the float32 rounding.  The device is held to the float32 form bit for bit; this file is
held to the truth by frames whose motion is known (tests/test_flow_oracle.py).  Parity with OpenCV's implementation is not
pinned: the formulas follow the published algorithm, not a build of that library."""
import numpy as np

F32 = np.float32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
DEFAULTS = dict(div=4, levels=1, winsize=20, iterations=2, poly_n=5, poly_sigma=0.3)


def config(**overrides):
    cfg = dict(DEFAULTS)
    cfg.update(overrides)
    return cfg


def tables(n, sigma):
    """g, xg, xxg [n + 1] and ig = (ig11, ig03, ig33, ig55) in float64: the Gaussian normalised over -n..n with its moments,
    and four entries of the inverse of the moment matrix of (1, x, y, x^2, y^2, xy).  sigma is the float32 the library is
    handed."""
    sigma = float(F32(sigma))
    k = np.arange(n + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * sigma * sigma))
    g /= g[0] + 2.0 * g[1:].sum()
    G = np.zeros((6, 6))
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            w = g[abs(y)] * g[abs(x)]
            G[0, 0] += w
            G[1, 1] += w * x * x
            G[3, 3] += w * x * x * x * x
            G[5, 5] += w * x * x * y * y
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    inv = np.linalg.inv(G)
    return g, k * g, k * k * g, np.array([inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5]])


def downscale(rgb, div):
    """stage 1: per-channel area mean over div x div pixels, integer: sum / 16 half to even, (a+b+c+d+2) >> 2, or a copy"""
    if div == 1:
        return rgb.copy()
    h, w = rgb.shape[0] // div, rgb.shape[1] // div
    s = rgb.reshape(h, div, w, div, 3).astype(np.int32).sum(axis=(1, 3))
    if div == 2:
        return ((s + 2) >> 2).astype(np.uint8)
    q, r = s >> 4, s & 15
    return (q + ((r > 8) | ((r == 8) & ((q & 1) == 1)))).astype(np.uint8)


def gray(small):
    """stage 2: channel 0 carries the 0.114 weight (the reference hands RGB data to COLOR_BGR2GRAY)"""
    c = small.astype(np.int32)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def smooth(g8, dt=F32):
    """stage 3: [0.25, 0.5, 0.25] horizontally then vertically, reflect-101"""
    a = g8.astype(dt)
    p = np.pad(a, ((0, 0), (1, 1)), mode="reflect")
    a = dt(0.5) * p[:, 1:-1] + dt(0.25) * (p[:, :-2] + p[:, 2:])
    p = np.pad(a, ((1, 1), (0, 0)), mode="reflect")
    return dt(0.5) * p[1:-1] + dt(0.25) * (p[:-2] + p[2:])


def expand(s, tab, n, dt=F32):
    """stage 4: the polynomial expansion, [H, W, 5]"""
    g, xg, xxg, ig = (np.asarray(t).astype(dt) for t in tab)
    H, W = s.shape
    P = np.pad(s, ((n, n), (0, 0)), mode="edge")
    r0 = g[0] * P[n:n + H]
    r1 = np.zeros_like(r0)
    r2 = np.zeros_like(r0)
    for k in range(1, n + 1):
        t0, t1 = P[n - k:n - k + H], P[n + k:n + k + H]
        r0 = r0 + g[k] * (t0 + t1)
        r1 = r1 + xg[k] * (t1 - t0)
        r2 = r2 + xxg[k] * (t0 + t1)
    Q0, Q1, Q2 = (np.pad(r, ((0, 0), (n, n)), mode="edge") for r in (r0, r1, r2))
    b1, b3, b5 = r0 * g[0], r1 * g[0], r2 * g[0]
    b2 = np.zeros_like(b1)
    b4 = np.zeros_like(b1)
    b6 = np.zeros_like(b1)
    for k in range(1, n + 1):
        r0p, r0m = Q0[:, n + k:n + k + W], Q0[:, n - k:n - k + W]
        r1p, r1m = Q1[:, n + k:n + k + W], Q1[:, n - k:n - k + W]
        r2p, r2m = Q2[:, n + k:n + k + W], Q2[:, n - k:n - k + W]
        tg = r0p + r0m
        b1 = b1 + tg * g[k]
        b2 = b2 + (r0p - r0m) * xg[k]
        b4 = b4 + tg * xxg[k]
        b3 = b3 + (r1p + r1m) * g[k]
        b6 = b6 + (r1p - r1m) * xg[k]
        b5 = b5 + (r2p + r2m) * g[k]
    return np.stack([b3 * ig[0], b2 * ig[0], b1 * ig[1] + b5 * ig[2], b1 * ig[1] + b4 * ig[2], b6 * ig[3]], axis=-1).astype(dt)


def _border_scale(size, dt):
    v = np.arange(size)
    b = np.array(BORDER).astype(dt)
    lo = np.where(v < 5, b[np.minimum(v, 4)], dt(1))
    hi = np.where(v >= size - 5, b[np.clip(size - v - 1, 0, 4)], dt(1))
    return (lo * hi).astype(dt)


def matrices(R0, R1, flow, dt=F32):
    """stage 5; flow None: zero"""
    H, W = R0.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    dx = np.zeros((H, W), dt) if flow is None else flow[..., 0]
    dy = np.zeros((H, W), dt) if flow is None else flow[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = xs.astype(dt) + dx, ys.astype(dt) + dy
        x1f, y1f = np.floor(fx), np.floor(fy)
        inside = (x1f >= 0) & (x1f < dt(W - 1)) & (y1f >= 0) & (y1f < dt(H - 1))
        x1, y1 = np.where(inside, x1f, 0).astype(np.int64), np.where(inside, y1f, 0).astype(np.int64)
        fx, fy = np.where(inside, fx - x1f, 0).astype(dt), np.where(inside, fy - y1f, 0).astype(dt)
        one = dt(1)
        w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
        x2, y2 = np.minimum(x1 + 1, W - 1), np.minimum(y1 + 1, H - 1)  # (only read where `inside`: never clipped there)
        ip = [R1[y1, x1, c] * w00 + R1[y1, x2, c] * w01 + R1[y2, x1, c] * w10 + R1[y2, x2, c] * w11 for c in range(5)]
        zero = np.zeros((H, W), dt)
        r2, r3 = np.where(inside, ip[0], zero), np.where(inside, ip[1], zero)
        r4 = np.where(inside, (R0[..., 2] + ip[2]) * dt(0.5), R0[..., 2])
        r5 = np.where(inside, (R0[..., 3] + ip[3]) * dt(0.5), R0[..., 3])
        r6 = np.where(inside, (R0[..., 4] + ip[4]) * dt(0.25), R0[..., 4] * dt(0.5))
        r2 = (R0[..., 0] - r2) * dt(0.5)
        r3 = (R0[..., 1] - r3) * dt(0.5)
        r2 = r2 + (r4 * dy + r6 * dx)
        r3 = r3 + (r6 * dy + r5 * dx)
        scale = _border_scale(W, dt)[None, :] * _border_scale(H, dt)[:, None]
        r2, r3, r4, r5, r6 = (r * scale for r in (r2, r3, r4, r5, r6))
        return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], axis=-1).astype(dt)


def blur_solve(M, m, dt=F32):
    """stage 6: the (2m+1)^2 box sums (clamped; horizontal taps in ascending x, then vertical taps in ascending y, every sum
    from 0) and the solve"""
    H, W = M.shape[:2]
    P = np.pad(M, ((m, m), (m, m), (0, 0)), mode="edge")
    hs = np.zeros((H + 2 * m, W, 5), dt)
    for k in range(2 * m + 1):
        hs = hs + P[:, k:k + W]
    vs = np.zeros((H, W, 5), dt)
    for k in range(2 * m + 1):
        vs = vs + hs[k:k + H]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        vs = vs * (dt(1) / dt((2 * m + 1) * (2 * m + 1)))
        g11, g12, g22, h1, h2 = (vs[..., c] for c in range(5))
        idet = (1.0 / ((g11 * g22 - g12 * g12).astype(np.float64) + 1e-3)).astype(dt)
        return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=-1).astype(dt)


def warp_positions(shape, flow, dt=F32):
    """stage 5's view of a flow [H, W, 2] (None: zero): (x1f, y1f, inside, fracx, fracy) -- the floors as floats, the branch
    taken and, where inside, the interpolation fractions.  The expressions of `matrices`, which does not hand them out."""
    H, W = shape
    ys, xs = np.mgrid[0:H, 0:W]
    dx = np.zeros((H, W), dt) if flow is None else flow[..., 0]
    dy = np.zeros((H, W), dt) if flow is None else flow[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = xs.astype(dt) + dx, ys.astype(dt) + dy
        x1f, y1f = np.floor(fx), np.floor(fy)
        inside = (x1f >= 0) & (x1f < dt(W - 1)) & (y1f >= 0) & (y1f < dt(H - 1))
        return x1f, y1f, inside, np.where(inside, fx - x1f, 0).astype(dt), np.where(inside, fy - y1f, 0).astype(dt)


def box_means(M, m, dt=F32):
    """stage 6 up to the solve: g11, g12, g22, h1, h2 as `blur_solve` sums them, [H, W, 5]"""
    H, W = M.shape[:2]
    P = np.pad(M, ((m, m), (m, m), (0, 0)), mode="edge")
    hs = np.zeros((H + 2 * m, W, 5), dt)
    for k in range(2 * m + 1):
        hs = hs + P[:, k:k + W]
    vs = np.zeros((H, W, 5), dt)
    for k in range(2 * m + 1):
        vs = vs + hs[k:k + H]
    return vs * (dt(1) / dt((2 * m + 1) * (2 * m + 1)))


def trace(out, cfg, dt=F32):
    """What `pair` computes on the way and does not keep, from its result `out`: per iteration a dict of `det` =
    g11*g22 - g12*g12 [H, W] (at `dt`, before the double addition of 1e-3), `idet`, the flow `flow_in` the iteration warps by
    (None in front of the first) and `warp_positions` of it as x1f, y1f, inside, fracx, fracy.  `flow` is the iteration's
    flow solved again from `det`: equal to out["flow_<i>"] bit for bit, or this function has drifted from `blur_solve`."""
    its = []
    flow = None
    for it in range(cfg["iterations"]):
        x1f, y1f, inside, fracx, fracy = warp_positions(out["R0"].shape[:2], flow, dt)
        vs = box_means(matrices(out["R0"], out["R1"], flow, dt), cfg["winsize"] // 2, dt)
        g11, g12, g22, h1, h2 = (vs[..., c] for c in range(5))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            det = g11 * g22 - g12 * g12
            idet = (1.0 / (det.astype(np.float64) + 1e-3)).astype(dt)
            again = np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=-1).astype(dt)
        its.append(dict(det=det, idet=idet, flow_in=flow, x1f=x1f, y1f=y1f, inside=inside, fracx=fracx, fracy=fracy, flow=again))
        flow = out[f"flow_{it}"]
    return its


def outputs(flow, dt=F32):
    """stage 8: magnitude, motion"""
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = flow[..., 0], flow[..., 1]
        mag = np.sqrt(x * x + y * y)
        v = (mag - dt(0.2)) / dt(4.8)
        v = np.where(v > 0, v, dt(0))
        v = np.where(v < 1, v, dt(1))
        return mag.astype(dt), v.astype(dt)


def prepare(rgb, cfg, tab, dt=F32):
    """stages 1-4 of one frame: (gray, smooth, R)"""
    g8 = gray(downscale(rgb, cfg["div"]))
    s = smooth(g8, dt)
    return g8, s, expand(s, tab, cfg["poly_n"], dt)


def pair(prev_rgb, next_rgb, cfg, tab=None, dt=F32):
    """every stage image of a frame pair.  tab: the tables the library hands out (float32), or None: tables() at `dt`"""
    if tab is None:
        tab = tables(cfg["poly_n"], cfg["poly_sigma"])
    g0, s0, R0 = prepare(prev_rgb, cfg, tab, dt)
    g1, s1, R1 = prepare(next_rgb, cfg, tab, dt)
    out = dict(gray0=g0, smooth0=s0, R0=R0, gray=g1, smooth=s1, R1=R1)
    flow = None
    for it in range(cfg["iterations"]):
        out["M"] = matrices(R0, R1, flow, dt)
        flow = blur_solve(out["M"], cfg["winsize"] // 2, dt)
        out[f"flow_{it}"] = flow
    out["flow"] = flow
    out["magnitude"], out["motion"] = outputs(flow, dt)
    return out
