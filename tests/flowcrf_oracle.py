"""The inference of the flow CRF (Core/Segmentation/Segmentation.cpp:819-1263) restated in numpy after the text of DESIGN.md
4.9: the checker of csrc/flowcrf_kernels.hpp.

Stages (a) track errors, (b) unaries, (c) projection probabilities and (e) fusion run in float32 (the projections of (a) in
float64) in the written order; (a), the cells and `invalid` are bit-exact to the device, (b), (c), (e) up to the library
functions exp / log.  Stage (d), the mean field, is EXACT Gaussian sums over every pair in float64, as in
tests/crf_oracle.py.
"""
import numpy as np

import crf_oracle as co

F32 = np.float32
F64 = np.float64

DEFAULTS = dict(iterations=10, weight_smoothness=40.0, weight_appearance=40.0, threshold=20.0, max_err=0.03, min_proj_prob=0.3)


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def round_half_away(u):
    a = np.abs(u)
    r = np.floor(a)
    r = r + ((a - r) >= 0.5)
    return np.copysign(r, u)


def project(T, co_, ts, ok, cam, W, H):
    """one end of every track in a model's frame (Model.cpp:524-579): has [n] (a keypoint exists), inside [n], px, py [n]"""
    fx, fy, cx, cy = (F64(F32(v)) for v in cam)
    T = np.asarray(T, F32).reshape(4, 4).astype(F64)
    c = np.asarray(co_, F32).reshape(-1, 3)
    has = (np.asarray(ok) != 0) & (np.asarray(ts) != 0) & np.isfinite(c).all(1)
    x, y, z = (c[:, i].astype(F64) for i in range(3))
    with np.errstate(all="ignore"):
        X, Y, Z = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3))
        u, v = cx + (X / Z) * fx, cy + (Y / Z) * fy
        good = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
        px = np.where(good, round_half_away(np.where(good, u, 0.0)), 0).astype(np.int64)
        py = np.where(good, round_half_away(np.where(good, v, 0.0)), 0).astype(np.int64)
    inside = good & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    return has, inside, px, py


def track_errors(W, H, cam, T_start, T_end, tracks, L):
    """(a): E [L][N] float32 (+inf where no track), cell [M][n] (-1: no sample).  tracks: dict of numpy arrays xy_* [n,2],
    co_* [n,3], ts_* [n] int64, ok_* [n]; `prev` is the start, `cur` the end; may be None"""
    w, h = W // 4, H // 4
    N = w * h
    M = len(T_start)
    E = np.full((L, N), np.inf, F32)
    n = 0 if tracks is None else len(tracks["ts_cur"])
    cell = np.full((M, n), -1, np.int64)
    for m in range(M):
        if n == 0:
            continue
        has0, in0, x0, y0 = project(T_start[m], tracks["co_prev"], tracks["ts_prev"], tracks["ok_prev"], cam, W, H)
        has1, in1, x1, y1 = project(T_end[m], tracks["co_cur"], tracks["ts_cur"], tracks["ok_cur"], cam, W, H)
        take = has0 & has1 & in0 & in1
        dx, dy = (x1 - x0).astype(F32), (y1 - y0).astype(F32)
        length = np.sqrt(dx.astype(F64) * dx.astype(F64) + dy.astype(F64) * dy.astype(F64))
        dt = (np.asarray(tracks["ts_cur"], np.int64).astype(np.uint64) - np.asarray(tracks["ts_prev"], np.int64).astype(np.uint64))
        with np.errstate(all="ignore"):
            v = (length / (dt.astype(F64) * 1e-9)).astype(F32)
        ccx, ccy = np.rint(0.25 * x1.astype(F64)).astype(np.int64), np.rint(0.25 * y1.astype(F64)).astype(np.int64)
        idx = ccy * w + ccx
        for k in range(n):  # in table order: a later track overwrites an earlier one
            if take[k] and idx[k] < N:
                cell[m, k] = idx[k]
                E[m, idx[k]] = v[k]
    return E, cell


def unaries(E, M, allow_new, threshold):
    """(b): U [L][N] float32 from E (not modified)"""
    L, N = E.shape
    thr = F32(threshold)
    act = E[:M]
    with np.errstate(all="ignore"):
        fin = np.isfinite(act)
        u = np.array(E, F32)
        u[:M] = np.where(fin, (act > thr).astype(F32), act)
        if allow_new:
            u[M] = np.where(fin.all(0), (act < thr).any(0).astype(F32), F32(np.inf))
        ex = np.exp(-u).astype(F32)
        tot = np.zeros(N, F32)
        for l in range(L):
            tot = (tot + ex[l]).astype(F32)
        soft = tot > 0
        p = np.where(soft[None], (ex / np.where(soft, tot, F32(1))[None]).astype(F32), F32(F32(1) / F32(L)))
        return (-np.log(p.astype(F32))).astype(F32)


def proj_prob(depth, vertex_z, allow_new, max_err, min_proj_prob, dtype=F32):
    """(c): proj [L][N], invalid [N] bool.  depth [H][W], vertex_z [M][H][W] (channel 2 of the vertex images).  dtype float64
    gives the values the tests use to find cells too close to min_proj_prob."""
    d = np.asarray(depth, F32)[::4, ::4].ravel().astype(dtype)
    z = np.asarray(vertex_z, F32)[:, ::4, ::4].reshape(len(vertex_z), -1).astype(dtype)
    M = z.shape[0]
    me = dtype(F32(max_err))
    with np.errstate(all="ignore"):
        inv = ((d[None] < dtype(F32(1e-6))) & (z < dtype(F32(1e-6)))).any(0)
        dist = np.abs(d[None] - z).astype(dtype)
        dist = np.where(dist < me, dist, me)
        e = np.exp((dtype(-1.0) * (dist / me).astype(dtype)).astype(dtype)).astype(dtype)
        s = np.zeros(d.shape, dtype)
        for m in range(M):
            s = (s + e[m]).astype(dtype)
        p = (e / s[None]).astype(dtype)
    p = np.where(inv[None], dtype(0), p)
    p = np.where(p < dtype(F32(min_proj_prob)), dtype(0), p)
    if allow_new:
        p = np.concatenate([p, np.zeros((1, p.shape[1]), dtype)])
    return p.astype(dtype), inv


def features(w, h, flow):
    """(d): smoothness (x / 3, y / 3) and appearance ((float)(x / 40), (float)(y / 40), 10 flow.x, 10 flow.y), float32"""
    k = np.arange(w * h)
    x, y = k % w, k // w
    fs = np.stack([x.astype(F32) / F32(3), y.astype(F32) / F32(3)], 1).astype(F32)
    f = np.asarray(flow, F32).reshape(-1, 2)
    fa = np.stack([(x // 40).astype(F32), (y // 40).astype(F32), f[:, 0] * F32(10), f[:, 1] * F32(10)], 1).astype(F32)
    return fs, fa


def pair_matrix(fs, fa, cfg):
    return co.pair_matrix(fs, fa, dict(weight_smoothness=4.0 * cfg["weight_smoothness"], weight_appearance=cfg["weight_appearance"]))


def mean_field(U, fs, fa, cfg, A=None):
    """(d): Q [L][N] float64.  +inf unaries are legal: exp(-inf) = 0"""
    u = -np.asarray(U, F64)
    with np.errstate(all="ignore"):
        Q = co.softmax(u)
        if int(cfg["iterations"]) > 0:
            A = pair_matrix(fs, fa, cfg) if A is None else A
            for _ in range(int(cfg["iterations"])):
                Q = co.softmax(u + (A @ Q.T).T)
    return Q


def brute_force_mean_field(U, w, h, flow, cfg):
    """(d) as a double loop over every pair: the truth the matrix form is held to (tiny images only)"""
    fs, fa = features(w, h, flow)
    fs, fa = fs.astype(F64), fa.astype(F64)
    N, L = w * h, U.shape[0]
    Ks, Ka = np.zeros((N, N)), np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            Ks[i, j] = np.exp(-0.5 * sum((fs[i, q] - fs[j, q]) ** 2 for q in range(2)))
            Ka[i, j] = np.exp(-0.5 * sum((fa[i, q] - fa[j, q]) ** 2 for q in range(4)))
    Ds = [1.0 / np.sqrt(sum(Ks[i]) + 1e-20) for i in range(N)]
    Da = [1.0 / np.sqrt(sum(Ka[i]) + 1e-20) for i in range(N)]
    u = -np.asarray(U, F64)
    Q = co.softmax(u)
    for _ in range(int(cfg["iterations"])):
        nxt = np.empty_like(Q)
        for i in range(N):
            for l in range(L):
                s = sum(Ds[i] * Ks[i, j] * Ds[j] * Q[l, j] for j in range(N))
                a = sum(Da[i] * Ka[i, j] * Da[j] * Q[l, j] for j in range(N))
                nxt[l, i] = u[l, i] + 4.0 * cfg["weight_smoothness"] * s + cfg["weight_appearance"] * a
        Q = co.softmax(nxt)
    return Q


def fuse(Q, motion, proj):
    """(e): prob [L][N] float32, label [N] (the first maximum)"""
    q = np.asarray(Q).astype(F32)
    mo = np.asarray(motion, F32).ravel()
    pf = (q * mo[None]).astype(F32)
    prob = (F32(1) - ((F32(1) - pf).astype(F32) * (F32(1) - np.asarray(proj, F32)).astype(F32)).astype(F32)).astype(F32)
    return prob, co.argmax_labels(prob)


def upscale4(ids):
    return np.repeat(np.repeat(ids, 4, axis=0), 4, axis=1)


def motion_of(flow):
    """the flow engine's third output: clamp((|flow| - 0.2) / 4.8, 0, 1), float32"""
    f = np.asarray(flow, F32)
    mag = np.sqrt((f[..., 0] * f[..., 0]).astype(F32) + (f[..., 1] * f[..., 1]).astype(F32)).astype(F32)
    return np.clip(((mag - F32(0.2)) / F32(4.8)).astype(F32), F32(0), F32(1)).astype(F32)


def infer(W, H, cam, ids, T_start, T_end, vertex_z, depth, flow, motion, tracks, allow_new, new_id, cfg, A=None):
    """the whole inference.  Returns a dict of every stage; `margin` [N] is the top-two margin of prob per cell"""
    w, h = W // 4, H // 4
    M = len(ids)
    L = M + int(bool(allow_new))
    E, cell = track_errors(W, H, cam, T_start, T_end, tracks, L)
    U = unaries(E, M, allow_new, cfg["threshold"])
    proj, inv = proj_prob(depth, vertex_z, allow_new, cfg["max_err"], cfg["min_proj_prob"])
    proj64, _ = proj_prob(depth, vertex_z, allow_new, cfg["max_err"], cfg["min_proj_prob"], dtype=F64)
    fs, fa = features(w, h, flow)
    Q = mean_field(U, fs, fa, cfg, A)
    prob, label = fuse(Q, motion, proj)
    all_ids = np.array(list(ids) + ([new_id] if allow_new else []), np.uint8)
    out_ids = all_ids[label].reshape(h, w)
    s = np.sort(prob.astype(F64), axis=0)
    margin = s[-1] - s[-2] if L > 1 else np.full(w * h, np.inf)
    return dict(E=E.reshape(L, h, w), cell=cell, U=U.reshape(L, h, w), proj=proj.reshape(L, h, w), proj64=proj64.reshape(L, h, w),
                invalid=inv.reshape(h, w), Q=Q.reshape(L, h, w), prob=prob.reshape(L, h, w), label=label.reshape(h, w).astype(np.int32),
                ids=out_ids, ids_full=upscale4(out_ids), margin=margin.reshape(h, w), features=(fs, fa))


# ---- scenes ---------------------------------------------------------------------------------------------------------------
DT = 33_000_000  # ns between two frames


def camera(W, H):
    return (F32(W), F32(W), F32(W / 2 - 0.5), F32(H / 2 - 0.5))


def back_project(px, py, z, cam):
    fx, fy, cx, cy = (F64(v) for v in cam)
    return np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], -1).astype(F32)


def translation(t):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = t
    return T


def shift_of(s):
    """the pixel shift that tells model / stripe s from the others: 2-pixel steps, so that a track is an inlier (0 px, 0 px/s)
    of its own model and an outlier (>= 2 px in 33 ms = 60 px/s) of every other"""
    return 2 * (s % 8), 2 * (s // 8)


def make_scene(w, h, L, allow_new, seed, edge_tracks=True):
    """A scene of M = L - allow_new models for the CRF image w x h: the image is cut into M vertical stripes; stripe s moves
    like model s (its tracks are inliers of model s alone, its depth is model s's prediction, its flow differs from its
    neighbours').  A few percent of the pixels have no depth in the frame and in every model.  With edge_tracks the table ends
    with: two tracks on one cell, a null slot, a NaN coordinate, an end pixel outside the frame, the wrap (x_end = W - 1) and the
    dropped index (x_end = W - 1, y_end = H - 1), and one pair of equal stamps and equal pixels (0 / 0)."""
    rng = np.random.default_rng(seed)
    W, H = 4 * w, 4 * h
    cam = camera(W, H)
    M = L - int(bool(allow_new))
    assert M >= 1
    Z0 = 1.5
    yy, xx = np.mgrid[0:H, 0:W]
    stripe_full = np.minimum(xx * M // W, M - 1)
    depth = (Z0 + 0.1 * np.sin(xx / 37.0) * np.cos(yy / 29.0)).astype(F32)
    hole = rng.random((H, W)) < 0.03
    depth[hole] = 0
    vz = np.empty((M, H, W), F32)
    for m in range(M):
        off = np.where(stripe_full == m, rng.uniform(0, 0.012, (H, W)), rng.uniform(0.02, 0.06, (H, W)))
        vz[m] = np.where(hole, 0, depth + off.astype(F32))
    cy_, cx_ = np.mgrid[0:h, 0:w]
    stripe = np.minimum(cx_ * 4 * M // W, M - 1)
    flow = np.stack([0.8 + 0.45 * (stripe % 5) + 0.002 * cx_, 0.5 + 0.4 * (stripe // 5) + 0.003 * cy_], -1)
    flow = (flow + rng.normal(0, 0.03, flow.shape)).astype(F32)
    motion = motion_of(flow)
    # tracks on a jittered grid: the end pixel, its stripe's shift back to the start pixel
    gx, gy = np.meshgrid(np.arange(6, W - 6, 11), np.arange(5, H - 5, 9))
    ex = (gx + rng.integers(-2, 3, gx.shape)).ravel()
    ey = (gy + rng.integers(-2, 3, gy.shape)).ravel()
    fxs = F64(cam[0])
    unit = Z0 / fxs  # metres per pixel at Z0
    st = np.minimum(ex * M // W, M - 1)
    n0 = len(ex)
    co_cur = back_project(ex.astype(F64), ey.astype(F64), np.full(n0, Z0), cam)
    sh = np.array([shift_of(s) for s in st], F64).reshape(-1, 2)  # (an image too small for the grid has no such track)
    co_prev = (co_cur.astype(F64) - np.concatenate([sh * unit, np.zeros((n0, 1))], 1)).astype(F32)
    # model m: T_start = identity, T_end takes the model's own motion out again
    T_start = [np.eye(4, dtype=F32) for _ in range(M)]
    T_end = [translation([-shift_of(m)[0] * unit, -shift_of(m)[1] * unit, 0.0]) for m in range(M)]
    xy_cur = np.stack([ex, ey], 1).astype(np.int32)
    xy_prev = (xy_cur - sh.astype(np.int32)).astype(np.int32)
    ts_prev = np.full(n0, 1_000_000_000, np.int64)
    ts_cur = ts_prev + DT
    ok_cur, ok_prev = np.ones(n0, np.int32), np.ones(n0, np.int32)
    tr = dict(xy_cur=xy_cur, co_cur=co_cur, ts_cur=ts_cur, ok_cur=ok_cur, xy_prev=xy_prev, co_prev=co_prev, ts_prev=ts_prev, ok_prev=ok_prev)
    if edge_tracks:
        def add(px_end, py_end, px_start, py_start, ok=(1, 1), nan=False, dt=DT):
            c1 = back_project(F64(px_end), F64(py_end), F64(Z0), cam)
            c0 = back_project(F64(px_start), F64(py_start), F64(Z0), cam)
            if nan:
                c0 = c0.copy()
                c0[1] = np.nan
            for key, val in (("xy_cur", [px_end, py_end]), ("xy_prev", [px_start, py_start]), ("co_cur", c1), ("co_prev", c0)):
                tr[key] = np.concatenate([tr[key], np.asarray(val, tr[key].dtype)[None]])
            tr["ts_prev"] = np.append(tr["ts_prev"], np.int64(1_000_000_000))
            tr["ts_cur"] = np.append(tr["ts_cur"], np.int64(1_000_000_000 + dt))
            tr["ok_cur"] = np.append(tr["ok_cur"], np.int32(ok[0]))
            tr["ok_prev"] = np.append(tr["ok_prev"], np.int32(ok[1]))
        add(9, 9, 9, 9), add(10, 8, 12, 8)          # two tracks on cell (2, 2): the later one (60 px/s for model 0) wins
        add(13, 5, 13, 5, ok=(1, 0))                 # a null start slot
        add(17, 5, 17, 5, ok=(0, 1))                 # a null end slot
        add(21, 5, 21, 5, nan=True)                  # a NaN coordinate
        add(W + 3, 6, W - 2, 6)                      # the end pixel outside the frame
        add(W - 1, 10, W - 1, 10)                    # the column w: wraps into the next row
        add(W - 1, H - 1, W - 1, H - 1)              # ... and past the last cell: dropped
        add(2, 13, 2, 13), add(6, 13, 6, 13)         # x = 2 -> column 0 (half to even), x = 6 -> column 2
        add(14, 14, 14, 14, dt=0)                    # equal stamps, equal pixels: 0 / 0
        add(26, 14, 25, 14, dt=0)                    # equal stamps: +inf
    ids = [0] + [3 + 2 * m for m in range(1, M)]
    new_id = 3 + 2 * M
    return dict(W=W, H=H, w=w, h=h, cam=cam, ids=ids, new_id=new_id, allow_new=bool(allow_new), T_start=T_start, T_end=T_end,
                vertex_z=vz, depth=depth, flow=flow, motion=motion, tracks=tr)


def run_scene(sc, cfg, A=None):
    return infer(sc["W"], sc["H"], sc["cam"], sc["ids"], sc["T_start"], sc["T_end"], sc["vertex_z"], sc["depth"], sc["flow"],
                 sc["motion"], sc["tracks"], sc["allow_new"], sc["new_id"], cfg, A)


def rectangle_scene(hole):
    """The scene whose answer is known, 48 x 36 cells, one model (the camera's) and the new label: a rectangle moves by (2, 1)
    flow pixels over a still background; the tracks inside it move by (8, 4) frame pixels (outliers of the still camera model),
    the tracks on the background do not move (inliers); the depth equals the model's prediction everywhere.  With `hole` the
    rectangle has no depth in the frame nor in the prediction (both 0: `invalid`); without, both are the same plane."""
    w, h = 48, 36
    W, H = 4 * w, 4 * h
    cam = camera(W, H)
    rx0, rx1, ry0, ry1 = 16, 34, 10, 26  # cells
    flow = np.zeros((h, w, 2), F32)
    flow[ry0:ry1, rx0:rx1] = (2, 1)
    depth = np.full((H, W), 1.5, F32)
    if hole:
        depth[4 * ry0:4 * ry1, 4 * rx0:4 * rx1] = 0
    vz = depth[None].copy()
    gx, gy = np.meshgrid(np.arange(4, W - 12, 8), np.arange(4, H - 8, 8))
    ex, ey = gx.ravel(), gy.ravel()
    inside = (ex // 4 >= rx0) & (ex // 4 < rx1) & (ey // 4 >= ry0) & (ey // 4 < ry1)
    sx, sy = ex - 8 * inside, ey - 4 * inside
    n = len(ex)
    tr = dict(xy_cur=np.stack([ex, ey], 1).astype(np.int32), xy_prev=np.stack([sx, sy], 1).astype(np.int32),
              co_cur=back_project(ex.astype(F64), ey.astype(F64), np.full(n, 1.5), cam),
              co_prev=back_project(sx.astype(F64), sy.astype(F64), np.full(n, 1.5), cam),
              ts_prev=np.full(n, 1_000_000_000, np.int64), ts_cur=np.full(n, 1_000_000_000 + DT, np.int64),
              ok_cur=np.ones(n, np.int32), ok_prev=np.ones(n, np.int32))
    sc = dict(W=W, H=H, w=w, h=h, cam=cam, ids=[0], new_id=1, allow_new=True, T_start=[np.eye(4, dtype=F32)], T_end=[np.eye(4, dtype=F32)],
              vertex_z=vz, depth=depth, flow=flow, motion=motion_of(flow), tracks=tr)
    return sc, (rx0, rx1, ry0, ry1)


# the device test's scenes: (w, h, labels), each with and without the new label (one label: without only).  8 x 8; 44 x 12
# crosses x / 40 with N no multiple of 64; 43 x 25; 80 x 60 crosses y / 40 as well
GPU_CASES = [c + (a,) for c in [(8, 8, 1), (8, 8, 2), (44, 12, 3), (43, 25, 2), (43, 25, 9), (80, 60, 3), (80, 60, 32)]
             for a in (False, True) if c[2] > 1 or not a]


def case_scene(w, h, L, allow_new):
    """the scene and configuration of a device case (the large images run two mean-field iterations: the oracle's N x N
    matrices cost seconds each)"""
    return make_scene(w, h, L, allow_new, seed=w + L), config(iterations=2 if w * h > 2000 else 10)
