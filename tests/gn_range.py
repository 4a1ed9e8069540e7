"""Shared by tests/test_gpu_gn_range.py and tests/test_gn_range_oracle.py: the input regimes that take the one-launch
Gauss-Newton chain (csrc/gn_fused.hpp) to the edges of its number ranges, the oracle's sums of ONE pass at a given pose, and
a float64 restatement of the solve and pose update the oracle runs between two passes (oracle/mmf_oracle.c,
orc_odom_get_incremental_transformation: ldlt solve, orc_rodrigues, the 4x4 product, the isometry inverse, K R K^-1, K t).

Every regime is array arithmetic on synth.render output; nothing here needs a GPU."""
import functools
import os

import numpy as np

from helpers import ANGLE_THRESH, DIST_THRESH, frame_pair, se3_sum_tolerance

REGIMES = ("R1", "R1r", "R2", "R3", "R3h", "R4", "R5", "R6", "R7", "R8a", "R8b")
SIZES = {"R1r": (176, 144), "R4": (640, 480)}  # everything else 160 x 120
ICP_WEIGHT = 10.0
SOBEL_SCALE = 0.125                # RGBDOdometry.cpp:31-32
MAX_DEPTH_DELTA = np.float32(0.07)  # :33
MIN_GRAD = (5.0, 3.0, 1.0)         # :103-105


class Regime:
    """w, h, K, model (the model's pose = the pose tracking starts from, float32 4x4), fp / fc (the model's and the sensor's
    frame: vertex, normal, rgb / depth, rgb), cutoff (the depth cut-off of initICP)."""


def _scaled(f, s):
    f = dict(f)
    f["depth"] = (f["depth"] * np.float32(s)).astype(np.float32)
    v = f["vertex"].copy()
    v[..., :3] *= np.float32(s)
    f["vertex"] = v
    return f


@functools.lru_cache(maxsize=None)
def regime(name):
    r = Regime()
    r.name = name
    r.w, r.h = SIZES.get(name, (160, 120))
    r.K, prev, cur, fp, fc = frame_pair(r.w, r.h, seed=1)
    fp, fc = dict(fp), dict(fc)
    r.model = prev.astype(np.float32).copy()
    r.cutoff = 15.0
    if name == "R2":    # near: the scene at 0.2 - 0.5 m
        fp, fc = _scaled(fp, 0.15), _scaled(fc, 0.15)
        r.model[:3, 3] *= np.float32(0.15)
    elif name == "R3":  # far: 5 - 14 m
        fp, fc = _scaled(fp, 4.0), _scaled(fc, 4.0)
        r.model[:3, 3] *= np.float32(4.0)
        r.cutoff = 60.0
    elif name == "R3h":  # half as far, 2.6 - 7 m: at x 4 the coarsest level has no ICP inlier and the whole chain is NaN on both sides
        fp, fc = _scaled(fp, 2.0), _scaled(fc, 2.0)
        r.model[:3, 3] *= np.float32(2.0)
        r.cutoff = 60.0
    elif name == "R4":  # an exposure step over the whole image: sum diff^2 passes 2^31 at level 0
        # (rgb // 2 alone passes the gradient test at some 13 000 pixels of 640 x 480, and no step of a byte brings those to
        # 2^31: two-pixel stripes of 40 grey levels, fixed to the image, let nearly every pixel take part)
        off = 100
        yy, xx = np.mgrid[0:r.h, 0:r.w]
        stripes = (((xx // 2 + yy // 2) % 2) * 40).astype(np.uint8)[..., None]
        fp["rgb"] = fp["rgb"] // 2 + stripes
        fc["rgb"] = (fc["rgb"] // 2 + stripes + off).astype(np.uint8)
    elif name == "R5":  # one textured patch in a flat image, and an exposure step: few correspondences with a large |d|
        y0, x0, n, off = 48, 68, 24, 120
        for f, base in ((fp, 60), (fc, 60 + off)):
            img = np.full_like(f["rgb"], base)
            img[y0:y0 + n, x0:x0 + n] = f["rgb"][y0:y0 + n, x0:x0 + n] // 2 + (base - 60)
            f["rgb"] = img
    elif name == "R6":  # the same frame twice, no motion: sum diff^2 = 0, the sigma = 1 branch
        fc = fp
    elif name == "R7":  # flat and black: no photometric correspondence at all (0 / 0).  (A flat grey image still has the
        # derivative's border response: 273 correspondences of difference 0, which is R6's branch.)
        fp["rgb"] = np.zeros_like(fp["rgb"])
        fc["rgb"] = np.zeros_like(fc["rgb"])
    elif name in ("R8a", "R8b"):  # large global coordinates in the ICP rows
        r.model[0, 3] += np.float32(10.0 if name == "R8a" else 50.0)
    for f in (fp, fc):
        for v in f.values():
            v.setflags(write=False)
    r.fp, r.fc = fp, fc
    return r


def setup(od, up, r, model=None):
    """The per-frame call sequence of Model::initICP (Model.cpp:390-407) on the product's or the oracle's odometry."""
    model = r.model if model is None else model
    product = hasattr(od, "buildDepthPyramid")
    od.initFirstRGB(up(r.fp["rgb"]))
    if product:
        od.initICPModel(up(r.fp["vertex"]), up(r.fp["normal"]), r.cutoff, model)
        od.initRGBModel(up(r.fp["rgb"]))
        od.buildDepthPyramid(up(r.fc["depth"]))
        od.initICP(depthCutoff=r.cutoff)
    else:
        od.initICPModel(r.fp["vertex"], r.fp["normal"], model)
        od.initRGBModel(r.fp["rgb"])
        od.initICP(r.fc["depth"], r.cutoff)
    od.initRGB(up(r.fc["rgb"]))
    return od


def oracle_odometry(orc, r, model=None):
    K = r.K
    return setup(orc.Odometry(r.w, r.h, K["cx"], K["cy"], K["fx"], K["fy"]), lambda a: a, r, model)


def level_intrinsics(K, level):
    d = np.float32(1 << level)
    return tuple(np.float32(K[k]) / d for k in ("fx", "fy", "cx", "cy"))


def inverse3f(orc, R):
    import ctypes as C
    m = np.ascontiguousarray(np.reshape(R, 9), np.float32)
    out = np.zeros(9, np.float32)
    orc.lib().orc_inverse3f(m.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def oracle_pass(orc, o, r, level, pose24, model=None):
    """One pass of the oracle at pyramid `level` with the pose (Rcurr[9], tcurr[3], krkinv[9], kt[3]) given: the 29 ICP sums
    (icpStep), the correspondence pass's {count, sum diff^2 as the reference's int}, the 29 photometric sums (rgbStep)."""
    model = r.model if model is None else model
    fx, fy, cx, cy = level_intrinsics(r.K, level)
    pose24 = np.asarray(pose24, np.float32)
    Rcurr, tcurr, krkinv, kt = pose24[:9], pose24[9:12], pose24[12:21], pose24[21:24]
    icp, _ = orc.icp_step(Rcurr, tcurr, o.buffer("vmaps_curr", level), o.buffer("nmaps_curr", level), inverse3f(orc, model[:3, :3]),
                          model[:3, 3], fx, fy, cx, cy, o.buffer("vmaps_g_prev", level), o.buffer("nmaps_g_prev", level),
                          DIST_THRESH, ANGLE_THRESH)
    dIdx, dIdy = orc.derivative_images(o.buffer("next_image", level))  # (the odometry's own are made by its tracking call, :230-235)
    last_depth = o.buffer("last_depth", level)
    min_scale = np.float32(MIN_GRAD[level] ** 2 / SOBEL_SCALE ** 2)
    corres, sumsq, count, _ = orc.rgb_residual(min_scale, dIdx, dIdy, last_depth, o.buffer("next_depth", level),
                                               o.buffer("last_image", level), o.buffer("next_image", level), MAX_DEPTH_DELTA, kt, krkinv)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.float32(np.sqrt(np.float64(sumsq)) / np.float64(count)) if count else np.float32(np.nan)  # RGBDOdometry.cpp:373
    sigma_val = 1.0 if err == 0 else float(count)
    rgb = orc.rgb_step(corres, sigma_val, orc.project_to_cloud(last_depth, fx, fy, cx, cy), fx, fy, dIdx, dIdy, SOBEL_SCALE)
    return dict(icp=icp, rgb=rgb, count=count, sumsq=sumsq)


def unpack(out29):
    """The 29 sums as the symmetric A (6 x 6) and b (reduce.cu:458-472), float64."""
    A, b = np.zeros((6, 6)), np.zeros(6)
    k = 0
    for i in range(6):
        for j in range(i, 7):
            if j == 6:
                b[i] = out29[k]
            else:
                A[i, j] = A[j, i] = out29[k]
            k += 1
    return A, b


def combined_system(p, w=ICP_WEIGHT):
    """A = A_rgb + w^2 A_icp, b = b_rgb + w b_icp (RGBDOdometry.cpp:431-435) and the bound of the float32 sums' error in
    each entry (helpers.se3_sum_tolerance of either term)."""
    Ai, bi = unpack(p["icp"])
    Ar, br = unpack(p["rgb"])
    dAi, dbi = unpack(se3_sum_tolerance(p["icp"]))
    dAr, dbr = unpack(se3_sum_tolerance(p["rgb"]))
    return Ar + w * w * Ai, br + w * bi, dAr + w * w * dAi, dbr + w * dbi


def one_iteration_bound(p, pose):
    """How far one Gauss-Newton step can move when every sum is off by its tolerance: |A^-1| (|db| + |dA| |x|) (2-norms,
    Frobenius for dA) plus 4 float32 ulps of the pose entries for the casts.  From the oracle's sums only."""
    A, b, dA, db = combined_system(p)
    try:
        Ainv = np.linalg.inv(A)
    except np.linalg.LinAlgError:
        return np.inf
    x = Ainv @ b
    dx = np.linalg.norm(Ainv, 2) * (np.linalg.norm(db) + np.linalg.norm(dA) * np.linalg.norm(x))
    if not np.isfinite(dx):
        return np.inf
    return dx + 4 * float(np.spacing(np.float32(np.abs(np.asarray(pose, np.float64)).max())))


class max_gn_iters:
    """`with max_gn_iters(n):` the oracle stops after n solved iterations (it reads the variable on every call)."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.saved = os.environ.get("ORC_MAX_GN_ITERS")
        os.environ["ORC_MAX_GN_ITERS"] = str(self.n)

    def __exit__(self, *exc):
        if self.saved is None:
            del os.environ["ORC_MAX_GN_ITERS"]
        else:
            os.environ["ORC_MAX_GN_ITERS"] = self.saved
        return False


# ---- (e): the solve and the pose update in float64 ------------------------------------------------------------------------
def rodrigues64(rv):
    """orc_rodrigues (OdometryProvider.h:32-67): the literal form, identity below DBL_EPSILON (and for a NaN)."""
    rv = np.asarray(rv, np.float64)
    theta = np.sqrt(rv @ rv)
    if not theta >= np.finfo(np.float64).eps:
        return np.eye(3)
    k = rv / theta
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * kx


def solve64(A, b):
    """np.linalg.solve; a singular matrix or a non-finite component makes the whole solution NaN, as the substitution passes
    of an LDL^T solve carry such a value into every component."""
    try:
        with np.errstate(all="ignore"):
            x = np.linalg.solve(np.asarray(A, np.float64).reshape(6, 6), np.asarray(b, np.float64))
    except np.linalg.LinAlgError:
        return np.full(6, np.nan)
    return x if np.isfinite(x).all() else np.full(6, np.nan)


def running_transform64(A, b, rt):
    """resultRt <- [R(x[3:6]) | x[0:3]; 0 0 0 1] resultRt (OdometryProvider.h:69-89): the three rows that change."""
    x = solve64(A, b)
    upd = np.eye(4)
    upd[:3, :3] = rodrigues64(x[3:])
    upd[:3, 3] = x[:3]
    with np.errstate(all="ignore"):
        return (upd @ np.asarray(rt, np.float64).reshape(4, 4))[:3]


def pose_from_transform(N, Rprev, tprev, intr):
    """Rcurr, tcurr (float32 products in the order the oracle states them, mmf_oracle.c:1183-1200) and K R K^-1, K t of the
    inverse running transform (float64, cast at the end, :1100-1111) from the transform's three rows N (3 x 4)."""
    f = np.float32
    N = np.asarray(N, np.float64).reshape(3, 4)
    Rprev, tprev = np.asarray(Rprev, f).reshape(3, 3), np.asarray(tprev, f)
    with np.errstate(all="ignore"):
        Ro, to = N[:, :3].astype(f), N[:, 3].astype(f)
        RoT = Ro.T
        ti = [f(f(f(-RoT[r, 0] * to[0]) + f(-RoT[r, 1] * to[1])) + f(-RoT[r, 2] * to[2])) for r in range(3)]
        Rcurr, tcurr = np.zeros((3, 3), f), np.zeros(3, f)
        for r in range(3):
            for j in range(3):
                s = f(0)
                for k in range(3):
                    s = f(s + f(Rprev[r, k] * RoT[k, j]))
                Rcurr[r, j] = s
            s = f(0)
            for k in range(3):
                s = f(s + f(Rprev[r, k] * ti[k]))
            tcurr[r] = f(s + tprev[r])
        fx, fy, cx, cy = (float(v) for v in intr)
        Kd = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        if np.isfinite(N).all() and abs(np.linalg.det(N[:, :3])) > 0:
            Ri = np.linalg.inv(N[:, :3])
        else:
            Ri = np.full((3, 3), np.nan)
        t3 = -(Ri @ N[:, 3])
        krkinv = Kd @ Ri @ np.linalg.inv(Kd)
        kt = Kd @ t3
        # what float64 itself leaves in the entries that are differences of larger terms
        floor = 64 * np.finfo(np.float64).eps * (fx + fy + cx + cy + 1) * max(1.0, np.abs(Ri).max() if np.isfinite(Ri).all() else 1.0) * (
            1.0 + (np.abs(N[:, 3]).max() if np.isfinite(N).all() else 0.0))
    return np.concatenate([Rcurr.ravel(), tcurr, krkinv.ravel().astype(f), kt.astype(f)]), floor


def solver_systems(seed=11, n_random=160):
    """The batch of (e): dicts of A (6 x 6), b, rt (4 x 4), Rprev, tprev, kind."""
    from multimotionfusion_amd import synth
    rng = np.random.default_rng(seed)
    out = []

    def rigid(scale_t=1.0):
        return synth.make_pose(rng.normal(size=3) * 0.3, rng.normal(size=3) * scale_t).astype(np.float64)

    def spd(cond):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = (Q * np.logspace(0, -np.log10(cond), 6)) @ Q.T * 10.0 ** rng.uniform(0, 6)
        return 0.5 * (A + A.T)

    def add(kind, A, b, rt=None):
        P = rigid()
        out.append(dict(kind=kind, A=np.asarray(A, np.float64), b=np.asarray(b, np.float64), rt=rigid() if rt is None else rt,
                        Rprev=P[:3, :3].astype(np.float32), tprev=P[:3, 3].astype(np.float32)))

    for k in range(n_random):  # SPD systems, condition numbers 1e2 .. 1e12, increments of a tracked frame and larger ones
        A = spd(10.0 ** rng.uniform(2, 12))
        x = np.concatenate([rng.normal(size=3), rng.normal(size=3)]) * 10.0 ** rng.uniform(-4, -0.5)
        add("spd", A, A @ x)
    e = np.eye(6) * 4.0  # x = b / 4 exactly: |r|^2 lands where it is put
    below, above = np.nextafter(0.125, 0.0), np.nextafter(0.125, 1.0)
    for kind, rx in (("y=1/64", 0.125), ("y<1/64", below), ("y>1/64", above), ("y=0.0153", 0.1237), ("y=0.0159", 0.1261),
                     ("y=0.2", np.sqrt(0.2)), ("y=0.3", np.sqrt(0.3))):
        for axis in range(3):
            x = np.array([0.01, -0.02, 0.03, 0, 0, 0], np.float64)
            x[3 + axis] = rx
            add(kind, e, 4.0 * x)
    for s in (1e-17, 1e-16, 2.2e-16, 3e-16, 1e-9):  # |r| around DBL_EPSILON: the identity on one side of it
        add("tiny", e, 4.0 * np.array([1e-3, 2e-3, -1e-3, s, 0, 0]))
        add("tiny", e, 4.0 * np.array([0, 0, 0, s * 0.6, -s * 0.5, s * 0.62]))
    for rv in ([np.pi, 0, 0], [0, -np.pi * 0.999, 0], [1.8, 1.8, 1.8], [0, 0, np.pi * 1.001]):  # |r| ~ pi
        add("pi", e, 4.0 * np.array([0.1, 0.2, -0.1] + rv))
    # a single plane z = 0 with normal (0, 0, 1): rows (0, 0, 1, y, -x, 0), rank 3, exactly representable
    pts = rng.integers(-8, 9, size=(40, 2)).astype(np.float64)
    J = np.stack([0 * pts[:, 0], 0 * pts[:, 0], 1 + 0 * pts[:, 0], pts[:, 1], -pts[:, 0], 0 * pts[:, 0]], 1)
    add("rank3", J.T @ J, J.T @ rng.integers(-3, 4, size=40).astype(np.float64))
    add("zero", np.zeros((6, 6)), np.zeros(6))
    add("zero", np.zeros((6, 6)), np.ones(6))
    bn = np.array([1e-3, 2e-3, np.nan, 1e-3, 0, 0])
    add("nan-b", spd(1e3), bn)
    add("nan-b", e, np.array([np.nan] + [1e-3] * 5))
    add("inf-b", e, np.array([1e-3, np.inf, 0, 0, 0, 0]))
    return out


def start_pose24(r):
    """The pose a chain without SO3 pre-alignment begins with: Rcurr, tcurr = the model's pose, K R K^-1 = 1, K t = 0."""
    return np.concatenate([r.model[:3, :3].ravel(), r.model[:3, 3], np.eye(3, dtype=np.float32).ravel(), np.zeros(3, np.float32)])


# ---- (d): an ICP term that leaves the fixed-point range -----------------------------------------------------------------
GN_ICP_PARTIAL_LIMIT = 2.0 ** 23  # kGnSumIcpExp = 30: |partial| x 2^30 must stay below 2^53
GN_PIXELS_PER_GROUP = 256         # 160 x 120 at level 0: one pixel per lane, 256 pixel lanes per workgroup (gn_geometry)


@functools.lru_cache(maxsize=None)
def scaled_identical(scale):
    """R6 (the same frame twice, no motion) with depth, vertices and the pose translation scaled: icpStep's rotational rows are
    v x n with v in the model's camera frame, so only a deeper scene makes them larger (a translated pose never enters them).
    With identical frames the correspondences keep coinciding pixel for pixel at level 0, whatever the scale."""
    base = regime("R6")
    r = Regime()
    r.name, r.w, r.h, r.K = f"R6x{scale}", base.w, base.h, base.K
    r.fp = _scaled(base.fp, float(scale))
    r.fc = r.fp
    r.model = base.model.copy()
    r.model[:3, 3] *= np.float32(scale)
    r.cutoff = 15.0 * scale
    for v in r.fp.values():
        v.setflags(write=False)
    return r


def icp_group_partials(orc, o, r, level=0, pixels=GN_PIXELS_PER_GROUP):
    """The oracle's own icpStep over every run of `pixels` consecutive pixels alone (the sensor's vertices outside the run set
    to NaN) at the start pose: the largest |sum| of the 27 products per run -- what one workgroup of the first launch adds up --
    and the inliers per run."""
    fx, fy, cx, cy = level_intrinsics(r.K, level)
    vc, nc = o.buffer("vmaps_curr", level), o.buffer("nmaps_curr", level)
    vp, npv = o.buffer("vmaps_g_prev", level), o.buffer("nmaps_g_prev", level)
    rows, cols = vc.shape[0] // 3, vc.shape[1]
    Rinv = inverse3f(orc, r.model[:3, :3])
    largest, inliers = [], []
    for k0 in range(0, rows * cols, pixels):
        keep = np.zeros(rows * cols, bool)
        keep[k0:k0 + pixels] = True
        v = np.where(np.tile(keep.reshape(rows, cols), (3, 1)), vc, np.float32(np.nan))
        out, _ = orc.icp_step(r.model[:3, :3], r.model[:3, 3], v, nc, Rinv, r.model[:3, 3], fx, fy, cx, cy, vp, npv, DIST_THRESH, ANGLE_THRESH)
        largest.append(float(np.abs(out[:27]).max()))
        inliers.append(int(out[28]))
    return np.array(largest), np.array(inliers)


@functools.lru_cache(maxsize=None)
def out_of_range_scale(orc):
    """The smallest scale, in steps of 50, at which some workgroup's partial is beyond TWICE the limit by the oracle's rows
    (the float32 partial of the launch differs from the oracle's double by parts in 1e5, not by a factor)."""
    for scale in range(50, 1001, 50):
        r = scaled_identical(scale)
        o = oracle_odometry(orc, r)
        largest, inliers = icp_group_partials(orc, o, r)
        o.close()
        if largest.max() > 2 * GN_ICP_PARTIAL_LIMIT:
            return scale, float(largest.max()), int(inliers.sum())
    raise AssertionError("no scale up to 1000 takes an ICP partial out of range")
