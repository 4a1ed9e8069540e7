"""Correspondence sets for the RigidRANSAC core and the device verifier: the sizes at which the kernel takes another
path (a wave's 64 lanes, its LDS capacity) and the kinds of input at which a fit or the hash order can go wrong."""
import numpy as np

SIZES = [3, 4, 5, 6, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 700, 1023, 1024]
KINDS = ["noise", "outliers30", "all_outliers", "duplicates", "signed_zeros", "coincident", "collinear", "coplanar", "mirrored"]
CONFIG = (10, 0.03, 0.8)  # MultiMotionFusion.cpp:513


def _rigid(rng):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-1, 1) * np.pi
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K, rng.uniform(-1, 1, 3)


def make(kind, n, rng):
    """(p0, p1): float32 [n, 3] with p0 ~ R p1 + t where the kind allows it."""
    R, t = _rigid(rng)
    p1 = rng.uniform(-1, 1, (n, 3))
    if kind == "collinear":
        p1 = np.outer(rng.uniform(-1, 1, n), rng.normal(size=3)) + rng.uniform(-1, 1, 3)
    elif kind == "coplanar":
        a, b = rng.normal(size=3), rng.normal(size=3)
        p1 = np.outer(rng.uniform(-1, 1, n), a) + np.outer(rng.uniform(-1, 1, n), b) + rng.uniform(-1, 1, 3)
    elif kind == "coincident":
        p1 = np.tile(rng.uniform(-1, 1, 3), (n, 1))
    p0 = p1 @ R.T + t + rng.normal(size=(n, 3)) * 0.0005  # 0.5 mm
    if kind == "outliers30":
        bad = rng.random(n) < 0.3
        p0[bad] = rng.uniform(-2, 2, (int(bad.sum()), 3))
    elif kind == "all_outliers":
        p0 = rng.uniform(-2, 2, (n, 3))
    elif kind == "mirrored":
        p0 = (p1 * np.array([1.0, 1.0, -1.0])) @ R.T + t  # a reflection: the det < 0 branch of the fit
    elif kind == "coincident":
        p0 = np.tile(p0[0], (n, 1))
    p0, p1 = p0.astype(np.float32), p1.astype(np.float32)
    if kind == "duplicates":  # equal rows: equal hashes, ordered by index
        for i in range(1, n, 2):
            p0[i], p1[i] = p0[i - 1], p1[i - 1]
    elif kind == "signed_zeros":  # +-0.0 hash alike and compare equal
        p0[::2, 0], p1[::3, 1] = 0.0, -0.0
        p0[1::4, 2] = -0.0
    return p0, p1


def problems(repeats, seed=0):
    """repeats x sizes x kinds problems, as a list of (kind, p0, p1)."""
    rng = np.random.default_rng(seed)
    return [(k, *make(k, n, rng)) for _ in range(repeats) for n in SIZES for k in KINDS]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
