"""numpy restatement of restoring a model's dense surfels: PLY records back into the 12-float AoS that
mmf_model_download_map returns, and the timestamps of a store set to one time.  Built on the arithmetic of
tests/modeldb_oracle.py (the export's: the import uses the same products and sums).  Test infrastructure only."""
import numpy as np

import modeldb_oracle as mo

IDENTITY = np.eye(4, dtype=np.float32)


def import_cloud(records, pose, confidence, time):
    """records (mo.CLOUD_DTYPE) -> surfels [n,12] float32: record i = surfel i.  pose None = identity, the same arithmetic."""
    r = np.ascontiguousarray(records, mo.CLOUD_DTYPE).reshape(-1)
    P = IDENTITY if pose is None else mo.f32(pose).reshape(4, 4)
    s = np.zeros((len(r), 12), np.float32)
    s[:, 0:3] = mo.apply_pose(P, np.stack([r["x"], r["y"], r["z"]], 1))
    s[:, 3] = np.float32(confidence)
    c = r["red"].astype(np.uint32) << 16 | r["green"].astype(np.uint32) << 8 | r["blue"].astype(np.uint32)
    s[:, 4] = c.astype(np.float32)  # exact: below 2^24
    s[:, 5] = 0.0
    s[:, 6] = s[:, 7] = np.float32(time)
    s[:, 8:11] = mo.rotate_negated(P, np.stack([r["nx"], r["ny"], r["nz"]], 1))
    s[:, 11] = r["radius"]
    return s


def set_timestamps(surfels, time):
    """timestamp = time for every surfel; initTime and everything else stay"""
    s = mo.f32(surfels).reshape(-1, 12).copy()
    s[:, 7] = np.float32(time)
    return s


def surfels_equal(a, b):
    """bit for bit as uint32, except that a lane that is NaN in both counts as equal"""
    a, b = mo.f32(a).reshape(-1, 12), mo.f32(b).reshape(-1, 12)
    if a.shape != b.shape:
        return False
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return bool(same.all())


def make_records(n, seed, special=True):
    """n records: positions in front of a camera at the origin (z in 0.8 .. 2.2), unit-scale normals without a zero component,
    random colours.  special: the first records carry the values a decoder can get wrong -- +-inf and denormal positions, -0.0,
    NaN, and colours at both ends of every channel."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, mo.CLOUD_DTYPE)
    r["x"], r["y"] = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n)
    r["z"] = rng.uniform(0.8, 2.2, n)
    for k in ("nx", "ny", "nz"):
        r[k] = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)
    r["radius"] = rng.uniform(0.002, 0.02, n)
    for k in ("red", "green", "blue"):
        r[k] = rng.integers(0, 256, n)
    if special:
        edge = [(np.inf, -np.inf, 1.0), (np.float32(1e-41), np.float32(-1e-41), np.float32(1e-45)), (-0.0, 0.0, -0.0),
                (np.nan, 1.0, 1.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), (2.0, 2.0, 2.0)]
        colours = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0)]
        for i, (p, c) in enumerate(zip(edge, colours)):
            if i < n:
                r["x"][i], r["y"][i], r["z"][i] = p
                r["red"][i], r["green"][i], r["blue"][i] = c
        if n > 8:
            r["nx"][8], r["ny"][8], r["nz"][8] = 0.0, -0.0, 1.0  # a zero normal component
    return r


def inverse_rigid(pose):
    """[R^T | -R^T t] of a rigid pose, in double, rounded to float32 once"""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = P[:3, :3].T
    out[:3, 3] = -P[:3, :3].T @ P[:3, 3]
    return out.astype(np.float32)
