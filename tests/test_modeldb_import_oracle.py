"""CPU: the numpy oracle of restoring dense surfels (tests/modeldb_import_oracle.py) against the semantics of DESIGN.md 4.11:
where every field of a record lands, on which records import then export is the identity and on which it is not, and what
float arithmetic guarantees for a rigid pose and its inverse."""
import numpy as np

import modeldb_import_oracle as io
import modeldb_oracle as mo

U = 2.0 ** -24  # unit round-off of float32


def test_every_field_lands_where_the_layout_says():
    r = np.zeros(4, mo.CLOUD_DTYPE)
    r["x"], r["y"], r["z"] = [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]
    r["nx"], r["ny"], r["nz"] = [0.5, 0.25, -0.5, 1], [-1, 2, 4, 0.125], [3, -3, 0.75, -0.75]
    r["radius"] = [0.01, 0.02, 0.03, 0.04]
    r["red"], r["green"], r["blue"] = [0, 255, 255, 1], [0, 255, 0, 2], [0, 255, 0, 3]
    for pose in (None, io.IDENTITY):
        s = io.import_cloud(r, pose, 7.5, 42)
        assert s.dtype == np.float32 and s.shape == (4, 12)
        assert np.array_equal(s[:, 0:3], np.stack([r["x"], r["y"], r["z"]], 1))
        assert np.array_equal(s[:, 3], np.full(4, 7.5, np.float32))
        assert s[:, 4].tolist() == [0.0, float(0xFFFFFF), float(0xFF0000), float(0x010203)]  # r << 16 | g << 8 | b
        assert np.array_equal(s[:, 5], np.zeros(4, np.float32))
        assert np.array_equal(s[:, 6], np.full(4, 42, np.float32)) and np.array_equal(s[:, 7], s[:, 6])  # initTime = timestamp
        assert np.array_equal(s[:, 8:11], -np.stack([r["nx"], r["ny"], r["nz"]], 1))  # the export negates, the import negates back
        assert np.array_equal(s[:, 11], r["radius"])
    for ch, shift in (("red", 16), ("green", 8), ("blue", 0)):  # each channel alone, at both ends
        for v in (0, 255):
            one = np.zeros(1, mo.CLOUD_DTYPE)
            one[ch] = v
            assert io.import_cloud(one, None, 1, 1)[0, 4] == np.float32(v << shift)
    # a translation lands in the position only; a rotation about z by 90 degrees turns x into y
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = [10, 20, 30]
    s = io.import_cloud(r, P, 1, 1)
    assert np.array_equal(s[:, 0:3], np.stack([r["x"] + 10, r["y"] + 20, r["z"] + 30], 1))
    assert np.array_equal(s[:, 8:11], -np.stack([r["nx"], r["ny"], r["nz"]], 1))
    Rz = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    s = io.import_cloud(r, Rz, 1, 1)
    assert np.array_equal(s[:, 0:3], np.stack([-r["y"], r["x"], r["z"]], 1))
    assert np.array_equal(s[:, 8:11], -np.stack([-r["ny"], r["nx"], r["nz"]], 1))


def test_set_timestamps_changes_the_timestamp_only():
    s = io.import_cloud(io.make_records(50, 3), None, 2.0, 5)
    t = io.set_timestamps(s, 300)
    assert np.array_equal(t[:, 7], np.full(50, 300, np.float32)) and np.array_equal(t[:, 6], np.full(50, 5, np.float32))
    keep = [c for c in range(12) if c != 7]
    assert io.surfels_equal(t[:, keep + [6]], s[:, keep + [6]]) and np.array_equal(s[:, 7], np.full(50, 5, np.float32))  # (a copy)


def test_import_then_export_is_the_identity_on_finite_records_without_negative_zero_and_zero_normals():
    r = io.make_records(5000, 11, special=False)
    r["x"][:3], r["y"][:3], r["z"][:3] = [0.0, 1e-41, 3e38], [0.0, -1e-41, -3e38], [0.0, 1e-45, 1.0]  # +0, denormals, large
    for c in (1.0, 0.5, 100.0):
        back = mo.export_cloud(io.import_cloud(r, io.IDENTITY, c, 9), io.IDENTITY, c - 1)
        assert back.tobytes() == r.tobytes()
        assert mo.export_cloud(io.import_cloud(r, None, c, 9), io.IDENTITY, c - 1).tobytes() == r.tobytes()
    assert len(mo.export_cloud(io.import_cloud(r, None, 1.0, 9), io.IDENTITY, 1.0)) == 0  # strict: at the threshold nothing is stable


def test_outside_that_set_the_round_trip_is_not_the_identity():
    """-0 + 0 = +0: a position component of -0.0 comes back as +0.0 (on import already).  A zero normal component changes its
    sign: -((1 * 0 + 0) + 0) = -0.0 on import, and -((1 * -0 + 0) + 0) = -(+0) = -0.0 on export -- +0.0 comes back as -0.0.
    Both are the stated arithmetic, not accidents."""
    r = io.make_records(2, 1, special=False)
    r["x"][0] = -0.0
    r["nx"][1] = 0.0
    s = io.import_cloud(r, io.IDENTITY, 2.0, 1)
    assert s[0, 0].view(np.uint32) == 0  # +0.0 in the store
    assert s[1, 8].view(np.uint32) == 0x80000000  # -0.0 in the store
    back = mo.export_cloud(s, io.IDENTITY, 1.0)
    assert back["x"][0].view(np.uint32) == 0 and r["x"][0].view(np.uint32) == 0x80000000
    assert back["nx"][1].view(np.uint32) == 0x80000000 and r["nx"][1].view(np.uint32) == 0
    assert back.tobytes() != r.tobytes()
    for name in mo.CLOUD_DTYPE.names:  # ... and nothing else moved
        if name not in ("x", "nx"):
            assert back[name].tobytes() == r[name].tobytes()
    assert back["x"][1] == r["x"][1] and back["nx"][0] == r["nx"][0]


def test_rigid_pose_and_its_inverse_stay_within_the_rounding_bound():
    """Import under a rigid Q, export under Q^-1 = [R^T | -R^T t] (computed in double from Q's floats, rounded once).  Per
    component, with u = 2^-24, ||.|| the 2-norm and R's rows of unit norm up to u:
      import:  6 roundings (3 products, 3 sums) of terms bounded by S = ||p|| + ||t||            -> 6 u S
      export:  that error through R^T (a vector of norm <= sqrt 3 * 6 u S)                        -> 6 sqrt(3) u S
               its own 6 roundings, terms bounded by (||p|| + ||t||) + ||t||                      -> 6 u (||p|| + 2 ||t||)
               the rounding of -R^T t to float                                                    -> u ||t||
      R's entries are rounded to float: R^T R = I up to 2 sqrt(3) u                               -> 3.5 u ||p||
    together below 24 u (||p|| + 2 ||t||); a normal has no translation and 5 roundings per pass: below 20 u ||n||.  Radius
    and colour are copied: equal.  Measured here over 8 poses x 4000 records: the worst position error is 0.075 of its bound,
    the worst normal error 0.173 of its bound (printed below): margins of 13 x and 5.8 x."""
    worst_p = worst_n = 0.0
    for seed in range(8):
        Q = mo.make_pose(seed)
        r = io.make_records(4000, 100 + seed, special=False)
        back = mo.export_cloud(io.import_cloud(r, Q, 3.0, 1), io.inverse_rigid(Q), 2.0)
        assert len(back) == len(r)
        p = np.stack([r["x"], r["y"], r["z"]], 1).astype(np.float64)
        n = np.stack([r["nx"], r["ny"], r["nz"]], 1).astype(np.float64)
        bp = np.stack([back["x"], back["y"], back["z"]], 1).astype(np.float64)
        bn = np.stack([back["nx"], back["ny"], back["nz"]], 1).astype(np.float64)
        bound_p = 24 * U * (np.linalg.norm(p, axis=1) + 2 * np.linalg.norm(Q[:3, 3].astype(np.float64)))
        bound_n = 20 * U * np.linalg.norm(n, axis=1)
        err_p, err_n = np.abs(bp - p).max(axis=1), np.abs(bn - n).max(axis=1)
        worst_p, worst_n = max(worst_p, (err_p / bound_p).max()), max(worst_n, (err_n / bound_n).max())
        assert (err_p <= bound_p).all() and (err_n <= bound_n).all()
        for name in ("radius", "red", "green", "blue"):
            assert back[name].tobytes() == r[name].tobytes()
    print(f"worst position error / bound {worst_p:.3f}, worst normal error / bound {worst_n:.3f}")
    assert 0 < worst_p and 0 < worst_n  # (the pose is no axis permutation: the round trip does round)
