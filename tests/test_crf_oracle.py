"""CPU: self-tests of the dense-CRF segmentation oracle (tests/crf_oracle.py), and the default configuration of the C ABI
and of the Python binding against the GUI defaults."""
import numpy as np
import pytest

import crf_oracle as co

F32 = np.float32


def test_two_cell_mean_field_by_hand():
    """Two cells, two labels, one iteration, worked out by hand: K_01 = exp(-|f0 - f1|^2 / 2), row sums 1 + K_01,
    D = 1 / sqrt(1 + K_01), so Kt = K / (1 + K_01) and Q1 = softmax(-U + w_s Kt_s Q0 + w_a Kt_a Q0)."""
    cfg = co.config(iterations=1, weight_smoothness=2.0, weight_appearance=3.0)
    fs = np.array([[0.0, 0.0], [0.5, 0.0]], F32)
    fa = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 1]], F32)
    U = np.array([[1.0, 2.0], [2.0, 1.0]], F32)
    ks, ka = np.exp(-0.5 * 0.25), np.exp(-0.5 * 2.0)
    Ks = np.array([[1, ks], [ks, 1]]) / (1 + ks)
    Ka = np.array([[1, ka], [ka, 1]]) / (1 + ka)
    q0 = np.exp(-U.astype(np.float64))
    q0 /= q0.sum(0)
    arg = -U + 2.0 * (Ks @ q0.T).T + 3.0 * (Ka @ q0.T).T
    want = np.exp(arg - arg.max(0))
    want /= want.sum(0)
    got = co.mean_field(U, fs, fa, cfg)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    # three cells, one of them far away in both feature spaces: it only sees itself (Kt_ii = 1)
    fs3 = np.array([[0, 0], [0.5, 0], [1e3, 0]], F32)
    fa3 = np.array([[0] * 6, [1, 0, 0, 0, 0, 1], [1e3] * 6], F32)
    U3 = np.array([[1.0, 2.0, 0.5], [2.0, 1.0, 0.25]], F32)
    q = co.mean_field(U3, fs3, fa3, cfg)
    q0 = np.exp(-U3[:, 2].astype(np.float64))
    q0 /= q0.sum()
    a = -U3[:, 2] + 5.0 * q0
    np.testing.assert_allclose(q[:, 2], np.exp(a - a.max()) / np.exp(a - a.max()).sum(), atol=1e-14)
    np.testing.assert_allclose(q[:, :2], got, atol=1e-14)


def test_zero_iterations_is_softmax_of_minus_unaries():
    rng = np.random.default_rng(0)
    U = rng.random((3, 40), dtype=F32) * 10
    fs, fa = rng.random((40, 2), dtype=F32), rng.random((40, 6), dtype=F32)
    q = co.mean_field(U, fs, fa, co.config(iterations=0))
    e = np.exp(-U.astype(np.float64))
    np.testing.assert_allclose(q, e / e.sum(0), rtol=1e-13)


def flood_fill(lab):
    H, W = lab.shape
    comp = -np.ones((H, W), np.int64)
    n = 0
    for y in range(H):
        for x in range(W):
            if comp[y, x] >= 0:
                continue
            stack = [(y, x)]
            comp[y, x] = n
            while stack:
                cy, cx = stack.pop()
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and comp[ny, nx] < 0 and lab[ny, nx] == lab[cy, cx]:
                        comp[ny, nx] = n
                        stack.append((ny, nx))
            n += 1
    return comp


@pytest.mark.parametrize("seed", range(6))
def test_components_match_a_flood_fill_with_raster_numbering(seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 3, (13, 17)).astype(np.uint8)
    if seed % 2:  # blobs and a spiral-like merge case
        lab = (rng.random((13, 17)) < 0.45).astype(np.uint8)
        lab[3, :] = 1
        lab[:, 5] = 1
    comp, stats = co.connected_labels(lab)
    want = flood_fill(lab)  # a flood fill started in raster order numbers components by their first cell
    assert np.array_equal(comp, want)
    for i, s in enumerate(stats):
        ys, xs = np.nonzero(comp == i)
        assert s["size"] == len(ys) and s["label"] == lab[ys[0], xs[0]]
        assert (s["top"], s["bottom"], s["left"], s["right"]) == (ys.min(), ys.max(), xs.min(), xs.max())


def post(raw, spx, spy, ids, next_id=9, allow_new=False, depth=None, S=16, **kw):
    cfg = co.config(**kw)
    W, H = spx * S, spy * S
    depth = np.ones(spx * spy, F32) if depth is None else depth
    return co.postprocess(np.asarray(raw, np.uint8).ravel(), spx, spy, W, H, S, ids, next_id, allow_new, depth,
                          np.zeros(len(ids), F32), cfg)


def test_keep_largest_tie_rule_and_smallest_key_skip():
    # label 1 has two components of 4 cells (tie: the earlier in raster order stays) and one of 2; label 0 (the smallest
    # key) keeps all of its components
    g = np.zeros((8, 8), np.uint8)
    g[2:4, 2:4] = 1   # component A, 4 cells, first cell (2,2)
    g[5:7, 5:7] = 1   # component B, 4 cells, later
    g[0, 6:8] = 1     # component C, 2 cells, first in raster order
    g[7, 0] = 2
    out, data, _ = post(g, 8, 8, [0, 1, 2])
    o = out.reshape(8, 8)
    assert (o[2:4, 2:4] == 1).all() and (o[5:7, 5:7] == 255).all() and (o[0, 6:8] == 255).all()
    assert o[7, 0] == 255 or o[7, 0] == 2  # (border rule decides below)
    assert (o[g == 0] == 0).all()
    # no background cell: the smallest object id is skipped instead and keeps both of its components
    g2 = np.full((8, 8), 2, np.uint8)
    g2[1:3, 2:4] = 1
    g2[5:7, 4:6] = 1
    out, data, _ = post(g2, 8, 8, [0, 1, 2])
    o = out.reshape(8, 8)
    assert (o[1:3, 2:4] == 1).all() and (o[5:7, 4:6] == 1).all()


def test_new_label_size_rule():
    g = np.zeros((10, 10), np.uint8)
    g[3:5, 3:5] = 9  # 4 of 100 cells
    for lo, hi, keep in ((0.05, 0.4, False), (0.01, 0.03, False), (0.01, 0.4, True)):
        out, data, has_new = post(g, 10, 10, [0], 9, True, min_rel_size_new=lo, max_rel_size_new=hi)
        assert has_new == keep and ((out.reshape(10, 10)[3:5, 3:5] == 9).all() == keep)
        assert len(data) == (2 if keep else 1)
        if keep:
            assert data[1]["id"] == 9 and data[1]["super_pixel_count"] == 4


def test_border_rule():
    # S = 16: mapToHigh(x) = 16x + 8.  An object in row 0 only: top = bottom = 8 < 20 -> removed.  Row 1: 24 -> kept.
    g = np.zeros((10, 12), np.uint8)
    g[0, 4:7] = 1
    out, data, _ = post(g, 12, 10, [0, 1])
    assert (out == 0).sum() == 117 and (out == 255).sum() == 3 and data[1]["super_pixel_count"] == 0
    g = np.zeros((10, 12), np.uint8)
    g[1, 4:7] = 1
    out, data, _ = post(g, 12, 10, [0, 1])
    assert (out == 1).sum() == 3 and data[1]["super_pixel_count"] == 3
    g = np.zeros((10, 12), np.uint8)  # last column: left = right = 16 * 11 + 8 = 184 > W - 20 = 172
    g[4:6, 11] = 1
    out, data, _ = post(g, 12, 10, [0, 1])
    assert data[1]["super_pixel_count"] == 0


def test_depth_statistics_and_trimming():
    g = np.zeros((6, 6), np.uint8)
    g[2:4, 2:5] = 1  # 6 cells
    d = np.full(36, 2.0, F32)
    obj = np.flatnonzero(g.ravel() == 1)
    d[obj] = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 4.0], F32)
    out, data, _ = post(g, 6, 6, [0, 1], depth=d)
    mean = F32(9.0) / F32(6)  # 1.5; deviations 0.5 x5 + 2.5 = 5 -> std 5/6; 4 > 1.1 * 0.8333 + 1.5 -> trimmed
    assert data[1]["super_pixel_count"] == 6
    assert data[1]["depth_mean"] == F32(1.0) and data[1]["depth_std"] == F32(F32(F32(5.0) - F32(2.5)) / F32(5))
    assert data[0]["depth_mean"] == F32(2.0) and data[0]["depth_std"] == F32(0.0)  # (background is never trimmed)
    assert mean == F32(1.5)


def test_unaries_follow_the_reference_expressions():
    cfg = co.config()
    err = np.array([[0.01, 0.2, 0.0], [0.05, 0.05, 0.3]], F32)
    conf = np.array([[0.2, 0.5, 0.5], [0.5, F32(0.4), 0.41]], F32)
    rng = F32(2.0)
    U = co.unaries(err.copy(), conf, rng, cfg, True)
    e0 = np.array([F32(np.float64(rng) * 0.01), 0.2, 0.0], F32)  # conf0 < 0.3 -> range * 0.01 (in double)
    e1 = np.array([0.05, F32(rng * F32(0.0375)), 0.3], F32)        # conf1 <= 0.4 (a double 0.4: f32(0.4) is above it)
    assert np.float64(conf[1, 1]) > 0.4  # f32(0.4) > 0.4 in double: not replaced
    e1[1] = F32(0.05)
    want0 = (F32(75) * (e0 / rng).astype(F32)).astype(F32)
    want1 = (F32(75) * (e1 / rng).astype(F32)).astype(F32)
    want0 = np.where(want0 <= 1e-5, F32(1e-5), want0)
    np.testing.assert_array_equal(U[0], want0)
    np.testing.assert_array_equal(U[1], want1)
    lowest = np.minimum(e0 / rng, e1 / rng).astype(F32)
    new = (F32(5.5) - (F32(75) * lowest).astype(F32)).astype(F32)
    np.testing.assert_array_equal(U[2], np.maximum(new, F32(0.01)))


def test_range_invalid_frame_is_all_background():
    """B4: zero depth everywhere -> range 0 -> every cell background, no new label"""
    spx, spy, S = 8, 6, 16
    N = spx * spy
    res = co.segment(np.zeros(N, F32), np.full((2, N), 0.1, F32), np.ones((2, N), F32), np.zeros(3 * N, np.uint8),
                     spx * S, spy * S, S, [0, 1], 2, True, co.config())
    assert res["range_invalid"] and res["range"] == 0
    assert (res["raw_map"] == 0).all() and (res["map"] == 0).all() and not res["has_new_label"]
    assert len(res["model_data"]) == 2 and res["model_data"][1]["super_pixel_count"] == 0
    assert co.range_invalid(co.depth_range(np.array([np.nan, -1.0, 200.0], F32)))


def test_grid_labels():
    g = co.grid_labels(37, 25, 11)
    assert g.shape == (25, 37) and g.max() == 3 * 2 - 1 and g[24, 36] == 5 and g[0, 12] == 1


def test_default_config_matches_the_gui():
    from multimotionfusion_amd import _capi
    from multimotionfusion_amd.segmentation import CrfConfig
    py = CrfConfig()
    for k, v in co.DEFAULTS.items():
        assert getattr(py, k) == pytest.approx(v), k
    c = _capi.mmf_crf_config()
    lib = _capi.load()
    assert lib.mmf_crf_default_config(_capi.C.byref(c)) == 0
    for k, v in co.DEFAULTS.items():
        assert getattr(c, k) == pytest.approx(v), k
