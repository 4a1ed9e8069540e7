"""CPU: tests/flowcrf_oracle.py -- the checker of the flow-CRF inference engine -- held to the truth: the mean
field against a double loop over every pair, its limits and symmetries, unaries computed by hand, the cell rule of the track
samples, equal timestamps, a scene whose answer is known, and the properties the device tests rely on (enough cells with a
clear winner, few projection probabilities at the threshold)."""
import numpy as np
import pytest

import crf_oracle as co
import flowcrf_oracle as fo

F32 = np.float32


def small_problem(seed, w=6, h=5, L=3):
    rng = np.random.default_rng(seed)
    U = rng.uniform(0.1, 2.0, (L, w * h)).astype(F32)
    U[0, 3] = np.inf  # a label that is impossible in a cell
    flow = rng.normal(0, 0.2, (h, w, 2)).astype(F32)
    return U, flow


def test_mean_field_equals_the_double_loop_over_every_pair():
    U, flow = small_problem(1)
    cfg = fo.config(iterations=3)
    fs, fa = fo.features(6, 5, flow)
    Q = fo.mean_field(U, fs, fa, cfg)
    B = fo.brute_force_mean_field(U, 6, 5, flow, cfg)
    assert np.abs(Q - B).max() < 1e-12
    assert np.allclose(Q.sum(0), 1.0, atol=1e-12) and (Q[0, 3] == 0)  # +inf survives as Q = 0


def test_the_integer_division_of_the_appearance_positions():
    _, fa = fo.features(90, 45, np.zeros((45, 90, 2), F32))
    fa = fa.reshape(45, 90, 4)
    assert fa[0, 39, 0] == 0 and fa[0, 40, 0] == 1 and fa[0, 80, 0] == 2 and fa[39, 0, 1] == 0 and fa[40, 0, 1] == 1
    fs, _ = fo.features(7, 4, np.zeros((4, 7, 2), F32))
    assert fs.reshape(4, 7, 2)[3, 6].tolist() == [F32(6) / F32(3), F32(3) / F32(3)]


def test_vanishing_weights_give_the_softmax_of_the_unaries():
    U, flow = small_problem(2)
    fs, fa = fo.features(6, 5, flow)
    Q = fo.mean_field(U, fs, fa, fo.config(weight_smoothness=0.0, weight_appearance=0.0, iterations=4))
    assert np.abs(Q - co.softmax(-U.astype(np.float64))).max() < 1e-15
    Q0 = fo.mean_field(U, fs, fa, fo.config(iterations=0))
    assert np.array_equal(Q0, co.softmax(-U.astype(np.float64)))


def test_permuting_the_labels_permutes_every_output():
    sc = fo.make_scene(12, 9, 3, False, seed=4)
    cfg = fo.config(iterations=3)
    a = fo.run_scene(sc, cfg)
    perm = [2, 0, 1]
    sp = dict(sc)
    for key in ("ids", "T_start", "T_end"):
        sp[key] = [sc[key][p] for p in perm]
    sp["vertex_z"] = sc["vertex_z"][perm]
    b = fo.run_scene(sp, cfg)
    assert np.array_equal(b["E"], a["E"][perm], equal_nan=True)
    for name in ("U", "proj"):  # (float32 sums over the labels run in label order: an ulp)
        assert np.allclose(b[name], a[name][perm], rtol=0, atol=1e-6), name
        assert np.array_equal(np.isinf(b[name]), np.isinf(a[name][perm])) and np.array_equal(b[name] == 0, a[name][perm] == 0), name
    assert np.abs(b["Q"] - a["Q"][perm]).max() < 1e-12
    assert np.abs(b["prob"] - a["prob"][perm]).max() < 1e-6
    clear = a["margin"] > 1e-3
    assert clear.mean() > 0.9 and np.array_equal(a["ids"][clear], b["ids"][clear])


def test_unaries_by_hand():
    """one model and the new label: an inlier sample gives (0.3133, 1.3133), an outlier the reverse, no sample log 2 twice"""
    E = np.array([[5.0, 60.0, np.inf, np.nan], [np.inf] * 4], F32)
    U = fo.unaries(E, 1, True, 20.0)
    lo, hi = np.log(1 + np.exp(-1.0)), 1 + np.log(1 + np.exp(-1.0))
    assert abs(lo - 0.3133) < 5e-5 and abs(hi - 1.3133) < 5e-5
    assert np.allclose(U[:, 0], [lo, hi], atol=1e-6) and np.allclose(U[:, 1], [hi, lo], atol=1e-6)
    assert np.allclose(U[:, 2], np.log(2.0), atol=1e-6) and np.allclose(U[:, 3], np.log(2.0), atol=1e-6)  # (NaN: 1 / L as well)
    # without the new label a lone model is certain; two models, one sample each way
    assert np.array_equal(fo.unaries(E[:1], 1, False, 20.0), np.zeros((1, 4), F32))
    E2 = np.array([[5.0, np.inf], [60.0, 7.0], [np.inf, np.inf]], F32)
    U2 = fo.unaries(E2, 2, True, 20.0)
    # column 0: both finite -> rows (0, 1, any(v < thr) = 1); column 1: model 0 has no sample -> (inf, 0, inf)
    p0 = np.exp(-np.array([0.0, 1.0, 1.0]))
    assert np.allclose(U2[:, 0], -np.log(p0 / p0.sum()), atol=1e-6)
    assert np.isposinf(U2[0, 1]) and U2[1, 1] == 0 and np.isposinf(U2[2, 1])


def one_track(W, H, px_end, py_end, px_start, py_start, dt=fo.DT):
    cam = fo.camera(W, H)
    z = np.array([1.5])
    return cam, dict(xy_cur=np.array([[px_end, py_end]], np.int32), xy_prev=np.array([[px_start, py_start]], np.int32),
                     co_cur=fo.back_project(np.array([float(px_end)]), np.array([float(py_end)]), z, cam),
                     co_prev=fo.back_project(np.array([float(px_start)]), np.array([float(py_start)]), z, cam),
                     ts_prev=np.array([10**9], np.int64), ts_cur=np.array([10**9 + dt], np.int64),
                     ok_cur=np.ones(1, np.int32), ok_prev=np.ones(1, np.int32))


def test_the_cell_rule():
    """x = 2 -> column 0 and x = 6 -> column 2 (half to even); x = 639 -> column 160 = the next row's column 0; the last
    cell's overflow is dropped"""
    W, H, w = 640, 480, 160
    eye = [np.eye(4, dtype=F32)]
    for x, y, want in [(2, 8, 2 * w + 0), (6, 8, 2 * w + 2), (10, 8, 2 * w + 2), (639, 8, 3 * w), (639, 479, -1), (636, 479, -1), (634, 477, 119 * w + 158)]:
        cam, tr = one_track(W, H, x, y, x, y)
        E, cell = fo.track_errors(W, H, cam, eye, eye, tr, 1)
        assert cell[0, 0] == want, (x, y, cell)
        assert np.isfinite(E).sum() == (want >= 0) and (want < 0 or E[0, want] == 0)
    # the speed: 3 and 4 pixels in 33 ms
    cam, tr = one_track(W, H, 103, 204, 100, 200)
    E, cell = fo.track_errors(W, H, cam, eye, eye, tr, 1)
    assert E[0, cell[0, 0]] == F32(5.0 / (33_000_000 * 1e-9))
    # the later track wins the cell
    cam, a = one_track(W, H, 100, 200, 100, 200)
    _, b = one_track(W, H, 101, 201, 98, 197)
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    E, cell = fo.track_errors(W, H, cam, eye, eye, both, 1)
    assert cell[0, 0] == cell[0, 1] and E[0, cell[0, 0]] == F32(5.0 / (33_000_000 * 1e-9))
    rev = {k: v[::-1].copy() for k, v in both.items()}
    assert fo.track_errors(W, H, cam, eye, eye, rev, 1)[0][0, cell[0, 0]] == 0


def test_equal_timestamps():
    W, H = 64, 48
    eye = [np.eye(4, dtype=F32)]
    cam, tr = one_track(W, H, 20, 20, 20, 20, dt=0)
    E, cell = fo.track_errors(W, H, cam, eye, eye, tr, 2)
    assert np.isnan(E[0, cell[0, 0]])
    U = fo.unaries(E, 1, True, 20.0)
    assert np.allclose(U[:, cell[0, 0]], np.log(2.0), atol=1e-6)  # the NaN column gets 1 / L
    cam, tr = one_track(W, H, 21, 20, 20, 20, dt=0)
    E, cell = fo.track_errors(W, H, cam, eye, eye, tr, 2)
    assert np.isposinf(E[0, cell[0, 0]])  # as if there were no sample
    assert np.allclose(fo.unaries(E, 1, True, 20.0)[:, cell[0, 0]], np.log(2.0), atol=1e-6)
    # a stamp that runs backwards wraps as the reference's uint64_t difference does: a huge time, speed ~ 0
    cam, tr = one_track(W, H, 25, 20, 20, 20, dt=-5)
    E, cell = fo.track_errors(W, H, cam, eye, eye, tr, 1)
    assert 0 < E[0, cell[0, 0]] < 1e-8


def test_skipped_tracks():
    W, H = 64, 48
    eye = [np.eye(4, dtype=F32)]
    cam, tr = one_track(W, H, 20, 20, 20, 20)
    for change in (dict(ok_cur=0), dict(ok_prev=0), dict(ts_prev=0), dict(co_cur=np.nan), dict(co_prev=np.inf)):
        t = {k: v.copy() for k, v in tr.items()}
        for k, v in change.items():
            t[k][0] = v
        E, cell = fo.track_errors(W, H, cam, eye, eye, t, 1)
        assert cell[0, 0] == -1 and np.isposinf(E).all(), change
    for x, y in [(-1, 5), (64, 5), (5, -1), (5, 48)]:  # an end or a start outside the frame
        for ends in ((x, y, 5, 5), (5, 5, x, y)):
            cam, t = one_track(W, H, *ends)
            assert fo.track_errors(W, H, cam, eye, eye, t, 1)[1][0, 0] == -1, ends
    # a model's transform moves the end pixel: 2 pixels to the right at Z0 = 1.5
    cam, t = one_track(W, H, 20, 20, 20, 20)
    T = fo.translation([2 * 1.5 / float(cam[0]), 0, 0])
    E, cell = fo.track_errors(W, H, cam, eye, [T], t, 1)
    assert cell[0, 0] == 5 * 16 + int(np.rint(22 / 4)) and E[0, cell[0, 0]] == F32(2.0 / (33_000_000 * 1e-9))


def test_projection_probabilities_by_hand():
    depth = np.full((4, 8), 1.0, F32)
    depth[0, 4] = 0
    vz = np.stack([depth + F32(0.003), depth + F32(0.5)]).astype(F32)
    vz[:, 0, 4] = 0
    p, inv = fo.proj_prob(depth, vz, True, 0.03, 0.3)
    e0, e1 = np.exp(-0.1), np.exp(-1.0)
    assert p.shape == (3, 2) and inv.tolist() == [False, True]
    assert abs(p[0, 0] - e0 / (e0 + e1)) < 1e-5 and p[1, 0] == 0 and p[2, 0] == 0  # e1 / (e0 + e1) = 0.289 < 0.3
    assert (p[:, 1] == 0).all()


def test_the_scene_whose_answer_is_known():
    """A rectangle that moves by (2, 1) flow pixels, outlier tracks inside it, inlier tracks on the still background, depth
    equal to the camera model's prediction.  The MAP is the new label inside the rectangle and model 0 outside, apart from a
    margin of 3 cells inside the rectangle's border (the smoothness kernel, sigma 3 cells, mixes the two sides there).

    This holds where the rectangle has no depth, in the frame and in the prediction alike (both 0, `invalid`).  Where both
    have the SAME valid depth, the arithmetic of (c) and (e) gives the lone model proj = e / e = 1 and hence prob = 1
    everywhere: no flow evidence can beat it, and the MAP is model 0 in every cell (in the reference the new label's row of
    prob_proj is uninitialised memory; here it is 0).  Both halves are pinned."""
    cfg = fo.config()
    sc, (x0, x1, y0, y1) = fo.rectangle_scene(hole=True)
    r = fo.run_scene(sc, cfg)
    want = np.zeros((sc["h"], sc["w"]), np.uint8)
    want[y0:y1, x0:x1] = 1
    sure = np.ones_like(want, bool)
    sure[y0:y1, x0:x1] = False
    sure[y0 + 3:y1 - 3, x0 + 3:x1 - 3] = True
    assert np.array_equal(r["ids"][sure], want[sure])
    assert (r["ids"][y0 + 3:y1 - 3, x0 + 3:x1 - 3] == 1).all() and (r["ids"][:, :x0] == 0).all()
    assert (r["margin"][sure] > 1e-3).all()
    sc2, _ = fo.rectangle_scene(hole=False)
    r2 = fo.run_scene(sc2, cfg)
    assert (r2["ids"] == 0).all() and (r2["prob"][0] == 1).all() and r2["prob"][1].max() < 0.43
    inner = r2["Q"][1, y0 + 3:y1 - 3, x0 + 3:x1 - 3]
    assert (inner > 0.5).all()  # the flow side does say `new` there


@pytest.mark.parametrize("w,h,L,allow_new", fo.GPU_CASES)
def test_the_device_scenes_have_clear_winners(w, h, L, allow_new):
    """at least 90 % of the cells have a top-two margin of prob >= 1e-3; under 1 % of the projection probabilities lie within
    1e-5 of the threshold; every edge track of the table does what it is there for"""
    sc, cfg = fo.case_scene(w, h, L, allow_new)
    r = fo.run_scene(sc, cfg)
    if L > 1:
        assert (r["margin"] >= 1e-3).mean() >= 0.9, (r["margin"] >= 1e-3).mean()
    near = np.abs(r["proj64"] - 0.3) < 1e-5
    assert near.mean() < 0.01
    assert r["invalid"].any() and not r["invalid"].all()
    n = len(sc["tracks"]["ts_cur"])
    cell = r["cell"][0]
    W = sc["W"]
    k = n - 12  # the edge tracks, in the order make_scene appends them
    assert cell[k] == cell[k + 1] == 2 * w + 2 and r["E"].reshape(L, -1)[0, 2 * w + 2] > 20
    assert (cell[k + 2:k + 6] == -1).all()
    assert cell[k + 6] == int(np.rint(10 / 4)) * w + w and cell[k + 7] == -1
    assert cell[k + 8] == 3 * w + 0 and cell[k + 9] == 3 * w + 2
    E0 = r["E"].reshape(L, -1)[0]
    assert np.isnan(E0[cell[k + 10]]) and np.isposinf(E0[cell[k + 11]]) and cell[k + 11] >= 0
    assert W - 1 == 4 * w - 1
