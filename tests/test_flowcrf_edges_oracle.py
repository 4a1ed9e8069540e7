"""CPU: the conditions the cases of tests/flowcrf_edges.py rest on, checked on the oracle alone (tests/flowcrf_oracle.py) and on
the library's host-side geometry query: a device comparison on a scene that misses its edge proves nothing.

The launch geometry of the pair pass (why test_gpu_flowcrf_edges.py exists), the scenes of fo.GPU_CASES unchanged by the
empty-grid fix of fo.make_scene, clear winners and few projection probabilities at the threshold in every new scene, exact
ties where ties are meant, the three outcomes of the threshold gate, the exact 0.5 of two identical models, and the depth
classes of the preparation."""
import numpy as np
import pytest

import flowcrf_edges as fe
import flowcrf_oracle as fo
from helpers import assert_bit_equal

F32 = np.float32


def test_the_scenes_of_the_device_cases_are_what_they_were():
    """the checksum was taken before fo.make_scene learned to build images too small for its track grid"""
    sc, _ = fo.case_scene(43, 25, 9, True)
    assert fe.scene_checksum(sc) == "d0dd3701a6a74fa95fb198d7f2b04d7719b7ee07341dc33544c8094821426588"
    sc, _ = fo.case_scene(8, 8, 2, False)
    assert fe.scene_checksum(sc) == "2e3f6c01745be86e2f2425e97852fdd60fe8e6b00f684ef3675d337ea4a16d20"


def test_no_older_case_gives_a_workgroup_more_than_one_chunk():
    """every size of fo.GPU_CASES has per == 1 at every label width: the chunk loop of fcrf_pair_kernel runs once, no range is
    empty.  The sizes the engine is used at all have per >= 2"""
    for w, h in sorted({(c[0], c[1]) for c in fo.GPU_CASES}):
        for width in fe.WIDTHS:
            nsplit, nchunk, per = fe.pair_geometry(w * h, width)
            assert per == 1 and nsplit == nchunk == (w * h + 255) // 256, (w, h, width, nsplit, nchunk, per)
            assert fe.empty_ranges(nsplit, nchunk, per) == 0
    for N in fe.PRODUCTION_CELLS:
        for width in fe.WIDTHS:
            nsplit, nchunk, per = fe.pair_geometry(N, width)
            assert per >= 2 and nsplit * per >= nchunk == (N + 255) // 256, (N, width, nsplit, nchunk, per)
    assert fe.pair_geometry(160 * 120, 8) == (11, 75, 7) and fe.pair_geometry(160 * 120, 32) == (6, 75, 13)
    assert fe.pair_geometry(320 * 240, 1)[2] == 100 and fe.pair_geometry(320 * 240, 32)[2] == 150


def test_the_geometry_query_refuses_what_is_no_width():
    from multimotionfusion_amd._capi import MmfError
    for n_cells, width in ((0, 1), (64, 0), (64, 3), (64, 64), (-5, 2)):
        with pytest.raises(MmfError, match="mmf_debug_flowcrf_pair_geometry"):
            fe.pair_geometry(n_cells, width)


@pytest.mark.parametrize("w,h,L,allow_new", fe.PAIR_CASES)
def test_the_pair_cases_take_several_chunks_and_leave_ranges_empty(w, h, L, allow_new):
    from multimotionfusion_amd.flowcrf import pad_labels
    assert max(w, h) > 2 * 44 + 1  # some cells have the blur cut at the radius on both sides, not by the image
    widths = fe.PAIR_WIDTHS[(w, h, L, allow_new)]
    assert pad_labels(L) in widths
    for width in widths:
        nsplit, nchunk, per = fe.pair_geometry(w * h, width)
        used = nsplit - fe.empty_ranges(nsplit, nchunk, per)
        assert per == 2 and nsplit - used >= 7, (nsplit, nchunk, per)
        assert min(nchunk, used * per) - (used - 1) * per == 2  # the last range that is not empty holds two chunks
    sc, cfg, r, soft, rs, moved = fe.pair_case(w, h, L, allow_new)
    assert cfg["iterations"] == soft["iterations"] == 2 and soft["weight_smoothness"] == soft["weight_appearance"] == 1.0
    for res in (r, rs):
        if res is None:
            continue
        clear = res["margin"] >= 1e-3
        assert clear.mean() >= 0.999, clear.mean()
        assert (np.abs(res["proj64"] - 0.3) < 1e-5).mean() < 1e-4
        assert np.isposinf(res["U"]).any() and res["invalid"].any()
    # a chunk of 256 cells j left out of every sum must move Q by a hundred times the 1e-4 the device is held to: it does at the
    # default weights with 17 labels; the two-label scene is saturated there and hides it, so it runs with soft weights too
    print(f"{w}x{h} L={L}: a chunk left out moves Q by {moved}")
    assert max(moved.values()) > 1e-2, moved
    assert ((w, h, L, allow_new) in fe.PAIR_SOFT) == (moved["default"] < 1e-2) == (rs is not None)
    if rs is not None:
        assert (rs["Q"].max(0) < 0.99).mean() > 0.5  # more than half of the cells are not saturated


@pytest.mark.parametrize("w,h,L,allow_new", fe.WIDTH8_CASES)
def test_the_width_8_cases_have_clear_winners(w, h, L, allow_new):
    from multimotionfusion_amd.flowcrf import pad_labels
    assert pad_labels(L) == 8
    sc, cfg, r = fe.case(w, h, L, allow_new)
    assert cfg["iterations"] == 10
    assert (r["margin"] >= 1e-3).mean() >= 0.99
    assert (np.abs(r["proj64"] - 0.3) < 1e-5).mean() < 0.01


@pytest.mark.parametrize("with_tracks", [True, False])
@pytest.mark.parametrize("w,h", fe.DEGENERATE_SIZES)
def test_the_degenerate_images_build_and_run(w, h, with_tracks):
    sc, cfg, r = fe.degenerate(w, h, with_tracks)
    assert (sc["w"], sc["h"], sc["W"], sc["H"]) == (w, h, 4 * w, 4 * h) and r["Q"].shape == (3, h, w)
    assert np.isfinite(r["Q"]).all() and np.abs(r["Q"].sum(0) - 1).max() < 1e-12
    clear = r["margin"] >= 1e-3
    assert clear.sum() >= min(w * h, 0.9 * w * h), (int(clear.sum()), w * h)
    assert (np.abs(r["proj64"] - 0.3) < 1e-5).mean() < 0.01
    if with_tracks:
        E = r["E"].reshape(3, -1)
        assert np.isfinite(E[0]).any() and np.isfinite(E[1]).any() and (r["cell"] >= 0).any() and (r["cell"][:, -4:] == -1).any()
        assert {0.0} < set(np.unique(E[:2][np.isfinite(E[:2])]).tolist())  # inliers (0 px/s) and outliers
    else:
        assert np.isposinf(r["E"]).all()


@pytest.mark.parametrize("w,h", fe.TIE_SIZES)
def test_the_constructed_ties_are_exact_in_the_oracle(w, h):
    sc, cfg, r = fe.tie_scene(w, h, "three")
    inv = r["invalid"]
    assert inv.any() and not inv.all() and not sc["motion"].any()
    assert_bit_equal(r["proj"][1], r["proj"][2], "proj of two identical models")
    assert_bit_equal(r["prob"][1], r["prob"][2], "prob of two identical models")
    assert (r["proj"][0] == 0).all() and (r["proj"][1][~inv] > 0.3).all()
    assert (r["label"][~inv] == 1).all() and (r["label"][inv] == 0).all() and (r["margin"] == 0).all()
    for kind, L in (("two", 2), ("two-new", 3)):
        sc, cfg, r = fe.tie_scene(w, h, kind)
        assert r["proj"].shape[0] == L and (r["proj"][:2][:, ~r["invalid"]] == F32(0.5)).all() and (r["label"] == 0).all()
        assert (r["prob"][:, r["invalid"]] == 0).all() and r["invalid"].any()
        if L == 3:
            assert (r["prob"][2] == 0).all()


def test_the_three_outcomes_of_the_threshold_gate():
    """one float below v the cells that carry v are outliers of the model (1.3133, 0.3133), at v neither `e > threshold` nor
    `e < threshold` holds (log 2 twice), one float above they are inliers (0.3133, 1.3133)"""
    sc, v, at = fe.threshold_scene()
    assert v == F32(271.03854) and at.sum() == 72
    lo, hi = np.log(1 + np.exp(-1.0)), 1 + np.log(1 + np.exp(-1.0))
    want = dict(below=(hi, lo), at=(np.log(2.0), np.log(2.0)), above=(lo, hi))
    U = {}
    for which, t in fe.thresholds(v):
        cfg, r = fe.threshold_reference(which)
        assert F32(cfg["threshold"]) == F32(t) and cfg["iterations"] == 0
        U[which] = r["U"][:, at]
        assert np.abs(U[which] - np.array(want[which])[:, None]).max() < 1e-6, which
        assert (r["margin"] >= 1e-3).all()
    names = list(U)
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(U[names[a]] - U[names[b]]).max(0).min() > 0.3
    t = [F32(t) for _, t in fe.thresholds(v)]
    assert t[0] < v == t[1] < t[2] and np.nextafter(t[0], F32(np.inf)) == v == np.nextafter(t[2], F32(0))


def test_two_identical_models_have_a_projection_probability_of_exactly_one_half():
    sc = fe.twin_scene()
    half_up = float(np.nextafter(F32(0.5), F32(1)))
    r = fo.run_scene(sc, fo.config(iterations=0, min_proj_prob=0.5))
    inv = r["invalid"]
    assert inv.any() and (r["proj"][:, ~inv] == F32(0.5)).all() and (r["proj"][:, inv] == 0).all()
    assert (r["proj64"][:, ~inv] == 0.5).all()
    r = fo.run_scene(sc, fo.config(iterations=0, min_proj_prob=half_up))
    assert (r["proj"] == 0).all()


def test_the_depth_classes():
    sc, cfg, r = fe.depth_class_scene()
    assert len(set(fe.depth_class_cells())) == len(fe.DEPTH_CLASSES)
    proj = {}
    for (x, y), (name, d, zs, inv) in zip(fe.depth_class_cells(), fe.DEPTH_CLASSES):
        got_d, got_z = sc["depth"][4 * y, 4 * x], sc["vertex_z"][:, 4 * y, 4 * x]
        assert np.array_equal(np.array([got_d, *got_z]), np.array([d, *zs], F32), equal_nan=True), name
        assert bool(r["invalid"][y, x]) == inv, name
        assert not np.isnan(r["proj"][:, y, x]).any() and (not inv or (r["proj"][:, y, x] == 0).all()), name
        proj[name] = r["proj"][:, y, x]
    third = F32(F32(1) / F32(3))
    for name in ("d=NaN", "d=NaN, one z=0", "d=+inf, z finite", "d=+inf, one z=+inf"):  # every distance becomes max_err
        assert np.abs(proj[name] - third).max() < 1e-6, name
    # a class that clamps one model and not the others shows which one
    for name, clamped in (("d>0, one z=0", 0), ("d>0, one z=NaN", 0), ("d>0, one z=+inf", 1), ("d=0, one z=NaN", 1), ("d=tiny, z=0", 0)):
        assert proj[name][clamped] == 0 and proj[name].max() > 0.45, (name, proj[name])
    assert len({tuple(p.tolist()) for p in proj.values()}) >= 8
    assert (r["margin"] >= 1e-3).mean() >= 0.9 and (np.abs(r["proj64"] - 0.3) < 1e-5).mean() < 0.01
    assert np.float32(1e-6) == fe.TINY and fe.TINY_LO < fe.TINY < fe.TINY_HI
