"""-m gpu: the flow-CRF inference engine (csrc/flowcrf_kernels.hpp, csrc/flowcrf_host.hpp) at the edges the
scenes of test_gpu_flowcrf.py do not reach, against tests/flowcrf_oracle.py under the bar of that file
(flowcrf_edges.check_against_oracle: E, the cells and `invalid` bit for bit, U and proj within 1e-5, Q and prob within 1e-4,
equal labels where the oracle's top-two margin is >= 1e-3, stage (e) replayed from the device's own Q and proj exactly at every
cell, a second run with the same bits).  test_flowcrf_edges_oracle.py asserts on the oracle alone that every case reaches its edge.

1  the pair pass where a workgroup takes several chunks and trailing ranges are empty (the geometry of every production size)
2  the label width 8; engines wider than the call; one engine at 32, 3 and 32 labels in turn; images of one cell, row, column
3  the first maximum of the fusion on constructed ties
4  the gates of the preparation at their values, the depth image's pathologies, the pixels that must not be read"""
import numpy as np
import pytest

import flowcrf_edges as fe
import flowcrf_oracle as fo
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu
F32 = np.float32


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,L,allow_new", fe.PAIR_CASES)
def test_a_workgroup_that_takes_several_chunks(gpu_ctx, w, h, L, allow_new):
    from multimotionfusion_amd.flowcrf import pad_labels
    widths = fe.PAIR_WIDTHS[(w, h, L, allow_new)]
    assert pad_labels(L) in widths
    for width in widths:  # the launch's own geometry: a later change of the split policy fails here, it does not hollow the case out
        nsplit, nchunk, per = fe.pair_geometry(w * h, width)
        print(f"{w}x{h} L={L} width {width}: nsplit {nsplit} nchunk {nchunk} per {per}, {fe.empty_ranges(nsplit, nchunk, per)} empty ranges")
        assert per >= 2 and fe.empty_ranges(nsplit, nchunk, per) >= 1, (width, nsplit, nchunk, per)
    sc, cfg, want, soft, want_soft, _ = fe.pair_case(w, h, L, allow_new)
    assert cfg["iterations"] == 2
    fe.check_against_oracle(gpu_ctx, sc, cfg, want)
    if want_soft is not None:  # pairwise weights of 1: Q is not saturated and follows the pair sums (fe.pair_case)
        print("soft weights:")
        fe.check_against_oracle(gpu_ctx, sc, soft, want_soft)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,L,allow_new", fe.WIDTH8_CASES)
def test_the_label_width_8(gpu_ctx, w, h, L, allow_new):
    sc, cfg, want = fe.case(w, h, L, allow_new)
    fe.check_against_oracle(gpu_ctx, sc, cfg, want)


@pytest.mark.parametrize("w,h,L,allow_new", [(8, 8, 2, False), (44, 12, 5, False)])
def test_an_engine_wider_than_the_call(gpu_ctx, w, h, L, allow_new):
    """max_labels = 32, as the fusion creates it, against the oracle and, bit for bit, against the engine made for L labels"""
    sc, cfg, want = fe.case(w, h, L, allow_new)
    wide = fe.check_against_oracle(gpu_ctx, sc, cfg, want, max_labels=32)
    fe.assert_same_run(wide, fe.run_once(gpu_ctx, sc, cfg), f"{fe.describe(sc)}: an engine for 32 labels and one for {L}")


def test_one_engine_at_32_then_3_then_32_labels(gpu_ctx):
    """xs, xa and hb are laid out per call, partial is sized over all widths, claim and cell by max_labels: each inference on
    the reused engine equals the one of a fresh engine made for its label count, bit for bit"""
    from multimotionfusion_amd.flowcrf import FlowCrf
    big, small = fe.case(80, 60, 32, False), fe.case(80, 60, 3, True)
    sc0, cfg = big[0], big[1]
    assert small[1] == cfg
    tracks = max(len(c[0]["tracks"]["ts_cur"]) for c in (big, small)) + 7
    e = FlowCrf(gpu_ctx, sc0["W"], sc0["H"], sc0["cam"], max_labels=32, max_tracks=tracks, **cfg)
    fresh = {}
    for step, (sc, _, _) in enumerate((big, small, big)):
        L = len(sc["ids"]) + int(sc["allow_new"])
        n = len(sc["tracks"]["ts_cur"])
        fe.infer(e, sc)
        got = fe.download(e, n)
        assert e.download("cell")[:, n:].max() == -1
        if L not in fresh:
            fresh[L] = fe.run_once(gpu_ctx, sc, cfg, max_tracks=tracks)
        fe.assert_same_run(got, fresh[L], f"step {step}: {L} labels on the reused engine against a fresh one")
        fe.replay_fusion(got, sc, f"step {step}")
    e.close()


@pytest.mark.parametrize("with_tracks", [True, False], ids=["tracks", "no-tracks"])
@pytest.mark.parametrize("w,h", fe.DEGENERATE_SIZES)
def test_degenerate_images(gpu_ctx, w, h, with_tracks):
    sc, cfg, want = fe.degenerate(w, h, with_tracks)
    got = fe.check_against_oracle(gpu_ctx, sc, cfg, want)
    assert got["Q"].shape == (3, h, w) and got["ids_full"].shape == (4 * h, 4 * w)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["three", "two", "two-new"])
@pytest.mark.parametrize("w,h", fe.TIE_SIZES)
def test_the_first_maximum_wins_a_tie(gpu_ctx, w, h, kind):
    sc, cfg, want = fe.tie_scene(w, h, kind)
    got = fe.check_against_oracle(gpu_ctx, sc, cfg, want, need_clear=False)
    inv = want["invalid"]
    assert inv.any() and not inv.all()
    assert_bit_equal(got["proj"][0 if kind != "three" else 1], got["proj"][1 if kind != "three" else 2], "proj of identical models")
    assert_bit_equal(got["prob"][0 if kind != "three" else 1], got["prob"][1 if kind != "three" else 2], "prob of identical models")
    first = 1 if kind == "three" else 0
    assert (got["label"][~inv] == first).all(), np.unique(got["label"][~inv])
    assert (got["label"][inv] == 0).all() and (got["prob"][:, inv] == 0).all()
    assert np.array_equal(got["label"], want["label"]) and np.array_equal(got["ids"], want["ids"])
    if kind == "two-new":
        assert (got["prob"][2] == 0).all() and not (got["ids"] == sc["new_id"]).any()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["below", "at", "above"])
def test_the_threshold_gate(gpu_ctx, which):
    """the threshold one float below, at and one float above the largest track error: outlier, neither, inlier"""
    sc, v, at = fe.threshold_scene()
    cfg, want = fe.threshold_reference(which)
    got = fe.check_against_oracle(gpu_ctx, sc, cfg, want)
    lo, hi = np.log(1 + np.exp(-1.0)), 1 + np.log(1 + np.exp(-1.0))
    target = dict(below=(hi, lo), at=(np.log(2.0), np.log(2.0)), above=(lo, hi))[which]
    assert at.sum() == 72 and np.abs(got["U"][:, at] - np.array(target)[:, None]).max() <= 1e-5, which


def test_the_min_proj_prob_gate(gpu_ctx):
    """two identical models: proj is exactly 0.5; `p < min_proj_prob` keeps it at 0.5 and drops it one float above"""
    sc = fe.twin_scene()
    for min_proj, value in ((0.5, F32(0.5)), (float(np.nextafter(F32(0.5), F32(1))), F32(0))):
        cfg = fo.config(iterations=0, min_proj_prob=min_proj)
        want = fo.run_scene(sc, cfg)
        got = fe.run_once(gpu_ctx, sc, cfg)
        inv = want["invalid"]
        assert np.array_equal(got["invalid"].astype(bool), inv) and inv.any()
        assert_bit_equal(got["proj"], want["proj"], f"proj at min_proj_prob {min_proj!r}")
        assert_bit_equal(got["proj"], np.where(inv[None], F32(0), value).astype(F32).repeat(2, 0), f"proj at min_proj_prob {min_proj!r}")
        fe.replay_fusion(got, sc, f"min_proj_prob {min_proj!r}")


def test_the_depth_classes(gpu_ctx):
    sc, cfg, want = fe.depth_class_scene()
    got = fe.check_against_oracle(gpu_ctx, sc, cfg, want)
    for (x, y), (name, d, zs, inv) in zip(fe.depth_class_cells(), fe.DEPTH_CLASSES):
        assert bool(got["invalid"][y, x]) == inv, name
        assert not np.isnan(got["proj"][:, y, x]).any() and np.abs(got["proj"][:, y, x] - want["proj"][:, y, x]).max() <= 1e-5, name
        assert np.array_equal(got["proj"][:, y, x] == 0, want["proj"][:, y, x] == 0), name


@pytest.mark.parametrize("w,h,L,allow_new", [(44, 12, 3, True)])
def test_only_the_sampled_pixels_are_read(gpu_ctx, w, h, L, allow_new):
    """every depth and vertex pixel that is not at (4x, 4y) is NaN: the same bits in every stage as without"""
    sc, cfg, want = fe.case(w, h, L, allow_new)
    clean = fe.check_against_oracle(gpu_ctx, sc, cfg, want)
    fe.assert_same_run(fe.run_once(gpu_ctx, sc, cfg, poison=True), clean, "poisoned pixels the engine must not read")
