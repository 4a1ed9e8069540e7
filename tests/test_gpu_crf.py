"""-m gpu: the dense-CRF motion segmentation on the device (mmf_crf_segment, csrc/crf_kernels.hpp) against tests/crf_oracle.py.

Stage 1 (super-pixel means) and stages 2-4 (range, confidences, unaries) are bit-exact; the mean field is compared with
the oracle's exact float64 Gaussian sums (|Q - Q_oracle| <= 1e-4) on scenes whose oracle top-two margin is >= 1e-3, where
the argmax maps must then be identical; stages 8-14 replayed by the oracle on the device's own argmax map must give the
device's mask, counts, floats and has_new_label exactly."""
import numpy as np
import pytest
import torch

import crf_oracle as co
from helpers import assert_bit_equal, slic_like_labels

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_scene(W, H, S, M, seed, new_region=True, background=True, zero_depth=False, tiny_new=False, boxes=()):
    """Full-resolution depth / colour and per-cell {icp, conf} maps of M models: model i >= 1 fits a box of cells, model 0
    everything else; cells that no model fits form the region a new label can take.  A few cells have low or non-finite
    confidence (the replacement rules of :274-285)."""
    rng = np.random.default_rng(seed)
    spx, spy = W // S, H // S
    N = spx * spy
    yy, xx = np.mgrid[0:spy, 0:spx]
    owner = np.zeros((spy, spx), np.int64) if background else np.ones((spy, spx), np.int64)
    for i in range(1, M):
        w, h = max(2, spx // (M + 2)), max(2, spy // 3)
        x0, y0 = 1 + (i * (spx - w - 2)) // max(M, 2), 1 + (i % 3) * max(1, (spy - h - 2) // 3)
        owner[y0:y0 + h, x0:x0 + w] = i
    if new_region:
        w = 1 if tiny_new else max(3, spx // 5)
        h = 1 if tiny_new else max(3, spy // 4)
        owner[spy - h - 1:spy - 1, spx - w - 1:spx - 1] = -1
    for i, x0, y0, w, h in boxes:  # extra cells model i fits (i < 0: no model)
        owner[y0:y0 + h, x0:x0 + w] = i
    owner = owner.ravel()
    icp = np.full((M, N), 0.5, F32)
    for i in range(M):
        icp[i, owner == i] = (rng.random(int((owner == i).sum()), dtype=F32) * 0.002).astype(F32)
    conf = (1.0 + rng.random((M, N), dtype=F32)).astype(F32)
    interior = np.flatnonzero((owner == 0) & (xx.ravel() > 2) & (xx.ravel() < spx // 3) & (yy.ravel() > 2))
    if len(interior) > 8:
        pick = rng.choice(interior, 6, replace=False)
        conf[0, pick[:2]] = 0.2   # model 0: conf < 0.3 -> error = range * 0.01
        if M > 1:
            conf[1, pick[2:4]] = 0.3  # conf <= 0.4 -> error = range * k
        conf[-1, pick[4]] = np.nan
        conf[0, pick[5]] = np.inf
    depth = (2.5 + 0.5 * np.random.default_rng(seed + 1).random((H, W), dtype=F32)).astype(F32)
    depth[np.random.default_rng(seed + 2).random((H, W)) < 0.05] = 0.0
    if zero_depth:
        depth[:] = 0.0
    rgb = np.random.default_rng(seed + 3).integers(0, 256, (H, W, 3)).astype(np.uint8)
    labels = slic_like_labels(W, H, S, seed=seed, empty_every=13)
    maps = np.stack([np.stack([icp[i], conf[i]]) for i in range(M)]).astype(F32)
    return labels, depth, rgb, maps


def run_device(gpu_ctx, labels, depth, rgb, maps, ids, next_id, allow_new, cfg):
    from multimotionfusion_amd import segmentation
    mask, data, has_new = segmentation.segment(gpu_ctx, dev(rgb), dev(depth), dev(maps), ids, next_id, allow_new,
                                               segmentation.CrfConfig(**cfg), labels=dev(labels))
    last = segmentation.last(gpu_ctx)
    return mask.cpu().numpy(), data, has_new, {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in last.items()}


def check_against_oracle(gpu_ctx, orc, W, H, S, M, allow_new, scene_kw=None, cfg=None, seed=3, need_margin=True):
    cfg = co.config(**(cfg or {}))
    cfg["spixel_size"] = S
    labels, depth, rgb, maps = make_scene(W, H, S, M, seed, **(scene_kw or {}))
    ids = list(range(M))
    next_id = M
    mask, data, has_new, last = run_device(gpu_ctx, labels, depth, rgb, maps, ids, next_id, allow_new, cfg)
    low_depth = orc.slic_downsample(labels, S, depth, threshold=0.02).ravel()
    ref = co.segment(low_depth, maps[:, 0], maps[:, 1], rgb.reshape(-1), W, H, S, ids, next_id, allow_new, cfg)
    assert last["range"] == ref["range"] and last["range_invalid"] == ref["range_invalid"]
    assert last["allow_new"] == bool(allow_new)
    if not ref["range_invalid"]:
        assert_bit_equal(last["unaries"], ref["unaries"], "unaries")
        dq = float(np.abs(last["q"].astype(np.float64) - ref["q"]).max())
        print(f"[crf] {W}x{H}/S{S} M={M} new={allow_new}: max |Q - Q_oracle| = {dq:.3e}, "
              f"oracle margin {co.top_two_margin(ref['q']):.3e}")
        assert dq <= 1e-4, dq
        if need_margin:
            assert co.top_two_margin(ref["q"]) >= 1e-3, "scene too close to a tie for a map comparison"
            assert np.array_equal(last["raw_map"], ref["raw_map"])
    # stages 8-14 of the oracle on the device's own argmax map
    spx, spy = W // S, H // S
    conf = maps[:, 1].copy()
    avg = co.avg_confidence(conf)
    out, odata, ohas = co.postprocess(last["raw_map"], spx, spy, W, H, S, ids, next_id, allow_new, low_depth, avg, cfg)
    assert np.array_equal(last["map"], out)
    assert np.array_equal(mask, orc.slic_upsample_u8(labels, out))
    assert has_new == ohas and len(data) == len(odata)
    for d, o in zip(data, odata):
        assert d["id"] == o["id"] and d["super_pixel_count"] == o["super_pixel_count"], (d, o)
        for k in ("avg_confidence", "depth_mean", "depth_std"):
            assert_bit_equal(np.array([d[k]], F32), np.array([o[k]], F32), k)
    # a second run gives the same bits
    mask2, data2, has2, last2 = run_device(gpu_ctx, labels, depth, rgb, maps, ids, next_id, allow_new, cfg)
    assert np.array_equal(mask, mask2) and data == data2 and has_new == has2
    assert_bit_equal(last["q"], last2["q"], "Q run to run")
    return ref, last, data, has_new


@pytest.mark.parametrize("W,H,S,M,allow_new", [
    (640, 480, 16, 1, True), (640, 480, 16, 2, False), (640, 480, 16, 2, True), (640, 480, 16, 3, True),
    (1280, 960, 16, 2, True), (1280, 960, 16, 10, False), (660, 470, 16, 3, True), (320, 240, 11, 10, True),
    (320, 240, 11, 1, False), (1280, 960, 16, 20, True)])
def test_standalone_parity(gpu_ctx, orc, W, H, S, M, allow_new):
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, W, H, S, M, allow_new)
    if allow_new:
        assert has_new and data[-1]["id"] == M  # the scene has a region no model fits


def test_new_label_never_chosen_is_dropped(gpu_ctx, orc):
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, 640, 480, 16, 2, True, dict(new_region=False))
    assert not has_new and len(data) == 2 and last["allow_new"]


def test_new_label_too_small_or_too_large(gpu_ctx, orc):
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, 640, 480, 16, 2, True, dict(tiny_new=True))
    assert not has_new and (last["raw_map"] == 2).any() and not (last["map"] == 2).any()
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, 640, 480, 16, 2, True, cfg=dict(max_rel_size_new=0.01))
    assert not has_new and (last["raw_map"] == 2).any()


def test_no_background_cell(gpu_ctx, orc):
    # with no background cell the smallest object id is the skipped key and keeps all of its components
    check_against_oracle(gpu_ctx, orc, 640, 480, 16, 3, True, dict(background=False))


def test_zero_depth_frame_is_all_background(gpu_ctx, orc):
    """B4: the depth range is 0 -> every cell background, no new label, flag set"""
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, 320, 240, 16, 2, True, dict(zero_depth=True))
    assert last["range_invalid"] and not has_new and (last["raw_map"] == 0).all()


def test_component_in_a_border_row(gpu_ctx, orc):
    """the only cells no model fits lie in the top row (box top = bottom = 8 px < 20): the new label wins them, and the
    border rule removes its component, so no new label is proposed"""
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, 640, 480, 16, 2, True,
                                                    dict(new_region=False, boxes=[(-1, 5, 0, 30, 1)]))
    assert (last["raw_map"][5:35] == 2).all() and not (last["map"] == 2).any() and not has_new


def test_tied_components(gpu_ctx, orc):
    """model 1 fits two disjoint boxes of equal size: the earlier one in raster order stays, the other becomes 255"""
    ref, last, data, has_new = check_against_oracle(gpu_ctx, orc, 640, 480, 16, 2, False,
                                                    dict(new_region=False, boxes=[(0, 0, 0, 40, 30), (1, 4, 4, 5, 4), (1, 20, 20, 5, 4)]))
    m = last["map"].reshape(30, 40)
    assert (m[4:8, 4:9] == 1).all() and (m[20:24, 20:25] == 255).all()
