"""-m gpu: the dense-CRF motion segmentation on the device (mmf_crf_segment, csrc/crf_kernels.hpp) against tests/crf_oracle.py.

Stage 1 (super-pixel means) and stages 2-4 (range, confidences, unaries) are bit-exact; the mean field is compared with
the oracle's exact float64 Gaussian sums (|Q - Q_oracle| <= 1e-4) on scenes whose oracle top-two margin is >= 1e-3, where
the argmax maps must then be identical; stages 8-14 replayed by the oracle on the device's own argmax map must give the
device's mask, counts, floats and has_new_label exactly.  The scenes and the check live in tests/crf_edges.py, which
test_gpu_crf_edges.py shares."""
import pytest

from crf_edges import check_against_oracle

pytestmark = pytest.mark.gpu


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
