"""-m gpu: the full-frame surfel passes (mmf_filter_depth, mmf_model_*) against the oracle at the shapes their kernels branch
on -- odd and unaligned filter inputs, the first and last widths around the two-pixel filter's INTERIOR workgroups, frame
sizes that are no multiple of the 16 x 16 resolve tiles or of the thumbnail's 20-pixel sample grid, sprites from one pixel to
the whole frame.  Bit for bit, as in test_gpu_surfel.py; test_oracle_surfel_shapes.py holds what the inputs must exercise."""
import numpy as np
import pytest
import torch

import surfel_shapes as sh
from helpers import assert_bit_equal
from multimotionfusion_amd import synth
from surfel_shapes import splat_bound  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("w,h", sh.FILTER_SHAPES)
def test_filter_depth_shapes(gpu_ctx, orc, w, h):
    """Odd widths run bilateral_filter_kernel (one pixel per lane), even ones bilateral_filter2_kernel, whose workgroup b of 128
    columns takes the INTERIOR instantiation when 128 b - 6 >= 0 and 128 b + 134 < cols: none at 262, b = 1 at 264, still only
    b = 1 at 390, b = 1 and 2 at 392 -- with a partly filled workgroup 3 beside them; 13 x 13 and smaller: every window
    leaves the image on all sides."""
    from multimotionfusion_amd.model import filterDepth
    d = sh.filter_input(w, h)
    out = filterDepth(gpu_ctx, dev(d), sh.CUTOFF)
    assert_bit_equal(out.cpu().numpy(), orc.bilateral_filter(d, sh.CUTOFF), f"bilateral filter {w} x {h}")


def test_filter_depth_unaligned_pointers(gpu_ctx, orc):
    """An even width whose input and output start 4 bytes into their buffers: no 8-byte loads, so the dispatcher must take the
    one-pixel kernel -- same bits as the aligned call and as the oracle."""
    from multimotionfusion_amd.model import filterDepth
    w, h = 264, 8
    d = sh.filter_input(w, h)
    src, dst = torch.zeros(w * h + 2, dtype=torch.float32, device="cuda"), torch.full((w * h + 2,), -1.0, dtype=torch.float32, device="cuda")
    d_in, d_out = src[1:1 + w * h].view(h, w), dst[1:1 + w * h].view(h, w)
    d_in.copy_(dev(d))
    assert src.data_ptr() % 8 == 0 and d_in.data_ptr() % 8 == 4 and d_out.data_ptr() % 8 == 4
    filterDepth(gpu_ctx, d_in, sh.CUTOFF, out=d_out)
    aligned = filterDepth(gpu_ctx, dev(d), sh.CUTOFF)
    want = orc.bilateral_filter(d, sh.CUTOFF)
    assert_bit_equal(d_out.cpu().numpy(), want, "unaligned against the oracle")
    assert_bit_equal(aligned.cpu().numpy(), want, "aligned against the oracle")
    assert dst[0].item() == -1.0 and dst[-1].item() == -1.0  # nothing written outside the view


@pytest.mark.parametrize("splat_bound", [-1, 1], indirect=True)
@pytest.mark.parametrize("w,h", sh.CYCLE_SHAPES)
def test_surfel_cycle_ragged_sizes(gpu_ctx, orc, w, h, splat_bound):
    """test_surfel_cycle_bit_exact's loop at the smallest size mmf_model_create allows and at sizes that are multiples of 4
    but not of 16 (a ragged last tile column and / or row in every splat resolve) nor of 20 (the thumbnail's samples do not
    divide the frame), wider than tall and taller than wide."""
    sh.surfel_cycle(orc, w, h, gpu_ctx)


@pytest.mark.parametrize("bound", [0, 1])
@pytest.mark.parametrize("w,h", sh.SPRITE_SHAPES)
def test_sprite_extremes(gpu_ctx, orc, w, h, bound):
    """splat_kernel_body on sprites of 1 pixel and of the whole frame in one wave (the packed x0 | x1 << 16, y0 | nseg << 16
    and the division by nseg by multiplication at their largest: 160 segments x 480 rows), sprites clipped on every image
    side, centres on pixel-grid lines, NaN normals; without and with the early depth test."""
    from multimotionfusion_amd.model import Model
    K = synth.intrinsics(w, h)
    s, _ = sh.sprite_store(w, h)
    pose, tick = np.eye(4, dtype=np.float32), sh.SPRITE_TICK
    m = Model(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], 0, sh.CONF)
    gpu_ctx.lib.mmf_debug_set_splat_bound(bound)
    try:
        m.uploadMap(s)
        m.overridePose(pose)
        m.predictIndices(tick, sh.MAXD, sh.TIME_DELTA)
        index, vc, ct, nr = orc.predict_indices(s, pose, K, w, h, sh.MAXD, tick, sh.TIME_DELTA)
        assert_bit_equal(m.texture("index").cpu().numpy().view(np.uint32), index, "index map")
        assert_bit_equal(m.texture("vertConf").cpu().numpy(), vc, "vertConf")
        assert_bit_equal(m.texture("colorTime").cpu().numpy(), ct, "colorTime")
        assert_bit_equal(m.texture("normRad").cpu().numpy(), nr, "normRad")
        m.combinedPredict(sh.MAXD, tick, tick, sh.TIME_DELTA)
        image, vcp, nrp, tm = orc.combined_predict(s, pose, K, w, h, sh.MAXD, sh.CONF, tick, tick, sh.TIME_DELTA)
        assert_bit_equal(m.texture("image").cpu().numpy(), image, "splat image")
        assert_bit_equal(m.texture("vertexConf").cpu().numpy(), vcp, "splat vertexConf")
        assert_bit_equal(m.texture("normalRadius").cpu().numpy(), nrp, "splat normalRadius")
        assert_bit_equal(m.texture("time").cpu().numpy().view(np.uint16), tm, "splat time")
        m.synthesizeDepth(sh.MAXD, sh.CONF, tick, tick, sh.TIME_DELTA)
        sd = orc.synthesize_depth(s, pose, K, w, h, sh.MAXD, sh.CONF, tick, tick, sh.TIME_DELTA)
        assert_bit_equal(m.texture("depth").cpu().numpy(), sd, "synthesized depth")
    finally:
        gpu_ctx.lib.mmf_debug_set_splat_bound(-1)
        m.close()
