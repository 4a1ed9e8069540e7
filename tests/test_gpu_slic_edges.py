"""-m gpu: the super-pixel resampling (mmf_slic_downsample, thresholded and plain, mmf_slic_downsample_rgb, mmf_slic_upsample_u8;
csrc/slic_kernels.hpp) at the edges of its run compaction, substitute chains, label range and sizes, against the plain-Python
reference of tests/slic_edges.py: ints, u8 and non-NaN floats bit for bit, NaN where the reference holds NaN (sign and payload
are no contract), a second call with the same bytes.  test_slic_edges_oracle.py pins that reference to the C oracle and asserts
that every case reaches the edge it is named for.

shape  11x11 (n = 1, a wave over several rows), 33x47 portrait, 75x26 odd S with a clamped centre row, 130x24 with a band as
       wide as the image and a label on the last row and column only, 160x128, 255x255 at S = 255
chain  thresholded chains of depth 2 and 3 into a finished mean, depth 2 into a raw sum, a self-substitute, absent labels,
       no substitute (NaN, or 0 in RGB)
index  the odd-S truncation and the clamped row each pick another substitute than the near misses
oob    labels -1, n and 2^31 - 1 as single pixels, as a run between two runs of one label, as first and last pixel, at n = 1
wave   runs across pixels 64, 128 and 256
sum    order-sensitive values, the threshold met exactly, NaN / inf / -0.0, four channels
rgb    3 and 4 channels, all 255 and all 0
up     a map of one entry and one larger than the grid"""
import numpy as np
import pytest

import slic_edges as se

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(se.CASES))
def test_edge_case(gpu_ctx, name):
    se.check_case(gpu_ctx, name)


def test_reused_workspace(gpu_ctx):
    """n = 80, 1, 12, 80, 10 on one context, the modes alternating: nothing of an earlier call's workspace shows"""
    for name, mode in se.SEQUENCE:
        se.check_case(gpu_ctx, name, modes=(mode,), twice=False)


def test_refusals(gpu_ctx):
    import torch
    from multimotionfusion_amd import MmfError, slic
    from multimotionfusion_amd.cudafuncs import _p

    W, H, S = 64, 48, 16
    labels = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    img4 = torch.zeros((H, W, 4), device="cuda")
    rgb2 = torch.zeros((H, W, 2), dtype=torch.uint8, device="cuda")
    rgb3 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    big = torch.zeros((512, 512), dtype=torch.int32, device="cuda")
    out = torch.zeros((H // S, W // S), device="cuda")
    full = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    small = torch.ones(12, dtype=torch.uint8, device="cuda")
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    refused = {
        "channel-is-channels": lambda: slic.downsample(gpu_ctx, labels, S, img4, channel=4),
        "channel-negative": lambda: slic.downsample(gpu_ctx, labels, S, img4, channel=-1),
        "rgb-2-channels": lambda: slic.downsample_rgb(gpu_ctx, labels, S, rgb2),
        "S10": lambda: slic.downsample(gpu_ctx, labels, 10, img4),
        "S256": lambda: slic.downsample(gpu_ctx, big, 256, torch.zeros((512, 512), device="cuda")),
        "nspix0": lambda: lib.mmf_slic_upsample_u8(h, _p(labels), W, H, _p(small), 0, _p(full)),
        "null-image": lambda: lib.mmf_slic_downsample(h, _p(labels), W, H, S, _p(None), 1, 0, 0, 0.0, _p(out), _p(None)),
        "null-labels": lambda: lib.mmf_slic_downsample_rgb(h, _p(None), W, H, S, _p(rgb3), 3, _p(out)),
    }
    assert list(refused) == se.REFUSALS
    slic.downsample(gpu_ctx, labels, S, img4, channel=3)  # (the calls themselves are fine)
    slic.downsample_rgb(gpu_ctx, labels, S, rgb3)
    for what, call in refused.items():
        try:
            status = call()
        except MmfError as e:
            status = e.status
        assert status == -1, f"{what}: status {status}, not MMF_ERR_INVALID"
        se.check_case(gpu_ctx, "chain-d2-lower", twice=False)  # a refused call leaves the next one correct
    slic.downsample(gpu_ctx, labels, 11, img4)  # the limits themselves are accepted
    slic.downsample(gpu_ctx, big, 255, torch.zeros((512, 512), device="cuda"))
    assert np.array_equal(slic.upsample_u8(gpu_ctx, labels, small[:1]).cpu().numpy(), np.ones((H, W), np.uint8))
