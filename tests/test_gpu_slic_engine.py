"""-m gpu: the super-pixel engine (mmf_slic_segment, csrc/slic_engine_kernels.hpp) against tests/slic_oracle.py: labels,
centres and counts BIT FOR BIT after 0, 1 and 5 iterations -- every pixel and every centre takes part in the comparison.
Integer sums and float32 in a fixed order make the results independent of the order the pixels are visited in, so two
calls, and a second context on another stream, give identical bytes as well."""
import numpy as np
import pytest
import torch

import slic_oracle as so
from helpers import assert_bit_equal
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frame(w, h, seed=0):
    objs = synth.make_objects(1, seed=21)
    traj = synth.object_trajectories(objs, 2, seed=21, trans_mm=60.0, rot_deg=2.0)
    return synth.render(synth.trajectory(2, seed=21)[1], w, h, seed=seed, objects=objs, object_poses=[t[1] for t in traj])["rgb"]


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def saturated(w, h):
    """flat regions at 0 and 255 (exact ties inside them, the largest colour distances across them) around a noisy band"""
    rgb = noise(w, h, 11)
    rgb[: h // 3] = 255
    rgb[2 * h // 3:] = 0
    rgb[:, : w // 4, 0] = 255
    return rgb


def references(rgb, S, centres=None, upto=5):
    """the oracle after 0 .. upto iterations from ONE run: k iterations end with the association that opens iteration k + 1"""
    trace = []
    lab, c, cnt = so.segment(rgb, S, upto, centres=centres, trace=trace)
    n = (rgb.shape[1] // S) * (rgb.shape[0] // S)
    start = so.init_centres(rgb, S) if centres is None else np.array(centres, F32)
    out = {0: (trace[0][0] if trace else lab, start, np.zeros(n, np.int32)), upto: (lab, c, cnt)}
    for k in range(1, upto):
        out[k] = (trace[k][0], trace[k - 1][1], trace[k - 1][2])
    return out


def compare(ctx, rgb, S, iterations, centres=None, what="", ref=None):
    from multimotionfusion_amd import slic
    lab, c, cnt = slic.segment(ctx, dev(rgb), S, iterations, centres=None if centres is None else dev(centres), with_centres=True)
    ref_lab, ref_c, ref_cnt = ref[iterations] if ref is not None else so.segment(rgb, S, iterations, centres=centres)
    lab, c, cnt = lab.cpu().numpy(), c.cpu().numpy(), cnt.cpu().numpy()
    n_diff = int((lab != ref_lab).sum())
    print(f"[slic engine] {what} {rgb.shape[1]}x{rgb.shape[0]} S={S} it={iterations}: {n_diff} labels differ, "
          f"{int((c.view(np.uint32) != ref_c.view(np.uint32)).sum())} centre words differ, {int((cnt != ref_cnt).sum())} counts differ")
    assert_bit_equal(lab, ref_lab, f"labels {what} S={S} it={iterations}")
    assert_bit_equal(c, ref_c, f"centres {what} S={S} it={iterations}")
    assert_bit_equal(cnt, ref_cnt, f"counts {what} S={S} it={iterations}")
    return lab, c, cnt


@pytest.mark.parametrize("w,h,S", [(320, 240, 16), (320, 240, 20), (640, 480, 16), (640, 480, 20), (640, 480, 32), (640, 480, 40),
                                   (1280, 960, 16), (1280, 960, 32)])
def test_synthetic_frames_bit_for_bit(gpu_ctx, w, h, S):
    rgb = frame(w, h, seed=w + S)
    ref = references(rgb, S)
    for it in (0, 1, 5):
        lab, c, cnt = compare(gpu_ctx, rgb, S, it, what="frame", ref=ref)
    n = (w // S) * (h // S)
    assert lab.min() >= 0 and lab.max() < n and cnt.sum() == w * h


@pytest.mark.parametrize("kind", ["noise", "constant", "saturated"])
def test_noise_constant_and_saturated_images_bit_for_bit(gpu_ctx, kind):
    w, h, S = 640, 480, 16
    rgb = {"noise": noise(w, h, 7), "constant": np.full((h, w, 3), 131, np.uint8), "saturated": saturated(w, h)}[kind]
    if kind == "constant":  # thousands of exact ties, resolved by scan order
        ref = so.associate(rgb, so.init_centres(rgb, S), S)
        g = ((np.arange(h)[:, None] // S) * (w // S) + np.arange(w)[None, :] // S)
        assert (ref != g).sum() > 1000
    ref = references(rgb, S)
    for it in (0, 1, 5):
        compare(gpu_ctx, rgb, S, it, what=kind, ref=ref)


def test_odd_sizes_and_unaligned_rows(gpu_ctx):
    """S = 11 on 99 x 77: rows are not a multiple of four pixels and the image is not a multiple of four either (the
    four-pixel threads straddle rows and cells, the last one is partial)"""
    for w, h, S in [(99, 77, 11), (143, 39, 13)]:
        ref = references(noise(w, h, w), S)
        for it in (0, 1, 5):
            compare(gpu_ctx, noise(w, h, w), S, it, what="odd", ref=ref)


def test_unaligned_image_buffer(gpu_ctx):
    """an image that starts at an odd address takes the byte-wise loads of the association: same bits"""
    from multimotionfusion_amd import slic
    w, h, S = 96, 64, 16
    rgb = noise(w, h, 23)
    buf = torch.empty(rgb.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = dev(rgb).reshape(-1)
    view = buf[1:].view(h, w, 3)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    got = slic.segment(gpu_ctx, view, S, 5, with_centres=True)
    for x, y, what in zip(got, so.segment(rgb, S, 5), ("labels", "centres", "counts")):
        assert_bit_equal(x.cpu().numpy(), y, what)


def test_large_superpixels_sums_beyond_2_pow_24(gpu_ctx):
    """S = 160 on 1280 x 960 noise: the x sums of a cluster pass 2^24 (float tree sums would round); integer totals
    converted once stay bit-exact against the oracle's integer sums"""
    w, h, S = 1280, 960, 160
    rgb = noise(w, h, 13)
    trace = []
    so.segment(rgb, S, 2, trace=trace)
    assert max(int(t[3].max()) for t in trace) > 2 ** 24
    ref = references(rgb, S)
    for it in (1, 5):
        compare(gpu_ctx, rgb, S, it, what="S=160", ref=ref)


def test_largest_superpixel_size(gpu_ctx):
    """S = 255: the window of an update is 765 x 765 pixels"""
    w, h, S = 765, 510, 255
    ref = references(noise(w, h, 17), S, upto=2)
    for it in (0, 2):
        compare(gpu_ctx, noise(w, h, 17), S, it, what="S=255", ref=ref)


def test_centres_in_empty_cluster_keeps_its_values_and_downsample_resamples_it(gpu_ctx, orc):
    """a centre no pixel can choose (handed in far away): count 0, position and colour kept through every update, the
    label absent -- and mmf_slic_downsample on these labels takes its resampleEmptyIndex path, against oracle/ as
    test_gpu_slic.py checks it for hand-made labels"""
    from multimotionfusion_amd import slic
    w, h, S = 320, 240, 16
    rgb = frame(w, h, seed=4)
    cin = so.init_centres(rgb, S)
    empty = [27, 150, 299]  # (299 = the last one: its substitute has a lower index)
    for k in empty:
        cin[k] = (3e5, 3e5, 0, 0, 0)
    cin[77] = np.nan        # every distance to it is NaN: `<` is false
    cin[78, :2] = 1e30      # ... and here +inf
    empty += [77, 78]
    ref = references(rgb, S, centres=cin)
    for it in (0, 1, 5):
        lab, c, cnt = compare(gpu_ctx, rgb, S, it, centres=cin, what="centres_in", ref=ref)
        for k in empty:
            assert k not in lab and c[k].tobytes() == cin[k].tobytes()
            assert it == 0 or cnt[k] == 0
    rng = np.random.default_rng(3)
    img = rng.random((h, w), dtype=np.float32)
    depth = rng.random((h, w), dtype=np.float32) * 4.0
    depth[rng.random((h, w)) < 0.25] = 0.0
    n = (w // S) * (h // S)
    got, counts = slic.downsample(gpu_ctx, dev(lab), S, dev(img), with_counts=True)
    assert_bit_equal(got.cpu().numpy(), orc.slic_downsample(lab, S, img), "means on the engine's labels")
    assert_bit_equal(counts.cpu().numpy().ravel(), orc.slic_counts(lab, n), "spixelCounts on the engine's labels")
    assert all(counts.cpu().numpy().ravel()[k] == 0 for k in empty)
    got = slic.downsample(gpu_ctx, dev(lab), S, dev(depth), threshold=0.02)
    assert_bit_equal(got.cpu().numpy(), orc.slic_downsample(lab, S, depth, threshold=0.02), "lowDepth on the engine's labels")


def test_two_calls_and_a_second_context_give_identical_bytes(gpu_ctx):
    from multimotionfusion_amd import slic
    from multimotionfusion_amd.cudafuncs import Context
    w, h, S = 640, 480, 16
    rgb = dev(frame(w, h, seed=9))
    a = slic.segment(gpu_ctx, rgb, S, with_centres=True)
    b = slic.segment(gpu_ctx, rgb, S, with_centres=True)
    other = Context(0, use_torch_stream=False)
    try:
        torch.cuda.synchronize()
        c = slic.segment(other, rgb, S, with_centres=True)
        other.synchronize()
        for x, y, z in zip(a, b, c):
            x, y, z = x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy()
            assert x.tobytes() == y.tobytes() == z.tobytes()
    finally:
        other.close()


def test_refuses_ragged_and_out_of_range_sizes(gpu_ctx):
    from multimotionfusion_amd import MmfError, slic
    for w, h, S in [(320, 240, 32), (330, 240, 16), (320, 240, 10), (512, 512, 256)]:
        with pytest.raises(MmfError):
            slic.segment(gpu_ctx, torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"), S)
