"""-m gpu: the optical-flow engine (csrc/flow_kernels.hpp) against tests/flow_oracle.py, every stage image bit
for bit -- grey, smoothed, both expansions, the matrices, the flow behind every iteration, magnitude and motion -- at
flow-image sizes where every access clamps (8 x 8: the window is larger than the image), almost everything is border
(16 x 12), a tile has one more column (33 x 9), several ragged tiles (37 x 23) and the reference's 160 x 120; at every div,
the largest window and expansion radius, one and three iterations.  Then determinism, the sequence form against the pair
form, and the launch count."""
import numpy as np
import pytest
import torch

import flow_oracle as fo
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu
F32 = np.float32
STAGES = ("gray0", "gray", "smooth0", "smooth", "R0", "R1", "M", "magnitude", "motion")


def frames(w, h, n, seed):
    """n frames of a blocky random texture (8-pixel cells: edges and flat areas) sliding by a few pixels per frame, with
    per-pixel noise: flows of every size, pixels whose flow leaves the image among them"""
    rng = np.random.default_rng(seed)
    pad = 8 * n
    low = rng.integers(0, 256, size=((h + pad) // 8 + 2, (w + pad) // 8 + 2, 3), dtype=np.uint8)
    big = np.kron(low, np.ones((8, 8, 1), np.uint8))
    out = []
    for i in range(n):
        ox, oy = 3 * i, 2 * i
        f = big[oy:oy + h, ox:ox + w].astype(np.int32) + rng.integers(-12, 13, size=(h, w, 3))
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def engine(gpu_ctx, w, h, **cfg):
    from multimotionfusion_amd.flow import FarnebackFlow
    return FarnebackFlow(gpu_ctx, w, h, **cfg)


def check_pair(e, prev, nxt, cfg, what):
    """one compute() against the oracle, every stage; returns the device's result"""
    res = e.compute(dev(prev), dev(nxt))
    want = fo.pair(prev, nxt, cfg, tab=e.tables())
    for name in STAGES + tuple(f"flow_{i}" for i in range(cfg["iterations"])):
        got = e.download(name)
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (what, name, got.dtype, got.shape)
        assert_bit_equal(got, want[name], f"{what}: {name}")
    flow, mag, motion = (t.cpu().numpy() for t in res)
    assert_bit_equal(flow, want["flow"], f"{what}: result flow")
    assert_bit_equal(mag, want["magnitude"], f"{what}: result magnitude")
    assert_bit_equal(motion, want["motion"], f"{what}: result motion")
    assert e.last_launches() == 1 + 2 * cfg["iterations"], what
    return flow, mag, motion


CASES = [
    # flow-image size, configuration
    ((8, 8), dict()),
    ((16, 12), dict()),
    ((33, 9), dict()),
    ((37, 23), dict()),
    ((160, 120), dict()),
    ((37, 23), dict(div=2)),
    ((37, 23), dict(div=1)),
    ((37, 23), dict(winsize=33)),
    ((33, 9), dict(poly_n=7, poly_sigma=1.5)),
    ((16, 12), dict(iterations=1)),
    ((37, 23), dict(iterations=3, winsize=2, poly_n=3, poly_sigma=1.1)),
]


@pytest.mark.parametrize("size,over", CASES, ids=[f"{s[0]}x{s[1]}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'reference'}" for s, o in CASES])
def test_every_stage_image_equals_the_oracles(gpu_ctx, size, over):
    cfg = fo.config(**over)
    w, h = size[0] * cfg["div"], size[1] * cfg["div"]
    a, b = frames(w, h, 2, seed=size[0] * 100 + size[1])
    e = engine(gpu_ctx, w, h, **over)
    assert (e.w, e.h) == size
    from multimotionfusion_amd.flow import make_tables
    for got, want in zip(e.tables(), make_tables(cfg["poly_n"], cfg["poly_sigma"])):
        assert_bit_equal(got, want, "tables")
    first = check_pair(e, a, b, cfg, f"{size} {over}")
    assert np.isfinite(first[0]).all() and float(np.abs(first[0]).max()) > 0.1  # (the frames do move)
    # the same call again: the same bits
    again = e.compute(dev(a), dev(b))
    for x, y in zip(first, again):
        assert_bit_equal(y.cpu().numpy(), x, "second run")
    e.close()


def test_sequence_of_four_frames_equals_the_three_pairs(gpu_ctx):
    """mmf_flow_next keeps the last frame's expansion: frames 0..3 through next() give no flow, then the flows of (0,1),
    (1,2), (2,3) -- each equal to compute() on that pair in a second engine, flow, magnitude, motion and both expansions.
    reset() starts over: the next frame yields no flow."""
    w, h = 148, 92
    fs = frames(w, h, 4, seed=9)
    seq, pairs = engine(gpu_ctx, w, h), engine(gpu_ctx, w, h)
    assert seq.next(dev(fs[0])) is None and seq.last_launches() == 1
    for i in range(1, 4):
        got = seq.next(dev(fs[i]))
        assert got is not None and seq.last_launches() == 5
        want = pairs.compute(dev(fs[i - 1]), dev(fs[i]))
        for x, y, name in zip(got, want, ("flow", "magnitude", "motion")):
            assert_bit_equal(x.cpu().numpy(), y.cpu().numpy(), f"pair {i}: {name}")
        for name in ("R0", "R1", "gray", "smooth", "M", "flow_0"):
            assert_bit_equal(seq.download(name), pairs.download(name), f"pair {i}: {name}")
    seq.reset()
    assert seq.next(dev(fs[2])) is None
    got = seq.next(dev(fs[3]))
    for x, y in zip(got, pairs.compute(dev(fs[2]), dev(fs[3]))):
        assert_bit_equal(x.cpu().numpy(), y.cpu().numpy(), "after reset")
    seq.close(), pairs.close()


def test_no_result_before_the_first_pair(gpu_ctx):
    from multimotionfusion_amd import MmfError
    e = engine(gpu_ctx, 64, 48)
    with pytest.raises(MmfError, match="mmf_flow_result"):
        e._result()
    with pytest.raises(MmfError, match="mmf_flow_download"):
        e.download("R0")
    assert e.next(dev(frames(64, 48, 1, seed=1)[0])) is None
    assert e.download("gray").shape == (12, 16)  # the frame's own images are there, the pair's are not
    with pytest.raises(MmfError, match="mmf_flow_download"):
        e.download("flow_0")
    with pytest.raises(MmfError, match="mmf_flow_result"):
        e._result()
    e.close()


def test_a_frame_that_is_not_dword_aligned_gives_the_same_bits(gpu_ctx):
    """div 4 reads a row of a cell as three dwords when the frame starts on a dword, byte by byte otherwise"""
    w, h = 132, 36
    a, b = frames(w, h, 2, seed=4)
    e = engine(gpu_ctx, w, h)
    want = [t.cpu().numpy() for t in e.compute(dev(a), dev(b))]
    buf_a, buf_b = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda"), torch.empty(b.size + 3, dtype=torch.uint8, device="cuda")
    ua, ub = buf_a[1:].view(h, w, 3), buf_b[3:].view(h, w, 3)
    ua.copy_(dev(a)), ub.copy_(dev(b))
    assert ua.data_ptr() % 4 != 0 and ub.data_ptr() % 4 != 0
    got = [t.cpu().numpy() for t in e.compute(ua, ub)]
    for x, y in zip(got, want):
        assert_bit_equal(x, y, "unaligned frames")
    e.close()


def test_the_launch_count_does_not_depend_on_the_size(gpu_ctx):
    counts = set()
    for w, h in ((32, 32), (132, 36), (640, 480)):
        e = engine(gpu_ctx, w, h)
        a, b = frames(w, h, 2, seed=2)
        e.compute(dev(a), dev(b))
        counts.add(e.last_launches())
        e.close()
    assert counts == {5}
