"""-m gpu: the optical-flow engine (csrc/flow_kernels.hpp) at the edges of its number ranges and tiles, on the
cases of tests/flow_edges.py: every stage image -- gray0, gray, smooth0, smooth, R0, R1, M, the flow behind every iteration,
magnitude, motion -- equals tests/flow_oracle.py bit for bit, the sign of zero included, through test_gpu_flow.check_pair.
tests/test_flow_edges_oracle.py asserts on the oracle alone what each case reaches: determinants that cancel to rounding
noise of either sign (negative idet, flows beyond 2^31 that take the warp's outside branch), exact zeros (idet == 1000.0f,
-0.0 flows, subnormal expansion coefficients), the warp's last inside and first outside positions, every rounding tie of the
integer front end, and the tile, halo and window combinations test_gpu_flow.py leaves out.  No case holds a NaN (asserted
there), so plain bit equality is the bar.  Then the launch count, a second run, the sequence form over a degenerate pair,
frames at byte offset 2, and the degenerate flow as the flow-CRF inference consumes it.

Not pinned: the warp's NaN branch.  No input reaches a non-finite flow within the limit of ten iterations (the growth is
about tenfold per iteration from about 1e3: 2e13 at the tenth), and the C ABI has no entry point that injects a flow; the
guard `x1f >= 0 && x1f < W-1 && ...` is pinned for finite flows of either sign beyond the integer range only."""
import numpy as np
import pytest
import torch

import flow_edges as fe
import flow_oracle as fo
from helpers import assert_bit_equal
from test_gpu_flow import check_pair, dev, engine

pytestmark = pytest.mark.gpu
F32 = np.float32


def size(c):
    return c.prev.shape[1], c.prev.shape[0]


def frames_of(c):
    """writable copies (torch.from_numpy warns about a read-only array; the case's own frames stay untouched)"""
    return c.prev.copy(), c.nxt.copy()


@pytest.mark.parametrize("name", fe.NAMES)
def test_every_stage_image_equals_the_oracles(gpu_ctx, name):
    c = fe.case(name)
    cfg = fo.config(**c.over)
    e = engine(gpu_ctx, *size(c), **c.over)
    assert (e.w, e.h) == fe.flow_size(c)
    prev, nxt = frames_of(c)
    first = check_pair(e, prev, nxt, cfg, name)  # (asserts 1 + 2 * iterations launches)
    assert all(np.isfinite(a).all() for a in first), name
    assert e.last_launches() == 1 + 2 * cfg["iterations"]
    again = e.compute(dev(prev), dev(nxt))
    for x, y, what in zip(first, again, ("flow", "magnitude", "motion")):
        assert_bit_equal(y.cpu().numpy(), x, f"{name}: second run, {what}")
    e.close()


@pytest.mark.parametrize("name", fe.SEQUENCE)
def test_the_kept_expansion_survives_a_degenerate_pair(gpu_ctx, name):
    """frames 0, 1, 0 through next(): the flows of (0, 1) and (1, 0), each equal to compute() on that pair in a second
    engine -- the expansion kept from frame 1 is the one compute() makes of it, whatever the solve did in between"""
    c = fe.case(name)
    cfg = fo.config(**c.over)
    prev, nxt = frames_of(c)
    fs = (prev, nxt, prev)
    seq, pairs = engine(gpu_ctx, *size(c), **c.over), engine(gpu_ctx, *size(c), **c.over)
    assert seq.next(dev(fs[0])) is None and seq.last_launches() == 1
    stages = ("gray0", "gray", "smooth0", "smooth", "R0", "R1", "M", "magnitude", "motion") + tuple(f"flow_{i}" for i in range(cfg["iterations"]))
    for i in (1, 2):
        got = seq.next(dev(fs[i]))
        assert got is not None and seq.last_launches() == 2 * cfg["iterations"] + 1
        want = pairs.compute(dev(fs[i - 1]), dev(fs[i]))
        for x, y, what in zip(got, want, ("flow", "magnitude", "motion")):
            assert_bit_equal(x.cpu().numpy(), y.cpu().numpy(), f"{name}, pair {i}: {what}")
        for s in stages:
            assert_bit_equal(seq.download(s), pairs.download(s), f"{name}, pair {i}: {s}")
    seq.close(), pairs.close()


@pytest.mark.parametrize("offsets", [(2, 2), (2, 0), (0, 2)])
def test_a_frame_at_byte_offset_2_gives_the_same_bits(gpu_ctx, offsets):
    """div 4 reads a row of a cell as three dwords when the frame starts on a dword, byte by byte otherwise: offset 2 is the
    one test_gpu_flow.py leaves out (it runs 1 and 3), here on the frames whose channel sums all stand on a rounding tie"""
    c = fe.case("front_div4")
    h, w = c.prev.shape[:2]
    prev, nxt = frames_of(c)
    e = engine(gpu_ctx, w, h, **c.over)
    want = [t.cpu().numpy() for t in e.compute(dev(prev), dev(nxt))]
    stages = {s: e.download(s) for s in ("gray0", "gray", "R0", "R1", "M")}
    views = []
    for f, off in zip((prev, nxt), offsets):
        buf = torch.empty(f.size + 4, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        v = buf[off:off + f.size].view(h, w, 3)
        v.copy_(dev(f))
        assert v.data_ptr() % 4 == off
        views.append(v)
    torch.cuda.synchronize()  # (the copies ran on torch's stream, the engine runs on the context's)
    got = [t.cpu().numpy() for t in e.compute(*views)]
    for x, y, what in zip(got, want, ("flow", "magnitude", "motion")):
        assert_bit_equal(x, y, f"offsets {offsets}: {what}")
    for s, a in stages.items():
        assert_bit_equal(e.download(s), a, f"offsets {offsets}: {s}")
    e.close()


def test_the_degenerate_flow_through_the_flow_crf_inference(gpu_ctx):
    """The device's flow and motion of the three-iteration diagonal bands (negative idet in the first iteration, flows above
    1000 in the second, 57 flow pixels left in the result) handed to FlowCrf.infer in a two-model scene, against
    flowcrf_oracle.infer under the tolerances of test_gpu_flowcrf.py: 1e-5 on U and proj, 1e-4 on Q and prob, the labels equal
    where the oracle's margin is at least 1e-3.  The appearance features are 10 * flow: distances of up to 900 (squared: 8e5)
    go through the pair kernel's exponential.  That 90 % of the cells are clear is asserted on the CPU
    (test_flow_edges_oracle.py: 99.9 %)."""
    import flowcrf_oracle as fc
    from test_gpu_flowcrf import STAGES, engine as crf_engine, infer
    c = fe.case(fe.CHAINED)
    e = engine(gpu_ctx, *size(c), **c.over)
    flow, _, motion = (t.cpu().numpy() for t in e.compute(*(dev(f) for f in frames_of(c))))
    e.close()
    assert np.isfinite(flow).all() and float(np.abs(flow).max()) > 10
    sc, cfg, want = fe.chained_scene(flow, motion)
    assert (sc["W"], sc["H"]) == (4 * motion.shape[1], 4 * motion.shape[0])
    ce = crf_engine(gpu_ctx, sc, cfg)
    infer(ce, sc)
    got = {name: ce.download(name) for name in STAGES}
    U, Uo = got["U"], want["U"]
    assert np.array_equal(np.isposinf(U), np.isposinf(Uo)) and not np.isnan(U).any()
    fin = np.isfinite(Uo)
    errU = np.abs(U[fin] - Uo[fin]) / np.maximum(1, np.abs(Uo[fin]))
    near = np.abs(want["proj64"] - 0.3) < 1e-5
    assert near.mean() < 0.01
    errP = np.abs(got["proj"] - want["proj"])[~near]
    errQ = np.abs(got["Q"].astype(np.float64) - want["Q"])
    errProb = np.abs(got["prob"].astype(np.float64) - want["prob"])
    print(f"chained: max |dU| {errU.max():.3g}  |dproj| {errP.max():.3g}  |dQ| {errQ.max():.3g}  |dprob| {errProb.max():.3g}")
    assert errU.max() <= 1e-5 and errP.max() <= 1e-5
    assert errQ.max() <= 1e-4 and errProb.max() <= 1e-4
    clear = want["margin"] >= 1e-3
    assert clear.mean() >= 0.9
    assert np.array_equal(got["label"][clear], want["label"][clear]) and np.array_equal(got["ids"][clear], want["ids"][clear])
    assert np.array_equal(got["ids_full"], fc.upscale4(got["ids"]))
    assert ce.last_launches() == 5 + 3 * cfg["iterations"]
    ce.close()
