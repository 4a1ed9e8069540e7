"""-m gpu: the photometric passes at their window, warp, gate and size edges (the cases of tests/photo_edges.py; what each
claims is checked on the CPU by tests/test_photo_edges_oracle.py).

The per-pixel decision of Core/Cuda/reduce.cu:773-812 exists in four hand-written copies; which cases reach which:
  stand-alone aligned   (track_kernels.hpp: residual_block4<false, true>)   every stand-alone case with cols % 4 == 0, dense
  stand-alone ragged    (residual_block4<false, false>)                      every case: the others as they are, those again
                                                                             with the next image one byte off and with a pitch
                                                                             that is no multiple of four
  two-launch, compact   (residual_block4<true, true> + rgb_gather<., true>)  the static cases through the whole pyramid with
                                                                             mmf_debug_set_gn_fused(0), and in rgbOnly
  one-launch            (gn_fused.hpp: gn_pixel_waves<PX, .>)                the 40 x 32 static cases with PX forced to 1, 2, 4
                                                                             and 5, each PX once at the size that picks it,
                                                                             and the pyramid with mmf_debug_set_gn_fused(1)
Everything is an exact integer, bit equality, helpers.se3_sum_tolerance or the bound of test_so3_step_parity.
"""
import numpy as np
import pytest
import torch

import gn_range as gr
import photo_edges as pe
from helpers import assert_bit_equal, se3_sum_tolerance
from test_gpu_gn_range import product, status, truncated  # (truncated runs under that file's `undisturbed` guard)

pytestmark = pytest.mark.gpu

CASES = pe.standalone_cases()
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in pe.FAMILIES}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cases are read-only)


def vec4_expected(cols, tensors, err):
    """csrc/mmf_hip.hip, residual_vec4_ok, from the pointers and strides this test chose"""
    nxt, dIdx, dIdy, nd, corres = (tensors[k] for k in ("next_image", "dIdx", "dIdy", "next_depth", "corres"))
    al = lambda t, n: t.data_ptr() % n == 0  # noqa: E731
    return (cols % 4 == 0 and nxt.stride(0) % 4 == 0 and dIdx.stride(0) % 4 == 0 and nd.stride(0) % 4 == 0 and al(nxt, 4) and al(dIdx, 8) and
            al(dIdy, 8) and al(nd, 16) and al(err, 16) and err.stride(0) % 4 == 0 and al(corres, 16))


def offset_image(img, how):
    """the same image one byte into a larger buffer, or with a pitch of cols + 1; what surrounds it is zero (a kernel that
    took a byte from beside the image for one inside it would find the window broken)"""
    rows, cols = img.shape
    if how == "offset":
        buf = torch.zeros(rows * cols + 64, dtype=torch.uint8, device="cuda")
        view = buf[1:1 + rows * cols].view(rows, cols)
    else:
        buf = torch.zeros(rows, cols + 1, dtype=torch.uint8, device="cuda")
        view = buf[:, :cols]
    view.copy_(dev(img))
    return view


def residual_on_device(gpu_ctx, case, how):
    from multimotionfusion_amd import cudafuncs as cf
    rows, cols = case.next_image.shape
    t = {k: dev(getattr(case, k)) for k in ("dIdx", "dIdy", "last_depth", "next_depth", "last_image")}
    t["next_image"] = dev(case.next_image) if how == "dense" else offset_image(case.next_image, how)
    out = []
    for _ in range(2):  # the second call on the same inputs gives the same bytes
        t["corres"] = torch.full((rows, cols, 16), 0xA5, dtype=torch.uint8, device="cuda")
        err = torch.full((rows, cols), -1.0, device="cuda")
        sigma, count = cf.computeRgbResidual(gpu_ctx, float(case.min_scale), t["dIdx"], t["dIdy"], t["last_depth"], t["next_depth"], t["last_image"],
                                             t["next_image"], t["corres"], float(case.max_depth_delta), case.kt, case.krkinv, err)
        out.append((t["corres"].cpu().numpy(), sigma, count, err.cpu().numpy()))
    return out, vec4_expected(cols, t, err)


# ---- stand-alone residual ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", pe.FAMILIES)
def test_standalone_residual_is_the_oracle_s_on_both_kernels(gpu_ctx, orc, family):
    """Records (all 16 bytes), error map, count and sum of every case, bit for bit: dense (the four-pixels-per-lane kernel where
    cols % 4 == 0, the ragged one elsewhere), and the cols % 4 == 0 cases again on the ragged kernel."""
    kernels = {True: 0, False: 0}
    for case in BY_FAMILY[family]:
        rows, cols = case.next_image.shape
        rec, sumsq, count, err = pe.oracle_result(orc, case.name)
        assert count == case.claim["count"]
        for how in ("dense",) + (("offset", "pitch") if cols % 4 == 0 else ()):
            (first, second), vec4 = residual_on_device(gpu_ctx, case, how)
            assert vec4 == (how == "dense" and cols % 4 == 0), (case.name, how)  # which kernel the host must have taken
            kernels[vec4] += 1
            for got in (first, second):
                assert (got[1], got[2]) == (sumsq, count), (case.name, how, got[1:3], sumsq, count)
                assert_bit_equal(got[0], rec, f"{case.name} {how}: records")
                assert_bit_equal(got[3], err, f"{case.name} {how}: error map")
    print(f"{family}: {kernels[True]} runs on the aligned kernel, {kernels[False]} on the ragged one")
    assert kernels[True] > 0 and kernels[False] > kernels[True]


# ---- rgbStep on the records --------------------------------------------------------------------------------------------------------
def pack27(A, b):
    got = np.zeros(27, np.float32)
    for k, (i, j) in enumerate(pe.SE3_PAIRS):
        got[k] = b[i] if j == 6 else A[i, j]
    return got


@pytest.mark.parametrize("family", pe.FAMILIES)
def test_rgb_step_on_the_cases_records(gpu_ctx, orc, family):
    """rgbStep on the oracle's records of every case for sigma = count, 1, -1, 0, FLT_EPSILON and the float after it (the
    weight's three branches, sigma + |diff| == FLT_EPSILON and 0 + 0 included), within helpers.se3_sum_tolerance"""
    from multimotionfusion_amd import cudafuncs as cf
    weights = set()
    for case in BY_FAMILY[family]:
        rows, cols = case.next_image.shape
        rec, _, count, _ = pe.oracle_result(orc, case.name)
        cloud, (dIdx, dIdy) = pe.plain_cloud(cols, rows), pe.plain_gradients(cols, rows)
        d_rec, d_cloud, d_dx, d_dy = dev(rec), dev(cloud), dev(dIdx), dev(dIdy)
        diffs = np.abs(rec.view(pe.RECORD)[..., 0]["diff"][rec.view(pe.RECORD)[..., 0]["valid"] == 1])
        for sigma in pe.step_sigmas(count):
            A, b = cf.rgbStep(gpu_ctx, d_rec, float(sigma), d_cloud, 50.0, 48.0, d_dx, d_dy, 0.125)
            out = orc.rgb_step(rec, float(sigma), cloud, 50.0, 48.0, dIdx, dIdy, 0.125)
            tol = se3_sum_tolerance(out)
            d = np.abs(pack27(A, b).astype(np.float64) - out[:27])
            assert np.isfinite(out).all() and (d <= tol[:27]).all(), (case.name, sigma, (d / tol[:27]).max())
            assert np.array_equal(A, A.T)
            if len(diffs):
                w = np.float32(sigma) + diffs
                weights |= {"eq" if (w == pe.FLT_EPSILON).any() else "", "zero" if (w == 0).any() else "", "minus" if sigma == -1 else ""}
    if family == "last":
        assert {"eq", "zero", "minus"} <= weights  # sigma + |diff| == FLT_EPSILON, sigma == 0 with diff == 0, sigma == -1


def test_rgb_step_exact_sums_bit_for_bit(gpu_ctx, orc):
    """Rows of small dyadic rationals (photo_edges.step_exact_case: the builder asserts that every float32 sum is exact in any
    order): the device equals the oracle bit for bit, at 1, 3, 4, 255, 256, 257 and 1025 records (one pixel per lane where the
    number is no multiple of four, four otherwise), with records at the first and last index only, everywhere, and nowhere; a
    point with Z == 0 under a record makes the same entries non-finite on both sides."""
    from multimotionfusion_amd import cudafuncs as cf
    seen = set()
    for case in pe.step_exact_cases():
        rows, cols = case.dIdx.shape
        A, b = cf.rgbStep(gpu_ctx, dev(case.corres), float(case.sigma), dev(case.cloud), float(case.fx), float(case.fy), dev(case.dIdx), dev(case.dIdy),
                          float(case.sobel_scale))
        out = orc.rgb_step(case.corres, float(case.sigma), case.cloud, float(case.fx), float(case.fy), case.dIdx, case.dIdy, float(case.sobel_scale))
        got = pack27(A, b)
        kind = case.claim["kind"]
        seen.add((kind, (cols * rows) % 4 == 0))
        if kind == "z0":
            with np.errstate(all="ignore"):
                assert_bit_equal(np.isfinite(got), np.isfinite(out[:27].astype(np.float32)), case.name + ": finite entries")
            assert not np.isfinite(got).all()
            continue
        assert_bit_equal(got, out[:27].astype(np.float32), case.name)
        if kind == "none":
            assert not A.any() and not b.any()
        else:
            assert A.any()
    assert {("ends", True), ("ends", False), ("dense", True), ("dense", False), ("none", True), ("none", False)} <= seen


# ---- so3Step -------------------------------------------------------------------------------------------------------------------------
def test_so3_step_at_its_warp_and_border_edges(gpu_ctx, orc):
    """3 x 3, 4 x 3, 5 x 8 and 20 x 12; the image basis puts warped.x / warped.z on a tie, the warp on 0, 1, cols - 2, cols - 1
    (rows likewise) and warped.z on 0 for a row; images of 0 / 255 steps.  `found` is exact everywhere, the exact cases (sums
    exact in float32, asserted by their builder) bit for bit, the others within the bound of test_so3_step_parity."""
    from multimotionfusion_amd import cudafuncs as cf
    ii = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
    for case in pe.so3_cases():
        A, b, res = cf.so3Step(gpu_ctx, dev(case.last_image), dev(case.next_image), case.B, case.kinv, case.krlr)
        out = orc.so3_step(case.last_image, case.next_image, case.B, case.kinv, case.krlr)
        got = np.array([A[0, 0], A[0, 1], A[0, 2], b[0], A[1, 1], A[1, 2], b[1], A[2, 2], b[2], res[0]], np.float32)
        assert res[1] == out[10], (case.name, res[1], out[10])
        if "found" in case.claim:
            assert res[1] == case.claim["found"], case.name
        if case.claim.get("exact"):
            assert_bit_equal(got, out[:10].astype(np.float32), case.name)
            continue
        assert np.isfinite(out).all(), case.name
        diag = np.array([out[0], out[4], out[7], out[9]])
        tol = np.array([2e-5 * np.sqrt(diag[i] * diag[j]) + 1e-9 for i, j in ii])
        d = np.abs(got.astype(np.float64) - out[:10])
        assert (d <= tol).all(), (case.name, d / tol)


# ---- the one-launch chain, every number of pixels per lane --------------------------------------------------------------------------
class forced_px:
    """`with forced_px(lib, px):` level 0 of the one-launch chain takes px pixels per lane; cleared afterwards"""

    def __init__(self, lib, px):
        self.lib, self.px = lib, px

    def __enter__(self):
        assert self.lib.mmf_debug_set_gn_px(self.px, 0, 0) == 0

    def __exit__(self, *exc):
        assert self.lib.mmf_debug_set_gn_px(-1, -1, -1) == 0
        return False


def one_launch_against_the_oracle(gpu_ctx, orc, case, launches):
    """the truncated chain's last launch against the oracle's pass at that launch's own pose"""
    g = product(gpu_ctx, case)
    try:
        got = truncated(gpu_ctx, g, case, launches, 0)
    finally:
        g.close()
    start = gr.start_pose24(case)
    assert_bit_equal(got["pose"][:12], start[:12], f"{case.name}: the pose stays the model's")
    assert np.abs(got["pose"][12:] - start[12:]).max() <= 1e-6  # K 1 K^-1, K 0
    assert_bit_equal(got["t"], case.model[:3, 3], case.name)
    assert_bit_equal(got["R"], case.model[:3, :3], case.name)
    o = gr.oracle_odometry(orc, case)
    ref = gr.oracle_pass(orc, o, case, 0, got["pose"])
    o.close()
    assert (ref["count"], ref["sumsq"]) == (case.claim["count"], 0), (case.name, ref["count"], ref["sumsq"])
    assert (got["count"], got["sumsq"]) == (ref["count"], ref["sumsq"]), (case.name, launches, got["count"], ref["count"], got["sumsq"])
    for term, sl in (("icp", slice(0, 29)), ("rgb", slice(29, 58))):
        tol = se3_sum_tolerance(ref[term])
        d = np.abs(got["tot"][sl] - ref[term])
        assert (d <= tol).all(), (case.name, term, np.argwhere(d > tol).ravel().tolist(), d[d > tol], tol[d > tol])
    return got


@pytest.mark.parametrize("px", [1, 2, 4, 5])
def test_one_launch_chain_with_forced_pixels_per_lane(gpu_ctx, orc, px):
    """The 40 x 32 static cases under mmf_debug_set_gn_px(px, 0, 0): the count and the sum of diff^2 of one launch, and of the
    second of two, are the oracle's exactly (and what the case claims from its geometry); the pose does not move."""
    cases = [c for c in pe.static_cases(orc) if (c.w, c.h) == pe.FORCED_PX_SIZE]
    assert len(cases) == 5 and pe.FORCED_PX_SIZE[0] % 20 == 0
    with forced_px(gpu_ctx.lib, px):
        for case in cases:
            for launches in (1, 2):
                got = one_launch_against_the_oracle(gpu_ctx, orc, case, launches)
            print(f"px {px} {case.name}: count {got['count']} of {case.claim['clean']} without the features")


def test_the_forced_pixels_per_lane_reach_the_launch_geometry(gpu_ctx, orc):
    """The hook is consulted: five pixels per lane cannot be had at a width of 32 (a lane's pixels lie in one row), so the
    geometry refuses, and a truncated chain -- which takes nothing but the one-launch chain -- says so before it launches
    anything.  Cleared, the same call runs."""
    case = next(c for c in pe.static_cases(orc) if c.name == "static_clean_32x32")
    lib = gpu_ctx.lib
    g = product(gpu_ctx, case)
    try:
        with forced_px(lib, 5):
            assert lib.mmf_debug_gn_truncate(1, 0) == 0
            with pytest.raises(RuntimeError, match="one-launch chain"):
                g.getIncrementalTransformation(case.model[:3, 3], case.model[:3, :3], False, gr.ICP_WEIGHT, False, False, False)
            lib.mmf_debug_gn_truncate(0, 0)
        got = truncated(gpu_ctx, g, case, 1, 0)
        assert got["count"] == case.claim["count"]
    finally:
        lib.mmf_debug_gn_truncate(0, 0)
        lib.mmf_debug_set_gn_px(-1, -1, -1)
        g.close()


@pytest.mark.parametrize("px", [2, 4, 5])
def test_one_launch_chain_at_the_size_that_picks_each_pixels_per_lane(gpu_ctx, orc, px):
    """Nothing forced: the smallest sizes at which the launch geometry itself goes from 1 to 2, from 2 to 4 and from 4 to 5
    pixels per lane (just above 65 536, 131 072 and 262 144 pixels), the window lattice tiled over the image.  The library does
    not expose the number it chose; photo_edges.geometry_px restates the choice, and the forced runs above show each number alone."""
    case = pe.natural_case(orc, px)
    assert pe.geometry_px(case.w, case.h) == px and gpu_ctx.lib.mmf_debug_set_gn_px(-1, -1, -1) == 0
    got = one_launch_against_the_oracle(gpu_ctx, orc, case, 1)
    print(f"{case.name}: count {got['count']} of {case.claim['clean']}")


# ---- both chains through the whole pyramid ---------------------------------------------------------------------------------------------
_chains = {}


def oracle_chain(orc, case, mode):
    if (case.name, mode) not in _chains:
        _chains[(case.name, mode)] = pe.oracle_chain(orc, case, mode)
    return _chains[(case.name, mode)]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("mode", ["default", "rgb_only"])
def test_both_chains_keep_the_static_cases_at_the_identity(gpu_ctx, orc, mode, fused):
    """getIncrementalTransformation on the static cases, 32 x 32 (level 2: 8 x 8, whole groups of four) and 40 x 32 (level 2:
    10 x 8, ragged), as one launch per iteration where that chain applies and as two: the pose bit-equal to the start,
    iterations_run, lastRGBCount and lastRGBError the oracle's, the photometric error image written (it starts as -1) and zero.
    The two-launch chain's compact records and their decoding are what this holds at both level-2 widths."""
    lib = gpu_ctx.lib
    rec0, _ = status(lib)
    ran = {True: 0, False: 0}
    try:
        assert lib.mmf_debug_set_gn_fused(fused) == 0
        for case in pe.static_cases(orc):
            if mode not in case.modes:
                continue
            t_o, R_o, st, err_o = oracle_chain(orc, case, mode)
            g = product(gpu_ctx, case)
            g.enableTiming(2)  # counts the launches of either chain (and computes the bits of the untimed run: test_gpu_odometry.py)
            icp_err, rgb_err = torch.full((case.h, case.w), -1.0, device="cuda"), torch.full((case.h, case.w), -1.0, device="cuda")
            t, R = g.getIncrementalTransformation(case.model[:3, 3], case.model[:3, :3], icpErrorSurface=icp_err, rgbErrorSurface=rgb_err, **pe.MODES[mode])
            what = f"{case.name} {mode} fused={fused}"
            assert_bit_equal(t, case.model[:3, 3], what + ": translation")
            assert_bit_equal(R, case.model[:3, :3], what + ": rotation")
            assert_bit_equal(t, t_o, what + ": the oracle's translation")
            assert_bit_equal(R, R_o, what + ": the oracle's rotation")
            assert (g.iterations_run, g.so3_iterations_run) == (st.iterations_run, st.so3_iterations_run) == pe.MODE_ITERATIONS[mode], what
            assert g.lastRGBCount == st.lastRGBCount == case.claim["count"], (what, g.lastRGBCount, st.lastRGBCount)
            assert_bit_equal(np.float32(g.lastRGBError), np.float32(st.lastRGBError), what + ": lastRGBError")
            assert_bit_equal(rgb_err.cpu().numpy(), err_o, what + ": photometric error image")
            assert not err_o.any()
            # which chain it was: one launch per iteration needs both terms and whole groups of four columns at every level
            one_launch = bool(fused) and mode == "default" and (case.w >> 2) % 4 == 0
            steps = [g.getTiming()[f"rgb_step_l{k}"]["launches"] for k in range(3)]
            assert steps == ([0, 0, 0] if one_launch else [10, 5, 4]), (what, steps)
            ran[one_launch] += 1
            g.close()
        assert ran[False] > 0 and (ran[True] > 0) == (bool(fused) and mode == "default"), ran
        assert status(lib) == (rec0, 1)  # no chain gave up
    finally:
        lib.mmf_debug_set_gn_fused(-1)
