"""-m gpu: the one-launch Gauss-Newton chain (csrc/gn_fused.hpp) at the edges of its number ranges.

The tracking tests elsewhere all run the synthetic room as rendered (1.3 - 3 m, matching exposure, dense texture, a camera
near the origin).  Here the same pair is taken, by array arithmetic (tests/gn_range.py), to where the chain's fixed-point
sums, its packed counter word and its wave-parallel solver could be wrong without those tests noticing:

  R1 as rendered (R1r: 176 x 144, ragged rows)   R2 near (x 0.15)         R3 far (x 4)
  R4 an exposure step that takes sum diff^2 past 2^31 (640 x 480)         R5 one textured patch + an exposure step
  R6 identical frames (sum diff^2 = 0, sigma = 1)  R7 black images (0 / 0)  R8a / R8b the poses at +10 m / +50 m

(a) the 58 sums and the counter of ONE launch against the oracle at the same pose, (b) the pose after exactly one iteration,
(c) the whole chain, (d) an ICP term that really leaves the fixed-point range (the give-up path with real input), (e) the
solver alone against float64.  (a), (b) use the truncated chain of mmf_debug_gn_truncate, (e) mmf_debug_gn_solve.

Every case asserts that the one-launch chain ran and that no recovery happened, unless the recovery is its subject: the
truncated chain refuses any other chain, the whole chains are run under the timing mode that counts each kind of launch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gn_range as gr
from helpers import assert_bit_equal, se3_sum_tolerance
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu

FULL = dict(rgbOnly=False, icpWeight=gr.ICP_WEIGHT, pyramid=True, fastOdom=False, so3=True)  # the GUI defaults: 19 iterations
POSE_BAR_T, POSE_BAR_R = 1e-4, 1e-3  # BASELINE.json north_star: 1e-4 relative translation, 1e-3 rad


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def status(lib):
    rec, use = C.c_int(0), C.c_int(0)
    assert lib.mmf_gn_chain_status(C.byref(rec), C.byref(use)) == 0
    return rec.value, use.value


class undisturbed:
    """The one-launch chain is in use before and after, and no chain gave up in between."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.mmf_debug_set_gn_fused(-1) == 0
        self.rec, use = status(self.lib)
        assert use == 1

    def __exit__(self, et, ev, tb):
        if et is None:
            rec, use = status(self.lib)
            assert use == 1 and rec == self.rec, ("a chain gave up and the frame was tracked on the two-launch chain", rec - self.rec, use)
        return False


def product(gpu_ctx, r, model=None):
    from multimotionfusion_amd.odometry import RGBDOdometry
    K = r.K
    return gr.setup(RGBDOdometry(gpu_ctx, r.w, r.h, K["cx"], K["cy"], K["fx"], K["fy"]), dev, r, model)


def truncated(gpu_ctx, g, r, n, level, so3=False):
    """n launches of the one-launch chain at `level` from the model's pose: what mmf_debug_gn_truncated gives, and the call's pose."""
    lib = gpu_ctx.lib
    with undisturbed(lib):
        assert lib.mmf_debug_gn_truncate(n, level) == 0
        try:
            t, R = g.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], False, gr.ICP_WEIGHT, level > 0, False, so3)
        finally:
            lib.mmf_debug_gn_truncate(0, 0)
        tot, cnt, rt, pose = np.zeros(58), np.zeros(2, np.uint32), np.zeros(12), np.zeros(24, np.float32)
        assert lib.mmf_debug_gn_truncated(g.handle, *(C.c_void_p(a.ctypes.data) for a in (tot, cnt, rt, pose))) == 0
    assert g.iterations_run == n - 1
    return dict(tot=tot, count=int(cnt[0]), sumsq=int(cnt[1]), rt=rt.reshape(3, 4), pose=pose, t=t, R=R)


_oracles = {}


def oracle_start(orc, r, level):
    """The oracle's pass at the pose the chain starts from (shared by (a) and (b); nothing changes it)."""
    key = (r.name, level)
    if key not in _oracles:
        o = gr.oracle_odometry(orc, r)
        _oracles[key] = gr.oracle_pass(orc, o, r, level, gr.start_pose24(r))
        o.close()
    return _oracles[key]


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 0])
@pytest.mark.parametrize("name", gr.REGIMES)
def test_sums_of_one_launch_match_the_oracle(gpu_ctx, orc, name, level):
    """The first launch's 29 ICP and 29 photometric totals, read back through the fixed-point sums exactly as the second launch
    would decode them, against icpStep / computeRgbResidual + rgbStep of the oracle at the same pose: helpers.se3_sum_tolerance
    (2e-5 sqrt(S_ii S_jj), the bound of a float32 grid sum) for every sum in every regime -- the quantum of the photometric
    scale 2^(4 + 2 floor(log2 sigma)) has to stay below it also where the rows are (sigma / (sigma + |d|))^2 smaller than the
    scale assumes (R4, R5) -- and the counter word exactly: the count, and sum diff^2 as the reference's int (mod 2^32)."""
    r = gr.regime(name)
    g = product(gpu_ctx, r)
    got = truncated(gpu_ctx, g, r, 1, level)
    g.close()
    start = gr.start_pose24(r)
    assert_bit_equal(got["pose"][:12], start[:12], "the first launch's pose is the model's")
    assert np.abs(got["pose"][12:] - start[12:]).max() <= 1e-6  # K 1 K^-1, K 0 (the oracle's pass below takes the launch's own)
    assert_bit_equal(got["rt"], np.eye(4)[:3], "the running transform starts as the identity")
    o = gr.oracle_odometry(orc, r)
    ref = gr.oracle_pass(orc, o, r, level, got["pose"])
    o.close()
    ideal = oracle_start(orc, r, level)
    assert (ref["count"], ref["sumsq"]) == (ideal["count"], ideal["sumsq"])
    worst = {}
    for term, sl in (("icp", slice(0, 29)), ("rgb", slice(29, 58))):
        tol = se3_sum_tolerance(ref[term])
        d = np.abs(got["tot"][sl] - ref[term])
        worst[term] = float(np.max(d / np.where(tol > 0, tol, 1.0)))
    print(f"{name} level {level}: count {got['count']} (oracle {ref['count']}), sum diff^2 {got['sumsq']} (oracle {ref['sumsq']}), "
          f"largest |sum - oracle| / tolerance: icp {worst['icp']:.3g} rgb {worst['rgb']:.3g}")
    assert got["count"] == ref["count"]
    assert got["sumsq"] == ref["sumsq"] % (1 << 32)
    if name == "R4" and level == 0:
        assert ref["sumsq"] < 0
    for term, sl in (("icp", slice(0, 29)), ("rgb", slice(29, 58))):
        tol = se3_sum_tolerance(ref[term])
        d = np.abs(got["tot"][sl] - ref[term])
        assert (d <= tol).all(), (term, np.argwhere(d > tol).ravel().tolist(), d[d > tol], tol[d > tol])


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 0])
@pytest.mark.parametrize("name", gr.REGIMES)
def test_one_iteration_matches_the_oracle(gpu_ctx, orc, name, level):
    """Two launches: the pose after exactly one solve, against the oracle stopped after one iteration.  The bound is worked out
    from the oracle's own sums (gn_range.one_iteration_bound): |A^-1| (|db| + |dA| |x|) with the sums' float32 tolerances,
    plus 4 float32 ulps of the pose entries.  The launch's own K R K^-1 and K t (what its pixel waves would have read) and
    Rcurr, tcurr are held against the restatement's pose of the running transform the solve left, as in (e), and that
    transform against the float64 solve of the oracle's system within the same bound."""
    r = gr.regime(name)
    g = product(gpu_ctx, r)
    got = truncated(gpu_ctx, g, r, 2, level)
    g.close()
    o = gr.oracle_odometry(orc, r)
    with gr.max_gn_iters(1):
        to, Ro = o.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], False, gr.ICP_WEIGHT, level > 0, False, False)
    st = o.stats()
    assert st.iterations_run == 1
    o.close()
    bound = gr.one_iteration_bound(oracle_start(orc, r, level), np.concatenate([to, Ro.ravel()]))
    fin_o, fin_g = np.isfinite(to).all() and np.isfinite(Ro).all(), np.isfinite(got["t"]).all() and np.isfinite(got["R"]).all()
    diff = max(float(np.abs(got["t"] - to).max()), float(np.abs(got["R"] - Ro).max())) if fin_o and fin_g else float("nan")
    print(f"{name} level {level}: bound {bound:.3g}, |pose - oracle| {diff:.3g}, step {np.linalg.norm(to - r.model[:3, 3]):.3g} m")
    assert fin_o == fin_g, (got["t"], to)
    ref_pose, floor = gr.pose_from_transform(got["rt"], r.model[:3, :3], r.model[:3, 3], gr.level_intrinsics(r.K, level))
    assert_bit_equal(np.isfinite(got["pose"]), np.isfinite(ref_pose), "finite entries of the launch's pose")
    if fin_o:
        assert diff <= bound, (diff, bound)
        N = gr.running_transform64(np.array(st.lastA), np.array(st.lastb), np.eye(4))
        assert np.abs(got["rt"] - N).max() <= bound, (np.abs(got["rt"] - N).max(), bound)
        d = np.abs(got["pose"].astype(np.float64) - ref_pose.astype(np.float64))
        ptol = 2 * np.spacing(np.abs(ref_pose).astype(np.float32)).astype(np.float64) + np.concatenate([np.zeros(12), np.full(12, floor)])
        assert (d <= ptol).all(), (np.argwhere(d > ptol).ravel().tolist(), d[d > ptol], ptol[d > ptol])


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gr.REGIMES)
def test_whole_chain_matches_the_oracle(gpu_ctx, orc, name):
    """19 iterations with the SO3 pre-alignment in every regime: the iterations run, the counts (within the 2 that threshold
    ties move after 18 float steps), the pose within north_star's bar (R1: the 2e-6 of test_gpu_odometry.py), and
    lastRGBError not a number exactly where the oracle's is (R4: sqrt of a negative int)."""
    r = gr.regime(name)
    lib = gpu_ctx.lib
    g = product(gpu_ctx, r)
    g.enableTiming(2)  # counts the launches of either chain (and computes the bits of the untimed run: test_gpu_odometry.py)
    with undisturbed(lib):
        tg, Rg = g.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], **FULL)
        tm = g.getTiming()
    assert [tm[f"producer_l{k}"]["launches"] for k in range(3)] == [10, 5, 4] and [tm[f"rgb_step_l{k}"]["launches"] for k in range(3)] == [0, 0, 0]
    o = gr.oracle_odometry(orc, r)
    to, Ro = o.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], **FULL)
    so = o.stats()
    o.close()
    dt, dR = float(np.linalg.norm(tg - to)), float(np.abs(Rg - Ro).max())
    print(f"{name}: |dt| {dt:.3g} |dR| {dR:.3g} counts rgb {g.lastRGBCount}/{so.lastRGBCount} icp {g.lastICPCount}/{so.lastICPCount} "
          f"lastRGBError {g.lastRGBError}/{so.lastRGBError}")
    assert g.iterations_run == so.iterations_run == 19 and g.so3_iterations_run == so.so3_iterations_run
    assert abs(g.lastRGBCount - so.lastRGBCount) <= 2 and abs(g.lastICPCount - so.lastICPCount) <= 2
    assert np.isnan(g.lastRGBError) == np.isnan(so.lastRGBError)
    if name == "R4":
        assert np.isnan(so.lastRGBError)
    assert np.isfinite(to).all() == np.isfinite(tg).all()
    if np.isfinite(to).all():
        bar_t, bar_r = (2e-6, 2e-6) if name == "R1" else (POSE_BAR_T * max(1.0, float(np.linalg.norm(to))), POSE_BAR_R)
        assert dt <= bar_t and dR <= bar_r, (dt, dR)
    g.close()


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_icp_term_gives_up_and_recovers(gpu_ctx, orc):
    """Identical frames scaled (depth, vertices, pose translation) until, by the oracle's own rows, one workgroup's ICP partial
    is beyond 2^23 -- a term >= 2^53 at the sums' scale 2^30 (gn_range.out_of_range_scale; a translation of the poses would not
    do: the rows hold v x n with v in the model's camera frame).  Levels 1 and 2 have no inlier at that depth, so level 0 alone
    (pyramid off).  The launch reports it (give-up value 2), the same call tracks the frame on the two-launch chain and
    returns that chain's bits, one recovery is counted and the process stops using the one-launch chain, as after any give-up
    (the next frames of such a scene would give up too): the following frame runs on the two-launch chain, and on the
    one-launch chain again once mmf_debug_set_gn_fused asks for it.  Nothing faults here: a status word written by kernels
    that complete."""
    lib = gpu_ctx.lib
    scale, largest, inliers = gr.out_of_range_scale(orc)
    assert largest > gr.GN_ICP_PARTIAL_LIMIT
    print(f"scale {scale}: largest 256-pixel partial {largest:.4g} (limit {gr.GN_ICP_PARTIAL_LIMIT:.4g}), {inliers} inliers at level 0")
    r = gr.scaled_identical(scale)
    mode = dict(FULL, pyramid=False)

    def run():
        g = product(gpu_ctx, r)
        t, R = g.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], **mode)
        return g, dict(t=t, R=R, iters=np.int32(g.iterations_run), icp=np.float32(g.lastICPCount), rgb=np.float32(g.lastRGBCount),
                       A=g.lastA.copy(), b=g.lastb.copy(), rgb_error=np.float32(g.lastRGBError), icp_error=np.float32(g.lastICPError))

    def launches(tm):
        return [tm[f"producer_l{k}"]["launches"] for k in range(3)], [tm[f"rgb_step_l{k}"]["launches"] for k in range(3)]

    r1 = gr.regime("R1")
    try:
        assert lib.mmf_debug_set_gn_fused(0) == 0
        rec0, _ = status(lib)
        g2, two = run()
        g2.close()
        assert status(lib)[0] == rec0
        assert lib.mmf_debug_set_gn_fused(-1) == 0  # the default; also asks for the one-launch chain again if something latched it off
        assert status(lib) == (rec0, 1)
        g, one = run()  # no hook is touched from here to the status checks
        assert status(lib) == (rec0 + 1, 0), "exactly one recovery, and the process stops using the one-launch chain"
        for k in two:
            assert_bit_equal(np.asarray(one[k]), np.asarray(two[k]), f"recovered call: {k}")
        assert one["iters"] == 10 and np.isfinite(one["t"]).all()
        # the following frame on the same odometry (R1 as rendered): on the two-launch chain while the latch holds ...
        gr.setup(g, dev, r1)
        g.enableTiming(2)
        t_two, R_two = g.getIncrementalTransformation(r1.model[:3, 3], r1.model[:3, :3], **FULL)
        assert launches(g.getTiming()) == ([10, 5, 4], [10, 5, 4]) and status(lib) == (rec0 + 1, 0)
        g.close()
        # ... and on the one-launch chain again once it is asked for
        g = product(gpu_ctx, r1)
        g.enableTiming(2)
        with undisturbed(lib):
            t, R = g.getIncrementalTransformation(r1.model[:3, 3], r1.model[:3, :3], **FULL)
            assert launches(g.getTiming()) == ([10, 5, 4], [0, 0, 0])
        assert g.iterations_run == 19 and np.isfinite(t).all()
        assert np.linalg.norm(t - t_two) <= 1e-6 and np.abs(R - R_two).max() <= 1e-6  # (test_one_launch_chain_equals_two_launch_chain's bound)
        g.close()
    finally:
        lib.mmf_debug_set_gn_fused(-1)


def test_truncated_chain_leaves_the_next_call_alone(gpu_ctx):
    """After a truncated chain (with the SO3 pre-alignment, so the image ring moves too) an ordinary call on the same odometry
    gives the bits a fresh odometry gives."""
    r = gr.regime("R1")

    def ordinary(g):
        t, R = g.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], **FULL)
        return dict(t=t, R=R, iters=np.int32(g.iterations_run), so3=np.int32(g.so3_iterations_run), icp=np.float32(g.lastICPCount),
                    rgb=np.float32(g.lastRGBCount), A=g.lastA.copy(), b=g.lastb.copy(), rgb_error=np.float32(g.lastRGBError))

    g = product(gpu_ctx, r)
    fresh = ordinary(g)
    g.close()
    g = product(gpu_ctx, r)
    for n, level in ((2, 2), (1, 0), (3, 0)):
        got = truncated(gpu_ctx, g, r, n, level, so3=True)
        assert np.isfinite(got["tot"]).all()
        gr.setup(g, dev, r)
    with undisturbed(gpu_ctx.lib):
        after = ordinary(g)
    g.close()
    for k in fresh:
        assert_bit_equal(np.asarray(after[k]), np.asarray(fresh[k]), f"after truncated chains: {k}")


# ---- (e) ----------------------------------------------------------------------------------------------------------------
def test_solver_wave_against_float64(gpu_ctx):
    """gn_solve_rows -- the 6x6 LDL^T with reciprocal pivots, the Rodrigues update with its series below |r|^2 = 1/64, the
    row-per-lane pose update -- on some 200 systems in one launch, against np.linalg.solve and the oracle's algebra in float64
    (gn_range.running_transform64 / pose_from_transform).  Running transform: 1e-12 cond(A), at most 1, for each of the
    three rows a lane of its own writes.  The 24 pose floats: 2 float32 ulps against the
    restatement's pose of the kernel's own transform (plus what float64 leaves in entries that are differences of larger
    terms), which keeps the ill-conditioned systems in the check.  Non-finite systems: non-finite in the same outputs."""
    lib = gpu_ctx.lib
    systems = gr.solver_systems()
    n = len(systems)
    intr = gr.level_intrinsics(synth.intrinsics(160, 120), 0)
    sys_h = np.stack([np.concatenate([s["A"].ravel(), s["b"]]) for s in systems])
    rt_h = np.stack([s["rt"].ravel() for s in systems])
    prev_h = np.stack([np.concatenate([s["Rprev"].ravel(), s["tprev"]]) for s in systems]).astype(np.float32)
    sys_d, rt_d, prev_d = dev(sys_h), dev(rt_h), dev(prev_h)
    rt_out = torch.full((n, 12), 7.0, dtype=torch.float64, device="cuda")
    pose_out = torch.full((n, 24), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert lib.mmf_debug_gn_solve(gpu_ctx.handle, *(C.c_void_p(t.data_ptr()) for t in (sys_d, rt_d, prev_d)), *(float(v) for v in intr), n,
                                  C.c_void_p(rt_out.data_ptr()), C.c_void_p(pose_out.data_ptr())) == 0
    torch.cuda.synchronize()
    N_k, pose_k = rt_out.cpu().numpy().reshape(n, 3, 4), pose_out.cpu().numpy()
    worst_rt, worst_pose, nonfinite = 0.0, 0.0, 0
    for i, s in enumerate(systems):
        N = gr.running_transform64(s["A"], s["b"], s["rt"])
        what = (i, s["kind"])
        assert_bit_equal(np.isfinite(N_k[i]), np.isfinite(N), f"{what}: finite entries of the running transform")
        ref_pose, floor = gr.pose_from_transform(N_k[i], s["Rprev"], s["tprev"], intr)
        assert_bit_equal(np.isfinite(pose_k[i]), np.isfinite(ref_pose), f"{what}: finite entries of the pose")
        if not np.isfinite(N).all():
            nonfinite += 1
            continue
        tol = min(1.0, 1e-12 * np.linalg.cond(s["A"]))
        for row in range(3):
            d = float(np.abs(N_k[i][row] - N[row]).max())
            worst_rt = max(worst_rt, d / tol)
            assert d <= tol, (what, "row", row, d, tol)
        ulp = np.spacing(np.abs(ref_pose).astype(np.float32)).astype(np.float64)
        d = np.abs(pose_k[i].astype(np.float64) - ref_pose.astype(np.float64))
        ptol = 2 * ulp + np.concatenate([np.zeros(12), np.full(12, floor)])
        worst_pose = max(worst_pose, float(np.max(d / ptol)))
        assert (d <= ptol).all(), (what, np.argwhere(d > ptol).ravel().tolist(), d[d > ptol], ptol[d > ptol])
    print(f"{n} systems ({nonfinite} non-finite): largest |transform - float64| / bound {worst_rt:.3g}, largest |pose - float64| / bound {worst_pose:.3g}")
    assert nonfinite >= 5
