"""CPU: what tests/test_gpu_gn_range.py takes for granted about its inputs, checked on the oracle alone -- the regimes reach
the number ranges they are named for, and the float64 restatement the solver test compares with is the oracle's algebra."""
import numpy as np

import gn_range as gr


def test_r4_sum_of_squares_is_negative_as_an_int(orc):
    r = gr.regime("R4")
    o = gr.oracle_odometry(orc, r)
    p = gr.oracle_pass(orc, o, r, 0, gr.start_pose24(r))
    o.close()
    print("R4 level 0: count", p["count"], "sum diff^2 as int", p["sumsq"])
    assert p["sumsq"] < 0 and p["count"] > 100000


def test_r5_count_window_and_r6_r7_branches(orc):
    for name, lo, hi in (("R5", 10, 1000), ("R6", 1000, 10 ** 6), ("R7", 0, 0)):
        r = gr.regime(name)
        o = gr.oracle_odometry(orc, r)
        p = gr.oracle_pass(orc, o, r, 0, gr.start_pose24(r))
        o.close()
        print(name, "level 0: count", p["count"], "sum diff^2", p["sumsq"])
        assert lo <= p["count"] <= hi, (name, p["count"])
        if name == "R5":
            assert p["sumsq"] / p["count"] > 100 ** 2  # |d| beyond 100 on average
        if name == "R6":
            assert p["sumsq"] == 0


def test_out_of_range_scale_exceeds_the_icp_limit(orc):
    """(d): identical frames scaled until one workgroup's ICP partial, by the oracle's own rows, is beyond 2^23 -- and the
    scene of R3 / R3h / R8b, which must stay on the one-launch chain, far inside it."""
    scale, largest, inliers = gr.out_of_range_scale(orc)
    print("scale", scale, ": largest 256-pixel partial", largest, "limit", gr.GN_ICP_PARTIAL_LIMIT, "level-0 inliers", inliers)
    assert largest > gr.GN_ICP_PARTIAL_LIMIT and inliers > 5000
    for name in ("R3", "R8b"):
        r = gr.regime(name)
        o = gr.oracle_odometry(orc, r)
        big, _ = gr.icp_group_partials(orc, o, r)
        o.close()
        print(name, "largest partial", big.max())
        assert big.max() < gr.GN_ICP_PARTIAL_LIMIT / 16, name


def test_float64_restatement_is_the_oracles_algebra(orc):
    """One iteration of the oracle on R1 (no SO3, so the running transform starts as the identity): its pose from its own
    lastA / lastb through the restatement."""
    r = gr.regime("R1")
    mode = dict(rgbOnly=False, icpWeight=gr.ICP_WEIGHT, pyramid=True, fastOdom=False, so3=False)
    o = gr.oracle_odometry(orc, r)
    with gr.max_gn_iters(1):
        t, R = o.getIncrementalTransformation(r.model[:3, 3], r.model[:3, :3], **mode)
    st = o.stats()
    o.close()
    assert st.iterations_run == 1
    N = gr.running_transform64(np.array(st.lastA), np.array(st.lastb), np.eye(4))
    pose, _ = gr.pose_from_transform(N, r.model[:3, :3], r.model[:3, 3], gr.level_intrinsics(r.K, 2))
    assert np.abs(pose[:9].reshape(3, 3) - R).max() <= 2 * np.spacing(np.float32(1)) and np.abs(pose[9:12] - t).max() <= 2 * np.spacing(np.float32(1))
    assert np.linalg.norm(t - r.model[:3, 3]) > 1e-4  # the step moved


def test_solver_batch_covers_its_cases():
    sys = gr.solver_systems()
    kinds = {s["kind"] for s in sys}
    assert 150 <= len(sys) <= 256 and {"spd", "y=1/64", "y<1/64", "y>1/64", "tiny", "pi", "rank3", "zero", "nan-b"} <= kinds
    y = {k: [float(np.sum(gr.solve64(s["A"], s["b"])[3:] ** 2)) for s in sys if s["kind"] == k] for k in ("y=1/64", "y<1/64", "y>1/64")}
    assert all(v == 0.015625 for v in y["y=1/64"]) and all(0.0156 < v < 0.015625 for v in y["y<1/64"]) and all(0.015625 < v < 0.01563 for v in y["y>1/64"])
    conds = [np.linalg.cond(s["A"]) for s in sys if s["kind"] == "spd"]
    assert min(conds) < 1e3 and max(conds) > 1e11
    for s in sys:
        if s["kind"] in ("rank3", "zero", "nan-b"):
            assert np.isnan(gr.running_transform64(s["A"], s["b"], s["rt"])).all(), s["kind"]
