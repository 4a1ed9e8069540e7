"""CPU: the orchestration oracle (oracle/fusion.py) and the host pose algebra it rests on (oracle/mmf_oracle_pose.c):
JacobiSVD / rodrigues2 / computeFusionWeight known answers, the multi-model bookkeeping, and the measured
sensitivity of object tracking to one-ulp input noise that the GPU parity tolerances are derived from."""
import numpy as np

from multimotionfusion_amd import synth
from oracle import oracle as orc
from oracle.fusion import OracleFusion


def test_jacobi_svd_reconstructs_and_orders():
    rng = np.random.default_rng(0)
    for k in range(600):
        a = rng.normal(size=(3, 3)).astype(np.float32)
        if k % 3 == 0:  # nearly a rotation: what rodrigues2 is given
            a = (synth.rodrigues(rng.normal(size=3) * 10 ** rng.uniform(-6, 0)) + rng.normal(size=(3, 3)) * 1e-7).astype(np.float32)
        if k % 50 == 1:
            a[:, 2] = a[:, 0]  # rank deficient
        U, s, V = orc.jacobi_svd3f(a)
        rec = U.astype(np.float64) @ np.diag(s.astype(np.float64)) @ V.T.astype(np.float64)
        assert np.abs(rec - a).max() < 5e-6 * max(1.0, np.abs(a).max())
        assert np.abs(U.T @ U - np.eye(3)).max() < 2e-6 and np.abs(V.T @ V - np.eye(3)).max() < 2e-6
        assert s[0] >= s[1] >= s[2] >= 0
        assert np.abs(np.linalg.svd(a.astype(np.float64), compute_uv=False) - s).max() < 5e-6 * max(1.0, float(s[0]))
    U, s, V = orc.jacobi_svd3f(np.zeros((3, 3), np.float32))
    assert np.array_equal(U, np.eye(3)) and np.array_equal(V, np.eye(3)) and not s.any()


def test_rodrigues2_known_answers():
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    for ang in (0.3, 1.0, 2.5, 3.1):
        r = orc.rodrigues2(synth.rodrigues(axis * ang).astype(np.float32))
        assert np.abs(r - axis * ang).max() < 2e-5 * max(1.0, 1.0 / np.sin(ang))
    # below the float32 resolution of acos((trace - 1) / 2) the rotation vector is exactly zero (Model.cpp:1311-1318):
    # the quantisation the reference's fusion weight lives with
    assert not orc.rodrigues2(synth.rodrigues(axis * 5e-5).astype(np.float32)).any()
    assert abs(np.linalg.norm(orc.rodrigues2(synth.rodrigues(axis * 1e-3).astype(np.float32))) - 2.0 ** -10) < 1e-9
    # a scaled / sheared matrix is orthonormalised first (the JacobiSVD projection, :1302-1303)
    R = synth.rodrigues(axis * 0.7)
    assert np.abs(orc.rodrigues2((1.7 * R).astype(np.float32)) - axis * 0.7).max() < 1e-5
    # rotation by pi about x: the s < 1e-5, c < 0 branch
    assert np.abs(orc.rodrigues2(np.diag([1, -1, -1]).astype(np.float32)) - [np.pi, 0, 0]).max() < 1e-6


def test_compute_fusion_weight_known_answers():
    I = np.eye(4, dtype=np.float32)
    assert orc.compute_fusion_weight(I, I, 1.0) == 1.0 and orc.compute_fusion_weight(I, I, 100.0) == 100.0
    L = I.copy()
    L[:3, 3] = [0.003, 0.0, 0.004]  # |t| = 5 mm of the 10 mm that saturate the weight (Model.cpp:883-888)
    assert abs(orc.compute_fusion_weight(I, L, 1.0) - 0.5) < 1e-6
    L[:3, 3] = [0.03, 0.0, 0.0]
    assert orc.compute_fusion_weight(I, L, 2.0) == 1.0  # clamped to minWeight 0.5
    L = I.copy()
    L[:3, :3] = synth.rodrigues([0.0, 0.004, 0.0])
    w = orc.compute_fusion_weight(I, L, 1.0)
    assert 0.55 < w < 0.65  # the rotation term, quantised by acos near 1
    # getLastTransform() = pose^-1 * lastPose: invariant to a common left factor
    P = synth.make_pose([0.1, -0.2, 0.3], [0.5, 0.1, -0.4]).astype(np.float32)
    assert abs(orc.compute_fusion_weight(orc.matmul4f(P, I), orc.matmul4f(P, L), 1.0) - w) < 0.1


def _scene(w, h, n_frames, n_objects, seed=21):
    K = synth.intrinsics(w, h)
    poses = synth.trajectory(n_frames, seed=seed)
    objs = synth.make_objects(n_objects, seed=seed)
    traj = synth.object_trajectories(objs, n_frames, seed=seed)
    return K, [synth.render(p, w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]


def _run(K, frames, w, h, eps=0.0, with_data=True):
    o = OracleFusion(w, h, K, enable_multiple_models=True, pose_logging=True)
    known, out = [0], []
    for i, f in enumerate(frames):
        spawn = 1 <= i <= 2
        if spawn:
            known.append(i)
        mask = np.where(np.isin(f["ids"], known), f["ids"], 0).astype(np.uint8)
        depth = f["depth"]
        if eps:
            rng = np.random.default_rng(i)
            depth = (depth.astype(np.float64) * (1 + eps * rng.standard_normal(depth.shape))).astype(np.float32)
        data = None
        if with_data and i > 0:
            data = [dict(id=k, super_pixel_count=int((mask == k).sum()) // 256, avg_confidence=0.4,
                         depth_mean=float(f["depth"][mask == k].mean()), depth_std=0.05) for k in known]
        o.process_frame(f["rgb"], depth, timestamp=i, mask=mask, has_new_label=spawn, model_data=data)
        out.append([m.pose.copy() for m in o.models])
    return o, out


def test_multi_model_bookkeeping():
    w, h = 160, 120
    K, frames = _scene(w, h, 4, 2)
    o, poses = _run(K, frames, w, h)
    assert [m.id for m in o.models] == [0, 1, 2] and o.next_id == 3 and o.tick == 5
    assert o.models[0].fill_in and not o.models[1].fill_in
    assert o.models[1].conf == np.float32(0.4) and o.models[0].conf == 10.0  # :616-620 raises object thresholds only
    assert 1.0 < o.models[1].max_depth < 3.0 and o.models[0].max_depth > 1e30  # getMaxDepth (:408, :586)
    assert [len(m.pose_log) for m in o.models] == [4, 3, 2]  # one entry per frame in the list (:829-846)
    assert all(m.surfels.shape[0] > 50 for m in o.models[1:])
    # a model that is not seen leaves the list (:606-613)
    mask = np.zeros((h, w), np.uint8)
    data = [dict(id=0, super_pixel_count=70, avg_confidence=0.4, depth_mean=2.0, depth_std=0.1),
            dict(id=1, super_pixel_count=0, avg_confidence=0.4, depth_mean=0.0, depth_std=0.0),
            dict(id=2, super_pixel_count=3, avg_confidence=0.4, depth_mean=1.5, depth_std=0.1)]
    o.process_frame(frames[-1]["rgb"], frames[-1]["depth"], timestamp=9, mask=mask, model_data=data)
    assert [m.id for m in o.models] == [0, 2] and [m.id for m in o.inactive] == [1]


def test_object_tracking_is_sensitive_to_one_ulp_noise():
    """The tolerance of the GPU parity tests for OBJECT models is a measured property of the restated algorithm:
    depth noise of 1e-7 relative (about one float32 ulp) moves the oracle's own object poses by orders of magnitude
    more than the global pose."""
    w, h = 320, 240
    K, frames = _scene(w, h, 5, 2)
    _, a = _run(K, frames, w, h, with_data=False)
    _, b = _run(K, frames, w, h, eps=1e-7, with_data=False)
    glob = max(float(np.abs(x[0] - y[0]).max()) for x, y in zip(a, b))
    obj = max(float(np.abs(p - q).max()) for x, y in zip(a, b) for p, q in zip(x[1:], y[1:]))
    assert glob < 1e-6, glob
    assert obj > 20 * glob, (glob, obj)  # measured: 1e-5 .. 1e-3 against < 1e-7


def _tracked_run(w, h, n, conf=10.0, seed=7, adopt_at=(), substitute=None):
    """A free-running oracle orchestration; before the frames in `adopt_at` the oracle takes over its own state
    (OracleFusion.adopt); `substitute`: the poses to hand in after each frame's tracking (substitute_poses)."""
    K = synth.intrinsics(w, h)
    poses = synth.trajectory(n, seed=seed)
    frames = [synth.render(p, w, h, seed=i) for i, p in enumerate(poses)]
    o = OracleFusion(w, h, K, conf=conf)
    out = []
    for i, f in enumerate(frames):
        if i in adopt_at:
            m = o.models[0]
            before = [m.image, m.vertexConf, m.normalRadius, m.time_tex, m.fillVertex, m.fillNormal, m.fillImage]
            prev = frames[i - 1]
            o.adopt(0, o.surfels.copy(), o.pose.copy(), prev["rgb"], orc.bilateral_filter(prev["depth"], o.depth_cutoff))
            after = [m.image, m.vertexConf, m.normalRadius, m.time_tex, m.fillVertex, m.fillNormal, m.fillImage]
            for a, b in zip(before, after):  # the images the end-of-frame predict() left, regenerated
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), i
        o.process_frame(f["rgb"], f["depth"], substitute_poses=None if substitute is None or i == 0 else substitute[i])
        out.append((o.pose.copy(), o.surfels.copy(), getattr(o.models[0], "tracked_pose", None), o.models[0].image.copy()))
    return o, out


def test_adopting_its_own_state_changes_no_bit():
    """OracleFusion.adopt (the re-synchronised GPU tests hand the oracle the device's map and pose before each frame) renders
    the predicted and fill-in images of the previous frame's end again: with the oracle's own state they are the same bits,
    and so is everything after.  Threshold 0.5: the splat draws most of the map (at 10 nothing is stable for ~12 frames)."""
    for conf in (10.0, 0.5):
        _, a = _tracked_run(160, 120, 6, conf=conf)
        _, b = _tracked_run(160, 120, 6, conf=conf, adopt_at=(3, 4))
        assert conf == 10.0 or (a[-1][3][..., 3] > 0).mean() > 0.5  # (non-empty predicted images were regenerated)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x[0], y[0]), (conf, i)
            assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), (conf, i)


def test_substituting_the_tracked_pose():
    """process_frame(substitute_poses=...) tracks, keeps the tracker's result in tracked_pose, then goes on with the pose handed
    in: its own poses give a plain run's bits; another pose moves the map, but not what the tracker found, and the fusion weight
    sees the substituted motion (last_pose is not reset)."""
    _, a = _tracked_run(160, 120, 5)
    _, b = _tracked_run(160, 120, 5, substitute=[x[0] for x in a])
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), i
        assert i == 0 or np.array_equal(y[2], x[0]), i
    nudged = [x[0].copy() for x in a]
    nudged[2][0, 3] += np.float32(2e-3)
    o, c = _tracked_run(160, 120, 3, substitute=nudged)
    assert np.array_equal(c[2][2], a[2][0]) and np.array_equal(c[2][0], nudged[2])
    assert c[2][1].shape != a[2][1].shape or not np.array_equal(c[2][1], a[2][1])
    m = o.models[0]
    assert np.array_equal(m.last_pose, a[1][0]) and orc.compute_fusion_weight(m.pose, m.last_pose, 1.0) < 1.0


def test_clean_rule_counts_add_up():
    """orc_clean_stats: the surfels each rule of Model::clean removed add up to the surfels removed, the kept ones to the map
    left behind; the plain entry point gives the same bits.  Two dictated sequences that reach the rules: 40 frames (stable
    surfels from frame 12: the window rules `count > 8` and `zCount > 4`, the 20-frame unstable rule) and a pan with
    timeDelta 10 (surfels outside the window kept by `time - t > timeDelta`)."""
    w, h = 160, 120
    K = synth.intrinsics(w, h)
    seen = dict.fromkeys(orc.CLEAN_RULES, 0)
    for poses, td in ((synth.trajectory(40, seed=23), 200),
                      ([synth.make_pose([0, np.deg2rad(1.5 * i), 0], [0, 0, 0]) for i in range(13)], 10)):
        o = OracleFusion(w, h, K, time_delta=td)
        for i, p in enumerate(poses):
            f = synth.render(p, w, h, seed=i)
            o.process_frame(f["rgb"], f["depth"], in_pose=None if i == 0 else (np.linalg.inv(poses[0]) @ p).astype(np.float32))
        for tick, mid, st, removed in o.clean_log:  # every clean of the sequence
            assert st["window_count"] + st["z_count"] + st["unstable"] + st["col_w"] == removed, (tick, st, removed)
            for k, v in st.items():
                seen[k] += v
        # one more clean by hand: the counts of that call, and the plain entry point's bits
        m, fil = o.models[0], orc.bilateral_filter(f["depth"], o.depth_cutoff)
        index, vc, ct, nr = orc.predict_indices(m.surfels, m.pose, K, w, h, o.max_depth, o.tick, td)
        s_upd, new = orc.fuse(m.surfels, f["rgb"], f["depth"], fil, o.mask, index, vc, nr, m.pose, K, o.tick, 1.0, 0, o.max_depth)
        args = (s_upd, new, m.pose, K, w, h, o.tick, td, m.conf, o.outlier_coeff, 0, index, vc, ct, fil, o.mask)
        plain = orc.clean(*args)
        stat_out, stats = orc.clean(*args, with_stats=True)
        assert np.array_equal(plain.view(np.uint32), stat_out.view(np.uint32))
        assert stats["kept"] + stats["kept_time_delta"] == plain.shape[0]
        assert sum(stats.values()) == s_upd.shape[0] + new.shape[0]
    assert all(seen[k] > 0 for k in ("window_count", "z_count", "unstable", "kept_time_delta")), seen
