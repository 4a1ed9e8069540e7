"""CPU: tests/backdate_oracle.py (the restatement mmf_tracker_backdate is compared with) against the
cases' own edges, against a transliteration of Model::refineTrackSubset (Core/Model/Model.cpp:649-737) over full track
histories, and against a float64 Kabsch fit on a known rigid motion.  No device: the search is the CPU oracle's, the
estimator the library's host class."""
import numpy as np
import pytest

import backdate_cases as bc
import backdate_oracle as bo
import tracker_oracle as to


class OracleDriver:
    def __init__(self, case, orc, width=bc.W, height=bc.H, intrinsics=bc.K):
        self.ora = bo.BackdateOracle(to.OracleTracker(width, height, intrinsics, capacity=case.capacity), 0)

    def log(self, frames):
        self.ora.set_view_log(frames)

    def add(self, xy, desc, ts, depth):
        self.ora.add(xy, desc, ts, depth, 0.7, 30)

    def associate(self, mask, ids):
        self.ora.t.associate(mask, ids)

    def prune(self, min_kps, min_time):
        self.ora.t.prune(min_kps, min_time)

    def reset(self):
        self.ora.reset()


def run_case(case, orc):
    d = OracleDriver(case, orc)
    bc.replay(case, d)
    return d, d.ora.backdate(case.label, case.history, case.max_points)


@pytest.mark.parametrize("case", bc.cases(), ids=lambda c: c.name)
def test_every_case_reaches_the_edge_it_is_named_for(orc, case):
    d, (entries, rows) = run_case(case, orc)
    assert case.expect, case.name
    for key, want in case.expect.items():
        assert [int(e[key]) for e in entries] == want, (case.name, key, [int(e[key]) for e in entries])
    # what holds in every case
    assert np.array_equal(entries[-1]["pose"], np.eye(4, dtype=np.float32)) and entries[0]["from"] == -1
    for j, (e, (p0, p1)) in enumerate(zip(entries, rows)):
        assert e["both"] >= e["nvalid"] and p0.shape == p1.shape == ((e["nvalid"], 3) if e["status"] == bo.OK and j else (0, 3))
        assert np.all(np.isfinite(e["pose"])) and np.all(np.isfinite(e["T"]))
        assert e["stamp"] == d.ora.stamp - len(entries) + 1 + j
        if len(entries) > 1:
            assert e["timestamp"] == d.ora.ts[e["stamp"]] > 0


def test_the_named_edges_beyond_the_counts(orc):
    by = {c.name: c for c in bc.cases()}
    d, _ = run_case(by["history_F_wrapped"], orc)
    assert d.ora.stamp > d.ora.frames  # the ring has wrapped
    d, _ = run_case(by["pruned_track"], orc)
    logged = {int(u) for s in d.ora.ring if s is not None for u in s["uid"]}
    assert logged - {t.uid for t in d.ora.t.tracks}  # a logged uid has left the table
    d, _ = run_case(by["other_labels"], orc)
    assert sorted({t.label for t in d.ora.t.tracks}) == [-1, 0, 1, 2]
    d, _ = run_case(by["table_1025_rows"], orc)
    rows_of_s = [i for i, t in enumerate(d.ora.t.tracks) if t.label == 1]
    assert len(d.ora.t.tracks) == 1025 and min(rows_of_s) < 1024 <= max(rows_of_s)
    d, _ = run_case(by["empty_slot"], orc)
    assert d.ora.slot(2)["uid"].size == 0
    d, _ = run_case(by["cut_by_L"], orc)
    assert len(d.ora.t.tracks[0]) == 2 and d.ora.stamp == 4 and all(d.ora.slot(s) is not None for s in (1, 2, 3, 4))
    d, (entries, _) = run_case(by["nan_track"], orc)
    assert not np.all(np.isfinite(d.ora.keypoint(2, 0))) and d.ora.keypoint(2, 0) is not None
    d, _ = run_case(by["reset_between_frames"], orc)
    assert d.ora.stamp == 2 and d.ora.slot(3) is None


# ---- Model::refineTrackSubset, line for line, over full histories (lists of Keypoint-or-None: what point_tracker.PointTracker
# and tracker_oracle.OracleTracker both keep).  The 4 x 4 arithmetic is the oracle's; the indexing, the chain and the engine are
# the reference's.
def refine_track_subset(tracks, n_parent_poses, history, running=True):
    from multimotionfusion_amd.ransac import RigidRANSAC
    if not tracks:
        return None
    rrs = RigidRANSAC(*bo.CONFIG)  # :665, ONE engine for the whole call
    n = min(len(tracks[0]), history)  # :667
    end = n_parent_poses - 1
    start = end - n + 1
    poses = [np.eye(4, dtype=np.float32)] + [None] * (n - 1)
    stamps, counts, Ts = [0] * n, [(0, 0)] * n, [None] * n
    ik = 0
    for jk in range(1, n):  # :681
        p0s, p1s, both, t1 = [], [], 0, 0
        for track in tracks:
            k0, k1 = track[start + ik], track[start + jk]
            if k0 is not None and k1 is not None:
                both += 1
                t1 = k1.timestamp
                if np.all(np.isfinite(k0.coordinate)) and np.all(np.isfinite(k1.coordinate)):
                    p0s.append(k0.coordinate)
                    p1s.append(k1.coordinate)
        stamps[jk], counts[jk] = t1, (both, len(p0s))
        if len(p0s) < 3:  # :706
            poses[jk] = poses[ik].copy()
            continue
        engine = rrs if running else RigidRANSAC(*bo.CONFIG)
        Ts[jk] = engine.estimate(np.array(p0s, np.float32), np.array(p1s, np.float32))[0]  # :716
        poses[jk] = bo.matmul4(poses[ik], Ts[jk])  # :718
        ik = jk
    E = bo.inverse(poses[-1])
    return dict(poses=[bo.matmul4(E, p) for p in poses], timestamps=stamps, counts=counts, T=Ts)  # :728-730


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def motion_scene(n_frames, drop=(), nodepth=(), n_obj=12, n_other=6, seed=3, W=320, H=240, K=(264.0, 264.0, 160.0, 120.0)):
    """an object of n_obj keypoints moving rigidly in front of a camera, n_other keypoints that stay: -> a BackdateOracle after
    n_frames adds and the association (object = label 1), and the float64 motions M[f] (object points of frame 0 -> frame f).
    drop / nodepth: (keypoint, frame) pairs that are not visible / lie on a depth of 0"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    P0 = np.concatenate([rng.uniform(-0.3, 0.3, (n_obj, 2)), rng.uniform(1.2, 1.8, (n_obj, 1))], 1)
    Q = np.concatenate([rng.uniform(-0.6, 0.6, (n_other, 2)), rng.uniform(2.0, 3.0, (n_other, 1))], 1)
    desc = bc.vo.unit_rows(rng, n_obj + n_other)
    ora = bo.BackdateOracle(to.OracleTracker(W, H, K), n_frames + 2)
    M, mask = [], None
    for f in range(n_frames):
        a = 0.03 * f
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([0.02 * f, -0.01 * f, 0.015 * f])
        c = P0.mean(0)
        Mf = np.eye(4)
        Mf[:3, :3], Mf[:3, 3] = R, c - R @ c + t  # (a rotation about the object's centre, and a drift)
        M.append(Mf)
        pts = np.concatenate([P0 @ Mf[:3, :3].T + Mf[:3, 3], Q])
        xy = np.stack([np.rint(fx * pts[:, 0] / pts[:, 2] + cx), np.rint(fy * pts[:, 1] / pts[:, 2] + cy)], 1).astype(np.int32)
        assert len({tuple(p) for p in xy}) == len(xy) and xy.min() >= 0 and np.all(xy[:, 0] < W) and np.all(xy[:, 1] < H)
        depth = np.zeros((H, W), np.float32)
        depth[xy[:, 1], xy[:, 0]] = pts[:, 2].astype(np.float32)
        for k, at in nodepth:
            if at == f:
                depth[xy[k, 1], xy[k, 0]] = 0.0
        vis = np.array([(k, f) not in drop for k in range(len(xy))])
        ora.add(xy[vis], desc[vis], 1_000_000 + 33_000 * f, depth, 0.7, 30)
        mask = np.zeros((H, W), np.uint8)
        mask[xy[:n_obj, 1], xy[:n_obj, 0]] = 1
    ora.t.associate(mask, [0, 1])
    return ora, M


def test_history_2_is_the_reference_bit_for_bit_and_longer_ones_up_to_the_stated_deviations(orc):
    """the table was never empty and the log holds every frame, so the reference's index (parent->poses.size()) and the stamp
    name the same frames.  history 2 -- the reference's only call: one pair, one estimate of a fresh engine -- equals the
    transliteration in every number but the last pose (the reference's near-identity E rel[len - 1], here exactly I).  Longer
    histories: the counts, the chain and the first estimate agree with the reference's ONE running engine; with a fresh
    engine per pair (the rule of B6 (4)) everything does."""
    ora, _ = motion_scene(6, drop={(3, 3)}, nodepth={(5, 3)})  # a gap in one track, a keypoint without depth in another
    S = [t for t in ora.t.tracks if t.label == 1]
    n_poses = len(ora.t.tracks[0])
    for history in (2, 3, 6, 50):
        entries, _ = ora.backdate(1, history)
        ref = refine_track_subset(S, n_poses, history, running=True)
        fresh = refine_track_subset(S, n_poses, history, running=False)
        n = min(6, history)
        assert len(entries) == n == len(ref["poses"])
        for j, e in enumerate(entries):
            assert (e["both"], e["nvalid"]) == ref["counts"][j], (history, j)
            if e["both"]:
                assert e["timestamp"] == ref["timestamps"][j]
            if j and e["status"] == bo.OK:
                assert np.array_equal(bits(e["T"]), bits(fresh["T"][j])), (history, j)
            if j < n - 1:
                assert np.array_equal(bits(e["pose"]), bits(fresh["poses"][j])), (history, j)
        first = next(j for j, e in enumerate(entries) if j and e["status"] == bo.OK)
        assert np.array_equal(bits(entries[first]["T"]), bits(ref["T"][first]))
        if history == 2:  # the reference's call: the running engine IS the fresh one
            assert np.array_equal(bits(entries[0]["pose"]), bits(ref["poses"][0]))
        assert np.abs(ref["poses"][-1] - np.eye(4)).max() < 1e-6 and np.array_equal(entries[-1]["pose"], np.eye(4, dtype=np.float32))
    assert [e["nvalid"] for e in ora.backdate(1, 6)[0]] == [0, 12, 12, 10, 10, 12]


def kabsch(p0, p1):
    """float64 least-squares T with p0 ~ T p1"""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    c0, c1 = p0.mean(0), p1.mean(0)
    U, _, Vt = np.linalg.svd((p1 - c1).T @ (p0 - c0))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, c0 - R @ c1
    return T


MEASURED = 1.5e-7  # the largest |oracle pose - float64 Kabsch chain| entry over the five pairs of the test below (1.485e-07)


def test_a_known_rigid_motion_over_six_frames_is_recovered(orc):
    """an object's 12 keypoints move rigidly (3 cm / 1.7 degrees a frame) for six frames; their logged coordinates are those of
    the rounded pixels, so a pair's rows are rigid up to about z / fx / 2 = 3 mm.  The oracle's poses are compared with the
    chain of float64 Kabsch fits of the SAME rows (all of them; the estimator refits to its inliers, which is where the two
    differ; here every row is an inlier).  Bound: four times the largest distance observed.  Measured: 1.485e-07 to the Kabsch
    chain (float32 rounding of entries near 1), 7.5e-03 to the true motion (the pixel rounding)."""
    ora, M = motion_scene(6)
    entries, rows = ora.backdate(1, 6)
    assert len(entries) == 6 and all(e["nvalid"] == 12 for e in entries[1:]) and [e["from"] for e in entries] == [-1, 0, 1, 2, 3, 4]
    rel = [np.eye(4)]
    for j in range(1, 6):
        rel.append(rel[-1] @ kabsch(*rows[j]))
    worst, truth = 0.0, 0.0
    for j, e in enumerate(entries):
        want = np.linalg.inv(rel[-1]) @ rel[j]
        worst = max(worst, float(np.abs(e["pose"].astype(np.float64) - want).max()))
        true = M[5] @ np.linalg.inv(M[j])  # frame j -> frame 5
        truth = max(truth, float(np.abs(e["pose"].astype(np.float64) - true).max()))
    print(f"largest distance to the float64 Kabsch chain {worst:.3e}, to the true motion {truth:.3e}")
    assert worst <= 4 * MEASURED, worst
    assert truth < 0.02, truth  # (five pairs of 3 mm noise on a 0.3 m object: well below the 3 cm inlier threshold)


def test_the_fusion_scene_has_tracks_to_back_date_over(orc):
    """tests/backdate_scene.py (the scene of tests/test_gpu_backdate_fusion.py): the oracle alone, driven as processFrame drives
    the tracker, finds at least three finite pairs in each frame of the window before SPAWN"""
    import backdate_scene as bs
    K, frames, kps = bs.build()
    intr = (K["fx"], K["fy"], K["cx"], K["cy"])
    ora = bo.BackdateOracle(to.OracleTracker(bs.W, bs.H, intr, capacity=512), 16)
    for i in range(bs.SPAWN + 1):
        xy, desc = kps[i]
        ora.add(xy, desc, 1000 + i, frames[i]["depth"], 0.7, 30)
        ora.t.prune(30, 0)
        if i == 0:
            ora.t.associate_all([0])
    ora.t.associate(bs.frame_mask(frames, bs.SPAWN), [0, 1])
    for history in (2, 4):
        entries, _ = ora.backdate(1, history)
        assert len(entries) == bs.SPAWN + 1 >= 2
        assert all(e["nvalid"] >= 3 and e["status"] == bo.OK for e in entries[1:]), [e["nvalid"] for e in entries]
