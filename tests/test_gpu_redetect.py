"""-m gpu: the batched, segmented descriptor matcher of the view store (csrc/redetect_kernels.hpp) and Model::getBestMatch
on top of it against the oracle (tests/redetect_oracle.py, oracle/mmf_oracle_match.c) -- bit for bit: the Gram tiles are
the fmaf chains of the oracle and RigidRANSAC is the same host code on both sides."""
import numpy as np
import pytest
import torch

import redetect_oracle as ro

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 31, 32, 33, 100]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_models(seed, n_views, n_models):
    """n_views views dealt to n_models models, sizes cycling through SIZES in a seeded order; descriptors drawn from a small
    pool so that exact duplicates (ties) occur inside views, across views and in the queries"""
    rng = np.random.default_rng(seed)
    pool = ro.unit_rows(rng, 160)
    models = [[] for _ in range(n_models)]
    for v in range(n_views):
        n = SIZES[(v + int(rng.integers(0, 6))) % 6] if n_views > 1 else 100
        desc = pool[rng.integers(0, len(pool), n)].copy()
        fresh = rng.uniform(size=n) < 0.5  # half of the rows are their own descriptor
        desc[fresh] = ro.unit_rows(rng, int(fresh.sum()))
        coord = rng.normal(size=(n, 3)).astype(np.float32)
        models[v % n_models].append((desc, coord))
    return pool, models


def queries(seed, pool, nq):
    rng = np.random.default_rng(seed + 7)
    q = pool[rng.integers(0, len(pool), nq)].copy()
    fresh = rng.uniform(size=nq) < 0.3
    q[fresh] = ro.unit_rows(rng, int(fresh.sum()))
    return q


def check_store(gpu_ctx, orc, vs, models, pool, seed, nqs, per_view_gpu):
    from multimotionfusion_amd.matcher import matchDescriptors
    flat = [(mid, i, view) for mid, views in enumerate(models) for i, view in enumerate(views)]
    assert [(m, i, r) for m, i, r in vs.views()] == [(m + 1, i, len(v[0])) for m, i, v in flat]
    ties = 0
    for nq in nqs:
        q = queries(seed + nq, pool, nq)
        idx, dist = vs.match(dev(q))
        assert idx.shape == (len(flat), nq)
        assert vs.lastLaunches() == (3 if sum(len(v[0]) for _, _, v in flat) else 0)
        for k, (_, _, (desc, _)) in enumerate(flat):
            oi, od = orc.match_descriptors(q, desc, 0.0)
            assert np.array_equal(idx[k], oi), (nq, k, len(desc), idx[k], oi)
            assert np.array_equal(dist[k].view(np.uint32), od.view(np.uint32)), (nq, k)
            ties += int((od[oi >= 0] == 0).sum())
            if per_view_gpu and len(desc):  # the same results as mmf_match_descriptors called per view
                gi, gd = matchDescriptors(gpu_ctx, dev(q), dev(desc), 0.0)
                assert np.array_equal(gi.cpu().numpy(), idx[k]) and np.array_equal(gd.cpu().numpy().view(np.uint32), dist[k].view(np.uint32))
    return ties


@pytest.mark.parametrize("n_views,n_models", [(1, 1), (7, 2), (7, 4), (300, 3)])
def test_batched_match_equals_the_oracle_view_by_view(gpu_ctx, orc, n_views, n_models):
    from multimotionfusion_amd.redetection import ViewStore
    seed = 100 + n_views + n_models
    pool, models = random_models(seed, n_views, n_models)
    vs = ViewStore(gpu_ctx)
    for mid, views in enumerate(models):
        assert vs.store(mid + 1, views) is True
    assert vs.store(1, models[0]) is False  # Model::store: stored before, skipped
    nqs = [3, 32, 65, 300] if n_views < 300 else [3, 65]
    ties = check_store(gpu_ctx, orc, vs, models, pool, seed, nqs, per_view_gpu=True)
    assert ties > 0 or n_views == 1  # duplicates (distance 0 matches) really occurred
    vs.close()


def test_launch_count_does_not_depend_on_the_store(gpu_ctx):
    from multimotionfusion_amd.redetection import ViewStore
    counts = []
    for n_views in (1, 800):
        pool, models = random_models(5, n_views, 4 if n_views > 1 else 1)
        vs = ViewStore(gpu_ctx)
        for mid, views in enumerate(models):
            vs.store(mid + 1, views)
        vs.match(dev(queries(5, pool, 64)))
        counts.append(vs.lastLaunches())
        vs.close()
    assert counts == [3, 3]


def test_empty_store_and_empty_views(gpu_ctx, orc):
    from multimotionfusion_amd.redetection import ViewStore
    vs = ViewStore(gpu_ctx)
    q = dev(ro.unit_rows(np.random.default_rng(1), 5))
    idx, dist = vs.match(q)
    assert idx.shape == (0, 5) and vs.lastLaunches() == 0
    assert vs.bestMatch(1, q, np.zeros((5, 3), np.float32))["found"] is False
    empty = (np.zeros((0, 256), np.float32), np.zeros((0, 3), np.float32))
    vs.store(9, [empty, empty])
    idx, dist = vs.match(q)
    assert idx.shape == (2, 5) and (idx == -1).all() and (dist == 0).all() and vs.lastLaunches() == 0
    idx, _ = vs.match(q[:0])
    assert idx.shape == (2, 0)
    vs.close()


def test_a_store_grown_between_matches_equals_one_built_at_once(gpu_ctx, orc):
    from multimotionfusion_amd.redetection import ViewStore
    pool, models = random_models(77, 120, 4)
    q = dev(queries(77, pool, 65))
    grown = ViewStore(gpu_ctx)
    grown.store(1, models[0])
    first = grown.match(q)
    for mid in (1, 2, 3):  # (30 views of up to 128 padded rows each: the buffers double at least once)
        grown.store(mid + 1, models[mid])
    again = grown.match(q)
    once = ViewStore(gpu_ctx)
    for mid, views in enumerate(models):
        once.store(mid + 1, views)
    ref = once.match(q)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1].view(np.uint32), ref[1].view(np.uint32))
    n0 = len(models[0])
    assert np.array_equal(first[0], ref[0][:n0]) and np.array_equal(first[1].view(np.uint32), ref[1][:n0].view(np.uint32))
    assert (ref[0] >= 0).any()
    grown.close(), once.close()


@pytest.mark.parametrize("seed", [3, 11, 29])
def test_best_match_equals_the_oracle(gpu_ctx, orc, seed):
    """same view, same inlier set, transformation and error bit-equal; the fixture and seeds of tests/test_redetect_oracle.py"""
    from multimotionfusion_amd.redetection import ViewStore
    vs = ViewStore(gpu_ctx)
    all_views = {}
    for mid, s in ((4, seed + 1000), (1, seed), (2, seed + 2000)):  # the object is model 1, between two unrelated models
        obj = ro.make_object(s)
        tracks, poses = ro.make_tracks(obj, 7, s + 100)
        all_views[mid] = ro.views_of(ro.project_first_frame(tracks, poses))
        vs.store(mid, all_views[mid])
    qd, qc, _, _ = ro.make_query(ro.make_object(seed), seed + 200)
    for mid in (1, 2, 4):
        got = vs.bestMatch(mid, dev(qd), qc)
        want = ro.get_best_match(orc, qd, qc, all_views[mid])
        assert got["found"] == want["found"] and got["view"] == want["view"] and got["n_matches"] == want["n_matches"], (mid, got, want)
        assert got["inliers"] == want["inliers"] and np.array_equal(got["inlier"], want["inlier"] if want["found"] else np.zeros(0, bool))
        assert np.array_equal(got["transformation"].view(np.uint32), np.asarray(want["transformation"], np.float32).view(np.uint32))
        assert np.float32(got["error"]).view(np.uint32) == np.float32(want["error"]).view(np.uint32)
    assert vs.bestMatch(1, dev(qd), qc)["error"] < 0.01 and vs.bestMatch(1, dev(qd), qc)["inliers"] > 5
    assert vs.bestMatch(7, dev(qd), qc)["found"] is False  # a model without stored views
    vs.close()
