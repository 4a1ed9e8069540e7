"""-m gpu: the view store with a device verifier attached (mmf_viewstore_set_verifier, mmf_viewstore_best_match_device)
against the per-view oracle (tests/verify_oracle.py): same view, same inlier flags, transformation and error bit for bit."""
import numpy as np
import pytest
import torch

import redetect_oracle as ro
import verify_oracle as vo

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def object_views(seed, n_views, k=70):
    obj = ro.make_object(seed, k=k)
    tracks, poses = ro.make_tracks(obj, n_views, seed + 100)
    return obj, ro.views_of(ro.project_first_frame(tracks, poses))


def build(n_views, n_models, seed):
    """n_views views dealt to models 1 .. n_models, each model its own object; among them (where there is room) an empty
    view, a view of two rows and a view of unrelated descriptors.  -> objects, {model id: views}"""
    per = [n_views // n_models + (1 if m < n_views % n_models else 0) for m in range(n_models)]
    objs, models = {}, {}
    rng = np.random.default_rng(seed)
    for m, nv in enumerate(per):
        objs[m + 1], views = object_views(seed + 10 * m, nv)
        if nv >= 3:
            views[1] = (np.zeros((0, 256), np.float32), np.zeros((0, 3), np.float32))
            views[2] = (views[2][0][:2], views[2][1][:2])  # fewer than 3 matches whatever the query
        if nv >= 5:
            views[4] = (ro.unit_rows(rng, 33), rng.normal(size=(33, 3)).astype(np.float32))
        models[m + 1] = views
    return objs, models


def query(obj, seed, nq):
    qd, qc, _, _ = ro.make_query(obj, seed, subset=0.9)
    assert len(qd) >= nq
    return qd[:nq], qc[:nq]


def same(got, want, what):
    assert got["found"] == want["found"] and got["view"] == want["view"] and got["n_matches"] == want["n_matches"], (what, got, want)
    assert got["inliers"] == want["inliers"], (what, got, want)
    assert np.array_equal(got["inlier"], want["inlier"] if want["found"] else np.zeros(0, bool)), what
    assert np.array_equal(got["transformation"].view(np.uint32), np.asarray(want["transformation"], np.float32).view(np.uint32)), what
    assert np.float32(got["error"]).view(np.uint32) == np.float32(want["error"]).view(np.uint32), what


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    from multimotionfusion_amd.ransac import RansacBatch
    b = RansacBatch(gpu_ctx, *ro.RANSAC_CONFIG, max_points=1024)
    yield b
    b.close()


@pytest.mark.parametrize("n_views,n_models", [(1, 1), (7, 3), (40, 4)])
def test_best_match_device_equals_the_per_view_oracle(gpu_ctx, orc, batch, n_views, n_models):
    from multimotionfusion_amd.redetection import ViewStore
    objs, models = build(n_views, n_models, 300 + n_views)
    vs = ViewStore(gpu_ctx)
    vs.setVerifier(batch)
    for mid, views in models.items():
        assert vs.store(mid, views) is True
    forgotten = n_models if n_models > 1 else None
    if forgotten:
        vs.forget(forgotten)
    found = 0
    for nq in (0, 2, 3, 64):
        for target in objs:  # the query shows the object of model `target`
            qd, qc = query(objs[target], 900 + target, nq)
            for mid in list(models) + [99]:  # every model of the store, and one that is not in it
                got = vs.bestMatchDevice(mid, dev(qd), dev(qc))
                gone = mid == 99 or mid == forgotten
                want = vo.get_best_match(orc, qd, qc, [] if gone else models[mid])
                same(got, want, (nq, target, mid))
                if not gone and nq > 0:
                    assert vs.lastLaunches() == 5, (nq, mid, vs.lastLaunches())  # whatever the store and the query hold
                found += int(got["found"])
                if nq == 64 and mid == target and not gone:
                    assert got["found"] and got["error"] < 0.01 and got["inliers"] > 5
    assert found >= (1 if n_models == 1 else 2)
    vs.close()


def test_a_view_stored_twice_the_first_wins(gpu_ctx, orc, batch):
    """one view stored under two models and twice inside one: equal estimates, so the first index wins inside the model and
    either model gives the same estimate"""
    from multimotionfusion_amd.redetection import ViewStore
    obj, views = object_views(41, 4)
    qd, qc = query(obj, 941, 64)
    solo = [vo.get_best_match(orc, qd, qc, [v]) for v in views]
    order = np.argsort([np.float32(s["error"]) for s in solo])
    best = views[int(order[0])]
    others = [v for k, v in enumerate(views) if k != int(order[0])]
    a = [others[0], best, others[1], best, others[2]]  # twice inside model 1: index 1 and 3
    b = [others[2], others[1], best]  # and under model 2
    vs = ViewStore(gpu_ctx)
    vs.setVerifier(batch)
    vs.store(1, a), vs.store(2, b)
    ga, gb = vs.bestMatchDevice(1, dev(qd), dev(qc)), vs.bestMatchDevice(2, dev(qd), dev(qc))
    same(ga, vo.get_best_match(orc, qd, qc, a), "a")
    same(gb, vo.get_best_match(orc, qd, qc, b), "b")
    assert ga["view"] == 1 and gb["view"] == 2
    assert np.array_equal(ga["transformation"].view(np.uint32), gb["transformation"].view(np.uint32)) and ga["error"] == gb["error"]
    vs.close()


def test_growth_attachment_order_and_launch_counts(gpu_ctx, orc, batch):
    """A store that doubled between two calls (descriptor rows, coordinates and the view table: more than 4096 rows and 256
    views) equals one built at once; a verifier attached after the views were stored equals one attached before; the launch
    count is 5 whatever the store holds, and 3 per set again once the verifier is detached."""
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.redetection import ViewStore
    objs, models = build(12, 2, 77)
    rng = np.random.default_rng(78)
    filler = [(ro.unit_rows(rng, 100), rng.normal(size=(100, 3)).astype(np.float32)) for _ in range(40)]  # 40 x 128 padded rows
    many = [(ro.unit_rows(rng, 3), rng.normal(size=(3, 3)).astype(np.float32)) for _ in range(300)]
    obj3, views3 = object_views(79, 5)
    qd, qc = query(objs[1], 901, 64)
    q3d, q3c = query(obj3, 903, 64)
    grown = ViewStore(gpu_ctx)
    grown.setVerifier(batch)
    grown.store(1, models[1]), grown.store(2, models[2])
    first = grown.bestMatchDevice(1, dev(qd), dev(qc))
    assert grown.lastLaunches() == 5
    same(first, vo.get_best_match(orc, qd, qc, models[1]), "before growth")
    grown.store(3, filler), grown.store(4, many), grown.store(5, views3)
    late = ViewStore(gpu_ctx)  # everything stored first, the verifier attached last
    for mid, views in ((1, models[1]), (2, models[2]), (3, filler), (4, many), (5, views3)):
        late.store(mid, views)
    late.match(dev(qd))
    assert late.lastLaunches() == 3
    with pytest.raises(MmfError):
        late.bestMatchDevice(1, dev(qd), dev(qc))
    late.setVerifier(batch)
    for mid, (d, c) in ((1, (qd, qc)), (2, (qd, qc)), (5, (q3d, q3c)), (3, (q3d, q3c))):
        g, l = grown.bestMatchDevice(mid, dev(d), dev(c)), late.bestMatchDevice(mid, dev(d), dev(c))
        assert grown.lastLaunches() == 5 and late.lastLaunches() == 5
        same(g, l, ("grown / late", mid))
        if mid in (1, 5):
            same(g, vo.get_best_match(orc, d, c, models[1] if mid == 1 else views3), ("oracle", mid))
            assert g["found"]
    late.setVerifier(None)
    late.match(dev(qd))
    assert late.lastLaunches() == 3
    with pytest.raises(MmfError):
        late.bestMatchDevice(1, dev(qd), dev(qc))
    host = late.bestMatch(1, dev(qd), qc)  # the host path is what it was
    same(host, ro.get_best_match(orc, qd, qc, models[1]), "host path")
    grown.close(), late.close()


def test_more_query_rows_than_the_verifier_takes(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.ransac import RansacBatch
    from multimotionfusion_amd.redetection import ViewStore
    small = RansacBatch(gpu_ctx, *ro.RANSAC_CONFIG, max_points=40)
    obj, views = object_views(5, 3)
    vs = ViewStore(gpu_ctx)
    vs.setVerifier(small)
    vs.store(1, views)
    qd, qc = query(obj, 905, 41)
    with pytest.raises(MmfError):
        vs.bestMatchDevice(1, dev(qd), dev(qc))
    assert vs.bestMatchDevice(1, dev(qd[:40]), dev(qc[:40]))["found"]
    vs.close(), small.close()


def test_scratch_regrows_and_shrinks_between_calls(gpu_ctx, batch):
    """3 query rows, then as many as the object gives (every scratch and staging buffer is released and allocated anew,
    larger), then 3 again (the buffers are reused oversized): each answer equals, bit for bit, the answer of a fresh store
    that was asked only that"""
    from multimotionfusion_amd.redetection import ViewStore
    objs, models = build(7, 3, 511)

    def fresh():
        vs = ViewStore(gpu_ctx)
        vs.setVerifier(batch)
        for mid, views in models.items():
            assert vs.store(mid, views) is True
        return vs

    big = min(200, len(ro.make_query(objs[1], 951, subset=0.9)[0]))  # (make_query gives fewer than 200 rows for these objects)
    assert big >= 4 * 3
    vs = fresh()
    for nq in (3, big, 3):
        qd, qc = query(objs[1], 951, nq)
        got = vs.bestMatchDevice(1, dev(qd), dev(qc))
        assert vs.lastLaunches() == 5
        idx, dist = vs.match(dev(qd))
        one = fresh()
        same(got, one.bestMatchDevice(1, dev(qd), dev(qc)), ("bestMatchDevice", nq))
        one.close()
        one = fresh()
        want_idx, want_dist = one.match(dev(qd))
        one.close()
        assert idx.shape == (7, nq) and np.array_equal(idx, want_idx), nq
        assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32)), nq
        if nq == big:
            assert got["found"] and (idx >= 0).any()
    vs.close()


def test_device_store_across_a_doubling_equals_the_host_store(gpu_ctx, batch):
    """store, then storeDevice of a model that takes the store past its first 4096 rows (descriptors and coordinates double,
    the old rows are copied), then storeDevice of a small one: the store equals one that took all three through store"""
    from multimotionfusion_amd.redetection import ViewStore
    rng = np.random.default_rng(80)
    obj1, views1 = object_views(81, 4)
    filler = [(ro.unit_rows(rng, 100), rng.normal(size=(100, 3)).astype(np.float32)) for _ in range(40)]  # 40 x 128 padded rows
    obj3, views3 = object_views(83, 5)

    def packed(views):
        return ([len(d) for d, _ in views], dev(np.concatenate([d for d, _ in views])), dev(np.concatenate([c for _, c in views])))

    mixed, host = ViewStore(gpu_ctx), ViewStore(gpu_ctx)
    mixed.setVerifier(batch), host.setVerifier(batch)
    assert mixed.store(1, views1) is True
    assert mixed.storeDevice(2, *packed(filler)) is True
    assert mixed.storeDevice(3, *packed(views3)) is True
    for mid, views in ((1, views1), (2, filler), (3, views3)):
        assert host.store(mid, views) is True

    def equal_stores():
        assert mixed.views() == host.views() and len(host.views()) == 4 + 40 + 5
        for v in range(len(host.views())):
            (dm, cm), (dh, ch) = mixed.downloadView(v), host.downloadView(v)
            assert np.array_equal(dm.view(np.uint32), dh.view(np.uint32)) and np.array_equal(cm.view(np.uint32), ch.view(np.uint32)), v

    def equal_answers():
        for mid, obj in ((1, obj1), (3, obj3)):
            qd, qc = query(obj, 980 + mid, 64)
            got = mixed.bestMatchDevice(mid, dev(qd), dev(qc))
            same(got, host.bestMatchDevice(mid, dev(qd), dev(qc)), mid)
            if mid == 3:
                assert got["found"] and got["error"] < 0.01 and got["inliers"] > 5

    equal_stores()
    equal_answers()
    assert mixed.storeDevice(2, *packed(filler)) is False  # (Model.cpp:1618-1621) ... and nothing changed
    equal_stores()
    equal_answers()
    mixed.close(), host.close()
