"""-m gpu: the keypoint selection behind the SuperPoint network at its tie, chain, count, border, non-finite and size edges
(tests/keypoint_edges.py), on maps installed with SuperPoint.setMaps -- the heat map, the descriptor map and the logits are
the cases' own, not what a network happens to produce.  Every case goes through BOTH selections (select: the host-looped one
of mmf_superpoint_get_features; selectDevice: the one of mmf_superpoint_get_features_device); xy, confidences, sampled
descriptors and the count equal the oracle's bit for bit (a NaN equals a NaN at the same place, and the number of rows that
hold one is the case's claim), the two paths equal each other, a second run gives the same bytes, the device path reports
status 0, and the case's own claims hold on the device's results.  test_keypoint_edges_oracle.py pins the oracle and the
claims without a device."""
import numpy as np
import pytest

import keypoint_edges as ke
from helpers import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(gpu_ctx, orc):
    """SuperPoint objects by (max height, max width, max_keypoints), made on first use and shared"""
    from multimotionfusion_amd.superpoint import SuperPoint
    weights = orc.sp_random_weights(seed=4)
    made = {}

    def get(H, W, max_keypoints, fresh=False):
        if fresh:
            return SuperPoint(gpu_ctx, weights, max_width=W, max_height=H, max_keypoints=max_keypoints)
        key = (H, W, max_keypoints)
        if key not in made:
            made[key] = SuperPoint(gpu_ctx, weights, max_width=W, max_height=H, max_keypoints=max_keypoints)
        return made[key]

    yield get
    for sp in made.values():
        sp.close()


def of(pool, name):
    c = ke.CASES[name]
    return pool(c.H, c.W, c.max_keypoints)


@pytest.mark.parametrize("name", [n for f in ("tie", "chain", "band", "nonfinite", "count", "size", "sample") for n in ke.names(f)])
def test_selection_case(pool, orc, name):
    got = ke.check_case(of(pool, name), name, orc)
    print(name, "keypoints", len(got["device"]["xy"]), "NaN rows", got["device"]["nan_rows"], "inf rows", got["device"]["inf_rows"])


@pytest.mark.parametrize("name", ke.names("logits") + ke.names("normalise"))
def test_installed_maps_case(pool, orc, name):
    """the heat map of sp_heatmap_kernel / the map of sp_l2_normalize_kernel<256> after setMaps equal the oracle's (check_case
    downloads them), and so do the keypoints selected from them"""
    c = ke.CASES[name]
    assert c.semi is not None or c.normalize
    got = ke.check_case(of(pool, name), name, orc)
    assert len(got["device"]["xy"]) > 0


def test_launches_depend_on_the_size_alone(pool, orc):
    """the device selection of every case: candidates from none to all, chains of 8 to 1120 passes, any max_keypoints"""
    launches = {}
    for name, c in ke.CASES.items():
        sp = of(pool, name)
        ke.install(sp, c)
        _, status, n = ke.run_device(sp, c, "device")
        assert status == 0 and n > 0
        launches.setdefault((c.H, c.W), set()).add(n)
    assert all(len(v) == 1 for v in launches.values()) and len(launches[(40, 56)]) == 1, launches


def test_one_object_serves_a_large_image_then_a_small_one(pool, orc):
    """stale state / flags / list contents: one object created for 40 x 56 runs a 40 x 56 chain, 16 x 24, 8 x 8 and 40 x 56
    again; each result is the oracle's and, bit for bit, a fresh object's"""
    one = pool(ke.H0, ke.W0, ke.H0 * ke.W0, fresh=True)
    try:
        for name in ke.STALE:
            c = ke.CASES[name]
            got = ke.check_case(one, name, orc)
            fresh = pool(c.H, c.W, c.max_keypoints, fresh=True)
            try:
                ke.install(fresh, c)
                for path in ("host", "device"):
                    r, status, _ = ke.run_device(fresh, c, path)
                    assert status == 0
                    for k in ("xy", "conf", "desc"):
                        assert np.array_equal(bits(r[k]), bits(got[path][k])), (name, path, k)
            finally:
                fresh.close()
    finally:
        one.close()


def test_refusals_leave_the_object_usable(pool, orc):
    from multimotionfusion_amd._capi import MmfError
    name = "sample-16x24"
    c = ke.CASES[name]
    sp = pool(c.H, c.W, c.max_keypoints, fresh=True)
    try:
        for call in (sp.select, sp.selectDevice):  # before any maps or forward pass
            with pytest.raises(MmfError) as e:
                call()
            assert e.value.status == -4, e.value
        ke.check_case(sp, name, orc)
        heat, semi = np.zeros((c.H, c.W), np.float32), np.zeros((c.H // 8, c.W // 8, 65), np.float32)
        refused = [dict(width=c.W, height=c.H, semi=semi, heat=heat), dict(width=c.W, height=c.H),  # both, neither
                   dict(width=12, height=8, heat=np.zeros((8, 12), np.float32)),                   # not a multiple of 8
                   dict(width=0, height=8, heat=np.zeros((8, 0), np.float32)),
                   dict(width=32, height=24, heat=np.zeros((24, 32), np.float32)),                 # larger than the object serves
                   dict(width=c.W + 8, height=8, heat=np.zeros((8, c.W + 8), np.float32))]
        for kw in refused:
            with pytest.raises(MmfError) as e:
                sp.setMaps(**kw)
            assert e.value.status == -1, (kw["width"], kw["height"], e.value)
            for path in ("host", "device"):  # the maps installed before are still the object's
                r, status, _ = ke.run_device(sp, c, path)
                ke.assert_same(r["xy"], ke.ref_of(name, orc)["xy"], f"after a refused setMaps, {path} path")
        for kw in (dict(nms_dist=-1), dict(border=-1)):
            for call in (sp.select, sp.selectDevice):
                with pytest.raises(MmfError) as e:
                    call(**kw)
                assert e.value.status == -1, (kw, e.value)
        ke.check_case(sp, name, orc)
    finally:
        sp.close()
