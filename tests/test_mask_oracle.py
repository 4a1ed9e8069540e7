"""tests/mask_oracle.py against Segmentation.cpp:89-147, one hand-made case per rule, and the size of DESIGN.md B7's
deviation (float64 sums against the reference's raster-order float32 sums) on rendered frames."""
import numpy as np
import pytest

import mask_oracle as mo
from multimotionfusion_amd import synth

F32 = np.float32


def table(**kw):
    t = np.zeros(256, np.uint8)
    for k, v in kw.items():
        t[int(k[1:])] = v
    return t


def test_raster_first_label_wins_over_a_larger_later_one():
    lab = np.array([[0, 0, 9, 0],
                    [7, 7, 7, 7],
                    [7, 7, 7, 7],
                    [0, 9, 0, 0]], np.uint8)
    depth = np.arange(16, dtype=F32).reshape(4, 4)
    r = mo.segment(lab, depth, [0], 1, True, np.zeros(256, np.uint8))
    assert r["has_new_label"] and r["new_label"] == 9 and r["mapping"][9] == 1 and r["mapping"][7] == 0
    assert np.array_equal(r["mask"], (lab == 9).astype(np.uint8))
    # the eight pixels of label 7 stay unmapped: not in id 0's count (6 zeros only), in id 0's depth statistics (14 pixels)
    assert [e["id"] for e in r["model_data"]] == [0, 1]
    assert r["model_data"][0]["super_pixel_count"] == 6 // 256 == 0 and r["model_data"][1]["super_pixel_count"] == 1
    sel = lab != 9
    assert r["model_data"][0]["depth_mean"] == F32(depth[sel].astype(np.float64).mean())
    assert r["model_data"][1]["depth_mean"] == F32((2 + 13) / 2)
    assert r["model_data"][1]["depth_std"] == F32(5.5)
    # next frame: 9 is mapped, 7 becomes the next new label
    r2 = mo.segment(lab, depth, [0, 1], 2, True, r["mapping"])
    assert r2["new_label"] == 7 and r2["mapping"][7] == 2 and r2["mapping"][9] == 1
    assert np.array_equal(r2["mask"], np.where(lab == 9, 1, np.where(lab == 7, 2, 0)))


def test_without_allow_new_unmapped_pixels_count_nowhere_but_enter_the_depth_statistics():
    lab = np.zeros((6, 5), np.uint8)
    lab[1:3, 1:4] = 5
    lab[4, :] = 3  # mapped to model 1
    depth = np.full((6, 5), 2.0, F32)
    depth[lab == 5] = 4.0
    depth[lab == 3] = 1.0
    r = mo.segment(lab, depth, [0, 1], 2, False, table(l3=1))
    assert not r["has_new_label"] and r["new_label"] == -1 and r["mapping"][5] == 0
    assert np.array_equal(r["mask"], (lab == 3).astype(np.uint8))
    assert len(r["model_data"]) == 2
    # id 0: 19 zero pixels counted; its statistics run over 19 + 6 pixels of the output id 0
    assert r["model_data"][0]["depth_mean"] == F32((19 * 2.0 + 6 * 4.0) / 25)
    m = r["model_data"][0]["depth_mean"]
    assert r["model_data"][0]["depth_std"] == F32((19 * np.float64(abs(m - F32(2))) + 6 * np.float64(abs(m - F32(4)))) / 25)
    assert r["model_data"][1]["depth_mean"] == F32(1.0) and r["model_data"][1]["depth_std"] == 0
    # the count of id 0 is what decides it: 256 zeros + 256 unmapped pixels give 1 super-pixel, not 2
    lab2 = np.zeros((32, 16), np.uint8)
    lab2[16:] = 5
    r2 = mo.segment(lab2, np.ones((32, 16), F32), [0], 1, False, np.zeros(256, np.uint8))
    assert r2["model_data"][0]["super_pixel_count"] == 1


def test_new_entry_has_at_least_one_super_pixel_and_an_existing_model_with_255_pixels_none():
    lab = np.zeros((24, 24), np.uint8)
    lab.ravel()[:255] = 4   # model 1: 255 pixels -> 0 (it will count as unseen)
    lab.ravel()[300:556] = 6  # model 2: 256 pixels -> 1
    lab[23, 23] = 8         # one new pixel -> max(0, 1) = 1
    r = mo.segment(lab, np.ones((24, 24), F32), [0, 1, 2], 3, True, table(l4=1, l6=2))
    assert [e["super_pixel_count"] for e in r["model_data"]] == [(576 - 255 - 256 - 1) // 256, 0, 1, 1]
    assert r["model_data"][3]["id"] == 3 and all(e["avg_confidence"] == F32(0.4) for e in r["model_data"])


def test_two_labels_on_one_id():
    lab = np.array([[10, 10, 0, 20], [0, 0, 20, 20], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8)
    depth = np.where(lab == 10, 1.0, np.where(lab == 20, 3.0, 7.0)).astype(F32)
    r = mo.segment(lab, depth, [0, 4], 5, True, table(l10=4, l20=4))
    assert not r["has_new_label"] and np.array_equal(r["mask"], np.where(lab != 0, 4, 0))
    assert r["model_data"][1]["depth_mean"] == F32((2 * 1.0 + 3 * 3.0) / 5)


def test_an_id_outside_the_list_keeps_its_pixels_and_enters_no_entry():
    lab = np.array([[0, 30, 30, 0], [0, 0, 40, 40], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8)
    depth = np.where(lab == 30, 9.0, np.where(lab == 40, 5.0, 1.0)).astype(F32)
    # label 30 -> model 7, which has left the list; label 40 -> next_id 3, whose spawn was inhibited earlier
    for ref in (False, True):
        r = mo.segment(lab, depth, [0, 1], 3, False, table(l30=7, l40=3), reference_float32=ref)
        assert np.array_equal(r["mask"], np.where(lab == 30, 7, np.where(lab == 40, 3, 0)))
        assert [e["id"] for e in r["model_data"]] == [0, 1]
        assert r["model_data"][0]["depth_mean"] == F32(1.0) and r["model_data"][0]["depth_std"] == 0
        assert r["model_data"][1]["depth_mean"] == 0 and r["model_data"][1]["super_pixel_count"] == 0


def test_reference_variant_is_the_raster_order_float32_loop():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 3, (6, 5)).astype(np.uint8)
    depth = rng.uniform(0.5, 4.0, (6, 5)).astype(F32)
    r = mo.segment(lab, depth, [0, 1, 2], 3, False, table(l1=1, l2=2), reference_float32=True)
    for e in r["model_data"]:
        s, n = F32(0), 0
        for l, v in zip(lab.ravel(), depth.ravel()):
            if l == e["id"]:
                s, n = F32(s + v), n + 1
        mean = F32(s / F32(n))
        t = F32(0)
        for l, v in zip(lab.ravel(), depth.ravel()):
            if l == e["id"]:
                t = F32(t + F32(abs(F32(mean - v))))
        assert e["depth_mean"] == mean and e["depth_std"] == F32(t / F32(n))


def test_ulp_distance():
    assert mo.ulp_distance(F32(1.0), np.nextafter(F32(1.0), F32(2.0))) == 1
    assert mo.ulp_distance(F32(0.0), F32(-0.0)) == 0 and mo.ulp_distance(F32(-1.0), F32(-1.0)) == 0


@pytest.mark.parametrize("w,h", [(320, 240), (640, 480)])
def test_distance_of_b7_from_the_reference_sums(w, h):
    """The size of the documented deviation: float64 sums against the reference's raster-order float32 sums,
    for depth_mean, depth_std and the max depth processFrame derives from them.  Printed; nothing but finiteness is asserted."""
    objs = synth.make_objects(2, seed=21)
    poses = synth.trajectory(3, seed=21)
    traj = synth.object_trajectories(objs, 3, seed=21)
    worst = dict(mean=0.0, std=0.0, max_depth=0.0)
    for i in range(3):
        f = synth.render(poses[i], w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj])
        lab = f["ids"].astype(np.uint8)
        a = mo.segment(lab, f["depth"], [0, 1, 2], 3, False, table(l1=1, l2=2), reference_float32=True)
        b = mo.segment(lab, f["depth"], [0, 1, 2], 3, False, table(l1=1, l2=2))
        assert np.array_equal(a["mask"], b["mask"])
        for x, y in zip(a["model_data"], b["model_data"]):
            assert x["super_pixel_count"] == y["super_pixel_count"]
            dm, ds = abs(float(x["depth_mean"]) - float(y["depth_mean"])), abs(float(x["depth_std"]) - float(y["depth_std"]))
            dmax = abs(float(F32(x["depth_mean"] + F32(1.2) * x["depth_std"])) - float(F32(y["depth_mean"] + F32(1.2) * y["depth_std"])))
            assert np.isfinite([dm, ds, dmax]).all()
            worst = dict(mean=max(worst["mean"], dm), std=max(worst["std"], ds), max_depth=max(worst["max_depth"], dmax))
            print(f"{w}x{h} frame {i} id {x['id']}: n/256={x['super_pixel_count']} |d mean|={dm:.3e} |d std|={ds:.3e} "
                  f"|d (mean + 1.2 std)|={dmax:.3e} m")
    print(f"{w}x{h} largest: {worst}")
