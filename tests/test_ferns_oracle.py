"""CPU: the oracle of the fern keyframe database (tests/ferns_oracle.py) against the cases worked by hand in
tests/ferns_cases.py, the nearest-sample rule of the small images, and what the library offers without a device: the table
of mmf_ferns_make_table, the defaults, the refusals that come before any device is touched, the export table."""
import ctypes as C

import numpy as np
import pytest

import ferns_cases as fc
import ferns_oracle as fo


def same(got, want):
    if isinstance(want, (float, np.floating)):
        return np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32) or (np.isnan(got) and np.isnan(want))
    return got == want


def test_the_codes_at_their_edges():
    """strict > at a pixel equal to its threshold and at int(z 1000) == t_d; the truncation; z of 0, negative and NaN; the 2^31 rule"""
    image, vert, _ = fc.code_images()
    codes, good = fo.encode(fc.CODE_TABLE, image, vert)
    assert codes.tolist() == fc.CODE_EXPECT.tolist()
    assert good == fc.CODE_GOOD
    # through the full-size images: the nearest sample of an 8 x 8 block is its pixel
    assert np.array_equal(fo.resize(fc.full_size(image)), image)
    assert np.array_equal(fo.resize(fc.full_size(vert)).view(np.uint32), vert.view(np.uint32))


@pytest.mark.parametrize("case", fc.DECISION_CASES, ids=lambda c: c["name"])
def test_the_decisions_worked_by_hand(case):
    db = fo.Database(16, 16, fc.DECISION_TABLE, num=4, **case["config"])
    for k, s in enumerate(case["steps"]):
        image, vert, norm = fc.frame_from_codes(s["codes"])
        res = db.process_small(image, vert, norm, fc.pose(k), s["time"], s["flags"])
        assert db.cur["codes"].tolist() == s["codes"], (k, db.cur["codes"])
        for name, want in s["expect"].items():
            assert same(res[name], want), (case["name"], k, name, res[name], want)
        if res["closest"] >= 0:  # the record carries the keyframe's pose and time
            assert np.array_equal(res["closest_pose"], db.frames[res["closest"]]["pose"])
            assert res["closest_time"] == db.frames[res["closest"]]["time"]
    assert [f["codes"].tolist() for f in db.frames] == [s["codes"] for s in case["steps"] if s["expect"].get("added")]


def test_similarity_and_dissimilarity_are_single_float_operations():
    assert fo.dissimilarity(3, 7, 1).view(np.uint32) == (np.float32(2) / np.float32(3)).view(np.uint32)
    assert np.isnan(fo.dissimilarity(0, 5, 0)) and np.isnan(fo.dissimilarity(5, 0, 0))
    a = np.array([1, 2, 255, 4, 5, 255, 7], np.uint8)
    b = np.array([1, 3, 9, 255, 5, 255, 7], np.uint8)
    assert fo.co_occurrence(a, b) == 3
    assert fo.block_hd_aware(a, b).view(np.uint32) == (np.float32(3) / np.float32(4)).view(np.uint32)
    assert np.isnan(fo.block_hd_aware(np.array([255, 1], np.uint8), np.array([1, 255], np.uint8)))


@pytest.mark.parametrize("width,height", [(64, 48), (104, 52), (640, 480), (9, 15)])
def test_the_small_image_samples_inside_its_cell(width, height):
    """texel((i + 0.5f) / w, width) lies in [i width / w, (i + 1) width / w): the sample of small pixel i comes from its own cell"""
    ty, tx = fo.small_indices(width, height)
    w, h = width // 8, height // 8
    assert len(tx) == w and len(ty) == h
    for t, n, size in ((tx, w, width), (ty, h, height)):
        i = np.arange(n)
        assert np.all(t * n >= i * size) and np.all(t * n < (i + 1) * size) and np.all(np.diff(t) > 0)
    if (width, height) == (104, 52):  # 13 x 6: 52 / 6 is no integer; worked by hand: (j + 0.5) * 52 / 6 = 4.33, 13, 21.67, 30.33, 39, 47.67
        assert ty.tolist() == [4, 13, 21, 30, 39, 47]


def test_make_table_is_deterministic_and_in_range():
    from multimotionfusion_amd import _capi
    lib = _capi.load()

    def make(seed, num, w, h, depth):
        out = np.zeros((num, 6), np.int32)
        assert lib.mmf_ferns_make_table(seed, num, w, h, depth, out.ctypes.data_as(C.POINTER(C.c_int))) == 0
        return out
    a, b, c = make(7, 500, 80, 60, 15000), make(7, 500, 80, 60, 15000), make(8, 500, 80, 60, 15000)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, fo.make_table(7, 500, 80, 60, 15000))
    lo, hi = a.min(axis=0), a.max(axis=0)
    assert np.all(lo >= [0, 0, 0, 0, 0, 400]) and np.all(hi <= [79, 59, 255, 255, 255, 15000])
    # ... and it uses its ranges: 500 draws reach both ends of the colour range's tenths and every column of a small image
    assert lo[2] < 26 and hi[2] > 229 and hi[5] > 13000 and lo[5] < 2000 and len(set(a[:, 0].tolist())) > 60
    one = make(1 << 63, 3, 1, 1, 400)  # degenerate ranges: one value each
    assert np.array_equal(one[:, [0, 1, 5]], [[0, 0, 400]] * 3)
    for bad in ((0, 8, 8, 5000), (5, 0, 8, 5000), (5, 8, 8, 399)):
        assert lib.mmf_ferns_make_table(1, *bad, a.ctypes.data_as(C.POINTER(C.c_int))) == -1
        assert b"mmf_ferns_make_table" in lib.mmf_last_error()


def test_defaults_and_the_refusals_that_need_no_device():
    from multimotionfusion_amd import _capi
    lib = _capi.load()
    cfg = _capi.mmf_ferns_config()
    assert lib.mmf_ferns_default_config(C.byref(cfg)) == 0
    got = {k: getattr(cfg, k) for k, _ in cfg._fields_}
    assert got == {k: (v if isinstance(v, int) else float(v)) for k, v in fo.DEFAULTS.items()}
    table = fo.make_table(0, 500, 8, 6, 15000)
    tp = table.ctypes.data_as(C.POINTER(C.c_int))
    h = C.c_void_p()

    def create(width=64, height=48, table_p=tp, **over):
        c = _capi.mmf_ferns_config()
        lib.mmf_ferns_default_config(C.byref(c))
        for k, v in over.items():
            setattr(c, k, v)
        return lib.mmf_ferns_create(None, width, height, C.byref(c), table_p, C.byref(h))
    for kw in (dict(width=7), dict(height=7), dict(num=0), dict(num=16385), dict(capacity=0), dict(max_depth_mm=399), dict(table_p=None),
               dict(threshold=float("nan"))):
        assert create(**kw) == -1, kw  # MMF_ERR_INVALID, before the (null) context is looked at
        assert b"mmf_ferns_create" in lib.mmf_last_error()
    for col, val in ((0, 8), (0, -1), (1, 6), (2, 256), (3, -1), (4, 256), (5, 399), (5, 15001)):
        bad = table.copy()
        bad[499, col] = val
        assert create(table_p=bad.ctypes.data_as(C.POINTER(C.c_int))) == -1, (col, val)
        assert b"fern 499" in lib.mmf_last_error()
    assert lib.mmf_ferns_last_launches(None) == -1


def test_the_new_names_are_exported():
    from multimotionfusion_amd import _capi
    lib = _capi.load()
    names = ["mmf_ferns_default_config", "mmf_ferns_make_table", "mmf_ferns_create", "mmf_ferns_destroy", "mmf_ferns_reset",
             "mmf_ferns_set_threshold", "mmf_ferns_process", "mmf_ferns_result", "mmf_ferns_keyframe", "mmf_ferns_download",
             "mmf_ferns_last_launches", "mmf_fusion_set_fern_database", "mmf_fusion_last_fern_result", "mmf_fusion_fern_database"]
    for n in names:
        assert n in _capi.SIGNATURES and hasattr(lib, n), n
