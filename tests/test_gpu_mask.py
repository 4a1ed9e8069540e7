"""-m gpu: the segmentation from a frame's given label image (mmf_mask_segment, csrc/mask_kernels.hpp) against
tests/mask_oracle.py, the numpy restatement of Segmentation.cpp:89-147.

Bit-exact: the id image, the label -> id table, has_new_label, the label that became new, every super_pixel_count.
depth_mean: within 1 float32 ulp of the oracle's (both are float32 roundings of float64 sums of the same float32 values in
different orders: a float64 sum of n <= 2^19 terms is off by < n 2^-53 relative, eleven orders below half a float32 ulp, so
only a rounding tie can move).  depth_std: within 1 ulp of the oracle's formula evaluated with the DEVICE's depth_mean -- a
mean one ulp off moves every term.  Two runs on one input give the same bits.

Sizes: 5x3 (less than one workgroup), 37x29 (an odd pixel count), 161x121 (several workgroups of 4096 pixels and a ragged
tail), 640x480 once."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_oracle as mo
from multimotionfusion_amd import segmentation
from multimotionfusion_amd._capi import MmfError, mmf_segmentation_model
from multimotionfusion_amd.cudafuncs import _p

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = [(5, 3), (37, 29), (161, 121)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def depth_image(rng, w, h):
    """metric depth with zero (invalid) patches and single zero pixels"""
    d = rng.uniform(0.3, 6.0, (h, w)).astype(F32)
    d[rng.random((h, w)) < 0.05] = 0
    d[h // 3:h // 3 + max(h // 5, 1), w // 4:w // 4 + max(w // 3, 1)] = 0
    return d


def device_run(ctx, lab, depth, ids, next_id, allow_new, mapping, misalign=False):
    if misalign:  # images that start one element into their buffers: the kernels' scalar-load form
        lb, db = torch.zeros(lab.size + 1, dtype=torch.uint8).cuda(), torch.zeros(lab.size + 1, dtype=torch.float32).cuda()
        lb[1:] = dev(lab).ravel()
        db[1:] = dev(depth).ravel()
        tl, td = lb[1:].view(lab.shape), db[1:].view(lab.shape)
        assert tl.data_ptr() % 4 == 1 and td.data_ptr() % 16 == 4
    else:
        tl, td = dev(lab), dev(depth)
    mask, data, has_new, new_label, table = segmentation.mask_segment(ctx, tl, td, ids, next_id, allow_new, mapping)
    return dict(mask=mask.cpu().numpy(), model_data=data, has_new_label=has_new, new_label=new_label, mapping=table)


def check(ctx, lab, depth, ids, next_id, allow_new, mapping, misalign=False):
    before = np.array(mapping, np.uint8).copy()
    got = device_run(ctx, lab, depth, ids, next_id, allow_new, mapping, misalign)
    again = device_run(ctx, lab, depth, ids, next_id, allow_new, mapping, misalign)
    assert np.array_equal(before, np.asarray(mapping, np.uint8)), "the caller's table is the mirror's input only"
    exp = mo.segment(lab, depth, ids, next_id, allow_new, mapping)
    assert np.array_equal(got["mask"], exp["mask"])
    assert np.array_equal(got["mapping"], exp["mapping"])
    assert got["has_new_label"] == exp["has_new_label"] and got["new_label"] == exp["new_label"]
    assert [e["id"] for e in got["model_data"]] == [e["id"] for e in exp["model_data"]]
    d = np.asarray(depth, F32).ravel()
    for g, e, a in zip(got["model_data"], exp["model_data"], again["model_data"]):
        assert g["super_pixel_count"] == e["super_pixel_count"], (g, e)
        assert F32(g["avg_confidence"]) == F32(0.4)
        gm, gs = F32(g["depth_mean"]), F32(g["depth_std"])
        um = mo.ulp_distance(gm, e["depth_mean"])
        std_at_device_mean = mo.depth_stats(d[exp["mask"].ravel() == e["id"]], mean=gm)[1]
        us = mo.ulp_distance(gs, std_at_device_mean)
        assert um <= 1, (g, e, um)
        assert us <= 1, (g, e, std_at_device_mean, us)
        assert gm.tobytes() == F32(a["depth_mean"]).tobytes() and gs.tobytes() == F32(a["depth_std"]).tobytes(), "run to run"
    assert np.array_equal(got["mask"], again["mask"]) and np.array_equal(got["mapping"], again["mapping"])
    return got


@pytest.mark.parametrize("w,h,allow_new", [(w, h, a) for w, h in SMALL for a in (0, 1)] + [(640, 480, 1)])
def test_every_label_some_mapped(gpu_ctx, w, h, allow_new):
    """all 255 non-zero labels where the image has room for them (every label the 15 pixels of 5x3 can hold there), a third
    of them mapped: to models of the list, two labels to one id, and one to an id that is in no list"""
    rng = np.random.default_rng(w * 1000 + h)
    n = w * h
    lab = rng.integers(0, 256, n).astype(np.uint8)
    if n >= 512:
        lab[rng.permutation(n)[:255]] = np.arange(1, 256)  # every label at least once
        assert len(np.unique(lab)) == 256
    lab = lab.reshape(h, w)
    ids = [0, 1, 2, 5, 9]
    mapping = np.zeros(256, np.uint8)
    mapped = rng.permutation(np.arange(1, 256))[:85]
    mapping[mapped] = rng.choice(ids[1:], 85)
    mapping[mapped[0]] = mapping[mapped[1]] = 2  # two labels on one id
    mapping[mapped[2]] = 7                       # a model that has left the list
    mapping[int(lab.ravel()[n // 2]) or 1] = 9   # (a mapped label that certainly is in the image)
    got = check(gpu_ctx, lab, depth_image(rng, w, h), ids, 11, allow_new, mapping)
    unmapped_present = [l for l in np.unique(lab) if l != 0 and mapping[l] == 0]
    assert got["has_new_label"] == bool(allow_new and unmapped_present)
    check(gpu_ctx, lab, depth_image(rng, w, h), ids, 11, allow_new, mapping, misalign=True)


@pytest.mark.parametrize("w,h", SMALL)
def test_raster_first_of_two_unmapped_labels(gpu_ctx, w, h):
    """two unmapped labels whose first pixels sit at every pair of positions from {0, 1, 63, 64, 255, 256, 1023, 1024, n - 1}
    the image has: the earlier one is a single pixel, the later one owns every free pixel behind its first (more pixels than
    the earlier one, except where its first pixel is the image's last).  The smaller label number is the LATER one in half
    of the pairs, so that neither the size nor the label's number can stand in for the raster order."""
    rng = np.random.default_rng(7)
    n = w * h
    pos = [p for p in (0, 1, 63, 64, 255, 256, 1023, 1024, n - 1) if p < n]
    pos = sorted(set(pos))
    depth = depth_image(rng, w, h)
    base = np.zeros(n, np.uint8)
    base[rng.random(n) < 0.2] = 3  # model 1's label, anywhere
    k = 0
    for i, p in enumerate(pos):
        for q in pos[i + 1:]:
            early, late = (200, 40) if k % 2 == 0 else (40, 200)
            k += 1
            lab = base.copy()
            lab[q:][lab[q:] == 0] = late
            lab[q] = late
            lab[p] = early
            if q < n - 1:
                assert (lab == late).sum() > (lab == early).sum() == 1
            mapping = np.zeros(256, np.uint8)
            mapping[3] = 1
            for allow_new in (1, 0):
                got = check(gpu_ctx, lab.reshape(h, w), depth, [0, 1], 2, allow_new, mapping)
                assert got["new_label"] == (early if allow_new else -1), (p, q)
                assert got["mapping"][late] == 0
    assert k == len(pos) * (len(pos) - 1) // 2 and k >= (3 if n < 64 else 10)


@pytest.mark.parametrize("w,h", SMALL[1:])
def test_255_and_256_pixels(gpu_ctx, w, h):
    """a model with 255 pixels has no super-pixel (it counts as unseen), one with 256 has one; a new label of one pixel has one"""
    rng = np.random.default_rng(11)
    n = w * h
    lab = np.zeros(n, np.uint8)
    where = rng.permutation(n)
    lab[where[:255]] = 21
    lab[where[255:511]] = 22
    lab[where[511]] = 23
    mapping = np.zeros(256, np.uint8)
    mapping[21], mapping[22] = 1, 2
    got = check(gpu_ctx, lab.reshape(h, w), depth_image(rng, w, h), [0, 1, 2], 3, 1, mapping)
    assert [e["super_pixel_count"] for e in got["model_data"]] == [(n - 512) // 256, 0, 1, 1]
    assert got["new_label"] == 23 and got["model_data"][3]["id"] == 3


@pytest.mark.parametrize("w,h", SMALL)
def test_one_label_only(gpu_ctx, w, h):
    rng = np.random.default_rng(13)
    depth = depth_image(rng, w, h)
    zeros = np.zeros(256, np.uint8)
    mapped = zeros.copy()
    mapped[77] = 4
    full = np.full((h, w), 77, np.uint8)
    got = check(gpu_ctx, np.zeros((h, w), np.uint8), depth, [0, 4], 5, 1, mapped)  # background only
    assert not got["has_new_label"] and got["model_data"][1]["depth_mean"] == 0 and got["model_data"][1]["depth_std"] == 0
    got = check(gpu_ctx, full, depth, [0, 4], 5, 1, mapped)  # one mapped label: id 0 has no pixel
    assert (got["mask"] == 4).all() and got["model_data"][0]["depth_mean"] == 0
    got = check(gpu_ctx, full, depth, [0], 1, 1, zeros)  # one unmapped label becomes new
    assert got["has_new_label"] and (got["mask"] == 1).all() and got["model_data"][1]["super_pixel_count"] == max(w * h // 256, 1)
    got = check(gpu_ctx, full, depth, [0], 1, 0, zeros)  # ... or stays unmapped: id 0's statistics, nobody's count
    assert (got["mask"] == 0).all() and got["model_data"][0]["super_pixel_count"] == 0 and got["model_data"][0]["depth_mean"] > 0
    got = check(gpu_ctx, full, np.zeros((h, w), F32), [0], 1, 1, zeros)  # all depth invalid
    assert got["model_data"][1]["depth_mean"] == 0 and got["model_data"][1]["depth_std"] == 0


def test_label_mapped_to_next_id_without_a_spawn(gpu_ctx):
    """the table entry of an inhibited or cancelled spawn: the label keeps next_id in the image and, with no new label in
    this frame, enters no entry; when another label becomes new in the same frame both share the new entry"""
    rng = np.random.default_rng(17)
    w, h = 37, 29
    lab = rng.choice(np.array([0, 0, 0, 50, 60], np.uint8), (h, w))
    mapping = np.zeros(256, np.uint8)
    mapping[50] = 2
    depth = depth_image(rng, w, h)
    got = check(gpu_ctx, lab, depth, [0, 1], 2, 0, mapping)
    assert len(got["model_data"]) == 2 and (got["mask"][lab == 50] == 2).all() and (got["mask"][lab == 60] == 0).all()
    got = check(gpu_ctx, lab, depth, [0, 1], 2, 1, mapping)
    assert got["new_label"] == 60 and got["model_data"][2]["super_pixel_count"] == ((lab == 50) | (lab == 60)).sum() // 256


def test_error_returns(gpu_ctx):
    w, h = 8, 4
    lab, depth = dev(np.zeros((h, w), np.uint8)), dev(np.ones((h, w), F32))
    zeros = np.zeros(256, np.uint8)

    def refused(ids, next_id):
        with pytest.raises(MmfError) as e:
            segmentation.mask_segment(gpu_ctx, lab, depth, ids, next_id, 1, zeros)
        assert e.value.status == -1  # MMF_ERR_INVALID

    refused([1, 0], 2)                # the list starts with the global model
    refused([0, 300], 2)              # an id the image cannot hold
    refused([0, 1], 256)              # a new id the image cannot hold
    refused(list(range(256)), 255)    # more than 255 models
    refused([0, 1, 1], 2)             # the same model twice
    refused([0, 1], 1)                # the new label's id is a model's
    # mask_out overlapping the label image
    lib = gpu_ctx.lib
    ids = (C.c_uint * 1)(0)
    out = (mmf_segmentation_model * 2)()
    n_out, has_new, new_label = C.c_int(), C.c_int(), C.c_int()
    big = dev(np.zeros(2 * w * h, np.uint8))
    for off in (0, w * h - 1):
        rc = lib.mmf_mask_segment(gpu_ctx.handle, w, h, _p(big), _p(depth), ids, 1, 1, 1, zeros.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  big.data_ptr() + off, out, C.byref(n_out), C.byref(has_new), C.byref(new_label))
        assert rc == -1 and b"overlaps" in lib.mmf_last_error()
    rc = lib.mmf_mask_segment(gpu_ctx.handle, w, h, _p(big), _p(depth), ids, 1, 1, 1, zeros.ctypes.data_as(C.POINTER(C.c_uint8)),
                              big.data_ptr() + w * h, out, C.byref(n_out), C.byref(has_new), C.byref(new_label))
    assert rc == 0 and n_out.value == 1 and new_label.value == -1
    # a refused call leaves the next one intact
    got = check(gpu_ctx, np.full((h, w), 9, np.uint8), np.ones((h, w), F32), [0], 1, 1, zeros)
    assert got["new_label"] == 9
