"""The segmentation from a frame's given label image (the `frame.mask.total() != 0` branch of
Segmentation::performSegmentation, Core/Segmentation/Segmentation.cpp:89-147) restated in numpy: the checker of
csrc/mask_kernels.hpp.

Everything integer -- the id image, the label -> id table, hasNewLabel, the label that became new, the pixel counts -- is the
reference's, statement by statement.  The depth statistics come in two variants:

  reference_float32=True   the reference's literal sums: float32, raster order (:131-144)
  reference_float32=False  DESIGN.md B7, what the device computes: the sums in float64; depth_mean = the float32 rounding of
                           the float64 quotient; every |depth_mean - d| one float32 subtraction of that rounded mean

An id the table maps a label to that is neither in `ids` nor the new label's has no entry: the reference indexes
modelIdToIndex[] uninitialised there (:98-101, :133); B7 keeps the id in the image and counts its pixels nowhere, and both
variants here do the same.
"""
import numpy as np

F32 = np.float32


def seq_sum(v):
    """float32 sum in element order (np.add.accumulate is sequential)"""
    v = np.asarray(v, F32)
    return F32(0.0) if v.size == 0 else F32(np.add.accumulate(np.concatenate([[F32(0.0)], v]), dtype=F32)[-1])


def depth_stats(d, mean=None, reference_float32=False):
    """(depth_mean, depth_std) over the float32 depths `d` of one entry, in raster order (:131-144).  `mean`: evaluate
    depth_std with this float32 mean instead of the variant's own (a device mean one ulp off moves every term)."""
    d = np.asarray(d, F32).ravel()
    n = d.size
    if n == 0:
        return F32(0.0), F32(0.0)  # (:137, :144: divided by 1, the sums are 0)
    if reference_float32:
        m = F32(seq_sum(d) / F32(n)) if mean is None else F32(mean)  # (:134, :137: float /= unsigned)
        return m, F32(seq_sum(np.abs(m - d)) / F32(n))               # (:141, :144)
    m = F32(np.sum(d, dtype=np.float64) / np.float64(n)) if mean is None else F32(mean)
    dev = np.abs(m - d)  # float32 - float32
    assert dev.dtype == F32
    return m, F32(np.sum(dev, dtype=np.float64) / np.float64(n))


def segment(labels, depth, ids, next_id, allow_new, mapping, reference_float32=False):
    """labels u8 [H][W], depth f32 [H][W], ids = model ids in list order (ids[0] == 0), mapping = the 256-entry table as
    the frame finds it (not modified).  Returns dict(mask, mapping, has_new_label, new_label, model_data)."""
    lab = np.asarray(labels, np.uint8).ravel()
    d = np.asarray(depth, F32).ravel()
    assert lab.size == d.size and ids[0] == 0
    table = np.asarray(mapping, np.uint8).reshape(256).copy()
    # :106-123 -- the only unmapped label that gets a value is the one met first (allowNew && !hasNewLabel)
    present, first = np.unique(lab, return_index=True)
    unmapped = [(int(i), int(l)) for l, i in zip(present, first) if l != 0 and table[l] == 0]
    has_new, new_label = False, -1
    if allow_new and unmapped:
        new_label = min(unmapped)[1]
        table[new_label] = next_id  # (:116)
        has_new = True
    lut = table.copy()
    lut[0] = 0  # (:108: vIn == 0 never reads the table)
    mask = lut[lab]
    counted = (lab == 0) | (mask != 0)  # (:108-122: an unmapped pixel increments nothing)
    out_ids = np.bincount(mask[counted], minlength=256)
    # :125-129
    data = [dict(id=int(i), super_pixel_count=int(out_ids[i]) // (16 * 16), avg_confidence=F32(0.4)) for i in ids]
    if has_new:
        data.append(dict(id=int(next_id), super_pixel_count=max(int(out_ids[next_id]) // (16 * 16), 1), avg_confidence=F32(0.4)))
    # :131-144 -- by the OUTPUT id: unmapped pixels are id 0's
    for e in data:
        e["depth_mean"], e["depth_std"] = depth_stats(d[mask == e["id"]], reference_float32=reference_float32)
    return dict(mask=mask.reshape(np.asarray(labels).shape), mapping=table, has_new_label=has_new, new_label=new_label,
                model_data=data)


def ulp_distance(a, b):
    """distance of two finite float32 values in units in the last place (0 for equal bits, +0 == -0)"""
    def key(x):
        i = int(np.array([x], F32).view(np.int32)[0])
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))
