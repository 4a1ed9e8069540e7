"""The reference of the batched frame preparation (csrc/prep_batch.hpp) and the crafted inputs of its tests.

`prepare` chains the oracle's per-stage functions in the reference's order (RGBDOdometry.cpp:108-235: initICPModel,
populateRGBDData, initICP, the gradient and point-cloud passes of getIncrementalTransformation; Model.cpp:359-407:
generateCUDATextures, Model::initICP) into every buffer the batched path writes, at all three levels.  The source choice
(Model.cpp:380, MultiMotionFusion.cpp:877-895) and the extents (csrc/extent.hpp) are restated in numpy, the extents from
the BUFFERS, not from the kernel's formulas.  Plain numpy on the oracle; nothing here touches a device.
"""
import numpy as np

MAX_DEPTH_RGB = 6.0  # RGBDOdometry.cpp:34
NUM_PYRS = 3
EXTENT_WORDS = 20


def level_intr(K, lvl):
    """CameraModel::operator()(level), types.cuh:94-98, in float32 as the library computes it."""
    return tuple(float(np.float32(K[k]) / np.float32(1 << lvl)) for k in ("fx", "fy", "cx", "cy"))


# ---- the source choice ---------------------------------------------------------------------------------------------
def takes_alt(sel, sel_total=0, sel_ratio=0.0):
    """Does a preparation with *sel = `sel` read the alt images?  sel None: there is no choice."""
    if sel is None:
        return False
    if sel_total:
        return bool(np.float32(sel) / np.float32(sel_total) < np.float32(sel_ratio))
    return sel != 0


def chosen(pred):
    """(vertex, normal, image) a preparation of `pred` reads."""
    if takes_alt(pred.get("sel"), pred.get("sel_total", 0), pred.get("sel_ratio", 0.0)):
        return pred["alt_vertex"], pred["alt_normal"], pred["alt_image"]
    return pred["vertex"], pred["normal"], pred["image"]


# ---- the buffers ---------------------------------------------------------------------------------------------------
def _cloud4(orc, depth, intr):
    c = orc.project_to_cloud(depth, *intr)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.concatenate([c, (np.float32(1.0) / depth)[..., None]], -1).astype(np.float32)


def _packed(vg, ng):
    rows = vg.shape[0] // 3
    return np.stack([vg[p * rows:(p + 1) * rows] for p in range(3)] + [ng[p * rows:(p + 1) * rows] for p in range(3)], -1)


def prepare_model(orc, K, pred):
    """The model side: {name: [level 0, 1, 2]} of prev_packed (vertex and normal in the global frame, an invalid vector NaN
    in x), last_depth, cloud4, last_image."""
    vertex, normal, image = chosen(pred)
    pose = np.asarray(pred["pose"], np.float32).reshape(4, 4)
    v, n = orc.copy_maps(vertex, normal)  # initICPModel
    vs, ns = [v], [n]
    for _ in range(1, NUM_PYRS):
        vs.append(orc.resize_map(vs[-1], False))
        ns.append(orc.resize_map(ns[-1], True))
    out = {"prev_packed": [], "last_depth": [], "cloud4": [], "last_image": []}
    for lvl in range(NUM_PYRS):
        vg, ng = orc.transform_maps(vs[lvl], ns[lvl], pose[:3, :3], pose[:3, 3])
        out["prev_packed"].append(_packed(vg, ng))
    d = orc.vertices_to_depth(vertex, MAX_DEPTH_RGB)  # populateRGBDData
    img = orc.image_to_intensity(image)
    for lvl in range(NUM_PYRS):
        out["last_depth"].append(d)
        out["last_image"].append(img)
        out["cloud4"].append(_cloud4(orc, d, level_intr(K, lvl)))  # getIncrementalTransformation: projectToPointCloud
        if lvl + 1 < NUM_PYRS:
            d, img = orc.pyrdown_gauss_f(d), orc.pyrdown_uchar_gauss(img)
    return out


def prepare_sensor(orc, K, depth, cutoff, rgb):
    """The sensor side: vmaps_curr, nmaps_curr, depth_pyr (level 0 is the input itself), next_image, dIdx, dIdy."""
    out = {"vmaps_curr": [], "nmaps_curr": [], "depth_pyr": [], "next_image": [], "dIdx": [], "dIdy": []}
    d, img = np.ascontiguousarray(depth, np.float32), orc.image_to_intensity(rgb)
    for lvl in range(NUM_PYRS):
        vm = orc.create_vmap(d, *level_intr(K, lvl), cutoff)
        out["vmaps_curr"].append(vm)
        out["nmaps_curr"].append(orc.create_nmap(vm))
        out["depth_pyr"].append(d)
        out["next_image"].append(img)
        dx, dy = orc.derivative_images(img)
        out["dIdx"].append(dx)
        out["dIdy"].append(dy)
        if lvl + 1 < NUM_PYRS:
            d, img = orc.pyrdown_gauss_f(d), orc.pyrdown_uchar_gauss(img)
    return out


# ---- the extents ---------------------------------------------------------------------------------------------------
def box_of(mask):
    """Inclusive bounding box (x0, y0, x1, y1) of the set pixels; None: there is none."""
    ys, xs = np.nonzero(mask)
    return None if xs.size == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def expected_extents(model_bufs, pred):
    """What the model's extent words must say, from the reference buffers: the boxes of levels 0 / 1 (valid depths in the last
    column or row) and 2 (all valid depths), and the vertices' (lo[3], hi[3]) of pixel x, pixel y, camera z."""
    out = {}
    for lvl in range(NUM_PYRS):
        ok = ~np.isnan(model_bufs["last_depth"][lvl])
        if lvl < 2:
            edge = np.zeros_like(ok)
            edge[:, -1] = edge[-1, :] = True
            ok &= edge
        out[f"depth{lvl}"] = box_of(ok)
    vertex = chosen(pred)[0]
    z = np.asarray(vertex, np.float32)[..., 2]
    ys, xs = np.nonzero(z != 0)
    if xs.size == 0:
        out["vertex"] = None
    else:
        zz = z[ys, xs]
        out["vertex"] = ((np.float32(xs.min()), np.float32(ys.min()), zz.min()), (np.float32(xs.max()), np.float32(ys.max()), zz.max()))
    return out


def expected_zmin(depth, cutoff):
    """The smallest sensor depth createVMap accepts (z != 0 && z < cutoff); None: there is none."""
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (d != 0) & (d < np.float32(cutoff))
    return d[ok].min() if ok.any() else None


def _unkey(k):
    k = int(k) & 0xFFFFFFFF
    b = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def decode_extents(words, gen):
    """The model's boxes and vertex box under generation `gen`; a word of another generation says "nothing noted"."""
    words = [int(w) for w in np.asarray(words, np.uint64)]
    assert len(words) == EXTENT_WORDS
    mine = lambda ws: all((w >> 32) == gen for w in ws)
    low = lambda w: w & 0xFFFFFFFF
    out = {}
    for lvl in range(NUM_PYRS):
        ws = words[4 * lvl:4 * lvl + 4]
        out[f"depth{lvl}"] = (0xFFFF - low(ws[0]), 0xFFFF - low(ws[2]), low(ws[1]), low(ws[3])) if gen and mine(ws) else None
    ws = words[12:18]
    out["vertex"] = (tuple(_unkey(0xFFFFFFFF - low(w)) for w in ws[:3]), tuple(_unkey(low(w)) for w in ws[3:])) if gen and mine(ws) else None
    return out


def decode_zmin(words, sensor_gen):
    """The sensor frame's smallest depth noted by sensor-side preparation number `sensor_gen` (slot gen & 1), or None."""
    w = int(np.asarray(words, np.uint64)[18 + (sensor_gen & 1)])
    return _unkey(0xFFFFFFFF - (w & 0xFFFFFFFF)) if sensor_gen and (w >> 32) == sensor_gen else None


def generations(words):
    return [int(w) >> 32 for w in np.asarray(words, np.uint64)]


# ---- crafted inputs ------------------------------------------------------------------------------------------------
def general_pose():
    from multimotionfusion_amd import synth
    return synth.make_pose((0.21, -0.34, 0.13), (0.31, -0.12, 0.47)).astype(np.float32)


def crafted_prediction(w, h, seed=0, channels=4, box=None, fill=None):
    """A prediction built by hand: {vertex, normal (h x w x 4 float32), image (h x w x channels uint8)}.

    Everywhere valid to begin with (z in [0.4, 5.6], normals within 35 degrees of -z so that no four of them average to
    zero), then: the top half empty (z == 0 with x and y left non-zero: invalid all the same) except, on its left, isolated
    texels and a checkerboard; texels beyond max_depth_rgb, exactly on it, and behind the camera (valid vertices, dropped
    depths); 2 x 2 blocks with exactly one empty texel; zeros and an all-zero region in the image.  box = (x0, y0, x1, y1):
    everything outside it is zero (what an object model's prediction looks like); fill = (x0, y0, x1, y1): so is everything
    outside THAT inside the box."""
    rng = np.random.default_rng(1000 + seed)
    v = np.zeros((h, w, 4), np.float32)
    v[..., 0] = rng.uniform(-1.5, 1.5, (h, w))
    v[..., 1] = rng.uniform(-1.0, 1.0, (h, w))
    v[..., 2] = rng.uniform(0.4, 5.6, (h, w))
    v[..., 3] = rng.uniform(0.0, 30.0, (h, w))
    n = np.zeros((h, w, 4), np.float32)
    n[..., 0] = rng.uniform(-0.45, 0.45, (h, w))
    n[..., 1] = rng.uniform(-0.45, 0.45, (h, w))
    n[..., 2] = -1.0
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    n[..., 3] = rng.uniform(0.001, 0.02, (h, w))
    img = rng.integers(1, 256, (h, w, channels), dtype=np.uint8)
    qx, qy = w // 2, h // 2
    v[:qy, :, 2] = 0.0  # the top half is empty (x and y stay non-zero), its right part without exception ...
    for k in range(6):  # ... its left part but for isolated texels
        v[(1 + 3 * k) % (qy // 2), (2 + 7 * k) % qx, 2] = 1.0 + 0.5 * k
    cb = np.indices((qy - qy // 2, qx // 2)).sum(0) % 2 == 0  # ... and a checkerboard of validity
    v[qy // 2:qy, :qx // 2, 2][cb] = 2.25
    far = [(h - 3, 1, 6.5), (h - 4, 2, 60.0), (h - 5, 3, MAX_DEPTH_RGB), (h - 6, 4, np.nextafter(np.float32(MAX_DEPTH_RGB), np.float32(10))),
           (h - 7, 5, -1.5), (h - 2, w - 2, 7.25)]
    for y, x, z in far:
        v[y, x, 2] = z
    v[h - 12:h - 8, qx + 2:qx + 8, 2] = 9.0  # a patch beyond the cut-off
    for k, (y, x) in enumerate([(qy + 2, qx + 2), (qy + 4, w - 4), (h - 2, qx + 4), (qy + 6, qx + 10)]):  # 2 x 2 blocks, one empty
        v[y + (k >> 1), x + (k & 1), 2] = 0.0
    img[rng.random((h, w)) < 0.08] = 0  # zero texels
    img[qy // 2:qy + qy // 2, qx // 2:qx + qx // 2] = 0  # all-zero 5 x 5 windows at every level
    if channels == 4:
        img[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)  # (the fourth byte takes no part)
    if box is not None:
        keep = np.zeros((h, w), bool)
        x0, y0, x1, y1 = fill if fill is not None else box
        if x1 >= x0 and y1 >= y0:
            keep[y0:y1 + 1, x0:x1 + 1] = True
        v[~keep], n[~keep], img[~keep] = 0, 0, 0
    return {"vertex": v, "normal": n, "image": img}


def alt_of(pred, seed=0):
    """Fill-in images that differ from the prediction's at EVERY pixel: validity flipped where that is possible (empty
    <-> valid), other coordinates, other normals, every intensity changed."""
    rng = np.random.default_rng(2000 + seed)
    v, n, img = pred["vertex"].copy(), pred["normal"].copy(), pred["image"].copy()
    empty = v[..., 2] == 0
    v[..., 0] += 0.25
    v[..., 1] -= 0.125
    v[..., 2] = np.where(empty, rng.uniform(0.5, 5.0, empty.shape), np.where(rng.random(empty.shape) < 0.3, 0.0, v[..., 2] * 0.75 + 0.1)).astype(np.float32)
    n[..., 0], n[..., 1] = -n[..., 1], n[..., 0]
    img[..., :3] = np.where(img[..., :3] < 128, img[..., :3] + 100, img[..., :3] - 100)
    return {"alt_vertex": v, "alt_normal": n, "alt_image": img}


def sparse_prediction(w, h, texels, channels=4, seed=0):
    """A prediction that is zero everywhere but at `texels` = [(x, y, z), ...]."""
    p = crafted_prediction(w, h, seed=seed, channels=channels)
    keep = np.zeros((h, w), bool)
    for x, y, z in texels:
        keep[y, x] = True
    for a in p.values():
        a[~keep] = 0
    for x, y, z in texels:
        p["vertex"][y, x, 2] = z
        p["image"][y, x, :3] = 200
    return p


def crafted_sensor(w, h, seed=0, channels=3, cutoff=3.0, mode="mixed"):
    """A sensor frame built by hand: {depth (float32), rgb (uint8, `channels`), cutoff}.  mode "mixed": valid depths with
    zeros, NaNs, the cut-off itself and its two neighbours, a checkerboard, an invalid quarter with isolated valid pixels;
    "edge": valid in the last column and the last row only; "none": nothing valid."""
    rng = np.random.default_rng(3000 + seed)
    c = np.float32(cutoff)
    d = rng.uniform(0.35, float(c) * 0.98, (h, w)).astype(np.float32)
    qx, qy = w // 2, h // 2
    if mode == "mixed":
        d[rng.random((h, w)) < 0.05] = 0.0
        d[rng.random((h, w)) < 0.05] = np.nan
        d[rng.random((h, w)) < 0.05] = float(c) * 1.5
        d[1, 1:4] = [c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(100))]
        d[h - 2, w - 4:w - 1] = [np.nextafter(c, np.float32(100)), c, np.nextafter(c, np.float32(0))]
        d[qy:, :qx] = np.where(np.indices((h - qy, qx)).sum(0) % 2 == 0, d[qy:, :qx], 0.0)  # checkerboard
        d[:qy, qx:] = np.nan  # an invalid quarter ...
        d[: qy // 2, qx + qx // 2:] = 0.0
        for k in range(5):  # ... with isolated valid pixels in its lower part
            d[qy // 2 + (2 + 3 * k) % (qy - qy // 2), qx + (1 + 5 * k) % qx] = 0.5 + 0.25 * k
    elif mode == "edge":
        keep = np.zeros((h, w), bool)
        keep[:, -1] = keep[-1, :] = True
        d[~keep] = 0.0
    else:
        d[:] = np.where(rng.random((h, w)) < 0.5, 0.0, np.nan)
        d[0, 0], d[h - 1, w - 1] = c, float(c) * 2
    rgb = rng.integers(1, 256, (h, w, channels), dtype=np.uint8)
    rgb[rng.random((h, w)) < 0.08] = 0
    rgb[qy // 2:qy + qy // 2, qx // 4:qx + qx // 4] = 0
    return {"depth": d, "rgb": rgb, "cutoff": float(c)}


def box_sequence(w, h):
    """The boxes (x0, y0, x1, y1; None fill = the whole box) an object model's prediction moves through: [(box, fill), ...].
    Every step that follows a non-empty one, but the step to the whole image, has a region that was non-empty before and is
    empty now."""
    return [
        ((w // 4, h // 4, w // 2, h // 2), (w // 4 + 3, h // 4 + 2, w // 2 - 5, h // 2 - 1)),  # interior, filled in part only
        ((w * 5 // 8, h * 5 // 8, w - 7, h - 5), None),                                          # disjoint from the first
        ((1, 1, 0, 0), None),                                                                    # empty
        ((w - 1, h - 1, w - 1, h - 1), None),                                                    # one pixel, the last
        ((64, 32, w - 5, 39), None),   # edges on x = 63 | 64 and on a tile edge of every level (4-row and 16-row tiles)
        ((30, 4, 63, 7), None),        # the other side of x = 63 | 64
        ((0, 0, w - 1, h - 1), None),  # the whole image
        ((5, 3, 38, 25), None),        # odd-aligned: the hulls of levels 1 and 2 depend on the reach and the shifts
        ((9, 9, 21, 14), None),        # inside the last one: what is left of it is "nothing here" now
    ]
