"""Inputs and loops shared by the surfel-path shape tests: test_gpu_surfel.py / test_gpu_surfel_shapes.py /
test_gpu_object_boxes.py run them on the device, test_oracle_surfel_shapes.py asserts on the oracle alone that they exercise
what those tests were written for (a device comparison on a degenerate input proves nothing)."""
import numpy as np
import pytest

from helpers import assert_bit_equal
from multimotionfusion_amd import synth

MAXD = 20.0      # maxDepthProcessed
CUTOFF = 15.0    # depthCutoff of the bilateral filter (GUI default)
TIME_DELTA = 200
CONF = 10.0      # confGlobalInit

# ---- A1: the depth filter ------------------------------------------------------------------------------------------------
FILTER_SHAPES = [(33, 17), (131, 9), (262, 8), (264, 8), (390, 6), (392, 6), (13, 13), (2, 1), (1, 1)]


def filter_input(w, h):
    """A rendered depth image cropped to w x h with a few pixels invalid (0), below the filter's 0.3 m floor (0.2) and above
    its cut-off (16.0 > CUTOFF).  No NaN: payload bits are no contract."""
    f = synth.render(np.eye(4), max(w, 32), max(h, 32), seed=3, depth_noise=1e-3)
    d = np.ascontiguousarray(f["depth"][:h, :w]).copy()
    rng = np.random.default_rng(1000 * w + h)
    k = min(3, d.size // 4)
    if k:
        at = rng.choice(d.size, 3 * k, replace=False)
        for j, val in enumerate((0.0, 0.2, 16.0)):
            d.reshape(-1)[at[j * k:(j + 1) * k]] = val
    elif d.size == 2:
        d[0, 1] = 0.2  # the two-pixel kernel with one of its two pixels skipped
    return d


# ---- A2: the surfel cycle ------------------------------------------------------------------------------------------------
CYCLE_SHAPES = [(32, 32), (36, 44), (100, 52), (52, 100), (132, 76), (268, 36)]


@pytest.fixture
def splat_bound(gpu_ctx, request):
    """combinedPredict's early depth test (splat_kernel<true>: the key image is read before a fragment is evaluated): -1 = by the surfel count, 1 = always"""
    gpu_ctx.lib.mmf_debug_set_splat_bound(request.param)
    yield request.param
    gpu_ctx.lib.mmf_debug_set_splat_bound(-1)


def surfel_cycle(orc, w, h, gpu_ctx=None, stats=None):
    """initialise -> (predictIndices, fuse, predictIndices, clean, combinedPredict, fill-in) x 3 frames on the oracle; with a
    device context the same passes on a Model, every output compared bit for bit.  stats (a dict): what the oracle saw."""
    K = synth.intrinsics(w, h)
    poses = synth.trajectory(4, seed=5)
    frames = [synth.render(p, w, h, seed=i) for i, p in enumerate(poses)]
    mask = np.zeros((h, w), np.uint8)
    m = None
    if gpu_ctx is not None:
        import torch
        from multimotionfusion_amd.model import Model, filterDepth
        m = Model(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], 0, CONF)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d_mask = dev(mask)

    def tex_is(name, want, what, view=None):
        if m is not None:
            got = m.texture(name).cpu().numpy()
            assert_bit_equal(got.view(view) if view is not None else got, want, what)

    def map_is(want, what):
        if m is not None:
            assert_bit_equal(m.downloadMap(), want, what)

    st = stats if stats is not None else {}
    st.update(merged=[], new=[], cover=[], fill_low=[], fill_conf=[])

    f0 = frames[0]
    fil0 = orc.bilateral_filter(f0["depth"], CUTOFF)
    s = orc.surfel_initialise(f0["rgb"], f0["depth"], fil0, K, 1, MAXD)
    st["first"] = s.shape[0]
    if m is not None:
        d_fil0 = filterDepth(gpu_ctx, dev(f0["depth"]), CUTOFF)
        m.overridePose(poses[0])
        m.initialise(dev(f0["rgb"]), dev(f0["depth"]), d_fil0, 1, MAXD)
        assert m.lastCount() == s.shape[0] > 0.8 * w * h
    map_is(s, "initialise")

    for t in range(1, 4):
        tick = t + 1
        f = frames[t]
        pose = poses[t].astype(np.float32)  # ground-truth pose stands in for the tracker here
        fil = orc.bilateral_filter(f["depth"], CUTOFF)
        if m is not None:
            d_rgb, d_raw = dev(f["rgb"]), dev(f["depth"])
            d_fil = filterDepth(gpu_ctx, d_raw, CUTOFF)
            m.overridePose(pose)
            m.predictIndices(tick, MAXD, TIME_DELTA)
        index, vc, ct, nr = orc.predict_indices(s, pose, K, w, h, MAXD, tick, TIME_DELTA)
        tex_is("index", index, f"index map t={t}", np.uint32)
        tex_is("vertConf", vc, f"vertConf t={t}")
        tex_is("colorTime", ct, f"colorTime t={t}")
        tex_is("normRad", nr, f"normRad t={t}")

        if m is not None:
            m.fuse(tick, d_rgb, d_mask, d_raw, d_fil, MAXD, 1.0)
        s_upd, new = orc.fuse(s, f["rgb"], f["depth"], fil, mask, index, vc, nr, pose, K, tick, 1.0, 0, MAXD)
        map_is(s_upd, f"fused surfels t={t}")
        st["merged"].append(int((s_upd.view(np.uint32) != s.view(np.uint32)).any(axis=1).sum()))
        st["new"].append(new.shape[0])

        if m is not None:
            m.predictIndices(tick, MAXD, TIME_DELTA)
        index, vc, ct, nr = orc.predict_indices(s_upd, pose, K, w, h, MAXD, tick, TIME_DELTA)
        tex_is("index", index, f"index map after fuse t={t}", np.uint32)

        if m is not None:
            m.clean(tick, TIME_DELTA, MAXD, d_fil, d_mask, 3.0)
        s = orc.clean(s_upd, new, pose, K, w, h, tick, TIME_DELTA, CONF, 3.0, 0, index, vc, ct, fil, mask)
        if m is not None:
            assert m.lastCount() == s.shape[0]
        map_is(s, f"cleaned surfels t={t}")

        # at confGlobalInit nothing is stable yet after three frames and the splat below draws nothing: a leg with the
        # model's threshold at 0.5 draws the sprites of most of the map (same pass, same threshold on both sides)
        if m is not None:
            m.setConfidenceThreshold(0.5)
            m.combinedPredict(MAXD, tick, tick, TIME_DELTA)
            m.setConfidenceThreshold(CONF)
        image, vcp, nrp, tm = orc.combined_predict(s, pose, K, w, h, MAXD, 0.5, tick, tick, TIME_DELTA)
        st["cover"].append(float((vcp[..., 2] > 0).mean()))
        st["fill_low"].append(orc.requires_fill_in(image, 0.75))
        assert (vcp[..., 2] > 0).mean() > 0.5, (t, float((vcp[..., 2] > 0).mean()))
        tex_is("image", image, f"splat image t={t} conf=0.5")
        tex_is("vertexConf", vcp, f"splat vertexConf t={t} conf=0.5")
        tex_is("normalRadius", nrp, f"splat normalRadius t={t} conf=0.5")
        tex_is("time", tm, f"splat time t={t} conf=0.5", np.uint16)
        if m is not None:  # the thumbnail count on the "enough is drawn" side of the decision
            assert m.requiresFillIn(0.75) == orc.requires_fill_in(image, 0.75)

        if m is not None:
            m.combinedPredict(MAXD, tick, tick, TIME_DELTA)
        image, vcp, nrp, tm = orc.combined_predict(s, pose, K, w, h, MAXD, CONF, tick, tick, TIME_DELTA)
        st["fill_conf"].append(orc.requires_fill_in(image, 0.75))
        tex_is("image", image, f"splat image t={t}")
        tex_is("vertexConf", vcp, f"splat vertexConf t={t}")
        tex_is("normalRadius", nrp, f"splat normalRadius t={t}")
        tex_is("time", tm, f"splat time t={t}", np.uint16)
        # ModelProjection::synthesizeDepth: the same sprites, depth only, explicit confidence threshold
        if m is not None:
            for conf in (CONF, 0.5):
                m.synthesizeDepth(MAXD, conf, tick, tick, TIME_DELTA)
                sd = orc.synthesize_depth(s, pose, K, w, h, MAXD, conf, tick, tick, TIME_DELTA)
                assert_bit_equal(m.texture("depth").cpu().numpy(), sd, f"synthesized depth t={t} conf={conf}")

            m.performFillIn(d_rgb, d_fil, False, False)
            vo, no, io = orc.fill_in(vcp, nrp, image, fil, f["rgb"], K, 0, 0)
            assert_bit_equal(m.texture("fillVertex").cpu().numpy(), vo, f"fill vertex t={t}")
            assert_bit_equal(m.texture("fillNormal").cpu().numpy(), no, f"fill normal t={t}")
            assert_bit_equal(m.texture("fillImage").cpu().numpy(), io, f"fill image t={t}")
            assert m.requiresFillIn(0.75) == orc.requires_fill_in(image, 0.75)
    if m is not None:
        m.close()
    return st


# ---- A3: sprite extremes -------------------------------------------------------------------------------------------------
SPRITE_SHAPES = [(36, 44), (132, 76), (640, 480)]
SPRITE_TICK = 2
COVERING = ((0.5, 0.3), (0.6, 0.3), (1.0, 0.6))  # (z, radius) of the frame-covering sprites
NEAR = 0.07  # every sprite corner stays this far in front of the camera: z - 1.4143 radius >= NEAR (behind it the sprite
#              size leaves the int range, and the (int)ceilf(...) the oracle shares with the kernel is undefined)


def sprite_store(w, h, seed=11):
    """(surfels [n, 12], rows of the frame-covering sprites): a hand-made store for the identity pose -- radii over 3.5
    decades at random pixels, three sprites larger than the frame, centres on pixel-grid lines and on the image borders,
    tilted and zero normals; all with confidence 20, shuffled.

    The covering sprites sit on the ray through the image centre.  The second one faces the camera squarely only where that
    is enough: a sprite is a SQUARE of 2 sqrt(2) fx radius / z = 1.414 w * 528 / 640 = 1.167 w pixels around its centre,
    which covers a frame as long as h <= 1.167 w.  At 36 x 44 it does not (42 < 44), so there the sprite is tilted by 30
    degrees about the x axis towards the side the principal point is off-centre on: the nearer corner's perspective then
    widens the sprite (48 pixels)."""
    K = synth.intrinsics(w, h)
    fx, fy, cx, cy = K["fx"], K["fy"], K["cx"], K["cy"]
    rng = np.random.default_rng(seed)
    rows = []

    def add(u, v, z, r, n=(0.0, 0.0, -1.0)):
        assert z - 1.4143 * r >= NEAR, (z, r)
        rows.append([(u - cx) / fx * z, (v - cy) / fy * z, z, 20.0, float(rng.integers(1, 1 << 24)), 0.0, 1.0, 1.0, n[0], n[1], n[2], r])

    for r in np.geomspace(1e-4, 0.3, 240):
        add(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(NEAR + 0.01 + 1.4143 * r, 3.0), r)
    first_covering = len(rows)
    for k, (z, r) in enumerate(COVERING):
        n = (0.0, 0.0, -1.0)
        if k == 1 and h > 2.0 * np.sqrt(2.0) * fx * r / z:
            a = np.deg2rad(30.0) * (-1.0 if h / 2.0 > cy else 1.0)
            n = (0.0, float(np.sin(a)), float(-np.cos(a)))
        add(w / 2.0, h / 2.0, z, r, n)
    for r in (0.002, 0.05):
        for u, v in ((0, 0), (w, h), (0, h), (w, 0), (w / 2, 0), (0, h / 2), (w, h / 2), (w / 2, h), (1, 1), (w - 1, h - 1), (16, 16),
                     (17, 23), (15.5, 15.5)):
            add(u, v, 1.5, r)
    for _ in range(12):  # tilted by 20 to 70 degrees, in any direction
        th, ph = np.deg2rad(rng.uniform(20, 70)), rng.uniform(0, 2 * np.pi)
        add(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.5, 3.0), rng.uniform(0.01, 0.1),
            (float(np.sin(th) * np.cos(ph)), float(np.sin(th) * np.sin(ph)), float(-np.cos(th))))
    for _ in range(4):  # a zero normal normalises to NaN: its fragments win every depth test
        add(rng.uniform(2, w - 2), rng.uniform(2, h - 2), rng.uniform(1.0, 2.5), rng.uniform(0.02, 0.05), (0.0, 0.0, 0.0))
    s = np.array(rows, np.float64).astype(np.float32)
    order = rng.permutation(s.shape[0])
    covering = [int(np.nonzero(order == first_covering + k)[0][0]) for k in range(len(COVERING))]
    return s[order], covering


def sprite_box(surfel, K, w, h):
    """The clipped bounding box (x0, y0, x1, y1, inclusive) of a surfel's point sprite at the identity pose: splat.vert as
    orc_combined_predict states it (mmf_oracle_surfel.c), in float32."""
    f = np.float32
    p, n, rad = surfel[:3].astype(f), surfel[8:11].astype(f), f(surfel[11])
    fx, fy, cx, cy = f(K["fx"]), f(K["fy"]), f(K["cx"]), f(K["cy"])
    n = n / np.sqrt((n * n).sum(dtype=f))
    a = np.array([n[1] - n[2], -n[0], n[0]], f)
    x1 = a / np.sqrt((a * a).sum(dtype=f)) * rad * f(1.41421356)
    y1 = np.cross(n, x1).astype(f)
    px, py = [], []
    for q in (p + x1, p + y1, p - y1, p - x1):
        px.append(fx * q[0] / q[2] + cx)
        py.append(fy * q[1] / q[2] + cy)
    size = max(f(0), abs(max(px) - min(px)), abs(max(py) - min(py)))
    size = size if size >= 1 else f(1)
    hw, hh, hs = f(w * 0.5), f(h * 0.5), f(size * f(0.5))
    xn, yn = ((fx * p[0] / p[2] + cx) - hw) / hw, ((fy * p[1] / p[2] + cy) - hh) / hh
    assert -1 <= xn <= 1 and -1 <= yn <= 1
    xw, yw = (xn + f(1)) * hw, (yn + f(1)) * hh
    x0, x1i = int(np.ceil(xw - hs - f(0.5))), int(np.ceil(xw + hs - f(0.5))) - 1
    y0, y1i = int(np.ceil(yw - hs - f(0.5))), int(np.ceil(yw + hs - f(0.5))) - 1
    return max(x0, 0), max(y0, 0), min(x1i, w - 1), min(y1i, h - 1)


# ---- B: object boxes -----------------------------------------------------------------------------------------------------
def static_frames(w, h, n):
    """A static scene (no rendered objects): the id masks come from the box generators below."""
    return [synth.render(p, w, h, seed=i) for i, p in enumerate(synth.trajectory(n, seed=39))]


def paint(w, h, boxes):
    """An id image from {id: (x0, y0, x1, y1) inclusive}; lower ids win where boxes overlap."""
    mask = np.zeros((h, w), np.uint8)
    for i in sorted(boxes, reverse=True):
        x0, y0, x1, y1 = boxes[i]
        mask[y0:y1 + 1, x0:x1 + 1] = i
    return mask


EDGE_SHAPES = [(100, 68), (320, 240)]
EDGE_FRAMES = 9


def edge_masks(w, h):
    """(masks, spawns) of nine frames: boxes clipped at column / row 0 (id 1) and at cols - 1 / rows - 1 (id 2), a 2 x 2
    box (id 3), a full-width band (id 4), one id spawned per frame from frame 1 on; frame 5 without ids 1 and 3; frame 6
    with id 1 elsewhere (the top-right corner) and id 2 on all the rest of the frame, nothing background; then frame 4's
    masks again."""
    home = {1: (0, 0, w // 3, h // 3), 2: (w - w // 3, h - h // 3, w - 1, h - 1), 3: (w // 2 - 1, h // 2 - 1, w // 2, h // 2),
            4: (0, h // 2, w - 1, h // 2 + 5)}
    masks = []
    for i in range(EDGE_FRAMES):
        if i == 5:
            boxes = {k: home[k] for k in (2, 4)}
        elif i == 6:
            boxes = {1: (w - w // 4, 0, w - 1, h // 4), 2: (0, 0, w - 1, h - 1)}
        else:
            boxes = {k: home[k] for k in home if k <= i}
        masks.append(paint(w, h, boxes))
    return masks, [1 <= i <= 4 for i in range(EDGE_FRAMES)]


GRID_SHAPE = (160, 120)
GRID_FRAMES = 11


def grid_masks():
    """(masks, spawns) of eleven 160 x 120 frames: ids 1 to 8 on a 4 x 2 grid, one spawned per frame from frame 1 on -- one
    object model more than a batch of restricted passes holds (kMaxPassBatch = 7)."""
    w, h = GRID_SHAPE
    boxes = {}
    for k in range(1, 9):
        c, r = (k - 1) % 4, (k - 1) // 4
        boxes[k] = (c * 40 + 4, r * 60 + 6, c * 40 + 35, r * 60 + 53)
    masks = [paint(w, h, {k: b for k, b in boxes.items() if k <= i}) for i in range(GRID_FRAMES)]
    return masks, [1 <= i <= 8 for i in range(GRID_FRAMES)]
