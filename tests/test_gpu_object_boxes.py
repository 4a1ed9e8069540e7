"""-m gpu: the object models' restricted passes (csrc/pass_rect.hpp, models_*_rect in csrc/model_host.hpp) against the passes
model by model, as test_gpu_multimodel.py::test_batched_passes_equal_passes_model_by_model compares them -- here with id
masks made by the test (surfel_shapes.py) on a static scene, so that the device-resident boxes take the values a rendered
object well inside a 320 x 240 frame never gives them: clipped at column / row 0 and at cols - 1 / rows - 1, the whole frame,
2 x 2 pixels, empty (an id absent from a frame: a stale generation, area == 0), moved (the hull of the old and the new box
must zero the old place), a frame size that is no multiple of mask_boxes_kernel's 64 x 16 tiles, more object models than
kMaxPassBatch, and a full-frame pass from outside between two restricted ones (prev_whole).  Every frame, every model: pose,
map and all eight textures bit for bit; test_oracle_surfel_shapes.py holds what the masks must make of the models."""
import numpy as np
import pytest
import torch

import surfel_shapes as sh
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu

TEXTURES = ("image", "vertexConf", "normalRadius", "time", "index", "vertConf", "colorTime", "normRad")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run(gpu_ctx, w, h, frames, masks, spawns, batch, n_models, between=None):
    """The sequence through processFrame under mmf_debug_set_pass_batch(batch): per frame (poses, maps, textures) of every
    model, and the ICP error images at the end.  between(g, i): public calls made after frame i."""
    from multimotionfusion_amd.fusion import MultiMotionFusion
    lib = gpu_ctx.lib
    K = synth.intrinsics(w, h)
    rgb, depth, ids = [dev(f["rgb"]) for f in frames], [dev(f["depth"]) for f in frames], [dev(m) for m in masks]
    lib.mmf_debug_set_pass_batch(batch)
    g = MultiMotionFusion(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, preallocated_models=n_models)
    out = []
    try:
        for i in range(len(frames)):
            g.processFrame(rgb[i], depth[i], timestamp=i, mask=ids[i], hasNewLabel=spawns[i])
            torch.cuda.synchronize()
            models = g.getModels()

            def tex_of(m, n):  # (the index-map getters copy on the MODEL's stream: wait for the device before reading)
                t = m.texture(n)
                torch.cuda.synchronize()
                return t.cpu().numpy().copy()
            out.append(([m.getPose() for m in models], [m.downloadMap() for m in models], [[tex_of(m, n) for n in TEXTURES] for m in models]))
            if between is not None:
                between(g, i)
                torch.cuda.synchronize()
        err = [g.getErrorTexture(k, "icp").cpu().numpy().copy() for k in range(len(g.getModels()))]
    finally:
        g.close()
        lib.mmf_debug_set_pass_batch(-1)
    return out, err


def assert_same_run(ref, got, mode):
    (fa, ea), (fb, eb) = ref, got
    assert len(fa) == len(fb)
    for i, ((pa, ma, ta), (pb, mb, tb)) in enumerate(zip(fa, fb)):
        assert len(pa) == len(pb), (mode, i)
        for k in range(len(pa)):
            assert np.array_equal(raw(pa[k]), raw(pb[k])), (mode, i, k, "pose")
            assert ma[k].shape == mb[k].shape and np.array_equal(raw(ma[k]), raw(mb[k])), (mode, i, k, "map", ma[k].shape, mb[k].shape)
            for n, x, y in zip(TEXTURES, ta[k], tb[k]):
                ne = raw(x) != raw(y)
                assert not ne.any(), (mode, i, k, n, int(ne.sum()), np.argwhere(ne.reshape(x.shape[0], x.shape[1], -1).any(axis=2))[:4].tolist())
    assert len(ea) == len(eb)
    for k, (x, y) in enumerate(zip(ea, eb)):
        assert np.array_equal(raw(x), raw(y)), (mode, k, "icp error image")


def full_frame_passes_from_outside(g, i):
    """After frame 6: a full-frame predictIndices / combinedPredict from a pose 0.2 m to the side, through the public
    wrappers, then the pose back.  They leave non-zero texels where none of the model's boxes is; the next frame's
    restricted resolves must clear them (prev_whole: a full-frame pass drops idx_nz_known / spl_nz_known).  On model 2,
    shifted along x -- and on model 1 along -y: model 2 fills the frame by now, so its restricted resolves walk all of it
    anyway, while model 1's two places span the frame's width but only its top rows, below which the shifted passes draw."""
    if i != 6:
        return
    tick = g.getTick()
    for k, axis, step in ((2, 0, 0.2), (1, 1, -0.2)):
        m = g.getModels()[k]
        assert m.id == k
        pose = m.getPose()
        aside = pose.copy()
        aside[axis, 3] += np.float32(step)
        m.overridePose(aside)
        m.predictIndices(tick, sh.MAXD, sh.TIME_DELTA)
        m.combinedPredict(sh.MAXD, tick, tick, sh.TIME_DELTA)
        m.overridePose(pose)


@pytest.mark.parametrize("w,h", sh.EDGE_SHAPES)
def test_boxes_at_the_image_edges(gpu_ctx, w, h):
    """surfel_shapes.edge_masks: boxes clipped on every image side, a 2 x 2 box, a full-width band, ids absent from a frame,
    an id that comes back elsewhere while another takes the whole frame, full-frame passes from outside after frame 6."""
    masks, spawns = sh.edge_masks(w, h)
    frames = sh.static_frames(w, h, sh.EDGE_FRAMES)
    ref = run(gpu_ctx, w, h, frames, masks, spawns, 0, 4, full_frame_passes_from_outside)
    assert [len(f[0]) for f in ref[0]] == [1, 2, 3, 4, 5, 5, 5, 5, 5]
    last = ref[0][-1][1]
    assert all(m.shape[0] > 0 for m in last) and last[3].shape[0] <= 8, [m.shape[0] for m in last]
    for mode in (2, -1):
        assert_same_run(ref, run(gpu_ctx, w, h, frames, masks, spawns, mode, 4, full_frame_passes_from_outside), mode)


def test_more_objects_than_a_batch_holds(gpu_ctx):
    """Eight object models: seven share the restricted launches, the eighth is predicted and fused on its own stream."""
    w, h = sh.GRID_SHAPE
    masks, spawns = sh.grid_masks()
    frames = sh.static_frames(w, h, sh.GRID_FRAMES)
    ref = run(gpu_ctx, w, h, frames, masks, spawns, 0, 8)
    assert len(ref[0][-1][0]) == 9 and all(m.shape[0] > 300 for m in ref[0][-1][1][1:]), [m.shape[0] for m in ref[0][-1][1]]
    for mode in (2, -1):
        assert_same_run(ref, run(gpu_ctx, w, h, frames, masks, spawns, mode, 8), mode)
