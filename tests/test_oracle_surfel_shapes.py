"""CPU: the inputs of the surfel-path shape tests (test_gpu_surfel_shapes.py, test_gpu_object_boxes.py) exercise what those
tests were written for -- asserted on the oracle alone, with the generators the device tests use (surfel_shapes.py).  The
conditions are looser than what the oracle gives (quoted per test)."""
import numpy as np
import pytest

import surfel_shapes as sh
from helpers import OracleFusion
from multimotionfusion_amd import synth


@pytest.mark.parametrize("w,h", sh.FILTER_SHAPES)
def test_filter_inputs_hold_every_kind_of_pixel(w, h):
    d = sh.filter_input(w, h)
    assert d.shape == (h, w) and d.dtype == np.float32 and np.isfinite(d).all()
    assert ((d >= 0.3) & (d <= sh.CUTOFF)).any()
    if w * h >= 4:
        assert (d == 0).any() and (d == np.float32(0.2)).any() and (d == 16.0).any()


@pytest.mark.parametrize("w,h", sh.CYCLE_SHAPES)
def test_surfel_cycle_inputs_fuse_add_and_draw(orc, w, h):
    """Measured: first frame 0.97 to 1.0 wh surfels; 0.22 to 0.23 wh merged per fused frame (the shader's quarter-rate lattice
    caps it at 0.25); 31 to 134 new unstable surfels in the first fused frame (32 x 32 adds none in the second, hence the
    total); the 0.5-threshold prediction covers at least 0.969 of the frame."""
    st = sh.surfel_cycle(orc, w, h)
    assert st["first"] > 0.9 * w * h, st
    assert all(n > 0.18 * w * h for n in st["merged"]) and len(st["merged"]) == 3, st
    assert sum(st["new"]) >= 25, st
    assert all(c > 0.9 for c in st["cover"]), st
    # both outcomes of the thumbnail decision
    assert st["fill_low"] == [False] * 3 and st["fill_conf"] == [True] * 3, st


@pytest.mark.parametrize("w,h", sh.SPRITE_SHAPES)
def test_sprite_store_covers_the_frame(orc, w, h):
    """Measured: 0.93 of the pixels drawn at 36 x 44, 0.99 at the other two sizes; four NaN texels (the zero normals)."""
    K = synth.intrinsics(w, h)
    s, covering = sh.sprite_store(w, h)
    assert 280 <= s.shape[0] <= 290 and (s[:, 3] == 20.0).all()
    assert (s[:, 2] - 1.4143 * s[:, 11] >= sh.NEAR).all()
    assert (np.abs(s[:, 8:11]).sum(axis=1) == 0).sum() == 4
    for k, (z, r) in zip(covering, sh.COVERING):
        assert s[k, 2] == np.float32(z) and s[k, 11] == np.float32(r)
        assert sh.sprite_box(s[k], K, w, h) == (0, 0, w - 1, h - 1), (k, sh.sprite_box(s[k], K, w, h))
    image, vcp, nrp, tm = orc.combined_predict(s, np.eye(4), K, w, h, sh.MAXD, sh.CONF, sh.SPRITE_TICK, sh.SPRITE_TICK, sh.TIME_DELTA)
    assert (image[..., 3] == 255).mean() > 0.9, float((image[..., 3] == 255).mean())
    assert np.isnan(vcp[..., 2]).any()
    # sprites from one pixel to the whole frame were drawn: the winners' radii span the store's
    won = nrp[..., 3][image[..., 3] == 255]
    assert won.min() < 0.01 and won.max() >= 0.3


def run_boxes(orc, w, h, masks, spawns):
    """Surfel counts per frame and model of the oracle orchestration on a static scene with the given id masks."""
    K = synth.intrinsics(w, h)
    o = OracleFusion(orc, w, h, K, enable_multiple_models=True)
    counts = []
    for i, f in enumerate(sh.static_frames(w, h, len(masks))):
        o.process_frame(f["rgb"], f["depth"], timestamp=i, mask=masks[i], has_new_label=spawns[i])
        counts.append([m.surfels.shape[0] for m in o.models])
    return counts, [m.id for m in o.models]


def test_edge_boxes_spawn_persist_and_move(orc):
    """Measured after the last frame at 100 x 68: 6819 / 1418 / 2756 / 4 / 606 surfels for models 0 to 4."""
    w, h = sh.EDGE_SHAPES[0]
    masks, spawns = sh.edge_masks(w, h)
    for wh in sh.EDGE_SHAPES:  # the masks themselves: boxes on all four image sides, a 2 x 2 box, a frame without background
        ms, _ = sh.edge_masks(*wh)
        assert ms[4][0, 0] == 1 and ms[4][-1, -1] == 2 and (ms[4] == 3).sum() == 4 and (ms[4][wh[1] // 2 + 5] == 4).all()
        assert not np.isin(ms[5], (1, 3)).any() and not (ms[6] == 0).any() and ms[6][0, -1] == 1 and (ms[6] == 2).mean() > 0.9
        assert all(np.array_equal(ms[k], ms[4]) for k in (7, 8))
    counts, ids = run_boxes(orc, w, h, masks, spawns)
    assert ids == [0, 1, 2, 3, 4] and all(len(c) == 5 for c in counts[4:])
    assert all(c > 0 for c in counts[-1]), counts[-1]
    assert max(c[3] for c in counts[3:]) <= 8 and counts[3][3] >= 2, [c[3] for c in counts[3:]]
    assert counts[5][1] == counts[4][1] > 0 and counts[5][3] == counts[4][3] > 0, (counts[4], counts[5])
    assert counts[6][2] > 2 * counts[5][2], (counts[5], counts[6])


def test_grid_boxes_spawn_eight_objects(orc):
    """Measured: 574 to 2581 surfels per object."""
    w, h = sh.GRID_SHAPE
    masks, spawns = sh.grid_masks()
    assert sorted(np.unique(masks[-1])) == list(range(9))
    counts, ids = run_boxes(orc, w, h, masks, spawns)
    assert ids == list(range(9))
    assert all(c > 300 for c in counts[-1][1:]), counts[-1]
