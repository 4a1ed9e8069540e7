"""-m gpu: processFrame with the built-in segmentation on the super-pixel engine's labels (mmf_fusion_set_superpixel_engine):
the sequence of test_gpu_crf_fusion.py (320 x 240, one moving box, spawn offset 2) with the engine on -- every frame's label
image against tests/slic_oracle.py bit for bit, the CRF recomputed by tests/crf_oracle.py ON THOSE LABELS under the parity
bar of test_gpu_crf_fusion.py, the spawn -- then the precedence of labels handed in, the sizes the setter refuses, and the
off state: a fusion whose engine is off computes what a fusion that never heard of it computes."""
import numpy as np
import pytest
import torch

import crf_oracle as co
import slic_oracle as so
from helpers import assert_bit_equal, slic_like_labels
from test_gpu_crf_fusion import dev, scene

pytestmark = pytest.mark.gpu
F32 = np.float32


def make(gpu_ctx, K, w, h, batch, cfg, engine):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    g = MultiMotionFusion(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, batch_tracking=batch,
                          conf_global_init=1.0)
    g.setCrfSegmentation(CrfConfig(**cfg))
    if engine:
        g.setSuperpixelEngine(True)
    return g


def spawn_iou(gpu_ctx, K, frames, w, h, batch, cfg, engine):
    """the sequence as test_gpu_crf_fusion.py::run drives it; (frame of the first spawn, IoU of the new segment with the box)"""
    g = make(gpu_ctx, K, w, h, batch, cfg, engine)
    keep, hit = [], None
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"])))
        n_before, next_id = len(g.getModels()), g.getNextModelID()
        g.processFrame(*keep[-1], timestamp=1000 + i)
        if hit is None and len(g.getModels()) > n_before:
            new, gt = g.getTexture("MASK").cpu().numpy() == next_id, f["ids"] > 0
            hit = (i, float((new & gt).sum()) / max(1, int((new | gt).sum())))
    g.close()
    return hit


@pytest.mark.parametrize("batch", [0, 1])
def test_engine_labels_feed_the_crf_and_the_box_is_spawned(gpu_ctx, orc, batch):
    """Every frame: getLastSuperpixels() == the oracle's labels of that frame's RGB, all pixels; stage 1 (oracle/ on those
    labels, from the device's own ICP-error images and the splats the previous frame left) and stages 2-13
    (tests/crf_oracle.py) under test_gpu_crf_fusion.py's bar: range, unaries and average confidences bit-exact, Q within
    1e-4, the argmax map where the oracle's margin is >= 1e-3, post-processing and mask exactly.  The moving box is spawned;
    its IoU with the ground truth is printed beside the grid's on the same sequence and held to the existing floor (0.2)."""
    w, h = 320, 240
    K, frames = scene(w, h, 8, 60.0)
    cfg = co.config(model_spawn_offset=2)
    S = cfg["spixel_size"]
    g = make(gpu_ctx, K, w, h, batch, cfg, True)
    keep, worst, compared, checked, spawn = [], 0.0, 0, 0, None
    moved = []
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"])))
        models = g.getModels()
        ids = [m.id for m in models]
        next_id = g.getNextModelID()
        splats = [m.texture("vertexConf").cpu().numpy() for m in models]  # what the previous frame predicted
        g.processFrame(*keep[-1], timestamp=1000 + i)
        if i == 0:
            continue
        labels = g.getLastSuperpixels().cpu().numpy()
        assert_bit_equal(labels, so.segment(f["rgb"], S)[0], f"engine labels, frame {i}")
        moved.append(float((labels != co.grid_labels(w, h, S)).mean()))
        now = [m.id for m in g.getModels()]
        last = g.getLastSegmentation()
        last = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in last.items()}
        low_depth = orc.slic_downsample(labels, S, f["depth"], threshold=0.02).ravel()
        avg = np.array([d["avg_confidence"] for d in last["model_data"][:len(ids)]], F32)
        if all(m in now for m in ids):  # (a model that left the list in this frame takes its error image with it)
            icp = [g.getErrorTexture(now.index(m)).cpu().numpy() for m in ids]
            low_depth, maps = co.stage1(orc, labels, S, f["depth"], icp, splats)
            ref = co.segment(low_depth, maps[:, 0], maps[:, 1], f["rgb"].reshape(-1), w, h, S, ids, next_id, last["allow_new"], cfg)
            assert last["range"] == ref["range"] and not ref["range_invalid"]
            assert_bit_equal(last["unaries"], ref["unaries"], f"unaries, frame {i}")
            assert_bit_equal(avg, ref["avg_conf"], f"average confidences, frame {i}")
            worst = max(worst, float(np.abs(ref["q"] - last["q"]).max()))
            assert worst <= 1e-4, worst
            qs = np.sort(ref["q"], axis=0)
            sure = (qs[-1] - qs[-2]) >= 1e-3 if len(qs) > 1 else np.ones(qs.shape[1], bool)  # cells the oracle decides clearly
            assert np.array_equal(ref["raw_map"][sure], last["raw_map"][sure]), i
            compared += int(sure.sum())
            checked += 1
        out, data, has_new = co.postprocess(last["raw_map"], w // S, h // S, w, h, S, ids, next_id, last["allow_new"],
                                            low_depth, avg, cfg)
        assert np.array_equal(out, last["map"]) and has_new == last["has_new_label"]
        assert [(d["id"], d["super_pixel_count"], F32(d["depth_mean"]), F32(d["depth_std"])) for d in data] == \
            [(d["id"], d["super_pixel_count"], F32(d["depth_mean"]), F32(d["depth_std"])) for d in last["model_data"]]
        mask = g.getTexture("MASK").cpu().numpy()
        assert np.array_equal(mask, orc.slic_upsample_u8(labels, out))
        if spawn is None and len(now) > len(ids):
            new, gt = mask == next_id, f["ids"] > 0
            spawn = (i, float((new & gt).sum()) / max(1, int((new | gt).sum())))
    g.close()
    n_cells = checked * (w // S) * (h // S)
    grid_hit = spawn_iou(gpu_ctx, K, frames, w, h, batch, cfg, False)
    print(f"[slic engine] processFrame batch={batch}: labels bit-exact on {len(frames) - 1} frames ({min(moved):.2f}-{max(moved):.2f} of the "
          f"pixels leave their grid cell), CRF stages checked on {checked} frames, max |Q - Q_oracle| {worst:.3e}, argmax compared on "
          f"{compared} of {n_cells} cells; spawn (frame, IoU): engine {spawn}, grid {grid_hit}")
    assert checked >= len(frames) - 3 and compared >= 0.9 * n_cells, (checked, compared, n_cells)
    assert spawn is not None, "the moving box must be spawned"
    assert spawn[0] >= 2 and spawn[1] >= 0.2, spawn  # (the floor of test_gpu_crf_fusion.py; no improvement over the grid is asserted)


def test_handed_in_labels_win_for_their_frame_only(gpu_ctx, orc):
    """engine on: the labels of setSuperpixels are used for the next frame, the frame after is the engine's again"""
    w, h = 320, 240
    K, frames = scene(w, h, 5, 60.0)
    cfg = co.config(model_spawn_offset=22)
    S = cfg["spixel_size"]
    g = make(gpu_ctx, K, w, h, 1, cfg, True)
    keep = []
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"])))
        given = None
        if i == 2:
            given = slic_like_labels(w, h, S, seed=5)
            keep.append(dev(given))
            g.setSuperpixels(keep[-1])
        g.processFrame(*keep[len(keep) - 1 - (given is not None)], timestamp=i)
        if i == 0:
            continue
        used = g.getLastSuperpixels().cpu().numpy()
        want = given if given is not None else so.segment(f["rgb"], S)[0]
        assert_bit_equal(used, want, f"labels used at frame {i}")
        last = g.getLastSegmentation()
        assert np.array_equal(g.getTexture("MASK").cpu().numpy(), orc.slic_upsample_u8(want, last["map"].cpu().numpy()))
    g.close()


def test_engine_off_is_the_fusion_that_never_heard_of_it(gpu_ctx, orc):
    """same sequence, same process: no call at all / setSuperpixelEngine(False) / on and off again before the first frame --
    masks, label images, poses and surfel counts of every frame are identical"""
    w, h = 320, 240
    K, frames = scene(w, h, 7, 60.0)
    cfg = co.config(model_spawn_offset=2)
    S = cfg["spixel_size"]
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames]

    def sequence(mode):
        g = make(gpu_ctx, K, w, h, 1, cfg, False)
        if mode == "off":
            g.setSuperpixelEngine(False)
        elif mode == "on-off":
            g.setSuperpixelEngine(True)
            g.setSuperpixelEngine(False)
        out = []
        for i in range(len(frames)):
            g.processFrame(*keep[i], timestamp=1000 + i)
            if i == 0:
                continue
            ms = g.getModels()
            out.append(dict(mask=g.getTexture("MASK").cpu().numpy(), labels=g.getLastSuperpixels().cpu().numpy(),
                            poses=[m.getPose().copy() for m in ms], counts=[m.lastCount() for m in ms], ids=[m.id for m in ms]))
        g.close()
        return out
    base = sequence("never")
    assert all(np.array_equal(e["labels"], co.grid_labels(w, h, S)) for e in base)  # B3: the grid
    assert any(len(e["ids"]) > 1 for e in base)
    for mode in ("off", "on-off"):
        got = sequence(mode)
        for i, (a, b) in enumerate(zip(base, got)):
            assert a["ids"] == b["ids"] and a["counts"] == b["counts"], (mode, i, a["counts"], b["counts"])
            assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["labels"], b["labels"]), (mode, i)
            for p, q in zip(a["poses"], b["poses"]):
                assert np.asarray(p).tobytes() == np.asarray(q).tobytes(), (mode, i)


def test_setter_refuses_a_size_the_superpixels_do_not_divide(gpu_ctx):
    """240 % 32 != 0: MMF_ERR_INVALID at the setter; and at the frame when the CRF configuration changes afterwards --
    never a silent fall back to the grid"""
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.segmentation import CrfConfig
    w, h = 320, 240
    K, frames = scene(w, h, 3, 60.0)
    g = make(gpu_ctx, K, w, h, 1, co.config(spixel_size=32), False)
    with pytest.raises(MmfError):
        g.setSuperpixelEngine(True)
    g.setCrfSegmentation(CrfConfig(**co.config(spixel_size=16)))
    g.setSuperpixelEngine(True)
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames]
    g.processFrame(*keep[0], timestamp=0)
    g.processFrame(*keep[1], timestamp=1)
    assert_bit_equal(g.getLastSuperpixels().cpu().numpy(), so.segment(frames[1]["rgb"], 16)[0], "labels")
    g.setCrfSegmentation(CrfConfig(**co.config(spixel_size=32)))
    with pytest.raises(MmfError):
        g.processFrame(*keep[2], timestamp=2)
    g.close()
