"""-m gpu: processFrame with the built-in dense-CRF segmentation (mmf_fusion_set_crf_segmentation): every frame's
segmentation against tests/crf_oracle.py computed from the device's own inputs (unaries, super-pixel depth, colour), the
spawn-offset gating (MultiMotionFusion.cpp:148, 410, 484), setSetInhibit (:413-415) and the precedence of a supplied
segmentation, under both tracking modes."""
import numpy as np
import pytest
import torch

import crf_oracle as co
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(w, h, n_frames, trans_mm, seed=21):
    K = synth.intrinsics(w, h)
    poses = synth.trajectory(n_frames, seed=seed)
    objs = synth.make_objects(1, seed=seed)
    traj = synth.object_trajectories(objs, n_frames, seed=seed, trans_mm=trans_mm, rot_deg=2.0)
    frames = [synth.render(p, w, h, seed=i, objects=objs, object_poses=[t[i] for t in traj]) for i, p in enumerate(poses)]
    return K, frames


def run(gpu_ctx, orc, batch, offset, inhibit=False, n_frames=8, trans_mm=60.0, w=320, h=240):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    K, frames = scene(w, h, n_frames, trans_mm)
    g = MultiMotionFusion(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, batch_tracking=batch,
                          conf_global_init=1.0)
    cfg = co.config(model_spawn_offset=offset, inhibit_new=int(inhibit))
    g.setCrfSegmentation(CrfConfig(**cfg))
    keep, log = [], []
    counter = 0  # spawnOffset: counts the multi-model tracked frames up to the offset, restarts at a spawn
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"])))
        n_before = len(g.getModels())
        next_id = g.getNextModelID()
        g.processFrame(*keep[-1], timestamp=1000 + i)
        if i == 0:
            continue
        counter = min(counter + 1, offset)
        # (the segmentation sees the models of the frame start; a spawn appends one)
        last = g.getLastSegmentation()
        assert last["n_components"] >= 1 and last["allow_new"] == (counter >= offset)
        assert last["unaries"].shape[0] == n_before + int(last["allow_new"])
        if len(g.getModels()) > n_before:
            counter = 0
        mask = g.getTexture("MASK").cpu().numpy()
        log.append(dict(frame=i, n_before=n_before, n_after=len(g.getModels()), has_new=last["has_new_label"],
                        next_id=next_id, mask=mask, ids=f["ids"], model_ids=[d["id"] for d in last["model_data"]]))
    return g, frames, log, cfg


@pytest.mark.parametrize("batch", [0, 1])
def test_no_new_label_before_the_spawn_offset(gpu_ctx, orc, batch):
    g, frames, log, cfg = run(gpu_ctx, orc, batch, offset=22, n_frames=6)
    for e in log:
        assert e["n_before"] == e["n_after"] == 1 and not e["has_new"]
    g.close()


@pytest.mark.parametrize("batch", [0, 1])
def test_crf_spawns_the_moving_object(gpu_ctx, orc, batch):
    g, frames, log, cfg = run(gpu_ctx, orc, batch, offset=2)
    spawned = [e for e in log if e["n_after"] > e["n_before"]]
    assert spawned, [(e["frame"], e["has_new"]) for e in log]
    e = spawned[0]
    assert e["frame"] >= 2  # the counter reaches the offset on the second multi-model tracked frame
    new = e["mask"] == e["next_id"]
    gt = e["ids"] > 0
    iou = float((new & gt).sum()) / max(1, int((new | gt).sum()))
    print(f"[crf] batch={batch}: spawned at frame {e['frame']}, IoU with the object {iou:.3f}")
    assert iou >= 0.2, iou  # (measured 0.243 under both tracking modes: the new segment covers where the box was and is)
    g.close()


def test_inhibit_keeps_the_mask_and_spawns_nothing(gpu_ctx, orc):
    g, frames, log, cfg = run(gpu_ctx, orc, 1, offset=2, inhibit=True)
    assert all(e["n_after"] == e["n_before"] == 1 for e in log)
    hits = [e for e in log if e["has_new"]]
    assert hits, "the scene must produce a new label"
    for e in hits:
        assert (e["mask"] == e["next_id"]).any()  # the new id's pixels stay in the mask
        assert e["model_ids"] == [0, e["next_id"]]  # ... and modelData keeps the new label's entry
    g.close()


@pytest.mark.parametrize("batch", [0, 1])
def test_processframe_segmentation_and_fusion_against_the_oracle(gpu_ctx, orc, batch):
    """Every frame: stage 1 recomputed by the oracle from what the segmentation must read -- each model's ICP-error image
    of this frame's tracking and channel 3 of its splat (the prediction the previous frame left, downloaded before the
    call) -- then stages 2-13 (tests/crf_oracle.py): range, unaries and average confidences bit-exact, Q within 1e-4, the
    argmax map where the oracle's margin allows, the post-processing and the mask exactly.  The oracle orchestration
    (oracle/fusion.py) is fed that segmentation and re-synchronised every frame as in test_gpu_multimodel.py: the same
    models, global pose within 1e-5 and its surfel count within 0.2 %, and the first surfels of a model the segmentation
    spawned bit-exact (fused at the identity pose through the segmentation's mask).  Object poses are not compared: the box
    moves 6 cm per frame (what it takes for its ICP error to pass the new-label threshold of the GUI settings) and the
    object model tracks a segment that covers where it was and where it is -- on identical inputs the oracle's and the
    device's object poses part by up to 1.7 cm, and both chains can give up (NaN) on the same frame: the float32
    summation order decides an ill-conditioned solve (cf. test_oracle_fusion.py::test_object_tracking_is_sensitive_to_one_ulp_noise)."""
    from helpers import OracleFusion, assert_bit_equal
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    w, h = 320, 240
    K, frames = scene(w, h, 7, 60.0)
    g = MultiMotionFusion(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, batch_tracking=batch,
                          conf_global_init=1.0)
    o = OracleFusion(orc, w, h, K, enable_multiple_models=True, conf=1.0)
    cfg = co.config(model_spawn_offset=2)
    g.setCrfSegmentation(CrfConfig(**cfg))
    S = cfg["spixel_size"]
    labels = co.grid_labels(w, h, S)
    keep, worst, compared, spawned, checked = [], 0.0, 0, 0, 0
    for i, f in enumerate(frames):
        keep.append((dev(f["rgb"]), dev(f["depth"])))
        models = g.getModels()
        ids = [m.id for m in models]
        next_id = g.getNextModelID()
        splats = [m.texture("vertexConf").cpu().numpy() for m in models]  # what the previous frame predicted
        g.processFrame(*keep[-1], timestamp=1000 + i)
        if i == 0:
            o.process_frame(f["rgb"], f["depth"], timestamp=1000 + i, mask=np.zeros((h, w), np.uint8))
            continue
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
        spawned += int(has_new)
        # the oracle orchestration, fed the device's segmentation
        o.process_frame(f["rgb"], f["depth"], timestamp=1000 + i, mask=mask, has_new_label=has_new, model_data=last["model_data"])
        gm = g.getModels()
        assert [m.id for m in gm] == [m.id for m in o.models], i
        assert np.abs(gm[0].getPose() - o.models[0].pose).max() <= 1e-5, i
        na, nb = gm[0].lastCount(), o.models[0].surfels.shape[0]
        assert abs(na - nb) <= max(8, 0.002 * nb), (i, na, nb)
        if has_new:  # the new model's first surfels: nothing of them went through a tracker
            fresh_g, fresh_o = gm[-1].downloadMap(), o.models[-1].surfels
            assert fresh_o.shape[0] > 0 and np.array_equal(fresh_g.view(np.uint32), fresh_o.view(np.uint32)), i
        for a, b in zip(gm, o.models):  # the next frame starts from the oracle's state
            a.uploadMap(b.surfels)
            a.overridePose(b.pose)
        g.predict()
    n_cells = checked * (w // S) * (h // S)
    print(f"[crf] processFrame batch={batch}: stages 1-4 checked on {checked} of {len(frames) - 1} frames, max |Q - Q_oracle| "
          f"{worst:.3e}, argmax compared on {compared} of {n_cells} cells (oracle margin >= 1e-3), {spawned} spawn(s)")
    assert spawned >= 1 and checked >= len(frames) - 3 and compared >= 0.9 * n_cells, (spawned, checked, compared, n_cells)
    g.close()


def test_supplied_segmentation_and_callback_take_precedence(orc):
    """a frame's own mask, and a segmentation callback, win over the built-in CRF, which then does not run (on a context
    of its own: nothing ran there)"""
    import ctypes as C
    from multimotionfusion_amd._capi import SEGMENTATION_FN, MmfError, check
    from multimotionfusion_amd.cudafuncs import Context, _p
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    ctx = Context(0)
    w, h = 160, 120
    K, frames = scene(w, h, 3, 3.0)
    zero = dev(np.zeros((h, w), np.uint8))
    keep = [(dev(f["rgb"]), dev(f["depth"])) for f in frames]
    g = MultiMotionFusion(ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g.setCrfSegmentation(CrfConfig(model_spawn_offset=0))
    for i in range(len(frames)):
        g.processFrame(*keep[i], timestamp=i, mask=zero)
    calls = []

    def cb(user, fusion, frame, out):
        out.contents.mask = _p(zero)
        calls.append(1)
        return 0
    fn = SEGMENTATION_FN(cb)
    g2 = MultiMotionFusion(ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1)
    g2.setCrfSegmentation(CrfConfig(model_spawn_offset=0))
    check(ctx.lib.mmf_fusion_set_segmentation_callback(g2.handle, C.cast(fn, C.c_void_p), None))
    for i in range(len(frames)):
        g2.processFrame(*keep[i], timestamp=i)
    assert len(calls) == len(frames) - 1
    with pytest.raises(MmfError):
        g.getLastSegmentation()
    g.close(), g2.close()
    ctx.close()


def test_superpixels_apply_to_the_next_frame_only(gpu_ctx, orc):
    """setSuperpixels: a label image for the next frame's segmentation; the regular grid handed in explicitly gives the
    bits of no label image at all, a gSLICr-like one gives its own mask, and the frame after falls back to the grid"""
    from helpers import slic_like_labels
    from multimotionfusion_amd.fusion import MultiMotionFusion
    from multimotionfusion_amd.segmentation import CrfConfig
    w, h = 320, 240
    K, frames = scene(w, h, 4, 60.0)
    runs = []
    for mode in ("none", "grid", "slic"):
        g = MultiMotionFusion(gpu_ctx, w, h, K["cx"], K["cy"], K["fx"], K["fy"], enable_multiple_models=1, conf_global_init=1.0)
        g.setCrfSegmentation(CrfConfig(model_spawn_offset=22))
        keep, out = [], []
        for i, f in enumerate(frames):
            keep.append((dev(f["rgb"]), dev(f["depth"])))
            lab = {"grid": co.grid_labels(w, h, 16), "slic": slic_like_labels(w, h, 16, seed=i)}.get(mode) if i == 2 else None
            if lab is not None:
                keep.append(dev(lab))
                g.setSuperpixels(keep[-1])
            g.processFrame(*keep[len(keep) - 1 - (lab is not None)], timestamp=i)
            if i >= 2:
                last = g.getLastSegmentation()
                out.append((g.getTexture("MASK").cpu().numpy(), last["map"].cpu().numpy(), lab))
        runs.append(out)
        g.close()
    (m0, s0, _), (m1, s1, _), (m2, s2, lab2) = runs[0][0], runs[1][0], runs[2][0]
    assert np.array_equal(m0, m1) and np.array_equal(s0, s1)
    assert np.array_equal(m2, orc.slic_upsample_u8(lab2, s2))
    grid = co.grid_labels(w, h, 16)
    for r in runs:  # the frame after: the grid again
        assert np.array_equal(r[1][0], orc.slic_upsample_u8(grid, r[1][1]))


