"""-m gpu: the fern keyframe database hook of processFrame (mmf_fusion_set_fern_database).  A static scene at
160 x 120 whose camera pans out by seven degrees and back, once with the hook off and once with it on: poses, surfel maps and
masks of every frame are the same bits; every frame's record equals a stand-alone engine and the oracle, both fed that frame's
downloaded fillImage / fillVertex / fillNormal, the pose and the tick the frame ran under; by the oracle the path adds at least
two keyframes and meets a candidate.  reset empties the database; a sharded fusion and the hook refuse each other."""
import numpy as np
import pytest

import ferns_oracle as fo
from ferns_scene import assert_database, assert_result, dev

pytestmark = pytest.mark.gpu
W, H = 160, 120
YAW = [0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1, 0]  # degrees: 3 degrees apart the views differ by more than the threshold
CONFIG = dict(min_time_gap=3, capacity=16)


def scene():
    from multimotionfusion_amd import synth
    K = synth.intrinsics(W, H)
    frames = [synth.render(synth.make_pose((0, np.deg2rad(a), 0)), W, H, seed=i) for i, a in enumerate(YAW)]
    return K, [(dev(f["rgb"]), dev(f["depth"])) for f in frames]


def make(gpu_ctx, K):
    from multimotionfusion_amd.fusion import MultiMotionFusion
    return MultiMotionFusion(gpu_ctx, W, H, K["cx"], K["cy"], K["fx"], K["fy"])


def state(g):
    m = g.getBackgroundModel()
    return dict(pose=np.asarray(g.getCurrPose()).tobytes(), map=m.downloadMap().tobytes(), count=m.lastCount(),
                mask=g.getTexture("MASK").cpu().numpy().tobytes())


def fill_images(g):
    m = g.getBackgroundModel()
    return tuple(m.texture(n).clone() for n in ("fillImage", "fillVertex", "fillNormal"))


def test_the_hook_changes_nothing_and_its_record_is_the_engines(gpu_ctx):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.ferns import FernDatabase, FernsConfig, make_table
    K, keep = scene()
    table = make_table(11, 500, W // 8, H // 8, 15000)
    base = make(gpu_ctx, K)
    with pytest.raises(MmfError, match="mmf_fusion_last_fern_result"):
        base.getLastFernResult()  # off
    assert base.getFernDatabase() is None
    want = []
    for i, (rgb, depth) in enumerate(keep):
        base.processFrame(rgb, depth, timestamp=1000 + i)
        want.append(state(base))
    base.reset()
    again = []
    for i in range(3):
        base.processFrame(*keep[i], timestamp=2000 + i)
        again.append(state(base))
    base.close()

    g = make(gpu_ctx, K)
    g.setFernDatabase(FernsConfig(**CONFIG), table)
    with pytest.raises(MmfError, match="mmf_fusion_last_fern_result"):
        g.getLastFernResult()  # on, no frame yet
    alone = FernDatabase(gpu_ctx, W, H, table=table, **CONFIG)
    db = fo.Database(W, H, table, **CONFIG)
    added = candidates = 0
    for i, (rgb, depth) in enumerate(keep):
        tick = g.getTick()
        g.processFrame(rgb, depth, timestamp=1000 + i)
        got = state(g)
        for k in ("pose", "map", "mask"):
            assert got[k] == want[i][k], (i, k)
        assert got["count"] == want[i]["count"], i
        rec = g.getLastFernResult()
        image, vert, norm = fill_images(g)
        pose = np.asarray(g.getCurrPose(), np.float32)
        alone.process(image, vert, norm, pose, tick)
        assert_result(rec, alone.result(), f"frame {i}: hook against the stand-alone engine")
        ref = db.process(image.cpu().numpy(), vert.cpu().numpy(), norm.cpu().numpy(), pose, tick)
        assert_result(rec, ref, f"frame {i}: hook against the oracle")
        assert g.getFernDatabase().last_launches() == 3
        added += ref["added"]
        candidates += ref["candidate"]
    # conditions on the input, by the oracle: the path makes keyframes and comes back to one
    assert added >= 2 and candidates >= 1, (added, candidates)
    assert len(db.frames) == added
    assert_database(g.getFernDatabase(), db, "the hook's database")
    assert_database(alone, db, "the stand-alone database", images=False)

    # reset: an empty database; the frames behind it are the same bits as without the hook
    g.reset(), db.reset()
    with pytest.raises(MmfError, match="mmf_fusion_last_fern_result"):
        g.getLastFernResult()
    for i in range(2):
        tick = g.getTick()
        g.processFrame(*keep[i], timestamp=2000 + i)
        assert state(g) == again[i], i
        image, vert, norm = fill_images(g)
        ref = db.process(image.cpu().numpy(), vert.cpu().numpy(), norm.cpu().numpy(), np.asarray(g.getCurrPose(), np.float32), tick)
        assert_result(g.getLastFernResult(), ref, f"after the reset, frame {i}")
    assert g.getLastFernResult()["count"] == 1 and db.frames[0]["time"] == 1
    # off again: the engine goes, the frames run as before
    g.setFernDatabase(False)
    assert g.getFernDatabase() is None
    g.processFrame(*keep[2], timestamp=2002)
    assert state(g) == again[2]
    with pytest.raises(MmfError, match="mmf_fusion_last_fern_result"):
        g.getLastFernResult()
    alone.close()
    g.close()


def test_the_hook_and_a_sharded_fusion_refuse_each_other(gpu_ctx):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.ferns import FernsConfig
    from multimotionfusion_amd import synth
    K = synth.intrinsics(W, H)
    g = make(gpu_ctx, K)
    g.setShard(0, 2)
    with pytest.raises(MmfError, match="mmf_fusion_set_fern_database.*sharded") as e:
        g.setFernDatabase(True)
    assert e.value.status == -4
    g.close()
    g = make(gpu_ctx, K)
    g.setFernDatabase(True)  # the default table
    with pytest.raises(MmfError, match="mmf_fusion_set_shard.*fern") as e:
        g.setShard(0, 2)
    assert e.value.status == -4
    # what the engine refuses the setter refuses, and the hook stays as it was
    for over in (dict(num=0), dict(capacity=0), dict(max_depth_mm=10)):
        with pytest.raises(MmfError, match="mmf_fusion_set_fern_database"):
            g.setFernDatabase(FernsConfig(**over))
    assert g.getFernDatabase() is not None
    g.close()
