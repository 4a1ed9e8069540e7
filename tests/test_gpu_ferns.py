"""-m gpu: the fern keyframe database engine (mmf_ferns_*) against its oracle (tests/ferns_oracle.py), bit for
bit: small images, codes, good, co, dissim, both minima, similarity, the decisions and the stored keyframes -- at the sizes,
numbers of ferns and database fills where the kernels take another path (the wave boundary of the ballot and of the search's
row reads, the workgroup boundary of the search, a full database), and on the cases worked by hand in tests/ferns_cases.py."""
import numpy as np
import pytest

import ferns_cases as fc
import ferns_oracle as fo
from ferns_scene import assert_database, dev, mutate, random_frame, step_both

pytestmark = pytest.mark.gpu
F = np.float32


def make(gpu_ctx, width, height, table=None, seed=3, **config):
    from multimotionfusion_amd.ferns import FernDatabase
    e = FernDatabase(gpu_ctx, width, height, table=table, seed=seed, **config)
    db = fo.Database(width, height, e.table, **config)
    return e, db


def views(width, height, seed):
    """eight frames: three scenes, views of them that differ in a few blocks (candidates, rejected adds) or in most"""
    a, b, c = (random_frame(width, height, seed + k) for k in range(3))
    return [a, mutate(a, 0.1, 1), b, mutate(a, 0.5, 2), a, c, mutate(b, 0.2, 3), mutate(c, 0.9, 4)]


@pytest.mark.parametrize("width,height,num", [(64, 48, 1), (64, 48, 63), (64, 48, 64), (64, 48, 65), (64, 48, 500), (104, 52, 65),
                                              (640, 480, 500)])
def test_a_sequence_equals_the_oracle(gpu_ctx, width, height, num):
    e, db = make(gpu_ctx, width, height, num=num, capacity=8, min_time_gap=1)
    seen = dict(added=0, rejected=0, candidate=0)
    for k, frame in enumerate(views(width, height, 10 * num)):
        r = step_both(e, db, frame, fc.pose(k), 10 + k, what=f"{width}x{height} num {num} frame {k}")
        seen["added"] += r["added"]
        seen["rejected"] += 1 - r["added"]
        seen["candidate"] += r["candidate"]
    if num >= 63:  # (one fern decides little)
        assert seen["added"] >= 3 and seen["rejected"] >= 1 and seen["candidate"] >= 1, seen
    assert_database(e, db, f"{width}x{height} num {num}")
    e.close()


def test_the_database_across_the_search_workgroups(gpu_ctx):
    """a threshold of -1 keeps every frame with a good code: n runs through 0, 1, 63, 64, 65 and on to 70; FIND alone, ADD alone
    and both along the way; the time gap hides the newest keyframes from find"""
    e, db = make(gpu_ctx, 64, 48, num=65, capacity=70, threshold=-1.0, min_time_gap=2)
    base = [random_frame(64, 48, 900 + k) for k in range(5)]
    for k in range(70):
        frame = mutate(base[k % 5], 0.02 * (k // 5), k)
        n = len(db.frames)
        if n in (1, 63, 64, 65):
            step_both(e, db, frame, fc.pose(k), 100 + k, flags=fo.FIND, what=f"n {n} find")
            assert len(db.frames) == n
        flags = fo.ADD if k % 7 == 3 else fo.FIND | fo.ADD
        r = step_both(e, db, frame, fc.pose(k), 100 + k, flags=flags, what=f"n {n}", full=n in (0, 1, 2, 63, 64, 65, 69))
        assert r["added"] == 1 and r["count"] == n + 1
        assert (r["closest"] >= 0) == (bool(flags & fo.FIND) and n > 2), (k, r)
    assert_database(e, db, "70 keyframes", images=False)
    for j in (0, 63, 64, 69):  # the keyframes at the ends of the search's workgroups, with their images
        kf, f = e.keyframe(j), db.frames[j]
        assert np.array_equal(kf["vert"].cpu().numpy().view(np.uint32), f["vert"].view(np.uint32)) and kf["time"] == f["time"]
        assert np.array_equal(kf["image"].cpu().numpy(), f["image"])
    from multimotionfusion_amd import MmfError
    with pytest.raises(MmfError, match="mmf_ferns_keyframe"):
        e.keyframe(70)
    e.close()


def test_a_full_database_drops_and_counts(gpu_ctx):
    """capacity 4: filled, overrun three times; a dropped frame leaves every bit of the database as it was; reset empties it"""
    from multimotionfusion_amd import MmfError
    e, db = make(gpu_ctx, 104, 52, num=64, capacity=4, min_time_gap=0)
    frames = [random_frame(104, 52, 40 + k) for k in range(7)]
    for k in range(4):
        assert step_both(e, db, frames[k], fc.pose(k), k + 1, what=f"fill {k}")["added"] == 1
    before = {n: e.download(n) for n in ("db_codes", "db_times", "db_good")}

    def snapshot(j):
        return {n: np.atleast_1d(v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)).tobytes() for n, v in e.keyframe(j).items()}
    kept = [snapshot(j) for j in range(4)]
    for k in range(4, 7):
        r = step_both(e, db, frames[k], fc.pose(k), k + 1, what=f"overrun {k}")
        assert r["added"] == 0 and r["count"] == 4 and r["dropped_total"] == k - 3
    r = step_both(e, db, frames[1], fc.pose(9), 20, what="a frame the rule rejects is not a drop")
    assert r["added"] == 0 and r["dropped_total"] == 3 and r["candidate"] == 1 and r["closest"] == 1
    for n, v in before.items():
        assert np.array_equal(e.download(n), v), n
    for j in range(4):
        assert snapshot(j) == kept[j], j
    assert_database(e, db, "full")
    e.reset(), db.reset()
    with pytest.raises(MmfError, match="mmf_ferns_result"):
        e.result()
    with pytest.raises(MmfError, match="mmf_ferns_keyframe"):
        e.keyframe(0)
    r = step_both(e, db, frames[5], fc.pose(0), 1, what="after the reset")
    assert r["added"] == 1 and r["count"] == 1 and r["dropped_total"] == 0 and r["closest"] == -1
    assert_database(e, db, "after the reset")
    e.close()


def test_the_codes_worked_by_hand(gpu_ctx):
    image, vert, norm = fc.code_images()
    e, db = make(gpu_ctx, 24, 16, table=fc.CODE_TABLE, num=len(fc.CODE_TABLE), capacity=2)
    r = step_both(e, db, tuple(fc.full_size(a) for a in (image, vert, norm)), fc.IDENT, 1, what="codes")
    assert e.download("codes").tolist() == fc.CODE_EXPECT.tolist()
    assert r["good_codes"] == fc.CODE_GOOD and r["added"] == 1
    e.close()


@pytest.mark.parametrize("case", fc.DECISION_CASES, ids=lambda c: c["name"])
def test_the_decisions_worked_by_hand(gpu_ctx, case):
    from test_ferns_oracle import same
    e, db = make(gpu_ctx, 16, 16, table=fc.DECISION_TABLE, num=4, **case["config"])
    for k, s in enumerate(case["steps"]):
        frame = tuple(fc.full_size(a) for a in fc.frame_from_codes(s["codes"]))
        r = step_both(e, db, frame, fc.pose(k), s["time"], s["flags"], what=f"{case['name']} step {k}")
        assert e.download("codes").tolist() == s["codes"]
        for name, want in s["expect"].items():
            assert same(r[name], want), (case["name"], k, name, r[name], want)
    assert_database(e, db, case["name"])
    e.close()


def test_the_launch_count_is_fixed(gpu_ctx):
    """three launches: for an empty database and one of 65 keyframes, for 64 x 48 and 640 x 480, for 1 and 500 ferns"""
    counts = []
    for width, height, num, fill in ((64, 48, 1, 0), (64, 48, 500, 65), (640, 480, 500, 0)):
        e, _ = make(gpu_ctx, width, height, num=num, capacity=66, threshold=-1.0)
        frame = tuple(dev(a) for a in random_frame(width, height, 5))
        for k in range(fill + 1):
            e.process(*frame, fc.IDENT, k)
            counts.append(e.last_launches())
        assert e.result()["count"] == (fill + 1 if e.result()["good_codes"] else 0)
        e.close()
    assert set(counts) == {3}


def test_the_engine_refuses_what_it_cannot_do(gpu_ctx):
    from multimotionfusion_amd import MmfError
    from multimotionfusion_amd.ferns import FernDatabase
    for kw in (dict(num=0), dict(capacity=0), dict(max_depth_mm=100)):
        with pytest.raises(MmfError, match="mmf_ferns"):
            FernDatabase(gpu_ctx, 64, 48, **kw)
    with pytest.raises(MmfError, match="at least 8 x 8"):
        FernDatabase(gpu_ctx, 64, 7, table=fo.make_table(0, 500, 8, 1, 15000))
    e, _ = make(gpu_ctx, 64, 48, num=8, capacity=2)
    with pytest.raises(MmfError, match="mmf_ferns_result"):
        e.result()  # nothing processed yet
    with pytest.raises(MmfError, match="mmf_ferns_download"):
        e.download("codes")
    frame = tuple(dev(a) for a in random_frame(64, 48, 1))
    with pytest.raises(MmfError, match="flags"):
        e.process(*frame, fc.IDENT, 1, flags=0)
    with pytest.raises(MmfError, match="flags"):
        e.process(*frame, fc.IDENT, 1, flags=4)
    import ctypes as C
    pose = np.eye(4, dtype=F).reshape(16)
    rc = gpu_ctx.lib.mmf_ferns_process(e.handle, None, C.c_void_p(frame[1].data_ptr()), C.c_void_p(frame[2].data_ptr()),
                                       pose.ctypes.data_as(C.POINTER(C.c_float)), 1, 3)
    assert rc == -1 and b"null image" in gpu_ctx.lib.mmf_last_error()
    e.close()
