"""What the GPU tests of the fern keyframe database share: random fill-in images with every kind of depth, and the comparison
of a device engine with the oracle (tests/ferns_oracle.py) after a process call -- small images, codes, good, co, dissim, both
minima, similarity, the decisions and the stored keyframes, bit for bit."""
import numpy as np
import torch

import ferns_oracle as fo
from helpers import assert_bit_equal

F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_frame(width, height, seed):
    """(image uint8 [H,W,4], vert, norm float32 [H,W,4]): depths from 0.3 to 7 m in blocks of 8 x 8 with pixel noise, a tenth
    of the pixels without depth (0, negative, NaN), a few far beyond any range"""
    rng = np.random.default_rng(seed)
    bh, bw = (height + 7) // 8, (width + 7) // 8
    up = lambda a: np.repeat(np.repeat(a, 8, axis=0), 8, axis=1)[:height, :width]  # noqa: E731
    image = up(rng.integers(0, 256, (bh, bw, 4), dtype=np.uint8)) ^ rng.integers(0, 4, (height, width, 4), dtype=np.uint8)
    z = up(rng.uniform(0.3, 7.0, (bh, bw)).astype(F)) + rng.uniform(-0.01, 0.01, (height, width)).astype(F)
    kind = up(rng.integers(0, 40, (bh, bw)))
    z[kind == 0], z[kind == 1], z[kind == 2], z[kind == 3] = 0.0, -1.5, np.nan, 4.0e6
    vert = np.stack([rng.normal(size=(height, width)).astype(F), rng.normal(size=(height, width)).astype(F), z,
                     np.ones((height, width), F)], axis=-1)
    norm = rng.normal(size=(height, width, 4)).astype(F)
    return np.ascontiguousarray(image), np.ascontiguousarray(vert), np.ascontiguousarray(norm)


def mutate(frame, fraction, seed):
    """the frame with `fraction` of its 8 x 8 blocks replaced by another random frame's: a view that resembles it"""
    image, vert, norm = (a.copy() for a in frame)
    height, width = image.shape[:2]
    other = random_frame(width, height, 100000 + seed)
    rng = np.random.default_rng(seed)
    pick = np.repeat(np.repeat(rng.random(((height + 7) // 8, (width + 7) // 8)) < fraction, 8, axis=0), 8, axis=1)[:height, :width]
    for a, b in zip((image, vert, norm), other):
        a[pick] = b[pick]
    return image, vert, norm


def assert_same_floats(a, b, what):
    """bit for bit, except that a NaN the arithmetic made (0 / 0) equals any NaN: its sign is the platform's"""
    a, b = np.atleast_1d(np.asarray(a, F)), np.atleast_1d(np.asarray(b, F))
    assert a.shape == b.shape, (what, a.shape, b.shape)
    nan = np.isnan(a) & np.isnan(b)
    ne = (a.view(np.uint32) != b.view(np.uint32)) & ~nan
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[:4].tolist()}: {a[ne][:4]} / {b[ne][:4]}"


def assert_result(got, want, what):
    for k in ("added", "dropped_total", "count", "good_codes", "closest", "candidate", "closest_time"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("add_minimum", "closest_dissim", "closest_similarity"):
        assert_same_floats(got[k], want[k], f"{what}: {k}")
    assert_bit_equal(np.asarray(got["closest_pose"], F).reshape(16), np.asarray(want["closest_pose"], F).reshape(16), f"{what}: closest_pose")


def assert_current(engine, db, n_before, what):
    """the engine's view of the frame it has just processed against the oracle's (`db.cur`); n_before: keyframes at the search"""
    cur = db.cur
    assert_bit_equal(engine.download("image"), cur["image"], f"{what}: small image")
    assert_bit_equal(engine.download("vert"), cur["vert"], f"{what}: small vert")
    assert_bit_equal(engine.download("norm"), cur["norm"], f"{what}: small norm")
    assert_bit_equal(engine.download("codes"), cur["codes"], f"{what}: codes")
    assert_bit_equal(engine.download("co")[:n_before], cur["co"], f"{what}: co")
    assert_same_floats(engine.download("dissim")[:n_before], cur["dissim"], f"{what}: dissim")


def assert_database(engine, db, what, images=True):
    """the stored keyframes against the oracle's"""
    n = len(db.frames)
    codes, times, good = engine.download("db_codes"), engine.download("db_times"), engine.download("db_good")
    if n:
        assert_bit_equal(codes[:n], np.stack([f["codes"] for f in db.frames]), f"{what}: db_codes")
    assert times[:n].tolist() == [f["time"] for f in db.frames], what
    assert good[:n].tolist() == [f["good"] for f in db.frames], what
    for j in range(n if images else 0):
        k, f = engine.keyframe(j), db.frames[j]
        assert k["time"] == f["time"] and k["good_codes"] == f["good"], (what, j)
        assert_bit_equal(k["pose"].reshape(16), f["pose"], f"{what}: pose {j}")
        for name in ("image", "vert", "norm"):
            assert_bit_equal(k[name].cpu().numpy(), f[name], f"{what}: keyframe {j} {name}")


def step_both(engine, db, frame, pose, time, flags=fo.FIND | fo.ADD, what="", full=True):
    """one process call on the device engine (a ferns.FernDatabase) and on the oracle, compared; -> the record"""
    n_before = len(db.frames)
    engine.process(dev(frame[0]), dev(frame[1]), dev(frame[2]), pose, time, flags)
    got = engine.result()
    want = db.process(frame[0], frame[1], frame[2], pose, time, flags)
    assert_result(got, want, what)
    if full:
        assert_current(engine, db, n_before, what)
    assert engine.last_launches() == 3, what
    return got
