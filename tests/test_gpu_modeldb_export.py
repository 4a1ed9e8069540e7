"""-m gpu: mmf_model_export_cloud (csrc/export_kernels.hpp) against tests/modeldb_oracle.py bit for bit -- the selection, the
order, the 31-byte records at every alignment of a workgroup's byte range -- mmf_model_export_ply's file, and the view store
giving its rows back (mmf_viewstore_download_view)."""
import ctypes as C

import numpy as np
import pytest

import modeldb_oracle as mo

pytestmark = pytest.mark.gpu
W, H, CAP = 64, 48, 8192
THR = np.float32(10.0)
COLOURS = [0, 0x123456, 0xFF0000, 0x00FF00, 0x0000FF, 2 ** 24 - 1]


@pytest.fixture(scope="module")
def model(gpu_ctx):
    from multimotionfusion_amd.model import Model
    m = Model(gpu_ctx, W, H, 31.5, 23.5, 60.0, 60.0, id=0, confidenceThresh=float(THR), max_surfels=CAP)
    yield m
    m.close()


def surfels(n, keep, seed=1):
    """n surfels, kept (confidence above THR) where `keep` says so; colours integer-valued floats below 2^24"""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(n, 12)).astype(np.float32)
    keep = np.asarray(keep, bool)
    assert keep.shape == (n,)
    s[:, 3] = np.where(keep, rng.uniform(10.5, 40, n), rng.uniform(0, 9.5, n)).astype(np.float32)
    s[:, 4] = rng.integers(0, 2 ** 24, n).astype(np.float32)
    s[:, 11] = rng.uniform(1e-3, 0.1, n).astype(np.float32)
    return s


def pattern_cases():
    rng = np.random.default_rng(2)
    out = []
    for n in [0, 1, 255, 256, 257, 1023, 4099]:  # round the workgroup's edge (256), several workgroups, ragged ends
        out.append((f"random-{n}", surfels(n, rng.random(n) < 0.5, seed=n)))
    n = 4099
    idx = np.arange(n)
    out += [("none", surfels(n, idx < 0)), ("all", surfels(n, idx >= 0)), ("every-other", surfels(n, idx % 2 == 0)),
            ("first-only", surfels(n, idx == 0)), ("last-only", surfels(n, idx == n - 1)),
            ("all-257", surfels(257, np.ones(257, bool))), ("first-only-1", surfels(1, [True])), ("none-1", surfels(1, [False]))]
    j = np.arange(768)
    out.append(("empty-workgroup-between-full", surfels(768, (j < 256) | (j >= 512))))
    for k in (1, 2, 3, 4):  # 31 k mod 4 = 3, 2, 1, 0: the second workgroup's byte range starts at every alignment
        j = np.arange(512)
        out.append((f"second-workgroup-after-{k}", surfels(512, ((j < 256) & (j % 61 == 7) & (j < 7 + 61 * k)) | (j >= 256))))
    return out


CASES = pattern_cases()


def export_raw(model, pose, thr, capacity, guard=0x5A):
    """-> (status, n_valid, destination bytes: capacity records and one guard record behind them)"""
    from multimotionfusion_amd._capi import fptr
    buf = np.full((capacity + 1) * 31, guard, np.uint8)
    p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
    n = C.c_uint(99999)
    rc = model.ctx.lib.mmf_model_export_cloud(model.handle, fptr(p), float(thr), buf.ctypes.data, capacity, C.byref(n))
    assert (buf[capacity * 31:] == guard).all(), "a write past capacity"
    return rc, n.value, buf


@pytest.mark.parametrize("name,s", CASES, ids=[c[0] for c in CASES])
def test_export_equals_the_oracle(model, name, s):
    pose = mo.make_pose(11)  # a rotation that is no axis permutation
    if name.startswith("second-workgroup-after-"):
        assert int((s[:256, 3] > THR).sum()) == int(name[-1])
    model.uploadMap(s)
    before = model.downloadMap()
    want = mo.export_cloud(s, pose, THR)
    got = model.exportCloud(pose, THR)
    assert got.dtype == mo.CLOUD_DTYPE and len(got) == len(want), (len(got), len(want))
    assert mo.records_equal(got, want)
    assert model.exportLastLaunches() == 3
    after = model.downloadMap()  # read-only: the map, the count, the ping-pong state
    assert model.lastCount() == len(s) and np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(after.view(np.uint32), s.view(np.uint32))
    rc, n, buf = export_raw(model, pose, THR, len(s))  # the bytes as they lie, nothing behind them
    assert rc == 0 and n == len(want) and (buf[n * 31:] == 0x5A).all()
    if not np.isnan(want["x"]).any():
        assert buf[:n * 31].tobytes() == want.tobytes()


def test_selection_is_strict_and_drops_nan(model):
    conf = np.array([10.0, np.nextafter(np.float32(10), np.float32(np.inf)), np.nan, np.inf, np.nextafter(np.float32(10), np.float32(0)),
                     -np.inf, 11.0], np.float32)
    s = surfels(len(conf), np.ones(len(conf), bool))
    s[:, 3] = conf
    model.uploadMap(s)
    pose = mo.make_pose(3)
    got, want = model.exportCloud(pose, THR), mo.export_cloud(s, pose, THR)
    assert len(want) == 3 and mo.records_equal(got, want)
    assert np.array_equal(got["radius"].view(np.uint32), s[[1, 3, 6], 11].view(np.uint32))
    # -0.0 against threshold 0 (and +0.0): not above it; a small positive number is
    s[:, 3] = np.array([-0.0, 0.0, 1e-30, -1e-30, np.nan, np.inf, -1.0], np.float32)
    model.uploadMap(s)
    got, want = model.exportCloud(pose, 0.0), mo.export_cloud(s, pose, 0.0)
    assert len(want) == 2 and mo.records_equal(got, want)
    assert np.array_equal(got["radius"].view(np.uint32), s[[2, 5], 11].view(np.uint32))


def test_colours_infinite_positions_and_identity(model):
    n = 300
    s = surfels(n, np.ones(n, bool), seed=8)
    s[:, 4] = np.array([COLOURS[i % len(COLOURS)] for i in range(n)], np.float32)
    s[5, 0], s[6, 1], s[7, 2], s[8, 0:3] = np.inf, -np.inf, np.inf, [np.inf, -np.inf, 0.0]
    model.uploadMap(s)
    for pose in (mo.make_pose(4), np.eye(4, dtype=np.float32)):
        got, want = model.exportCloud(pose, THR), mo.export_cloud(s, pose, THR)
        assert len(got) == n and mo.records_equal(got, want)
        for i, c in enumerate(COLOURS):
            assert (got["red"][i], got["green"][i], got["blue"][i]) == (c >> 16 & 255, c >> 8 & 255, c & 255)
    assert np.isinf(got["x"][5]) and np.isinf(got["y"][6])
    ident = model.exportCloud(np.eye(4, dtype=np.float32), THR)
    assert np.array_equal(ident["x"][:5].view(np.uint32), s[:5, 0].view(np.uint32))
    assert np.array_equal(ident["nz"][:5].view(np.uint32), (-s[:5, 10]).view(np.uint32))


def test_capacity_one_short_is_refused_and_nothing_is_written(model):
    s = surfels(1023, np.arange(1023) % 3 != 0, seed=4)
    n_valid = int((s[:, 3] > THR).sum())
    model.uploadMap(s)
    pose = mo.make_pose(6)
    rc, n, buf = export_raw(model, pose, THR, n_valid - 1)
    assert rc == -1 and n == n_valid and (buf == 0x5A).all()
    assert b"mmf_model_export_cloud" in model.ctx.lib.mmf_last_error()
    rc, n, buf = export_raw(model, pose, THR, n_valid)
    assert rc == 0 and n == n_valid and buf[:n * 31].tobytes() == mo.export_cloud(s, pose, THR).tobytes()


def test_launch_count_does_not_depend_on_the_count(model):
    launches = []
    for n in (1, 4099):
        model.uploadMap(surfels(n, np.ones(n, bool)))
        assert len(model.exportCloud(np.eye(4), THR)) == n
        launches.append(model.exportLastLaunches())
    assert launches[0] == launches[1] == 3


def test_export_ply_is_the_oracles_file(model, tmp_path):
    from multimotionfusion_amd import modeldb
    s = surfels(300, np.arange(300) % 5 != 1, seed=12)
    model.uploadMap(s)
    pose = mo.make_pose(9)
    path = tmp_path / "cloud-0.ply"
    model.exportModelPLY(path, pose)  # the model's own threshold: THR
    want = mo.export_cloud(s, pose, model.confidenceThreshold())
    assert len(want) == 240 and path.read_bytes() == mo.cloud_bytes(want)
    assert modeldb.readCloud(path).tobytes() == want.tobytes()


def test_view_store_gives_its_rows_back(gpu_ctx):
    """three views of 3, 0 and 40 rows (40 is no multiple of the tile's 32: the padding must not leak)"""
    from multimotionfusion_amd.redetection import ViewStore
    views = mo.make_views([3, 0, 40], seed=13)
    vs = ViewStore(gpu_ctx)
    assert vs.store(4, views) is True
    assert vs.views() == [(4, 0, 3), (4, 1, 0), (4, 2, 40)]
    for v, (d, c) in enumerate(views):
        gd, gc = vs.downloadView(v)
        assert gd.shape == d.shape and gc.shape == c.shape
        assert np.array_equal(gd.view(np.uint32), d.view(np.uint32)) and np.array_equal(gc.view(np.uint32), c.view(np.uint32))
    lib = gpu_ctx.lib
    desc, coord = np.full((41, 256), -7, np.float32), np.full((41, 3), -7, np.float32)
    assert lib.mmf_viewstore_download_view(vs.handle, 2, 39, desc.ctypes.data, coord.ctypes.data) == -1
    assert (desc == -7).all() and (coord == -7).all()
    assert lib.mmf_viewstore_download_view(vs.handle, 3, 64, desc.ctypes.data, coord.ctypes.data) == -1
    assert lib.mmf_viewstore_download_view(vs.handle, -1, 64, desc.ctypes.data, coord.ctypes.data) == -1
    assert lib.mmf_viewstore_download_view(vs.handle, 2, 40, desc.ctypes.data, coord.ctypes.data) == 0
    assert np.array_equal(desc[:40], views[2][0]) and (desc[40] == -7).all() and (coord[40] == -7).all()
    vs.close()
