"""-m gpu: mmf_model_import_cloud / mmf_model_set_timestamps (csrc/import_kernels.hpp) on a bare model against
tests/modeldb_import_oracle.py bit for bit; the imported store against the same surfels handed in through
mmf_model_upload_map, through the predictions; the prediction window; replacing and refusing; and the round trip through
mmf_model_export_cloud and the PLY file."""
import numpy as np
import pytest

import modeldb_import_oracle as io
import modeldb_oracle as mo

pytestmark = pytest.mark.gpu
W, H, CAP = 64, 48, 8192
THR = 10.0
CONF = THR + 1.0
# one record, the workgroup's edge (256) from both sides, several workgroups; 258 adds the ragged end 31 n mod 4 = 2, which the
# other sizes (3, 1, 0, 3, 1, 1) do not reach
SIZES = [0, 1, 255, 256, 257, 258, 1023, 4099]
INDEX_IMAGES = ("index", "vertConf", "colorTime", "normRad")
SPLAT_IMAGES = ("image", "vertexConf", "normalRadius", "time")


def new_model(gpu_ctx, cap=CAP):
    from multimotionfusion_amd.model import Model
    return Model(gpu_ctx, W, H, 31.5, 23.5, 60.0, 60.0, id=0, confidenceThresh=THR, max_surfels=cap)


@pytest.fixture(scope="module")
def models(gpu_ctx):
    a, b = new_model(gpu_ctx), new_model(gpu_ctx)
    yield a, b
    a.close()
    b.close()


def facing_records(n, seed):
    """records whose surfels lie in front of the camera at the identity and face it (the store holds the negated normal)"""
    r = io.make_records(n, seed, special=False)
    r["nz"] = np.abs(r["nz"]) * 0.5 + 0.5
    r["nx"], r["ny"] = r["nx"] * 0.3, r["ny"] * 0.3
    return r


def predictions(m, time, time_delta):
    """predictIndices and combinedPredict at `time` -> the bytes of every image they write"""
    m.predictIndices(time, 20.0, time_delta)
    m.combinedPredict(20.0, time, time, time_delta)
    views = {name: m.texture(name) for name in INDEX_IMAGES + SPLAT_IMAGES}  # (the index map's row-major copies are made here)
    m.ctx.synchronize()
    return {name: v.cpu().numpy().copy() for name, v in views.items()}


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a) and a.keys() == b.keys()


def test_the_sizes_cover_every_ragged_end():
    assert {31 * n % 4 for n in SIZES if n} == {0, 1, 2, 3}
    assert 1 in SIZES and {255, 256, 257} <= set(SIZES) and max(SIZES) > 2 * 256 and 0 in SIZES


@pytest.mark.parametrize("pose_name", ["identity", "null", "rigid"])
@pytest.mark.parametrize("n", SIZES)
def test_import_equals_the_oracle(models, n, pose_name):
    m = models[0]
    pose = {"identity": io.IDENTITY, "null": None, "rigid": mo.make_pose(11)}[pose_name]
    r = io.make_records(n, seed=n + 1)  # +-inf, denormals, -0.0, NaN, colours at both ends (in the first records)
    if n:  # the last record of the last workgroup, next to the padding: extreme bytes in every field
        r["x"][-1], r["radius"][-1], r["red"][-1], r["green"][-1], r["blue"][-1] = -0.0, np.float32(3e38), 255, 0, 255
    m.importCloud(r, pose, confidence=2.5, time=7)
    want = io.import_cloud(r, pose, 2.5, 7)
    assert m.lastCount() == n and m.importLastLaunches() == 1
    got = m.downloadMap()
    assert got.shape == want.shape and io.surfels_equal(got, want)
    if n >= 8:
        assert np.isinf(got[0, 0]) or np.isnan(got[0, 0])  # (an infinite coordinate times a zero of the pose is a NaN)
        assert np.isnan(got[3, 0]) and got[1, 4] == np.float32(0xFFFFFF) and got[0, 4] == 0.0
    if n >= 8 and pose_name != "rigid":
        assert got[1, 0] == np.float32(1e-41) and got[1, 2] == np.float32(1e-45)  # denormals are kept
        assert got[2, 0].view(np.uint32) == 0  # -0.0 + 0 = +0.0


def test_one_launch_whatever_the_count(models):
    m = models[0]
    launches = []
    for n in (0, 1, 4099):
        m.importCloud(io.make_records(n, 5), None, 1.0, 1)
        launches.append(m.importLastLaunches())
    assert launches == [1, 1, 1]


def test_imported_store_predicts_like_the_uploaded_one(models):
    a, b = models
    r = facing_records(1500, 21)
    a.importCloud(r, None, CONF, 5)
    b.uploadMap(io.import_cloud(r, None, CONF, 5))
    pa, pb = predictions(a, 6, 200), predictions(b, 6, 200)
    assert same_bytes(pa, pb)
    # the splat and the index map are not empty
    assert (pa["vertexConf"][..., 2] > 0).sum() > 100 and (pa["vertConf"][..., 2] > 0).sum() > 100 and len(np.unique(pa["index"])) > 100


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4099])
def test_set_timestamps_brings_the_store_into_the_window(models, n):
    a, b = models
    r = facing_records(n, 30 + n)
    a.importCloud(r, None, CONF, 5)
    want5 = io.import_cloud(r, None, CONF, 5)
    stale = predictions(a, 300, 200)
    assert (stale["vertexConf"][..., 2] > 0).sum() == 0  # the premise: 300 - 5 > 200, nothing is predicted
    a.setTimestamps(300)
    want300 = io.set_timestamps(want5, 300)
    got = a.downloadMap()
    assert a.lastCount() == n and io.surfels_equal(got, want300)
    assert (got[:, 6] == 5).all() and (got[:, 7] == 300).all()  # initTime still says when they were loaded
    b.uploadMap(want300)
    pa, pb = predictions(a, 300, 200), predictions(b, 300, 200)
    assert same_bytes(pa, pb)
    if n:
        assert (pa["vertexConf"][..., 2] > 0).sum() > 0


def test_import_replaces_the_content(models):
    m = models[0]
    r1, r2 = io.make_records(1023, 40), io.make_records(257, 41)
    m.importCloud(r1, None, 3.0, 1)
    assert m.lastCount() == 1023
    m.importCloud(r2, mo.make_pose(2), 4.0, 2)
    assert m.lastCount() == 257 and io.surfels_equal(m.downloadMap(), io.import_cloud(r2, mo.make_pose(2), 4.0, 2))
    m.importCloud(r1[:0], None, 3.0, 1)
    assert m.lastCount() == 0 and len(m.downloadMap()) == 0


def test_capacity_is_the_limit_and_one_more_is_refused(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    cap = 600
    m = new_model(gpu_ctx, cap)
    r = io.make_records(cap + 1, 50)
    m.importCloud(r[:cap], None, 3.0, 1)
    assert m.lastCount() == cap
    before = m.downloadMap().copy()
    assert io.surfels_equal(before, io.import_cloud(r[:cap], None, 3.0, 1))
    with pytest.raises(MmfError) as e:
        m.importCloud(r, None, 9.0, 2)
    assert e.value.status == -1 and "mmf_model_import_cloud" in str(e.value)
    assert m.lastCount() == cap and io.surfels_equal(m.downloadMap(), before)
    m.close()


def test_round_trip_through_the_device(models, tmp_path):
    from multimotionfusion_amd import modeldb
    m = models[0]
    r = io.make_records(4099, 60, special=False)  # finite, no -0.0 position, no zero normal component
    m.importCloud(r, None, CONF, 3)
    back = m.exportCloud(io.IDENTITY, THR)
    assert back.tobytes() == r.tobytes()
    # a store some of whose surfels are not stable, under a rigid pose: file and back
    s = io.import_cloud(r, mo.make_pose(4), CONF, 3)
    s[::3, 3] = 1.0
    m.uploadMap(s)
    path = tmp_path / "cloud.ply"
    P = mo.make_pose(7)
    m.exportModelPLY(path, P)
    exported = mo.export_cloud(s, P, THR)
    assert len(exported) == 4099 - len(s[::3]) and modeldb.readCloud(path).tobytes() == exported.tobytes()
    Q = io.inverse_rigid(P)
    m.importPly(path, Q, confidence=CONF, time=9)
    assert m.lastCount() == len(exported) and io.surfels_equal(m.downloadMap(), io.import_cloud(exported, Q, CONF, 9))
    m.importPly(path, None, confidence=CONF, time=9)
    assert io.surfels_equal(m.downloadMap(), io.import_cloud(exported, None, CONF, 9))


def test_import_ply_refuses_a_broken_file_and_keeps_the_store(models, tmp_path):
    from multimotionfusion_amd._capi import MmfError
    m = models[0]
    r = io.make_records(300, 70)
    m.importCloud(r, None, 2.0, 1)
    before = m.downloadMap().copy()
    path = tmp_path / "cut.ply"
    path.write_bytes(mo.cloud_bytes(r)[:-3])
    for p in (path, tmp_path / "missing.ply"):
        with pytest.raises(MmfError) as e:
            m.importPly(p, None, confidence=2.0, time=1)
        assert e.value.status == -1 and "mmf_ply_read_cloud" in str(e.value)
    assert m.lastCount() == 300 and io.surfels_equal(m.downloadMap(), before)
