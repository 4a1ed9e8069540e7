"""-m gpu: the flow-CRF inference engine (csrc/flowcrf_kernels.hpp) against tests/flowcrf_oracle.py on the scenes
of flowcrf_oracle.GPU_CASES (CRF images 8 x 8, 44 x 12, 43 x 25, 80 x 60; 1, 2, 3, 9 and 32 labels, with and without the new
label): the track errors, the tracks' cells and `invalid` bit for bit; unaries and projection probabilities up to the library
functions; Q, prob and the labels with the tolerances of test_gpu_crf.py; stage (e) replayed exactly from the device's own Q and
proj (flowcrf_edges.check_against_oracle, shared with test_gpu_flowcrf_edges.py).  Then the structure of the result,
determinism, the launch count, the tracker entry point, the two large sizes and every refusal."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flowcrf_oracle as fo
from flowcrf_edges import STAGES, check_against_oracle, dev, engine, infer, same_bits_nan_as_nan
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu
F32 = np.float32


@functools.lru_cache(maxsize=None)
def reference(w, h, L, allow_new):
    sc, cfg = fo.case_scene(w, h, L, allow_new)
    return sc, cfg, fo.run_scene(sc, cfg)


@pytest.mark.parametrize("w,h,L,allow_new", fo.GPU_CASES)
def test_every_stage_against_the_oracle(gpu_ctx, w, h, L, allow_new):
    """flowcrf_edges.check_against_oracle: stages (a) to (e), the replay of (e) from the device's own Q and proj, the structure,
    the launch count and a second run with the same bits"""
    sc, cfg, want = reference(w, h, L, allow_new)
    check_against_oracle(gpu_ctx, sc, cfg, want)


def test_the_launch_count_does_not_depend_on_size_labels_or_tracks(gpu_ctx):
    counts = set()
    for (w, h, L, allow_new), tracks in (((8, 8, 2, False), "scene"), ((80, 60, 3, True), "scene"), ((80, 60, 32, False), None)):
        sc, _, _ = reference(w, h, L, allow_new)
        e = engine(gpu_ctx, sc, fo.config(iterations=2))
        infer(e, sc, tracks=tracks)
        counts.add(e.last_launches())
        e.close()
    assert counts == {11}
    sc, _, _ = reference(8, 8, 2, False)
    e = engine(gpu_ctx, sc, fo.config(iterations=0))
    infer(e, sc)
    assert e.last_launches() == 4
    U = e.download("U").astype(np.float64)
    ex = np.exp(-U)
    assert np.abs(e.download("Q") - ex / ex.sum(0)).max() <= 1e-6  # no mean field: Q = softmax(-U)
    e.close()


def test_without_tracks_every_unary_is_log_L(gpu_ctx):
    sc, cfg, _ = reference(44, 12, 3, True)
    e = engine(gpu_ctx, sc, cfg)
    infer(e, sc, tracks=None)
    assert np.isposinf(e.download("E")).all()
    assert np.abs(e.download("U") - np.log(3.0)).max() <= 1e-6
    e.close()


def test_the_tracker_entry_point_reads_the_table_as_the_plain_one_reads_arrays(gpu_ctx):
    """two frames of keypoints into a device tracker (the second frame's match the first's: `cur` and `prev` are filled, some
    slots stay null); the inference from the tracker equals the inference from the downloaded table, bit for bit"""
    from multimotionfusion_amd.tracker import DevicePointTracker
    w, h = 16, 12
    sc = fo.make_scene(w, h, 2, True, seed=3, edge_tracks=False)
    W, H = sc["W"], sc["H"]
    rng = np.random.default_rng(5)
    trk = DevicePointTracker(gpu_ctx, W, H, sc["cam"], capacity=128, max_keypoints=64)
    desc = rng.standard_normal((60, 256)).astype(F32)
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    xy0 = np.stack([rng.integers(2, W - 4, 60), rng.integers(2, H - 4, 60)], 1).astype(np.int32)
    depth = dev(np.where(rng.random((H, W)) < 0.1, 0, 1.5).astype(F32))
    trk.addKeypointsPixels(xy0[:50], desc[:50], 1_000_000_000, depth)
    xy1 = xy0.copy()
    xy1[::3] += (2, 1)  # every third keypoint moves
    trk.addKeypointsPixels(xy1[10:], desc[10:], 1_033_000_000, depth)
    tab = trk.download()
    n = tab["n_tracks"]
    assert n == 60 and tab["nonnull"][1].sum() >= 30 and (tab["nonnull"][0] == 0).any()
    plain = dict(xy_cur=tab["xy"][0], xy_prev=tab["xy"][1], co_cur=tab["coordinate"][0], co_prev=tab["coordinate"][1],
                 ts_cur=tab["timestamp"][0], ts_prev=tab["timestamp"][1], ok_cur=tab["nonnull"][0], ok_prev=tab["nonnull"][1])
    cfg = fo.config(iterations=2)
    e = engine(gpu_ctx, sc, cfg, max_tracks=128)
    infer(e, sc, tracks=plain)
    a = {name: e.download(name) for name in STAGES}
    cells = e.download("cell")[:, :n]
    assert np.isfinite(a["E"]).sum() >= 20
    infer(e, sc, tracks=trk)
    for name in STAGES:
        assert_bit_equal(e.download(name), a[name], f"tracker entry point: {name}")
    assert np.array_equal(e.download("cell")[:, :n], cells)
    want = fo.infer(W, H, sc["cam"], sc["ids"], sc["T_start"], sc["T_end"], sc["vertex_z"], sc["depth"], sc["flow"], sc["motion"], plain,
                    True, sc["new_id"], cfg)
    same_bits_nan_as_nan(a["E"], want["E"], "tracker table: E")
    larger = DevicePointTracker(gpu_ctx, W, H, sc["cam"], capacity=256, max_keypoints=64)
    with pytest.raises(RuntimeError, match="capacity"):
        infer(e, sc, tracks=larger)
    e.close()


@pytest.mark.parametrize("W,H", [(640, 480), (1280, 960)])
def test_the_large_sizes_run(W, H):
    """status, ranges and the launch count only (tests/flowcrf_large_run.py); the image does not fit in LDS.  Each run is a
    child process with a time limit of its own"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flowcrf_large_run.py")
    r = subprocess.run([sys.executable, script, str(W), str(H)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert f"flowcrf large run {W}x{H}: ok" in r.stdout


def test_create_refuses_what_it_cannot_do(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.flowcrf import FlowCrf
    cam = fo.camera(64, 48)
    for kw, word in ((dict(width=66), "4 must divide"), (dict(height=50), "4 must divide"), (dict(width=0), "4 must divide"),
                     (dict(iterations=-1), "iterations"), (dict(iterations=51), "iterations"), (dict(weight_smoothness=0.0), "weights"),
                     (dict(weight_appearance=-1.0), "weights"), (dict(weight_appearance=float("nan")), "weights"),
                     (dict(max_labels=33), "32 labels"), (dict(max_labels=0), "32 labels"), (dict(div=2), "div"),
                     (dict(threshold=0.0), "threshold"), (dict(max_err=0.0), "max_err")):
        kw = dict(kw)
        width, height = kw.pop("width", 64), kw.pop("height", 48)
        with pytest.raises(MmfError, match=word) as err:
            FlowCrf(gpu_ctx, width, height, cam, **kw)
        assert err.value.status == -1, kw  # MMF_ERR_INVALID
    e = FlowCrf(gpu_ctx, 64, 48, cam, max_labels=2, max_tracks=4, iterations=50)
    sc = fo.make_scene(16, 12, 3, True, seed=1)  # three labels, an engine for two
    with pytest.raises(MmfError, match="labels"):
        infer(e, sc)
    sc2 = fo.make_scene(16, 12, 2, False, seed=1)  # two labels; more tracks than four
    with pytest.raises(MmfError, match="more tracks"):
        infer(e, sc2)
    with pytest.raises(MmfError, match="nothing has been inferred"):
        e.download("ids")
    e.close()
