"""CPU: tests/slic_oracle.py, the restatement of the super-pixel engine's specification that the device is
held to bit for bit -- analytic known answers, the vectorised association against the scalar loop, the integer sums'
size (B5: gSLICr's float tree sums agree with integer sums while every total stays below 2^24), the committed fixtures,
and the sizes the engine refuses."""
import os

import numpy as np
import pytest

import slic_oracle as so
from multimotionfusion_amd import synth

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def frame(w, h, seed=0):
    return synth.render(synth.trajectory(2, seed=21)[1], w, h, seed=seed)["rgb"]


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def grid(w, h, S):
    return ((np.arange(h)[:, None] // S) * (w // S) + np.arange(w)[None, :] // S).astype(np.int32)


def test_constant_image_first_association_is_the_tie_rule():
    """every colour distance is 0, the centres sit at cell * S + S/2: with even S the pixel x = cx S is as far from the
    centre on its left as from its own, and the left one comes first in scan order; x = 0 has no left neighbour.  Rows alike."""
    S, w, h = 16, 96, 64
    rgb = np.full((h, w, 3), 77, np.uint8)
    lab = so.associate(rgb, so.init_centres(rgb, S), S)
    mx = w // S
    want_col = np.array([0 if x == 0 else (x - 1) // S if x % S == 0 else x // S for x in range(w)])
    want_row = np.array([0 if y == 0 else (y - 1) // S if y % S == 0 else y // S for y in range(h)])
    assert np.array_equal(lab, (want_row[:, None] * mx + want_col[None, :]).astype(np.int32))
    assert (lab != grid(w, h, S)).sum() == (mx - 1) * h + (h // S - 1) * w - (mx - 1) * (h // S - 1)
    # the iterations move nothing that matters: the labels stay connected blocks and no cluster is empty
    lab5, c, cnt = so.segment(rgb, S)
    assert cnt.min() > 0 and np.all(c[:, 2:] == 77)


def test_step_edge_pulls_the_labels_to_the_edge():
    """two colours meeting at x = 40 inside the cell column [32, 48): after the iterations no super-pixel straddles the edge
    and every centre has one of the two colours exactly"""
    S, w, h = 16, 96, 64
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[:, :40] = (200, 30, 30)
    rgb[:, 40:] = (20, 180, 220)
    lab, c, cnt = so.segment(rgb, S)
    left, right = set(np.unique(lab[:, :40])), set(np.unique(lab[:, 40:]))
    assert not (left & right), left & right
    # (the colour term of a wrong-coloured centre is ~46, the largest spatial term in the window ~2.4: a pixel never takes
    # a centre across the edge while one of its own colour is among the nine)  The cell column [32, 48) is split AT the edge:
    mx = w // S
    assert np.all(lab[:, 32:40] % mx == 1) and np.all(lab[:, 40:48] % mx == 2)
    assert np.all(grid(w, h, S)[:, 32:40] % mx == 2)  # ... where the grid has one block
    assert set(np.unique(c[:, 2])) <= {F32(200), F32(20)}


@pytest.mark.parametrize("w,h,S", [(160, 120, 20), (320, 240, 16), (99, 66, 11)])
def test_labels_stay_in_the_3x3_neighbourhood_and_in_range(w, h, S):
    for rgb in (frame(w, h), noise(w, h, 1)):
        lab, c, cnt = so.segment(rgb, S)
        mx, my = w // S, h // S
        assert lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < mx * my
        ly, lx = np.divmod(lab, mx)
        g = grid(w, h, S)
        gy, gx = np.divmod(g, mx)
        assert np.abs(ly - gy).max() <= 1 and np.abs(lx - gx).max() <= 1
        assert cnt.sum() == w * h and cnt.min() > 0
        assert (lab != g).any()  # (these images have colour edges off the grid lines: some pixel must leave its cell)


def test_vectorised_association_equals_the_scalar_loop():
    for rgb, S in ((frame(66, 44, 2), 11), (noise(48, 36, 3), 12), (np.full((24, 36, 3), 9, np.uint8), 12)):
        c = so.init_centres(rgb, S)
        for _ in range(3):
            a, b = so.associate(rgb, c, S), so.associate_scalar(rgb, c, S)
            assert np.array_equal(a, b)
            c = so.update(rgb, a, c, S)[0]
    # centres handed in: one far away, one NaN
    rgb, S = noise(48, 36, 4), 12
    c = so.init_centres(rgb, S)
    c[5, :2] = 1e6
    c[7] = np.nan
    a = so.associate(rgb, c, S)
    assert np.array_equal(a, so.associate_scalar(rgb, c, S)) and 5 not in a and 7 not in a


def test_update_reproduces_hand_computed_means_and_keeps_an_empty_centre():
    S, w, h = 12, 24, 12
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[..., 0] = np.arange(w)[None, :]
    rgb[..., 1] = np.arange(h)[:, None] * 2
    rgb[..., 2] = 7
    lab = np.zeros((h, w), np.int32)  # everything belongs to centre 0; centre 1 has no pixel
    c0 = np.array([[1, 2, 3, 4, 5], [60, 61, 62, 63, 64]], F32)
    c, cnt, tot = so.update(rgb, lab, c0, S)
    n = w * h
    sx, sy = h * sum(range(w)), w * sum(range(h))
    assert cnt.tolist() == [n, 0] and tot[0].tolist() == [sx, sy, sx, 2 * sy, 7 * n]
    assert c[0].tolist() == [F32(sx) / F32(n), F32(sy) / F32(n), F32(sx) / F32(n), F32(2 * sy) / F32(n), F32(7)]
    assert np.array_equal(c[1], c0[1])
    # ... and through segment(): a centre no pixel can choose keeps position and colour, its count is 0
    rgb = noise(48, 36, 5)
    cin = so.init_centres(rgb, S)
    cin[6] = (1e5, 1e5, 0, 0, 0)
    lab, c, cnt = so.segment(rgb, S, 5, centres=cin)
    assert cnt[6] == 0 and np.array_equal(c[6], cin[6]) and 6 not in lab


def test_integer_sums_stay_below_2_pow_24_on_the_test_inputs():
    """B5: gSLICr adds floats in a tree; that equals the integer sum while every total is exactly representable"""
    worst = 0
    for rgb, S in ((frame(320, 240), 16), (frame(320, 240, 1), 20), (frame(640, 480), 16), (frame(640, 480), 40), (noise(640, 480), 32)):
        trace = []
        so.segment(rgb, S, trace=trace)
        worst = max(worst, max(int(t[3].max()) for t in trace))
    assert worst < 2 ** 24, worst


@pytest.mark.parametrize("name", ["slic_engine_160x120_s20.npz", "slic_engine_320x240_s16.npz"])
def test_oracle_reproduces_the_committed_fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    S = int(z["spixel_size"])
    trace = []
    lab, c, cnt = so.segment(z["rgb"], S, 5, trace=trace)
    assert np.array_equal(lab, z["labels"].astype(np.int32)) and np.array_equal(trace[0][0], z["labels_first"].astype(np.int32))
    assert np.array_equal(np.stack([t[1] for t in trace]).view(np.uint32), z["centres_iter"].view(np.uint32))
    assert np.array_equal(np.stack([t[2] for t in trace]), z["counts_iter"])
    assert np.array_equal(c.view(np.uint32), z["centres"].view(np.uint32)) and np.array_equal(cnt, z["counts"])
    # 0 and 1 iterations are the trace's first steps
    assert np.array_equal(so.segment(z["rgb"], S, 0)[0], trace[0][0])
    assert np.array_equal(so.segment(z["rgb"], S, 1)[1], trace[0][1])


@pytest.mark.parametrize("w,h,S", [(320, 240, 32), (330, 240, 16), (320, 240, 10), (320, 240, 256), (512, 512, 256)])
def test_ragged_and_out_of_range_sizes_are_refused(w, h, S):
    with pytest.raises(ValueError):
        so.segment(np.zeros((h, w, 3), np.uint8), S)


def test_library_refuses_ragged_sizes_without_a_device():
    """mmf_slic_segment checks its sizes before it touches the device: MMF_ERR_INVALID, never a fall back"""
    import ctypes as C
    from multimotionfusion_amd import _capi
    lib = _capi.load()
    one = C.c_void_p(16)  # (never dereferenced: the size check comes first; a context is needed for anything else)
    for w, h, S in [(320, 240, 32), (330, 240, 16), (320, 240, 10), (320, 240, 256)]:
        assert lib.mmf_slic_segment(one, one, w, h, S, 5, None, one, None, None) == -1, (w, h, S)
        assert b"mmf_slic_segment" in lib.mmf_last_error()


def test_slic_shim_compiles_and_links_without_warnings(tmp_path):
    """multimotionfusion_amd/cpp/Slic.h and the setter in cpp/MultiMotionFusion.h build with plain g++ under
    -Wall -Wextra -Werror against the C ABI (the program itself needs a device: tests/test_gpu_slic_shim.py runs it)"""
    import subprocess
    from multimotionfusion_amd import build
    build.build(verbose=False)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "multimotionfusion_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                    os.path.join(repo, "tests", "cpp", "slic_shim_sequence.cpp"), "-o", str(tmp_path / "slic_shim_sequence"), f"-L{pkg}",
                    "-lmmf_hip", "-lamdhip64", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
