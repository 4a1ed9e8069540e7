"""-m gpu: the dense-CRF motion segmentation (mmf_crf_segment, csrc/crf_kernels.hpp) at the edges of its ranges, against
tests/crf_oracle.py under the bar of test_gpu_crf.py (crf_edges.check_against_oracle: unaries bit-exact, |Q - Q_oracle| <= 1e-4,
equal argmax maps where the oracle's top-two margin is >= 1e-3, stages 8-14 replayed on the device's own argmax map exactly,
a second run with the same bits).  test_crf_edges_oracle.py asserts on the oracle alone that every case reaches its edge.

A  label counts at both ends of every crf_pair_kernel / crf_softmax_kernel instantiation, up to kCrfMaxLabels = 32
B  cell counts on and around the 64 x 128 tiles of the pair kernel and the 1024 lanes of the post kernel, one row, one
   column, ragged images, spixel_size 11 and 255, half of them without a label image (crf_grid_labels_kernel)
C  kCrfMaxCells = 16384
D  model ids that are not list positions
E  component shapes: 1200 components, a serpentine, a late merge, rings, ties across component 1024, the border band, the
   new label's size limits
F  float32-against-double thresholds, infinite and zero errors, depths on and above the 100 m clamp
G  two models with identical maps stay exactly tied
H  0, 1 and 2 iterations
I  one workspace reused at shrinking and growing sizes
J  every refusal"""
import numpy as np
import pytest

import crf_edges as ce
import crf_oracle as co

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.mark.parametrize("name", ce.names("A-") + ce.names("B-") + ce.names("D-") + ce.names("F-") + ce.names("H-"))
def test_edge_case(gpu_ctx, orc, name):
    c = ce.CASES[name]
    ref, last, data, has_new = ce.check_case(gpu_ctx, orc, name)
    assert last["cells"] == c["owner"].shape
    if name.startswith("D-"):
        assert [d["id"] for d in data] == c["ids"] + [c["next_id"]] and has_new


@pytest.mark.parametrize("name", ce.names("C-"))
def test_cell_limit(gpu_ctx, orc, name):
    """16384 cells, iterations = 0: unaries, Q = softmax(-U), the map and stages 8-14 are compared.  The pair sums are not
    compared at this size: the exact oracle holds an N x N float64 matrix (2 GiB here) and a blocked one takes tens of seconds;
    the pair kernel's grid edges are covered by group B and its size by the 4800-cell cases of test_gpu_crf.py."""
    c = ce.CASES[name]
    ref, last, data, has_new = ce.check_case(gpu_ctx, orc, name)
    assert np.array_equal(last["raw_map"], ce.intended_map(c))
    assert last["n_components"] == (16384 if name == "C-checkerboard" else 2)


@pytest.mark.parametrize("name", ce.names("E-"))
def test_component_shapes(gpu_ctx, orc, name):
    c = ce.CASES[name]
    ref, last, data, has_new = ce.check_case(gpu_ctx, orc, name)
    assert np.array_equal(last["raw_map"], ce.intended_map(c))  # before anything else says something about components
    spy, spx = c["owner"].shape
    assert last["n_components"] == len(co.connected_labels(last["raw_map"].reshape(spy, spx))[1])
    if name == "E-checkerboard":
        assert last["n_components"] == 1200
        out = last["map"].reshape(spy, spx)
        ones = out[c["owner"] == 1]
        assert (out[c["owner"] == 0] == 0).all() and ones[0] == 1 and (ones[1:] == 255).all()
    if name == "E-ties":
        out = last["map"].reshape(spy, spx)
        assert [int(out[y, x]) for y, x in ce.TIE_CELLS] == [1, 255, 255, 255, 255]
    if name == "E-u-shape":
        out = last["map"].reshape(spy, spx)
        assert out[2, 5] == out[2, 30] == out[27, 17] == 1 and (out[2:6, 8:27] == 255).all()


@pytest.mark.parametrize("name", ce.names("G-"))
def test_twin_models_stay_tied(gpu_ctx, orc, name):
    ref, last, data, has_new = ce.check_case(gpu_ctx, orc, name)
    ids = ce.CASES[name]["ids"]
    assert np.array_equal(last["q"][1].view(np.uint32), last["q"][2].view(np.uint32))
    assert (last["raw_map"] == ids[1]).any() and not (last["raw_map"] == ids[2]).any()


def test_reused_workspace(gpu_ctx, orc):
    """(N, L) = (1200, 32), (64, 2), (1200, 3) without the mean field, (1025, 17) on one context, one after the other"""
    for name in ce.REUSE_ORDER:
        ce.check_case(gpu_ctx, orc, name)


def test_refusals(gpu_ctx, orc):
    import torch
    from multimotionfusion_amd import MmfError, segmentation

    def call(W=320, H=240, M=2, ids=None, next_id=None, allow_new=True, **cfg):
        S = cfg.get("spixel_size", 16)
        n = max((W // S) * (H // S), 1)
        ids = list(range(M)) if ids is None else ids
        segmentation.segment(gpu_ctx, torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"),
                             torch.ones((H, W), dtype=torch.float32, device="cuda"),
                             torch.ones((M, 2, n), dtype=torch.float32, device="cuda"), ids, M if next_id is None else next_id,
                             allow_new, segmentation.CrfConfig(**cfg))

    refused = {
        "M33": dict(M=33, allow_new=False), "M32+new": dict(M=32), "M0": dict(M=0), "N16512": dict(W=129 * 11, H=128 * 11, spixel_size=11),
        "id255": dict(ids=[0, 255]), "duplicate": dict(M=3, ids=[0, 4, 4]), "next_id-taken": dict(ids=[0, 7], next_id=7),
        "next_id255": dict(next_id=255), "S10": dict(spixel_size=10), "S256": dict(W=512, H=512, spixel_size=256),
        "tiny-image": dict(W=15, H=240), "sigma0": dict(sigma_depth=0.0), "iterations-1": dict(iterations=-1)}
    assert list(refused) == ce.REFUSALS
    call()  # (the call itself is fine)
    for what, kw in refused.items():
        with pytest.raises(MmfError):
            call(**kw)
            pytest.fail(f"{what} was not refused")
    call(M=32, allow_new=False)  # the limits themselves are accepted
    call(W=128 * 11, H=128 * 11, spixel_size=11, iterations=0)
    call(ids=[0, 254], next_id=253)
    ce.check_case(gpu_ctx, orc, "A-L5-new-soft")  # a valid call afterwards still matches the oracle
