"""CPU: the oracle of the keypoint selection (oracle/mmf_oracle_superpoint.c from orc_sp_heatmap on) against plain references
written here, and every case of test_gpu_keypoint_edges.py against its own claim -- asserted on the oracle's results, with the
inputs the device tests use (a device comparison on a case that misses its edge proves nothing).

  orc.sp_keypoints           against a sequential greedy suppression in Python (keypoint_edges.greedy): the same keypoints in
                             the same order, and against the synchronous fixed point on the chain cases;
  orc.sp_heatmap             against float64 exp / sum where the outputs are finite and in the normal range.  Bound 70 * 2^-24
                             relative: 2 ulp of mmf_expf, 66 sequential additions of positive terms (each at most one rounding
                             of a partial sum that never exceeds the total), one division.  Measured on this draw: 3.7e-7
                             (the cell of logits near -87.4, whose terms lie at the edge of the normal range);
  orc.sp_sample_descriptors  against float64 bilinear + normalisation on the rows whose float64 norm exceeds 1e-3.  Bound 2e-5
                             absolute per component: 4 products and 3 additions on values <= 1 (7 roundings of 2^-24), a
                             256-term fmaf chain, sqrt and divide (130 roundings, relative, of a component <= 1: 7.8e-6), with
                             room for the tap roundings of a row whose taps partly cancel.  Rows of norm below 1e-3 -- the
                             zero and 1e-40 cells and whatever cancels that far -- are left out: there the division amplifies
                             the tap roundings without limit.  Measured: 1.3e-7."""
import numpy as np
import pytest

import keypoint_edges as ke
from helpers import assert_bit_equal

F32 = np.float32
SELECTION = list(ke.CASES)


@pytest.mark.parametrize("name", SELECTION)
def test_oracle_is_the_sequential_greedy(orc, name):
    c, ref = ke.CASES[name], ke.ref_of(name, orc)
    xy, conf = ke.greedy(ref["heat"], F32(c.conf_thresh), c.nms_dist, c.border)
    assert_bit_equal(ref["full_xy"], xy, "keypoints in order")
    assert_bit_equal(ref["full_conf"], conf, "their confidences")
    assert len(ref["xy"]) == min(len(xy), c.max_keypoints)


@pytest.mark.parametrize("name", SELECTION)
def test_claim_holds(orc, name):
    c = ke.CASES[name]
    assert c.claim, "a case without a claim"
    ke.assert_inputs(c)
    ke.verify(c, ke.reference(c, orc), orc)


def test_families_are_complete():
    assert {p: len(ke.names(p)) for p in ke.FAMILIES} == ke.FAMILIES
    assert sum(ke.FAMILIES.values()) == len(ke.CASES) == 56
    assert {(c.H, c.W) for c in ke.CASES.values()} == {(40, 56), (8, 8), (8, 16), (16, 8), (24, 40), (16, 24), (24, 32)}
    for m in ke.COUNT_M:
        assert f"count-m{m}" in ke.CASES
    for m in ke.CUT_M:
        assert {ke.CASES[f"count-m{m}-cut{k}"].max_keypoints for k in (1, m - 1, m, m + 1)} == {1, m - 1, m, m + 1}
        assert any(ke.CASES[f"count-m{m}-cut{k}"].claim.get("cut_tie") for k in (1, m - 1))
    assert {ke.CASES[n].border for n in ke.names("band")} == {0, 4, 20, 100} and ke.CASES["band-radius-64-max-band"].nms_dist == 64
    assert all(ke.CASES[n].H * ke.CASES[n].W <= 40 * 56 for n in ke.STALE) and [ke.CASES[n].H for n in ke.STALE] == [40, 16, 8, 40]
    assert ke.CASES["sample-16x24"].max_keypoints == 384


def test_chains_are_far_longer_than_the_fixed_passes(orc):
    """synchronous passes to the fixed point (keypoint_edges.sync_fixed_point: every candidate decides on the previous pass's
    states): 38 on either ramp, 1120 / 154 on the serpentine.  The device runs 8 list passes with the whole chip and leaves
    the rest to the finisher workgroup."""
    got = {n: ke.sync_fixed_point(ke.CASES[n].heat, F32(ke.CASES[n].conf_thresh), ke.CASES[n].nms_dist)[0] for n in ke.names("chain")}
    assert got == {"chain-raster-up": 38, "chain-raster-down": 38, "chain-serpentine-r1": 1120, "chain-serpentine-r4": 154}, got


def test_pairs_at_the_radius_and_one_past_it(orc):
    for d in (1, 4):
        at, past = ke.ref_of(f"tie-pair-d{d}-at", orc), ke.ref_of(f"tie-pair-d{d}-past", orc)
        assert len(at["xy"]) == 4 and len(past["xy"]) == 8
        firsts = {p for p, _, _ in ke.CASES[f"tie-pair-d{d}-at"].claim["pairs"]}
        assert {tuple(p) for p in at["xy"].tolist()} == firsts


def test_the_suppressed_one_does_not_come_back(orc):
    c = ke.CASES["band-suppressor-dropped"]
    assert len(ke.ref_of(c.name, orc)["xy"]) == 1
    inner = ke.reference(c._replace(border=0), orc)  # without the band the four strong ones are keypoints, the weak ones never
    assert len(inner["xy"]) == 5 and not {w for _, w in c.claim["band"]} & {tuple(p) for p in inner["xy"].tolist()}


def test_stale_sequence_changes_size_and_count(orc):
    counts = [len(ke.ref_of(n, orc)["xy"]) for n in ke.STALE]
    assert counts[1] == 384 and min(counts) > 0 and len(set(counts)) == 4, counts


def test_heatmap_against_float64(orc):
    c = ke.CASES["logits-24x32"]
    heat = orc.sp_heatmap(c.semi)
    with np.errstate(all="ignore"):
        e = np.exp(c.semi.astype(np.float64))
        dense = e[..., :64] / (e.sum(axis=2, keepdims=True) + np.float64(F32(0.00001)))
        total32 = e.sum(axis=2)
    want = dense.reshape(3, 4, 8, 8).transpose(0, 2, 1, 3).reshape(24, 32)
    tame = np.repeat(np.repeat(np.isfinite(total32) & (total32 < 1e38), 8, 0), 8, 1)  # the float32 sum does not overflow
    use = tame & np.isfinite(heat) & (heat >= ke.FLT_MIN) & np.isfinite(want)
    assert int(use.sum()) >= 128, int(use.sum())
    rel = np.abs(heat[use].astype(np.float64) - want[use]) / want[use]
    print("heat map: compared", int(use.sum()), "values, max relative error", rel.max())
    assert rel.max() <= 70 * 2.0 ** -24
    for (hc, wc), counts in c.claim["heat_cells"].items():
        assert ke.classify(heat[8 * hc:8 * hc + 8, 8 * wc:8 * wc + 8])[:3] == counts


def sample64(cdesc, xy, H, W):
    """grid_sample (corner aligned, zero padding) + normalisation in float64 -> (rows, norms)"""
    Hc, Wc = cdesc.shape[:2]
    d = np.zeros((Hc + 2, Wc + 2, 256))
    d[1:-1, 1:-1] = cdesc
    out, norms = [], []
    for x, y in xy.tolist():
        ix, iy = x / (W / 2.0) / 2.0 * (Wc - 1), y / (H / 2.0) / 2.0 * (Hc - 1)
        x0, y0 = int(np.floor(ix)), int(np.floor(iy))
        fx, fy = ix - x0, iy - y0
        v = (d[y0 + 1, x0 + 1] * (1 - fx) * (1 - fy) + d[y0 + 1, x0 + 2] * fx * (1 - fy) + d[y0 + 2, x0 + 1] * (1 - fx) * fy
             + d[y0 + 2, x0 + 2] * fx * fy)
        n = np.sqrt((v * v).sum())
        norms.append(n)
        out.append(v / n if n > 0 else v)
    return np.array(out).reshape(-1, 256), np.array(norms)


@pytest.mark.parametrize("name", ke.names("size") + ["sample-16x24", "tie-plateaus-r0", "band-border-0"])
def test_sampling_against_float64(orc, name):
    c, ref = ke.CASES[name], ke.ref_of(name, orc)
    with np.errstate(all="ignore"):
        want, norms = sample64(ref["cdesc"].astype(np.float64), ref["xy"], c.H, c.W)
    use = norms > 1e-3
    assert use.sum() >= min(len(norms), 8) // 2 and use.any()
    err = np.abs(ref["desc"][use].astype(np.float64) - want[use]).max()
    print(name, "sampled rows compared", int(use.sum()), "of", len(norms), "max abs error", err)
    assert err <= 2e-5


def test_l2_normalize_binding(orc):
    c = ke.CASES["normalise-16x24"]
    with np.errstate(all="ignore"):
        got = orc.sp_l2_normalize(c.desc)
    row = c.desc[0, 0].astype(np.float64)
    assert np.abs(got[0, 0] - row / np.sqrt((row * row).sum())).max() <= 130 * 2.0 ** -24
    assert got.shape == c.desc.shape and not np.shares_memory(got, c.desc)
