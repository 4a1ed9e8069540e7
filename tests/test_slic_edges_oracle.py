"""CPU: the plain-Python reference of tests/slic_edges.py against the C oracle (oracle/mmf_oracle_slic.c) wherever that one is
defined, and every case of test_gpu_slic_edges.py against its own claim -- asserted on the reference alone, with the inputs the
device tests use (a device comparison on a case that misses its edge proves nothing).

The C oracle indexes its arrays by label and divides integers by the count, so it is compared on the cases whose labels all
lie in [0, n); the others rest on the four rules of DESIGN.md section 6, which the reference states and the claims pin."""
import numpy as np
import pytest

import slic_edges as se
from helpers import assert_bit_equal

F32 = np.float32


@pytest.mark.parametrize("name", [n for n, c in se.CASES.items() if se.oracle_defined(c)])
def test_reference_is_the_oracle(orc, name):
    c, ref = se.CASES[name], se.REF[name]
    i = c.inputs
    assert_bit_equal(ref["plain"], orc.slic_downsample(c.labels, c.S, i["image"], channel=i["channel"]), "plain")
    assert_bit_equal(ref["thr"], orc.slic_downsample(c.labels, c.S, i["image"], channel=i["channel"], threshold=i["threshold"]), "thresholded")
    assert_bit_equal(ref["counts"], orc.slic_counts(c.labels, se.cells(c)), "counts")
    assert_bit_equal(ref["rgb"], orc.slic_downsample_rgb(c.labels, c.S, i["rgb"]), "rgb")
    if c.labels.max() < i["map"].size:
        assert_bit_equal(ref["up"], orc.slic_upsample_u8(c.labels, i["map"]), "upsample")


def test_the_oracle_covers_most_cases():
    defined = [n for n, c in se.CASES.items() if se.oracle_defined(c)]
    undefined = sorted(set(se.CASES) - set(defined))
    assert undefined == sorted(se.names("oob") + ["chain-no-substitute", "up-map-larger-than-the-grid"])
    assert len(defined) == len(se.CASES) - 7


@pytest.mark.parametrize("name", list(se.CASES))
def test_claim_holds(name):
    """(the builder asserted it already; a case that loses its claim fails at import, this keeps the claims in the report)"""
    c = se.CASES[name]
    assert c.claim, "a case without a claim"
    se.verify(c, se.reference(c))


def test_families_are_complete():
    assert {p: len(se.names(p)) for p in se.FAMILIES} == se.FAMILIES
    assert sum(se.FAMILIES.values()) == len(se.CASES) == 34
    shapes = {(c.W, c.H, c.S) for c in se.CASES.values()}
    assert {(11, 11, 11), (33, 47, 11), (75, 26, 13), (130, 24, 12), (160, 128, 16), (255, 255, 255)} <= shapes
    assert max(c.W * c.H for c in se.CASES.values()) == 255 * 255


def test_chain_depths_are_the_claimed_ones():
    """depth 2 and 3 into a finished mean, depth 2 into a raw sum, a self-substitute, an absent label, no substitute"""
    got = {n: se.REF[n]["chains_thr"] for n in se.names("chain")}
    assert got["chain-d2-lower"] == {30: (1, "lower"), 50: (2, "lower")}
    assert got["chain-d3-lower"] == {33: (1, "lower"), 51: (2, "lower"), 70: (3, "lower")}
    assert got["chain-d2-higher"] == {20: (1, "higher"), 40: (2, "higher")}
    assert got["chain-self"] == {3: (1, "self"), 45: (2, "self")}
    for n in ("chain-d2-lower", "chain-d3-lower", "chain-d2-higher", "chain-self"):  # plain mode cannot chain: every label has pixels
        assert se.REF[n]["chains_plain"] == {} and (se.REF[n]["counts"] > 0).all()
    assert se.REF["chain-absent"]["chains_plain"] == {37: (1, "lower"), 62: (1, "higher")}
    assert set(se.REF["chain-no-substitute"]["chains_plain"].values()) == {(1, "none")}
    # the values are the in-place walk's: each level divides by the plain count of the substitute it reads
    c, r = se.CASES["chain-d3-lower"], se.REF["chain-d3-lower"]
    thr, cnt = r["thr"].ravel(), r["counts"]
    assert thr[33] == thr[14] / F32(cnt[14]) and thr[51] == thr[33] / F32(cnt[33]) and thr[70] == thr[51] / F32(cnt[51])
    assert thr[70] != 0 and np.isfinite(thr[70])
    c, r = se.CASES["chain-d2-higher"], se.REF["chain-d2-higher"]
    thr, cnt = r["thr"].ravel(), r["counts"]
    raw = se.pixel_order_sums(c.labels, 80, c.inputs["image"].ravel(), c.inputs["threshold"])[0][60]
    assert thr[20] == raw / F32(cnt[60]) and thr[40] == thr[20] / F32(cnt[20]) and thr[20] != thr[60]


def test_truncation_and_clamp_pick_other_substitutes():
    c = se.CASES["index-odd-S-truncation"]
    assert c.S % 2 == 1 and se.resample_empty_index(c.labels, c.S, 3) == 8 and se.resample_empty_index(c.labels, c.S, 3, "round") == 6
    assert not se.same(se.reference(c, "round")["plain"], se.REF[c.name]["plain"])
    c = se.CASES["index-clamped-row"]
    assert (4 // 2) * 13 + 6 >= c.H and se.resample_empty_index(c.labels, c.S, 4) == 7 == c.labels[c.H - 1, 58]
    assert se.resample_empty_index(c.labels, c.S, 4, "spx") == 3 and se.resample_empty_index(c.labels, c.S, 4, "clamp") == 9
    for variant in ("spx", "clamp"):
        assert not se.same(se.reference(c, variant)["plain"], se.REF[c.name]["plain"])
    for name in ("shape-33x47-S11", "shape-75x26-S13"):  # portrait and landscape: index / spy is visible both ways
        c = se.CASES[name]
        assert (c.W // c.S != c.H // c.S) and not se.same(se.reference(c, "spx")["plain"], se.REF[name]["plain"])


def test_order_sensitive_sums_differ_when_reversed():
    c = se.CASES["sum-order-sensitive"]
    for s in c.claim["order"]:
        vals = c.inputs["image"][c.labels == s]
        zeros = np.zeros(len(vals), np.int32)
        assert se.pixel_order_sums(zeros, 1, vals, None)[0][0] != se.pixel_order_sums(zeros, 1, vals[::-1], None)[0][0]


def test_sequence_shrinks_and_grows():
    ns, dedup = [se.cells(se.CASES[n]) for n, _ in se.SEQUENCE], []
    for n in ns:
        if not dedup or dedup[-1] != n:
            dedup.append(n)
    assert dedup == [80, 1, 12, 80, 10]
    modes = [m for _, m in se.SEQUENCE]
    assert set(modes) == {"plain", "thr", "rgb"} and all(a != b for a, b in zip(modes, modes[1:]))
    assert any(a == ("chain-d3-lower", "thr") and b == ("chain-d3-lower", "plain") for a, b in zip(se.SEQUENCE, se.SEQUENCE[1:]))


def test_same_excludes_only_the_nan_payload():
    a = np.array([1.0, np.nan, -0.0], F32)
    b = a.copy()
    b.view(np.uint32)[1] ^= 0x80000001  # another sign and payload
    assert se.same(a, b) and not se.same(a, np.array([1.0, np.nan, 0.0], F32)) and not se.same(a, np.array([1.0, 2.0, -0.0], F32))
    with pytest.raises(AssertionError):
        se.assert_same(a, np.array([1.0, np.nan, 0.0], F32), "signed zero")
