"""CPU: the cases of tests/photo_edges.py hold what they claim on the oracle, the oracle agrees record for record with a
plain restatement of Core/Cuda/reduce.cu:773-836, and the cases tell that restatement from each of its deliberately wrong
variants.  Nothing here needs a GPU; tests/test_gpu_photo_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import photo_edges as pe
from helpers import assert_bit_equal

CASES = pe.standalone_cases()
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in pe.FAMILIES}


def records(orc, case):
    rec, sumsq, count, err = pe.oracle_result(orc, case.name)
    return rec.view(pe.RECORD)[..., 0], sumsq, count, err


@pytest.mark.parametrize("family", pe.FAMILIES)
def test_every_claim_holds_on_the_oracle(orc, family):
    assert BY_FAMILY[family]
    for case in BY_FAMILY[family]:
        rec, sumsq, count, err = records(orc, case)
        claim = case.claim
        rows, cols = case.next_image.shape
        assert np.array_equal(rec["valid"] == 1, claim["valid"]), (case.name, np.argwhere((rec["valid"] == 1) != claim["valid"])[:6].tolist())
        assert count == claim["count"] == int(claim["valid"].sum()), case.name
        # a record is the pixel itself, where it lands, and the difference of the two intensities; zeros where there is none
        yy, xx = np.nonzero(claim["valid"])
        assert np.array_equal(rec["one_x"][yy, xx], xx) and np.array_equal(rec["one_y"][yy, xx], yy), case.name
        landed = case.last_image[rec["zero_y"][yy, xx], rec["zero_x"][yy, xx]].astype(np.int64)
        assert np.array_equal(rec["diff"][yy, xx], (case.next_image[yy, xx].astype(np.int64) - landed).astype(np.float32)), case.name
        assert sumsq == int(((case.next_image[yy, xx].astype(np.int64) - landed) ** 2).sum()), case.name
        assert not pe.record_bytes(rec)[~claim["valid"]].any(), case.name
        assert_bit_equal(err, np.where(claim["valid"], np.float32(0.001) * (rec["diff"] * rec["diff"]).astype(np.int32).astype(np.float32),
                                       np.float32(0)).astype(np.float32), case.name + ": error map")
        for (x, y), (u0, v0) in claim.get("zero", {}).items():
            assert (rec["zero_x"][y, x], rec["zero_y"][y, x], rec["valid"][y, x]) == (u0, v0, 1), (case.name, x, y)
        for x, y in claim.get("invalid", ()):
            assert rec["valid"][y, x] == 0, (case.name, x, y)
        if "sumsq" in claim:
            assert sumsq == claim["sumsq"], case.name
        if claim.get("oob"):
            assert count == 0, case.name
        if "zero" not in claim and np.array_equal(case.krkinv, pe.EYE) and not case.kt[2]:  # a pure shift (the identity but for `last_shifted`)
            assert np.array_equal(rec["zero_x"][yy, xx], xx + int(case.kt[0])) and np.array_equal(rec["zero_y"][yy, xx], yy + int(case.kt[1])), case.name


def test_window_lattice_covers_every_column_and_row_position():
    cols, rows = 40, 16
    zeros = {z for c in BY_FAMILY["window"] if "lattice" in c.name for z in c.claim["zeros"]}
    assert {x for x, _ in zeros} == set(range(cols)) and {y for _, y in zeros} == set(range(rows))
    assert zeros == {(x, y) for x in range(cols) for y in range(rows)}
    for case in BY_FAMILY["window"]:  # the claim is geometry: the band minus a 4 x 4 box per zero
        want = pe.band(cols, rows)
        for x0, y0 in case.claim["zeros"]:
            assert case.next_image[y0, x0] == 0
            for y in range(y0 - 1, y0 + 3):
                for x in range(x0 - 1, x0 + 3):
                    if 0 <= x < cols and 0 <= y < rows:
                        want[y, x] = False
        assert np.array_equal(want, case.claim["valid"]) and int((case.next_image == 0).sum()) == len(case.claim["zeros"]), case.name
    blocks = next(c for c in BY_FAMILY["window"] if c.name == "window_blocks").claim["zeros"]
    assert {(3, 5), (4, 5)} <= set(blocks) and {(15, 10), (16, 10)} <= set(blocks)  # across the boundary of two groups of four


def test_border_sizes_are_the_issue_s():
    assert {c.next_image.shape[::-1] for c in BY_FAMILY["border"]} == {(c, r) for c in (4, 5, 6, 8, 9, 12, 13, 20, 24) for r in (1, 2, 3, 5)}
    for c in BY_FAMILY["border"]:
        rows, cols = c.next_image.shape
        assert c.claim["count"] == max(cols - 5, 0) * max(rows - 1, 0)


def test_the_restatement_agrees_with_the_oracle_record_for_record(orc):
    """every family (the issue asks for the integer ones; the float ones agree as well, being the same float32 operations)"""
    for case in CASES:
        rec, sumsq, count, _ = pe.oracle_result(orc, case.name)
        mine, n, s = pe.restate(case)
        assert (n, s) == (count, sumsq), case.name
        assert_bit_equal(pe.record_bytes(mine), rec, case.name)


def test_ties_and_equalities_are_exact_in_float64():
    n_ties = n_eq = n_beyond = 0
    for case in BY_FAMILY["warp"]:
        rows, cols = case.next_image.shape
        K, kt = case.krkinv.astype(np.float64).reshape(9), case.kt.astype(np.float64)
        for x, y, qx, qy in case.claim["ties"]:
            z = K[6] * x + K[7] * y + K[8] + kt[2]
            ex, ey = (K[0] * x + K[1] * y + K[2] + kt[0]) / z, (K[3] * x + K[4] * y + K[5] + kt[1]) / z  # depth 1
            assert (ex, ey) == (qx, qy) and (qx % 1 == 0.5 or qy % 1 == 0.5), (case.name, x, y)
            for q in (qx, qy):
                if q % 1 == 0.5:
                    assert pe.rn(np.float32(q)) % 2 == 0 and abs(pe.rn(np.float32(q)) - q) == 0.5
                    n_ties += 1
    for case in BY_FAMILY["depth"]:
        for td1, d0, delta, side in case.claim.get("exact64", ()):
            a = abs(np.float64(td1) - np.float64(d0))
            assert {"==": a == np.float64(delta), "<": a < np.float64(delta), ">": a > np.float64(delta)}[side], (case.name, td1, d0)
            if side != "==":  # one ulp of d0 away from the equality, on the stated side
                assert abs(a - np.float64(delta)) <= np.spacing(np.float32(d0))
                n_beyond += 1
            else:
                n_eq += 1
    print(f"ties {n_ties}, depth equalities {n_eq}, one ulp beside {n_beyond}")
    assert n_ties > 200 and n_eq == 6 and n_beyond == 12


def test_the_cases_discriminate(orc):
    """Each wrong variant of the restatement changes the count or a record of at least one case.  The one variant that cannot
    (photo_edges.UNOBSERVABLE: the arithmetic of reduce.cu:808, 816 makes :806 redundant) is shown to change nothing."""
    right = {c.name: pe.restate(c) for c in CASES}
    table = {}
    for variant in pe.VARIANTS:
        caught = []
        for case in CASES:
            rec, n, s = pe.restate(case, variant)
            ref, rn_, rs = right[case.name]
            if (n, s) != (rn_, rs) or not np.array_equal(pe.record_bytes(rec), pe.record_bytes(ref)):
                caught.append(case.name)
        table[variant] = caught
    print("\nvariant -> cases that catch it")
    for variant, caught in table.items():
        print(f"  {variant:28s} {len(caught):3d}  {', '.join(caught[:4])}{' ...' if len(caught) > 4 else ''}")
    for variant, caught in table.items():
        if variant in pe.UNOBSERVABLE:
            assert not caught, (variant, caught)
            assert any(np.isnan(c.next_depth).any() for c in BY_FAMILY["depth"])  # (the NaN depths are there)
        else:
            assert caught, variant
    # and the family each variant belongs to is among those that catch it
    expect = {"window 3x3": "window", "window rows i-2..i+2": "window", "window not clipped": "border", "x < cols - 4": "border",
              "y < rows": "border", "mTwo > min_scale": "gate", "round half up": "warp", "truncate": "warp", "u0 <= cols": "warp",
              "v0 < rows - 1": "warp", "d0 >= 0": "depth", "|td1 - d0| < delta": "depth", "last_image test dropped": "last"}
    families = {c.name: c.family for c in CASES}
    for variant, family in expect.items():
        assert family in {families[n] for n in table[variant]}, (variant, family)


def test_step_and_so3_cases_are_what_they_say(orc):
    """the exact rgbStep cases: the oracle's double sums ARE the float64 restatement's (so the asserted exactness is the
    oracle's); the SO3 cases: the claimed `found` counts are the oracle's"""
    for case in pe.step_exact_cases():
        rows, cols = case.dIdx.shape
        assert (cols, rows) in pe.STEP_SIZES and case.sigma == -1
        rec = case.corres.view(pe.RECORD)[..., 0]
        assert int(rec["valid"].sum()) == case.claim["valid"]
        assert (rec["zero_x"] >= 0).all() and (rec["zero_x"] < cols).all() and (rec["zero_y"] >= 0).all() and (rec["zero_y"] < rows).all()
        out = orc.rgb_step(case.corres, case.sigma, case.cloud, case.fx, case.fy, case.dIdx, case.dIdy, case.sobel_scale)
        if case.claim["kind"] == "z0":
            assert not np.isfinite(out[:27]).all()
            continue
        r = pe.step_rows64(case)
        want = np.array([(r[:, i] * r[:, j]).sum() for i, j in pe.SE3_PAIRS])
        assert np.array_equal(out[:27], want), case.name
        assert np.array_equal(out[:27].astype(np.float32).astype(np.float64), out[:27])
        if case.claim["kind"] == "none":
            assert not out.any()
    for case in pe.so3_cases():
        out = orc.so3_step(case.last_image, case.next_image, case.B, case.kinv, case.krlr)
        if "found" in case.claim:
            assert out[10] == case.claim["found"], case.name
        if case.claim.get("exact"):
            r, found = pe.so3_rows64(case)
            want = np.array([(r[:, i] * r[:, j]).sum() for i in range(4) for j in range(i, 4)]) if len(r) else np.zeros(10)
            assert np.array_equal(out[:10], want) and out[10] == found, case.name


def test_static_cases_stay_at_the_identity_on_the_oracle(orc):
    """(the builders assert it; this names what they asserted) the pose bit-equal to the start in every mode of the case, the
    iterations the mode prescribes, lastRGBCount the claimed count, the error image zero"""
    cases = pe.static_cases(orc)
    assert {(c.w, c.h) for c in cases} == {pe.FORCED_PX_SIZE, pe.ALIGNED_PYRAMID_SIZE}
    w2, h2 = (v >> 2 for v in pe.ALIGNED_PYRAMID_SIZE)
    assert w2 % 4 == 0 and w2 >= 8 and h2 >= 4 and (pe.FORCED_PX_SIZE[0] >> 2) % 4 != 0
    for c in cases:
        pe.assert_static(orc, c)
        assert c.claim["count"] == c.claim["clean"] - c.claim["removed"] and c.claim["count"] > 0
        print(c.name, c.modes, c.claim)
    for px in pe.NATURAL_PX_SIZES:
        c = pe.natural_case(orc, px)
        assert pe.geometry_px(c.w, c.h) == px and c.claim["removed"] > 1000
        print(c.name, c.claim)
