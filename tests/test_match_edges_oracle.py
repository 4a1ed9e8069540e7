"""CPU: the matcher's edge cases (tests/match_edges.py) against the oracle (oracle/mmf_oracle_match.c) -- every case has the
property it claims, the oracle follows the non-finite contract, and the oracle is pinned to float64 at every dim.

The rounding bound.  d2 = fl(fl(qn + tn) - 2 g) with qn, tn, g the fmaf chains s_k = fl(s_{k-1} + a_k b_k), s_0 = 0, of
n = dim terms, u = 2^-24, no underflow (the partial sums of these inputs are normal numbers or exact zeros).

  * A chain is the recursive summation of the n exact products (an fmaf rounds once) in n roundings, so
    |chain - sum| <= n u sum |a_k b_k| with no higher-order term (Jeannerod and Rump, "Improved error bounds for inner
    products in floating-point arithmetic", 2013).  Hence |qn^ - |q|^2| <= n u |q|^2, the same for tn, and
    |g^ - <q, t>| <= n u |q| |t| by Cauchy-Schwarz.
  * The three chains therefore move (qn + tn) - 2 g by at most n u (|q|^2 + |t|^2 + 2 |q| |t|) = n u S, S = (|q| + |t|)^2.
  * First rounding, A = qn^ + tn^ -> A (1 + d1): at most u A <= u (1 + n u) (|q|^2 + |t|^2).  2 g^ is exact.
  * Second rounding, B = fl(A) - 2 g^ -> B (1 + d2): at most u |B| <= u (|q - t|^2 + n u S + u A).
  * |q|^2 + |t|^2 + |q - t|^2 = 2 S - 4 |q| |t| - 2 <q, t> <= 2 S - 2 |q| |t|.

Sum: |d2 - d2_exact| <= (n + 2) u S - 2 u |q| |t| + (2 n + 2) u^2 S, and the last term is below the one before it whenever
|q| |t| / S > (n + 1) u, i.e. unless one norm is some 1e-5 of the other (both rows zero: every term is 0).  So the bound
is (dim + 2) 2^-24 (|q| + |t|)^2; the test asserts the norm condition on the cases it uses, and the float64 reference's own
error (n 2^-53 S) disappears in the same slack.
"""
import numpy as np
import pytest

import match_edges as me
from helpers import assert_bit_equal
from test_oracle_match import brute_force

U = 2.0 ** -24


@pytest.fixture(scope="module")
def cases(orc):
    return me.all_cases(orc)


def d2_f64(q, t):
    q, t = q.astype(np.float64), t.astype(np.float64)
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)


def bound(q, t):
    """(dim + 2) 2^-24 (|q_i| + |t_j|)^2 for every pair, in float64"""
    nq, nt = np.linalg.norm(q.astype(np.float64), axis=1), np.linalg.norm(t.astype(np.float64), axis=1)
    return (q.shape[1] + 2) * U * (nq[:, None] + nt[None, :]) ** 2


def check_expect(case, idx, dist):
    for i, j in case.claim.get("expect", {}).items():
        assert idx[i] == j and dist[i] == 0, (case.name, i, j, idx[i], dist[i])


def test_the_case_table(cases):
    names = [c.name for c in cases]
    assert sum(n.startswith("dims") for n in names) == 31 and max(max(len(c.q), len(c.t)) for c in cases) <= 130
    for dims, kernel in ((me.ONE_WAVE_DIMS, False), (me.TILE64_DIMS, True)):
        assert all((d % 32 == 0) == kernel for d in dims)
        seen = {s for d in dims for s in me.DIMS_SHAPES[d]}
        assert seen == set(range(len(me.SHAPES)))  # each kernel meets every shape
    assert me.EPS == np.float32(2.0 ** -23)


def test_sign_cases_have_their_sign_pattern(orc, cases):
    sign = [c for c in cases if c.name.startswith("sign")]
    assert len(sign) == 8
    for c in sign:
        d2 = orc.match_d2(c.q, c.t)
        special = set(c.claim["zero"]) | set(c.claim["neg"])
        for p in c.claim["zero"]:
            assert d2[p] == 0 and not np.signbit(d2[p]), (c.name, p, d2[p])
        for p in c.claim["neg"]:
            assert d2[p] < 0, (c.name, p, d2[p])
        r, k = c.claim["pos_row"], c.claim["pos_col"]
        assert all(d2[r, j] > 0 for j in range(len(c.t)) if (r, j) not in special), c.name
        assert all(d2[i, k] > 0 for i in range(len(c.q)) if (i, k) not in special), c.name
        if "more_negative" in c.claim:
            a, b = c.claim["more_negative"]
            assert d2[a] < d2[b] < 0, (c.name, d2[a], d2[b])
        far = [abs(a - b) for (i, a) in c.claim["zero"] for (_, b) in c.claim["neg"]] if c.name.endswith("train") else \
              [abs(a - b) for (a, _) in c.claim["zero"] for (b, _) in c.claim["neg"]]
        assert min(far) >= 64  # the duplicate and its neighbours lie in different workgroups of either kernel
        check_expect(c, *orc.match_descriptors(c.q, c.t, c.gate))


def test_tie_cases_tie_where_they_say(orc, cases):
    tie = [c for c in cases if c.name.startswith("tie")]
    assert len(tie) == 12
    for c in tie:
        d2 = orc.match_d2(c.q, c.t)
        if c.claim.get("all_zero_d2"):
            assert d2.shape == (130, 130) and (d2 == 0).all()
        else:
            axis, at, other = c.claim["copies"]
            line = d2[other] if axis == "t" else d2[:, other]
            assert (line[list(at)] == 0).all() and (np.delete(line, list(at)) > 0).all(), c.name
            assert {a // 64 for a in at} == {0, 1, 2} or at == me.TIE_LATE  # TIE_ALL: copies in three 64-row workgroups
        check_expect(c, *orc.match_descriptors(c.q, c.t, c.gate))


def test_gate_cases(orc, cases):
    gate = {c.name: c for c in cases if c.name.startswith("gate")}
    assert len(gate) == 8
    q, t = gate["gate_zero"].q, gate["gate_zero"].t
    off_i, off_d = orc.match_descriptors(q, t, 0.0)
    for c in gate.values():
        idx, dist = orc.match_descriptors(c.q, c.t, c.gate)
        if c.claim.get("gate_off"):
            assert_bit_equal(idx, off_i, c.name), assert_bit_equal(dist, off_d, c.name)
        elif c.claim.get("none"):
            assert (idx == -1).all() and (dist == 0).all()
        else:  # the gate is on: exactly the gate-off matches at a distance <= gate
            keep = (off_i >= 0) & (off_d <= np.float32(c.gate))
            assert_bit_equal(idx, np.where(keep, off_i, -1).astype(np.int32), c.name)
            assert_bit_equal(dist, np.where(keep, off_d, 0).astype(np.float32), c.name)
            check_expect(c, idx, dist)
            if "kept" in c.claim:
                m = c.claim["kept"]
                assert idx[m] == off_i[m] >= 0 and dist[m] == np.float32(c.gate) and 0 < keep.sum() < (off_i >= 0).sum()
            if "dropped" in c.claim:
                m = c.claim["dropped"]
                assert idx[m] == -1 and off_i[m] >= 0 and off_d[m] == np.nextafter(np.float32(c.gate), np.float32(1))
    assert (orc.match_descriptors(q, t, float(me.EPS))[0] >= 0).sum() == 1  # only the exact duplicate passes the smallest gate


def nonfinite(cases):
    return [c for c in cases if c.name.startswith("nonfinite")]


def test_nonfinite_cases_are_nonfinite(orc, cases):
    assert len(nonfinite(cases)) == 24
    for c in nonfinite(cases):
        d2 = orc.match_d2(c.q, c.t)
        bad = np.zeros(d2.shape, bool)
        bad[list(c.claim["bad_q"]), :] = True
        bad[:, list(c.claim["bad_t"])] = True
        assert bad.any() and np.isfinite(d2[~bad]).all(), c.name
        kinds = {k for k, hit in (("inf", np.isposinf(d2[bad]).any()), ("nan", np.isnan(d2[bad]).any())) if hit}
        assert kinds == set(c.claim["kinds"]) and not np.isfinite(d2[bad]).any() and not np.isneginf(d2[bad]).any(), (c.name, kinds)


@pytest.mark.parametrize("name", [c.name for c in me.nonfinite_cases()])
def test_nonfinite_rows_match_nothing_and_change_nothing(orc, cases, name):
    """the contract (the matcher): the result is that of the sets without the offending rows.  An oracle whose
    scans take the first pair of a row or column unconditionally fails 10 of these 24: all_fillers with the gate off (query
    0 matched to filler 0 at distance +inf), and nan_query and nan_train at either gate (a NaN taken first is never replaced,
    and sqrt(max(NaN, 0)) reports it as a match at distance 0, which passes every gate)."""
    c = next(c for c in cases if c.name == name)
    q, t, kq, kt = me.without_bad_rows(c)
    want_i, want_d = me.map_back(c, *orc.match_descriptors(q, t, c.gate), kq, kt)
    idx, dist = orc.match_descriptors(c.q, c.t, c.gate)
    assert_bit_equal(idx, want_i, c.name), assert_bit_equal(dist, want_d, c.name)
    assert (want_i >= 0).any() or "all_fillers" in c.name


def test_scale_cases_scale_exactly(orc, cases):
    scale = {c.name: c for c in cases if c.name.startswith("scale")}
    assert len(scale) == 6
    for c in scale.values():
        if "base" in c.claim:
            b, s = scale[c.claim["base"]], np.float32(c.claim["scale"])
            assert_bit_equal(orc.match_d2(c.q, c.t), orc.match_d2(b.q, b.t) * s * s, c.name)
            (bi, bd), (ci, cd) = orc.match_descriptors(b.q, b.t, b.gate), orc.match_descriptors(c.q, c.t, c.gate)
            assert_bit_equal(ci, bi, c.name), assert_bit_equal(cd, bd * s, c.name)
            assert 0 < (bi >= 0).sum() < len(bi)


def test_d2_within_the_rounding_bound_of_float64_for_every_pair(orc, cases):
    pairs = 0
    for c in cases:
        if not me.finite(c) or not c.q.size or not c.t.size:
            continue
        nq, nt = np.linalg.norm(c.q.astype(np.float64), axis=1), np.linalg.norm(c.t.astype(np.float64), axis=1)
        lo, hi = min(nq.min(), nt.min()), max(nq.max(), nt.max())
        assert hi == 0 or lo / hi > 2.0 ** -4, c.name  # the condition of the derivation, with room
        err = np.abs(orc.match_d2(c.q, c.t).astype(np.float64) - d2_f64(c.q, c.t))
        assert (err <= bound(c.q, c.t)).all(), (c.name, float((err / np.maximum(bound(c.q, c.t), 1e-300)).max()))
        pairs += err.size
    assert pairs > 100000


def test_matches_equal_float64_brute_force_where_the_margin_allows(orc, cases):
    """a query is decidable when, in float64, its row's best beats the second best by more than twice the bound, and so does
    the column of that best: then no rounding within the bound can change either arg-min"""
    decidable = total = 0
    for c in cases:
        if not c.name.startswith("dims"):
            continue
        d2, b = d2_f64(c.q, c.t), 2 * bound(c.q, c.t)
        ref, _ = brute_force(c.q, c.t, 0.0)
        idx, _ = orc.match_descriptors(c.q, c.t, 0.0)
        for i in range(len(c.q)):
            j = int(d2[i].argmin())
            row, col = np.sort(d2[i]), np.sort(d2[:, j])
            ok = (len(row) < 2 or row[1] - row[0] > b[i].max()) and (len(col) < 2 or col[1] - col[0] > b[:, j].max())
            total += 1
            if ok:
                decidable += 1
                assert idx[i] == ref[i], (c.name, i, idx[i], ref[i])
    assert total > 1500 and decidable >= 0.9 * total, (decidable, total)


def test_dims_cases_find_their_tracked_rows(orc, cases):
    for c in cases:
        if c.name.startswith("dims"):
            idx, dist = orc.match_descriptors(c.q, c.t, c.gate)
            perm = c.claim["perm"]
            assert (idx[:len(perm)] == perm).all() and (dist[:len(perm)] < 0.7).all(), c.name
