"""-m gpu: the descriptor matcher (csrc/match_kernels.hpp: the one-wave kernel for dim % 32 != 0, the 64 x 64 kernel otherwise)
and the view store's batched matcher (csrc/redetect_kernels.hpp) on the edge cases of tests/match_edges.py -- negative d2
beside an exact duplicate's 0, ties across tiles and workgroups, gates at a match's distance and at the epsilon, rows of
1e30 / NaN / inf, exact scalings, and one context's workspace reused by calls that shrink and grow.  Against the oracle bit
for bit (tests/test_match_edges_oracle.py pins the oracle and the cases' claims on the CPU), and the metamorphic expectations
on the device's own results."""
import numpy as np
import pytest
import torch

import match_edges as me
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()  # (a copy: the cases are read-only)


def device_match(gpu_ctx, q, t, gate, what):
    """matchDescriptors twice on the same inputs: the same bits both times"""
    from multimotionfusion_amd.matcher import matchDescriptors
    dq, dt = dev(q), dev(t)
    (i1, d1), (i2, d2) = matchDescriptors(gpu_ctx, dq, dt, gate), matchDescriptors(gpu_ctx, dq, dt, gate)
    i1, d1 = i1.cpu().numpy(), d1.cpu().numpy()
    assert_bit_equal(i2.cpu().numpy(), i1, what + ": indices of the second run")
    assert_bit_equal(d2.cpu().numpy(), d1, what + ": distances of the second run")
    return i1, d1


def run_both(gpu_ctx, orc, q, t, gate, what):
    gi, gd = device_match(gpu_ctx, q, t, gate, what)
    oi, od = orc.match_descriptors(q, t, gate)
    assert_bit_equal(gi, oi, what + ": train indices")
    assert_bit_equal(gd, od, what + ": distances")
    return gi, gd


def check_expect(case, idx, dist):
    for i, j in case.claim.get("expect", {}).items():
        assert idx[i] == j and dist[i] == 0, (case.name, i, j, idx[i], dist[i])


@pytest.mark.parametrize("family", ["dims", "sign", "tie", "gate", "nonfinite", "scale"])
def test_every_case_equals_the_oracle(gpu_ctx, orc, family):
    cases = me.by_prefix(orc, family)
    assert len(cases) == {"dims": 31, "sign": 8, "tie": 12, "gate": 8, "nonfinite": 24, "scale": 6}[family]
    for c in cases:
        idx, dist = run_both(gpu_ctx, orc, c.q, c.t, c.gate, c.name)
        check_expect(c, idx, dist)
        if "perm" in c.claim:
            perm = c.claim["perm"]
            assert (idx[:len(perm)] == perm).all(), c.name
        if c.claim.get("none"):
            assert (idx == -1).all() and (dist == 0).all(), c.name
        if "kept" in c.claim:
            assert idx[c.claim["kept"]] >= 0 and dist[c.claim["kept"]] == np.float32(c.gate), c.name
        if "dropped" in c.claim:
            assert idx[c.claim["dropped"]] == -1, c.name


def test_nonfinite_rows_match_nothing_and_change_nothing(gpu_ctx, orc):
    """on the device's own results: the sets with the offending rows deleted give the same matches"""
    for c in me.by_prefix(orc, "nonfinite"):
        q, t, kq, kt = me.without_bad_rows(c)
        want_i, want_d = me.map_back(c, *device_match(gpu_ctx, q, t, c.gate, c.name + " reduced"), kq, kt)
        idx, dist = device_match(gpu_ctx, c.q, c.t, c.gate, c.name)
        assert_bit_equal(idx, want_i, c.name + ": train indices"), assert_bit_equal(dist, want_d, c.name + ": distances")
        assert (idx[list(c.claim["bad_q"])] == -1).all() and not np.isin(idx, list(c.claim["bad_t"])).any(), c.name


def test_a_power_of_four_scales_the_distances_exactly(gpu_ctx, orc):
    scale = {c.name: c for c in me.by_prefix(orc, "scale")}
    for c in scale.values():
        if "base" in c.claim:
            b, s = scale[c.claim["base"]], np.float32(c.claim["scale"])
            bi, bd = device_match(gpu_ctx, b.q, b.t, b.gate, b.name)
            ci, cd = device_match(gpu_ctx, c.q, c.t, c.gate, c.name)
            assert_bit_equal(ci, bi, c.name + ": train indices"), assert_bit_equal(cd, bd * s, c.name + ": distances")
            assert 0 < (bi >= 0).sum() < len(bi)


@pytest.mark.parametrize("dim", [256, 24])
def test_workspace_reused_by_calls_that_shrink_and_grow(gpu_ctx, orc, dim):
    """one context: the column keys of a call (keys + nq) lie where an earlier call kept its row keys"""
    for k, (q, t, gate) in enumerate(me.workspace_calls(dim)):
        assert (len(q), len(t)) == me.WORKSPACE_SEQUENCE[k]
        run_both(gpu_ctx, orc, q, t, gate, f"call {k} {q.shape} x {t.shape}")


def view_cuts(t):
    """three views of 100, 33 and 1 rows (fewer where the train set is smaller) cut from a train set"""
    n = len(t)
    return [t[:min(100, n)], t[max(0, n - 33):], t[n // 2:n // 2 + 1]]


@pytest.mark.parametrize("family", ["sign_d256", "tie_d256", "nonfinite_d256"])
def test_view_store_on_the_edge_cases(gpu_ctx, orc, family):
    from multimotionfusion_amd.redetection import ViewStore
    cases = [c for c in me.by_prefix(orc, family) if c.gate == 0.0]  # (the view store has no gate)
    assert len(cases) == {"sign_d256": 4, "tie_d256": 6, "nonfinite_d256": 6}[family]
    for c in cases:
        for views in ([c.t], view_cuts(c.t)):
            vs = ViewStore(gpu_ctx)
            assert vs.store(1, [(v, np.zeros((len(v), 3), np.float32)) for v in views]) is True
            q = dev(c.q)
            idx, dist = vs.match(q)
            idx2, dist2 = vs.match(q)
            assert idx.shape == (len(views), len(c.q))
            assert_bit_equal(idx2, idx, c.name + ": second run"), assert_bit_equal(dist2, dist, c.name + ": second run")
            for k, v in enumerate(views):
                oi, od = orc.match_descriptors(c.q, v, 0.0)
                assert_bit_equal(idx[k], oi, f"{c.name} view {k} of {len(views)}: train indices")
                assert_bit_equal(dist[k], od, f"{c.name} view {k} of {len(views)}: distances")
            if len(views) == 1:
                check_expect(c, idx[0], dist[0])
            vs.close()


def raw_call(gpu_ctx, q_ptr, nq, t_ptr, nt, dim, idx, dist):
    from multimotionfusion_amd._capi import check
    check(gpu_ctx.lib.mmf_match_descriptors(gpu_ctx.handle, q_ptr, nq, t_ptr, nt, dim, 0.0, idx.data_ptr(), dist.data_ptr()))


def test_refusals_launch_nothing(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    buf_q, buf_t = torch.ones(8 * 24 + 4, device="cuda"), torch.ones(8 * 24 + 4, device="cuda")
    idx = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    dist = torch.full((8,), 77.0, dtype=torch.float32, device="cuda")
    assert buf_q.data_ptr() % 16 == 0 and buf_t.data_ptr() % 16 == 0
    for dim in (0, 4, 12):
        with pytest.raises(MmfError, match="multiple of 8"):
            raw_call(gpu_ctx, buf_q.data_ptr(), 8, buf_t.data_ptr(), 8, dim, idx, dist)
    for off_q, off_t in ((4, 0), (0, 4)):  # rows that are not 16-byte aligned
        with pytest.raises(MmfError, match="aligned"):
            raw_call(gpu_ctx, buf_q.data_ptr() + off_q, 8, buf_t.data_ptr() + off_t, 8, 24, idx, dist)
    torch.cuda.synchronize()
    assert (idx.cpu() == 77).all() and (dist.cpu() == 77.0).all()  # no kernel wrote a result
    raw_call(gpu_ctx, buf_q.data_ptr(), 8, buf_t.data_ptr(), 8, 24, idx, dist)  # the same call, aligned, runs
    assert idx.cpu().tolist() == [0] + [-1] * 7 and (dist.cpu() == 0).all()
