"""-m gpu: the batch a frame's redetection runs -- several query sets behind one another against several inactive models
(csrc/redetect_host.hpp: viewstore_batch_run / viewstore_batch_best, through mmf_debug_viewstore_best_match_batch) -- against
the CPU oracles per pair, bit for bit: tests/redetect_batch_cases.py has the cases and their references.  Everything the
single-pair calls leave at its first value is here at another: a set's offset V * q0 in the match results and in the
verifier's rows, blockIdx.y > 0 in the verify and pick launches, several asked models, records and inlier flags at
s * n_asked + a, the pick's carry over more than 64 views."""
import ctypes as C

import numpy as np
import pytest
import torch

import redetect_batch_cases as bc
import redetect_oracle as ro
import verify_oracle as vo

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    assert got["found"] == want["found"] and got["view"] == want["view"] and got["n_matches"] == want["n_matches"], (what, got, want)
    assert got["inliers"] == want["inliers"], (what, got, want)
    assert np.array_equal(got["inlier"], want["inlier"] if want["found"] else np.zeros(0, bool)), what
    assert np.array_equal(got["transformation"].view(np.uint32), np.asarray(want["transformation"], np.float32).view(np.uint32)), what
    assert np.float32(got["error"]).view(np.uint32) == np.float32(want["error"]).view(np.uint32), what


@pytest.fixture(scope="module")
def verifiers(gpu_ctx):
    from multimotionfusion_amd.ransac import RansacBatch
    made = {mp: RansacBatch(gpu_ctx, *ro.RANSAC_CONFIG, max_points=mp) for mp in (40, 64)}
    yield made
    for b in made.values():
        b.close()


def make_store(gpu_ctx, verifier, models=None, forget=bc.FORGOTTEN):
    from multimotionfusion_amd.redetection import ViewStore
    vs = ViewStore(gpu_ctx)
    if verifier is not None:
        vs.setVerifier(verifier)
    models = bc.store_models() if models is None else models
    for mid in (bc.STORE_ORDER if models is bc.store_models() else models):
        assert vs.store(mid, models[mid]) is True
    if forget is not None:
        vs.forget(forget)
    return vs


def check_batch(orc, vs, rule, asked, max_points, sets=None, what=""):
    """one batch of all sets (or the sets with the given indices) against the oracle of its rule, pair by pair"""
    which = list(range(len(bc.SIZES))) if sets is None else sets
    got, host = vs.bestMatchBatch([bc.batch_sets()[s] for s in which], asked, rule)
    assert vs.lastLaunches() == 3 * len(which) + (2 if rule == 1 else 0), (what, vs.lastLaunches())
    assert host == (sum(bc.SIZES[s] > max_points for s in which) if rule == 1 else 0), (what, host)
    assert len(got) == len(which) and all(len(row) == len(asked) for row in got)
    for k, s in enumerate(which):
        for a, mid in enumerate(asked):
            assert got[k][a]["model_id"] == mid, (what, s, a, got[k][a]["model_id"])
            same(got[k][a], bc.reference(orc, rule, s, mid), (what, rule, s, mid))
    return got


@pytest.mark.parametrize("max_points", [40, 64])
def test_the_device_rule_equals_the_per_view_oracle_pair_by_pair(gpu_ctx, orc, verifiers, max_points):
    """rule 1: six sets (q0 = 0, 3, 8, 39, 72, 112) x six asked models in two verification launches.  With 40 points the set
    of 41 rows goes to the host core (counted) and the other five are verified on the device in the same batch."""
    bc.check_batch_conditions(orc)
    vs = make_store(gpu_ctx, verifiers[max_points])
    got = check_batch(orc, vs, 1, bc.ASKED, max_points, what="asked")
    found = sum(r["found"] for row in got for r in row)
    assert found >= 4 and len(bc.SIZES) * len(bc.ASKED) - found >= 4
    assert got[5][bc.ASKED.index(1)]["found"] and got[4][bc.ASKED.index(2)]["found"]
    # a pair's record does not depend on where its model stands among the asked ones, or on who else is asked
    check_batch(orc, vs, 1, bc.ASKED_OTHER_ORDER, max_points, what="other order")
    check_batch(orc, vs, 1, (1,), max_points, what="model 1 alone")
    # the device's own single-pair call agrees (a cross-check, not the reference)
    for s in (2, 4):
        qd, qc = bc.batch_sets()[s]
        for a, mid in enumerate(bc.ASKED):
            same(vs.bestMatchDevice(mid, dev(qd), dev(qc)), got[s][a], ("single pair", s, mid))
    vs.close()


def test_the_host_rule_equals_the_one_engine_oracle_pair_by_pair(gpu_ctx, orc):
    """rule 0: the host reads set s at V * q0 of the match results, one engine per (set, model); 3 launches per set"""
    vs = make_store(gpu_ctx, None)
    got = check_batch(orc, vs, 0, bc.ASKED, 0, what="asked")
    assert sum(r["found"] for row in got for r in row) >= 4
    check_batch(orc, vs, 0, bc.ASKED_OTHER_ORDER, 0, what="other order")
    for s in (1, 5):
        qd, qc = bc.batch_sets()[s]
        for a, mid in enumerate(bc.ASKED):
            same(vs.bestMatch(mid, dev(qd), qc), got[s][a], ("single pair", s, mid))
    vs.close()


def test_both_rules_on_one_store(gpu_ctx, orc, verifiers):
    """a store with a verifier attached answers rule 0 as one without, and rule 1 after it as before it"""
    vs = make_store(gpu_ctx, verifiers[40])
    check_batch(orc, vs, 1, bc.ASKED, 40, what="rule 1")
    check_batch(orc, vs, 0, bc.ASKED, 40, what="rule 0")
    check_batch(orc, vs, 1, bc.ASKED, 40, what="rule 1 again")
    vs.close()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_pick_carries_its_best_across_the_chunks_of_64_views(gpu_ctx, orc, verifiers, name):
    """model 1 with 70 views (redetect_batch_cases.chunk_layouts), asked for as the second set and the third model of a batch:
    a) the best view stored at 3 and at 67 -- view 3; b) nothing usable among the first 64, the best at 69; c) usable views
    in both chunks, the unique best at 64"""
    views, winner = bc.chunk_layouts(orc)[name]
    qd, qc = bc.chunk_query()
    models = {4: bc.store_models()[4], 1: views, 2: bc.store_models()[2]}
    vs = make_store(gpu_ctx, verifiers[64], models, forget=None)
    asked = (2, 4, 1)
    sets = [bc.batch_sets()[1], (qd, qc), bc.batch_sets()[2]]
    got, host = vs.bestMatchBatch(sets, asked, 1)
    assert host == 0 and vs.lastLaunches() == 3 * 3 + 2
    for s, (d, c) in enumerate(sets):
        for a, mid in enumerate(asked):
            assert got[s][a]["model_id"] == mid
            same(got[s][a], vo.get_best_match(orc, d, c, models[mid]), (name, s, mid))
    assert got[1][2]["found"] and got[1][2]["view"] == winner, (name, got[1][2]["view"])
    vs.close()


def test_state_between_calls(gpu_ctx, orc, verifiers):
    """the full batch, a batch of one set of 3 rows, the full batch again in ONE store: the stride of the flags and every
    scratch size change between the calls; each answer equals that of a fresh store asked only that, the third the first"""
    def records(rule, which, store=None):
        vs = store or make_store(gpu_ctx, verifiers[40])
        got, host = vs.bestMatchBatch([bc.batch_sets()[s] for s in which], bc.ASKED, rule)
        if store is None:
            vs.close()
        return got, host

    def equal(x, y, what):
        assert x[1] == y[1], what
        for rx, ry in zip(x[0], y[0]):
            for gx, gy in zip(rx, ry):
                assert gx["model_id"] == gy["model_id"]
                same(gx, gy, what)
                assert np.array_equal(gx["inlier"], gy["inlier"]), what

    everything, small = list(range(len(bc.SIZES))), [0]
    for rule in (1, 0):
        vs = make_store(gpu_ctx, verifiers[40])
        first = records(rule, everything, vs)
        second = records(rule, small, vs)
        third = records(rule, everything, vs)
        equal(first, records(rule, everything), ("first", rule))
        equal(second, records(rule, small), ("second", rule))
        equal(third, first, ("third", rule))
        for a, mid in enumerate(bc.ASKED):  # (and the oracle's, so that "equal" is not "equally wrong")
            same(third[0][5][a], bc.reference(orc, rule, 5, mid), ("third", rule, mid))
            same(second[0][0][a], bc.reference(orc, rule, 0, mid), ("second", rule, mid))
        vs.close()


def test_a_small_batch_first_then_a_wide_one(gpu_ctx, orc, verifiers):
    """sets in another order and number than the cases' own: 41 rows first (q0 of the next = 41), an empty batch, no model"""
    vs = make_store(gpu_ctx, verifiers[64])
    check_batch(orc, vs, 1, bc.ASKED, 64, sets=[5, 0, 4], what="5, 0, 4")
    check_batch(orc, vs, 0, bc.ASKED, 64, sets=[5, 0, 4], what="5, 0, 4 host")
    got, host = vs.bestMatchBatch([], bc.ASKED, 1)
    assert got == [] and host == 0 and vs.lastLaunches() == 0
    got, host = vs.bestMatchBatch([bc.batch_sets()[2]], [], 1)
    assert got == [[]] and host == 0 and vs.lastLaunches() == 3
    vs.close()


def test_refusals(gpu_ctx, verifiers):
    from multimotionfusion_amd._capi import MmfError, mmf_debug_redetect_record
    vs = make_store(gpu_ctx, None)
    lib = gpu_ctx.lib
    qd, qc = bc.batch_sets()[2]
    nq, asked = np.array([len(qd)], np.int32), np.array([1, 2], np.int32)
    rec = (mmf_debug_redetect_record * 2)()
    host = C.c_int()

    def call(n_sets, nq_p, n_asked, asked_p, rule):
        return lib.mmf_debug_viewstore_best_match_batch(vs.handle, n_sets, nq_p, qd.ctypes.data, qc.ctypes.data, n_asked, asked_p, rule,
                                                        C.addressof(rec), None, 0, C.byref(host))

    assert call(1, nq.ctypes.data, 2, asked.ctypes.data, 0) == 0
    assert [r.model_id for r in rec] == [1, 2] and rec[0].found == 1
    assert call(-1, nq.ctypes.data, 2, asked.ctypes.data, 0) == -1
    assert call(1, nq.ctypes.data, -1, asked.ctypes.data, 0) == -1
    assert call(1, None, 2, asked.ctypes.data, 0) == -1
    assert call(1, nq.ctypes.data, 2, None, 0) == -1
    assert call(1, nq.ctypes.data, 2, asked.ctypes.data, 2) == -1
    assert call(1, nq.ctypes.data, 2, asked.ctypes.data, 1) == -4  # MMF_ERR_STATE: no verifier attached
    assert b"no verifier attached" in lib.mmf_last_error()
    with pytest.raises(MmfError) as e:
        vs.bestMatchBatch([(qd, qc)], [1], 1)
    assert e.value.status == -4
    vs.setVerifier(verifiers[40])
    assert call(1, nq.ctypes.data, 2, asked.ctypes.data, 1) == 0 and rec[0].found == 1 and rec[1].model_id == 2
    vs.close()
