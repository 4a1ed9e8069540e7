"""Test helper: the seeded cases of tests/test_gpu_redetect_batch.py -- a frame's redetection batch (several query sets against
several inactive models, mmf_debug_viewstore_best_match_batch) -- and their references from the CPU oracles alone
(redetect_oracle.get_best_match: one engine per pair; verify_oracle.get_best_match: a fresh engine per view).  No device
here: tests/test_redetect_oracle.py checks on the CPU that the committed seeds give the cases their GPU tests need.

The store, in this order (store order, id order and asked order all differ):
  model 4  an unrelated object, 3 views          model 7  two empty views
  model 1  70 views of object A                  model 9  views of object A again, stored and then forgotten
  model 2  5 views of object B
One batch holds the sets SIZES = 3, 5, 31, 33, 40, 41 rows, i.e. q0 = 0, 3, 8, 39, 72, 112: no set after the first starts
on a multiple of 32, and with a verifier of 40 points the last one is too large for it."""
import functools

import numpy as np

import redetect_oracle as ro
import verify_oracle as vo

K = 45  # keypoints per object: views of a few dozen rows, queries of up to 41
STORE_ORDER = (4, 1, 2, 7, 9)
FORGOTTEN = 9
ASKED = (2, 9, 1, 4, 7, 99)  # 99 is not in the store: an inactive model without stored views
ASKED_OTHER_ORDER = (99, 7, 4, 1, 9, 2)
SIZES = (3, 5, 31, 33, 40, 41)
Q0 = (0, 3, 8, 39, 72, 112)
SEED_A, SEED_B, SEED_X = 61, 62, 63
EMPTY = (np.zeros((0, ro.DIM), np.float32), np.zeros((0, 3), np.float32))


def _views(obj, n_views, seed):
    tracks, poses = ro.make_tracks(obj, n_views, seed)
    return ro.views_of(ro.project_first_frame(tracks, poses))


def _object_rows(obj, seed, n):
    """n rows of a query of `obj` (the object seen again, moved), its own keypoints first in the query's order"""
    qd, qc, _, is_obj = ro.make_query(obj, seed, subset=0.9)
    order = np.concatenate([np.flatnonzero(is_obj), np.flatnonzero(~is_obj)])[:n]
    assert len(order) == n
    order.sort()
    return qd[order], qc[order]


@functools.lru_cache(maxsize=None)
def store_models():
    """{model id: views} as handed to ViewStore.store, STORE_ORDER; model 9 is forgotten afterwards"""
    a, b, x = ro.make_object(SEED_A, k=K), ro.make_object(SEED_B, k=K), ro.make_object(SEED_X, k=K)
    return {4: _views(x, 3, SEED_X + 100), 1: _views(a, 70, SEED_A + 100), 2: _views(b, 5, SEED_B + 100), 7: [EMPTY, EMPTY],
            9: _views(a, 4, SEED_A + 300)}


def views_asked(model):
    """what Model::getBestMatch of an asked model sees: nothing for the forgotten model and for one never stored"""
    return [] if model == FORGOTTEN or model not in store_models() else store_models()[model]


@functools.lru_cache(maxsize=None)
def batch_sets():
    """[(descriptor [n,256], coordinate [n,3])] of SIZES rows: 3 rows that give fewer than 3 matches with any view (two
    descriptors, one of them twice: equal rows share their nearest view row, which takes one of them back) | 5 of B | 31 of
    A | 33 unrelated unit rows | 40 of B | 41 of A"""
    a, b = ro.make_object(SEED_A, k=K), ro.make_object(SEED_B, k=K)
    rng = np.random.default_rng(64)
    two_d, two_c = _object_rows(a, SEED_A + 210, 2)
    sets = [(two_d[[0, 0, 1]], (two_c[[0, 0, 1]] + rng.normal(size=(3, 3)).astype(np.float32) * np.float32(1e-3))),
            _object_rows(b, SEED_B + 201, 5),
            _object_rows(a, SEED_A + 201, 31),
            (ro.unit_rows(rng, 33), (rng.uniform(-1, 1, size=(33, 3)) + np.array([0.0, 0.0, 2.0])).astype(np.float32)),
            _object_rows(b, SEED_B + 200, 40),
            _object_rows(a, SEED_A + 202, 41)]
    assert tuple(len(d) for d, _ in sets) == SIZES
    assert tuple(int(q) for q in np.concatenate([[0], np.cumsum(SIZES)[:-1]])) == Q0 and all(q % 32 for q in Q0[1:])
    return [(np.ascontiguousarray(d, np.float32), np.ascontiguousarray(c, np.float32)) for d, c in sets]


_REFERENCES = {}


def reference(orc, rule, s, model):
    """the oracle's answer for (set s of batch_sets, model): rule 0 = one engine per pair, 1 = a fresh engine per view (the
    device verifier's rule, and the host core's for a set too large for it).  Computed once."""
    key = (rule, s, model)
    if key not in _REFERENCES:
        qd, qc = batch_sets()[s]
        best = (vo if rule == 1 else ro).get_best_match(orc, qd, qc, views_asked(model))
        _REFERENCES[key] = best
    return _REFERENCES[key]


def check_batch_conditions(orc):
    """what the GPU tests need of the committed seeds, from the oracle alone"""
    for rule in (0, 1):
        found = {(s, m): reference(orc, rule, s, m)["found"] for s in range(len(SIZES)) for m in ASKED}
        assert sum(found.values()) >= 4 and sum(not f for f in found.values()) >= 4, found
        assert any(found[(s, 1)] for s in range(len(SIZES))) and any(found[(s, 2)] for s in range(len(SIZES))), found
        assert not any(found[(3, m)] for m in ASKED), "the unrelated set finds nothing"
        assert not any(found[(0, m)] for m in ASKED), "fewer than 3 matches against every view"
        assert not any(found[(s, m)] for s in range(len(SIZES)) for m in (9, 7, 99)), found
        best = reference(orc, rule, 5, 1)  # the set of 41 rows: found, and well enough to re-activate the model
        assert best["found"] and best["error"] < 0.01 and best["inliers"] > 5, best
        best = reference(orc, rule, 4, 2)
        assert best["found"] and best["error"] < 0.01 and best["inliers"] > 5, best
    for views in store_models().values():
        assert max(int((idx >= 0).sum()) for idx, _ in ro.match_views(orc, batch_sets()[0][0], views)) < 3


# ---- rd_pick_kernel's carry across its chunks of 64 views: three layouts of a model's 70 views --------------------------------
@functools.lru_cache(maxsize=None)
def chunk_query():
    return _object_rows(ro.make_object(SEED_A, k=K), SEED_A + 203, 40)


_LAYOUTS = {}


def chunk_layouts(orc):
    """{name: (views [70], the index that wins)}.  Eight distinct views of object A are ranked by the error each gives alone
    under the per-view rule; `best` is the smallest, `others` all give an estimate with a larger error.
      a  best at 3 and at 67: equal errors on both sides of the chunk boundary, the first wins
      b  0..63 unusable (empty / two rows / unrelated descriptors, in turn), others at 64..68, best at 69: nothing usable in
         the first chunk
      c  others everywhere, the best at 64 only: usable views in both chunks, the winner first in the second"""
    if _LAYOUTS:
        return _LAYOUTS
    qd, qc = chunk_query()
    base = store_models()[1][:8]
    solo = [vo.get_best_match(orc, qd, qc, [v]) for v in base]
    assert all(s["found"] for s in solo), [s["found"] for s in solo]
    errors = [np.float32(s["error"]) for s in solo]
    order = np.argsort(errors, kind="stable")
    assert errors[order[0]] < errors[order[1]], "a unique best"
    best, others = base[int(order[0])], [base[int(k)] for k in order[1:]]
    rng = np.random.default_rng(65)
    a = [others[k % 7] for k in range(70)]
    a[3] = a[67] = best
    unusable = []
    for k in range(64):
        kind = k % 3
        if kind == 0:
            unusable.append(EMPTY)
        elif kind == 1:
            unusable.append((others[k % 7][0][:2], others[k % 7][1][:2]))
        else:
            unusable.append((ro.unit_rows(rng, 33), rng.normal(size=(33, 3)).astype(np.float32)))
    for v in unusable:
        assert not vo.get_best_match(orc, qd, qc, [v])["found"]
    b = unusable + others[:5] + [best]
    c = [others[k % 7] for k in range(70)]
    c[64] = best
    layouts = dict(a=(a, 3), b=(b, 69), c=(c, 64))
    for name, (views, winner) in layouts.items():
        assert len(views) == 70
        assert vo.get_best_match(orc, qd, qc, views)["view"] == winner, name
    _LAYOUTS.update(layouts)
    return _LAYOUTS
