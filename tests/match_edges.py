"""Seeded edge cases of the descriptor matcher (csrc/match_kernels.hpp, the view store's rd_tile_kernel), shared by
tests/test_match_edges_oracle.py (CPU) and tests/test_gpu_match_edges.py.  numpy and the oracle only: a builder that needs a
sign pattern or a tie finds it by a seeded search with `orc.match_d2` and asserts it, so a case never claims a property its
inputs do not have.

A case is a `Case(name, q, t, gate, claim)`.  `claim` is a dict of what the case promises beyond "the device equals the
oracle":
  expect    {query row: train row or -1}, each at distance 0
  neg       [(i, j)]: d2[i, j] < 0;   zero [(i, j)]: d2[i, j] == 0 exactly
  pos_row / pos_col   a row / column whose every other entry is > 0
  bad_q / bad_t       the non-finite rows; `kinds` = which of "inf", "nan" their d2 entries take
  base, scale         the name of the case this one is an exact power-of-4 multiple of

The one-wave kernel (dim % 32 != 0) and the 64 x 64 kernel (dim % 32 == 0) each see every shape of SHAPES.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name q t gate claim")

EPS = np.float32(1.1920929e-7)  # the gate is off below this (PointTracker.cpp:108); == 2^-23
FILLER = np.float32(1e30)       # a padding row of the tracker's search: this in every component
ONE_WAVE_DIMS = (8, 16, 24, 40, 72, 136)
TILE64_DIMS = (32, 64, 96, 256)
SHAPES = ((1, 1), (1, 33), (33, 1), (31, 32), (32, 33), (63, 64), (64, 65), (65, 129), (129, 65))
DIMS_SHAPES = {8: (0, 4, 7), 16: (1, 5, 8), 24: (2, 3, 6), 40: (1, 4, 8), 72: (2, 5, 7), 136: (0, 3, 6),
               32: (0, 3, 7), 64: (1, 5, 8), 96: (2, 4, 6), 256: (1, 6, 7, 8)}
NOISE = 0.02  # sigma of a tracked keypoint's descriptor noise: d2 ~ NOISE^2 dim, far above the rounding bound of any dim
WORKSPACE_SEQUENCE = ((100, 100), (10, 150), (150, 0), (0, 50), (150, 10), (1, 1), (129, 65))
EDGE_DIMS = (24, 256)  # one dim per kernel for the sign, tie and non-finite cases


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)


def tracked(seed, nq, nt, dim):
    """noisy copies of distinct train rows first, fresh rows after them (the inputs of tests/test_gpu_matcher.py)"""
    rng = np.random.default_rng(seed)
    t = unit_rows(rng, nt, dim)
    ncopy = (min(nq, nt) * 3 + 3) // 4
    perm = rng.permutation(nt)[:ncopy]
    q = np.concatenate([t[perm] + np.float32(NOISE) * rng.standard_normal((ncopy, dim)).astype(np.float32),
                        unit_rows(rng, nq - ncopy, dim)]).astype(np.float32)
    return q, t, perm


def dims_cases():
    out = []
    for dim in ONE_WAVE_DIMS + TILE64_DIMS:
        for s in DIMS_SHAPES[dim]:
            nq, nt = SHAPES[s]
            q, t, perm = tracked(dim * 1000 + s, nq, nt, dim)
            out.append(Case(f"dims_d{dim}_{nq}x{nt}", q, t, 0.7 if s % 2 else 0.0, {"perm": perm}))
    return out


# ---- sign: a negative d2 beside an exact duplicate's 0 --------------------------------------------------------------
def perturbations(rng, row, n, max_elems, max_ulps):
    """n copies of `row` with up to max_elems components moved by up to max_ulps ulps (a step on the bit pattern)"""
    steps = rng.integers(-max_ulps, max_ulps + 1, (n, len(row))).astype(np.int32)
    rank = rng.random((n, len(row))).argsort(1)
    steps[rank >= rng.integers(1, max_elems + 1, (n, 1))] = 0
    return (row.view(np.int32)[None] + steps).view(np.float32)


def negative_neighbours(orc, rng, row, distinct):
    """rows a few ulps from `row` whose d2 to it is negative (their true squared distance is below 1e-11 |row|^2):
    one of them, or for distinct = 2 two with different d2, the more negative one last"""
    found = {}
    for max_elems, max_ulps in ((1, 1), (4, 2), (len(row), 2), (len(row), 4), (len(row), 8), (len(row), 16)):
        cand = perturbations(rng, row, 4096, max_elems, max_ulps)
        d2 = orc.match_d2(row[None], cand)[0]
        for r in np.nonzero(d2 < 0)[0]:
            found.setdefault(float(d2[r]), cand[r])
        if len(found) >= distinct:
            break
    assert len(found) >= distinct, (len(found), distinct)
    vals = sorted(found)  # the most negative value first
    return [found[vals[-1]], found[vals[0]]] if distinct == 2 else [found[vals[0]]]


def sign_cases(orc):
    out = []
    for dim in EDGE_DIMS:
        for two in (False, True):
            rng = np.random.default_rng(500 + dim + two)
            scale = np.float32(4.0 if two else 1.0)  # (an exact scaling: the same pattern in another binade)
            t = unit_rows(rng, 130, dim) * scale
            q = unit_rows(rng, 5, dim) * scale
            i, ja, jb, jc = 2, 3, 3 + 64, 100
            q[i] = t[ja]
            near = negative_neighbours(orc, rng, t[ja], 2 if two else 1)
            t[jb] = near[0]
            claim = {"zero": [(i, ja)], "neg": [(i, jb)], "pos_row": i, "pos_col": jb, "expect": {i: jb}}
            if two:  # the more negative one at the larger index, in another tile: the value decides, not the index
                t[jc] = near[1]
                claim.update(neg=[(i, jb), (i, jc)], pos_col=jc, expect={i: jc}, more_negative=((i, jc), (i, jb)))
            name = f"sign_d{dim}_{'two' if two else 'one'}"
            out.append(Case(name + "_train", q, t, 0.0, claim))
            # the mirror image: d2 is symmetric bit for bit (a + b and fmaf(a, b, s) commute), so this is the transpose
            win = jc if two else jb
            mirror = {"zero": [(b, a) for a, b in claim["zero"]], "neg": [(b, a) for a, b in claim["neg"]],
                      "pos_col": i, "pos_row": win, "expect": {win: i, ja: -1}}
            if two:
                mirror.update(more_negative=((jc, i), (jb, i)))
                mirror["expect"][jb] = -1
            out.append(Case(name + "_query", t.copy(), q.copy(), 0.0, mirror))
    return out


# ---- ties across tiles and workgroups -------------------------------------------------------------------------------
TIE_ALL = (0, 31, 32, 63, 64, 127, 128)
TIE_LATE = (63, 64, 128)


def tie_cases():
    out = []
    for dim in EDGE_DIMS:
        for tag, at in (("all", TIE_ALL), ("late", TIE_LATE)):
            rng = np.random.default_rng(700 + dim + len(at))
            many, few = unit_rows(rng, 129, dim), unit_rows(rng, 3, dim)
            many[list(at)] = few[1]
            out.append(Case(f"tie_d{dim}_{tag}_train", few, many, 0.0, {"expect": {1: at[0]}, "copies": ("t", at, 1)}))
            exp = {i: -1 for i in at[1:]}
            exp[at[0]] = 1
            out.append(Case(f"tie_d{dim}_{tag}_query", many.copy(), few.copy(), 0.0, {"expect": exp, "copies": ("q", at, 1)}))
        same = np.repeat(unit_rows(np.random.default_rng(800 + dim), 1, dim), 130, 0)
        first = {i: (0 if i == 0 else -1) for i in range(130)}
        out.append(Case(f"tie_d{dim}_identical", same, same.copy(), 0.0, {"expect": first, "all_zero_d2": True}))
        zero = np.zeros((130, dim), np.float32)
        out.append(Case(f"tie_d{dim}_zero", zero, zero.copy(), 0.0, {"expect": first, "all_zero_d2": True}))
    return out


# ---- the gate -------------------------------------------------------------------------------------------------------
def gate_base(dim=24):
    q, t, perm = tracked(900 + dim, 64, 65, dim)
    q[5] = t[perm[5]]  # an exact duplicate: distance 0 passes a gate that is on at its smallest value
    return q, t


def gate_cases(orc):
    q, t = gate_base()
    idx, dist = orc.match_descriptors(q, t, 0.0)
    matched = np.nonzero((idx >= 0) & (dist > EPS))[0]
    m = int(matched[np.argsort(dist[matched])[len(matched) // 2]])  # the match at the median distance
    at, below = dist[m], np.nextafter(dist[m], np.float32(0))
    c = lambda name, gate, claim: Case("gate_" + name, q, t, float(gate), claim)
    return [c("at_match", at, {"kept": m, "gate_on": True}), c("below_match", below, {"dropped": m, "gate_on": True}),
            c("eps", EPS, {"gate_on": True, "expect": {5: int(idx[5])}}),
            c("below_eps", np.nextafter(EPS, np.float32(0)), {"gate_off": True}),
            c("zero", 0.0, {"gate_off": True}), c("minus_one", -1.0, {"gate_off": True}),
            c("inf", np.inf, {"gate_off": True}), c("nan", np.nan, {"none": True})]


# ---- non-finite rows ------------------------------------------------------------------------------------------------
def insert_rows(x, at, rows):
    """x with `rows` inserted so that they end up at the indices `at` (ascending)"""
    out = list(x)
    for k, r in zip(at, rows):
        out.insert(k, r)
    return np.stack(out).astype(np.float32)


def nonfinite_cases():
    out = []
    for dim in EDGE_DIMS:
        q0, t0, _ = tracked(1100 + dim, 40, 70, dim)
        fill = lambda n: np.full((n, dim), FILLER, np.float32)
        variants = []
        variants.append(("fillers", q0, insert_rows(t0, (0, 31, 32, 64), fill(4)), (), (0, 31, 32, 64), ("inf",)))
        variants.append(("filler_tile", q0, insert_rows(t0, range(32, 64), fill(32)), (), tuple(range(32, 64)), ("inf",)))
        variants.append(("all_fillers", q0, fill(33), (), tuple(range(33)), ("inf",)))
        qn = q0.copy()
        qn[0, dim // 2] = np.nan  # row 0: a scan that takes its first pair unconditionally never leaves a NaN
        variants.append(("nan_query", qn, t0, (0,), (), ("nan",)))
        tn = t0.copy()
        tn[0, 1] = np.nan
        variants.append(("nan_train", q0, tn, (), (0,), ("nan",)))
        ti = t0.copy()
        ti[33, dim - 1] = np.inf  # <q, t> = +-inf by the sign of q's last component: d2 = inf - inf = NaN, or +inf
        variants.append(("inf_train", q0, ti, (), (33,), ("inf", "nan")))
        for tag, q, t, bad_q, bad_t, kinds in variants:
            for gate in (0.0, 0.7):
                out.append(Case(f"nonfinite_d{dim}_{tag}_g{gate}", q, t, gate, {"bad_q": bad_q, "bad_t": bad_t, "kinds": kinds}))
    return out


def without_bad_rows(case):
    """(q', t', kept query rows, kept train rows): the case with its non-finite rows deleted"""
    kq = np.array([i for i in range(len(case.q)) if i not in case.claim["bad_q"]], np.int64)
    kt = np.array([j for j in range(len(case.t)) if j not in case.claim["bad_t"]], np.int64)
    return case.q[kq], case.t[kt], kq, kt


def map_back(case, idx, dist, kq, kt):
    """the result on the reduced sets in the indices of the full ones; a deleted query row is -1 at distance 0"""
    full_i, full_d = np.full(len(case.q), -1, np.int32), np.zeros(len(case.q), np.float32)
    m = idx >= 0
    full_i[kq[m]] = kt[idx[m]]
    full_d[kq] = dist
    return full_i, full_d


# ---- scale ----------------------------------------------------------------------------------------------------------
def scale_cases():
    """a power of 4 scales every product and every partial sum exactly: the same indices, distances exactly `s` times"""
    out = []
    for dim in EDGE_DIMS:
        q, t, _ = tracked(1300 + dim, 64, 65, dim)
        out.append(Case(f"scale_d{dim}_x1", q, t, 0.7, {}))
        for tag, s in (("x4", 4.0), ("x0.25", 0.25)):
            out.append(Case(f"scale_d{dim}_{tag}", q * np.float32(s), t * np.float32(s), float(np.float32(0.7) * np.float32(s)),
                            {"base": f"scale_d{dim}_x1", "scale": s}))
    return out


# ---- the workspace of one context, reused by calls that shrink and grow ---------------------------------------------
def workspace_calls(dim):
    """[(q, t, gate)] in the order of WORKSPACE_SEQUENCE: col_best = keys + nq of one call lies on the row keys of the last"""
    out = []
    for k, (nq, nt) in enumerate(WORKSPACE_SEQUENCE):
        if nq and nt:
            q, t, _ = tracked(1500 + dim + k, nq, nt, dim)
        else:
            rng = np.random.default_rng(1500 + dim + k)
            q, t = unit_rows(rng, nq, dim), unit_rows(rng, nt, dim)
        out.append((q, t, 0.7 if k % 2 else 0.0))
    return out


def finite(case):
    """every d2 of the case is a finite number (the gate may be anything)"""
    return "bad_q" not in case.claim


_cache = {}


def all_cases(orc):
    """every case, built once per session (the searches take a moment) and never modified"""
    if "cases" not in _cache:
        cases = dims_cases() + sign_cases(orc) + tie_cases() + gate_cases(orc) + nonfinite_cases() + scale_cases()
        for c in cases:
            c.q.setflags(write=False), c.t.setflags(write=False)
        assert len({c.name for c in cases}) == len(cases)
        _cache["cases"] = cases
    return _cache["cases"]


def by_prefix(orc, *prefixes):
    return [c for c in all_cases(orc) if c.name.startswith(prefixes)]
