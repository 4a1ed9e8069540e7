"""The edge cases of the keypoint selection behind the SuperPoint network (csrc/superpoint_kernels.hpp from sp_heatmap_kernel
on: the heat map, the fixed-point suppression in its host-looped and its device-finished form, the two ordered compactions,
sp_rank_select_kernel, the bilinear sampling, sp_l2_normalize_kernel), their expected results from the C oracle, and the
device-against-oracle check of test_gpu_keypoint_edges.py.  test_keypoint_edges_oracle.py pins the oracle and asserts every
claim without a device.

A case is Case(name, heat, semi, desc, normalize, H, W, conf_thresh, nms_dist, border, max_keypoints, claim): exactly one of
heat [H][W] and semi [H/8][W/8][65] is given; desc is the coarse descriptor map [H/8][W/8][256] (normalised on the way in when
`normalize`).  claim is a dict; what it says about the inputs is asserted when the case is built (assert_inputs), what it says
about results is asserted on the oracle's (verify) -- a case never claims a property it lacks.  Every case claims its number
of sampled rows that hold a NaN ("nan_rows", 0 where absent), so the NaN-equals-NaN rule of the comparison cannot hide a row.

Heat maps keep to the contract of include/mmf_hip.h: values in [0, 1], +inf or NaN.

numpy only at import; the oracle is an argument; torch and the device bindings are imported where a device is used."""
import collections

import numpy as np

from helpers import bits

F32 = np.float32
Case = collections.namedtuple("Case", "name heat semi desc normalize H W conf_thresh nms_dist border max_keypoints claim")
H0, W0 = 40, 56  # 2240 pixels: more than the finisher's 1024 lanes, more than one 256-key tile, 35 rank blocks
THRESH = F32(0.015)
BELOW = np.nextafter(THRESH, F32(0))
FLT_MIN = np.finfo(F32).tiny


# ---- expected results -------------------------------------------------------------------------------------------------------
def heat_of(c, orc):
    return c.heat if c.heat is not None else orc.sp_heatmap(c.semi)


def reference(c, orc):
    """the oracle's results for case c: heat, cdesc (the coarse map as sampled), full_xy / full_conf (before the max_keypoints
    cut), xy, conf, desc, nan_rows, inf_rows"""
    heat = heat_of(c, orc)
    with np.errstate(all="ignore"):
        cdesc = orc.sp_l2_normalize(c.desc) if c.normalize else c.desc
    full_xy, full_conf = orc.sp_keypoints(heat, c.conf_thresh, c.nms_dist, c.border)
    xy, conf = full_xy[:c.max_keypoints], full_conf[:c.max_keypoints]
    desc = orc.sp_sample_descriptors(cdesc, xy, c.H, c.W) if len(xy) else np.zeros((0, 256), F32)
    nan = np.isnan(desc).any(1)
    return dict(heat=heat, cdesc=cdesc, full_xy=full_xy, full_conf=full_conf, xy=xy, conf=conf, desc=desc,
                nan_rows=int(nan.sum()), inf_rows=int((np.isinf(desc).any(1) & ~nan).sum()))


_REF = {}


def ref_of(name, orc):
    if name not in _REF:
        _REF[name] = reference(CASES[name], orc)
    return _REF[name]


def greedy(heat, thresh, dist, border):
    """nms_fast in plain Python: sort by (-conf, index), visit, suppress the window -> (xy, conf), strongest first"""
    H, W = heat.shape
    flat = heat.ravel()
    cand = [i for i in range(H * W) if flat[i] >= thresh]
    cand.sort(key=lambda i: (-float(flat[i]), i))
    alive = np.zeros((H, W), bool)
    alive.ravel()[cand] = True
    xy, conf = [], []
    for i in cand:
        y, x = divmod(i, W)
        if not alive[y, x]:
            continue
        alive[max(y - dist, 0):y + dist + 1, max(x - dist, 0):x + dist + 1] = False
        if border <= x < W - border and border <= y < H - border:
            xy.append((x, y))
            conf.append(flat[i])
    return np.array(xy, np.int32).reshape(-1, 2), np.array(conf, F32)


def _window_min(a, dist, big):
    H, W = a.shape
    p = np.full((H, W + 2 * dist), big, a.dtype)
    p[:, dist:dist + W] = a
    m = p[:, 0:W].copy()
    for s in range(1, 2 * dist + 1):
        np.minimum(m, p[:, s:s + W], out=m)
    p = np.full((H + 2 * dist, W), big, a.dtype)
    p[dist:dist + H] = m
    m = p[0:H].copy()
    for s in range(1, 2 * dist + 1):
        np.minimum(m, p[s:s + H], out=m)
    return m


def sync_fixed_point(heat, thresh, dist):
    """the suppression's fixed point with SYNCHRONOUS passes (every candidate decides on the previous pass's states): the
    number of passes until nothing is undecided, and the kept mask.  A third statement of the same outcome, and the measure
    of a dependency chain: the device's in-place passes need no more than this."""
    H, W = heat.shape
    flat = heat.ravel()
    cand = np.flatnonzero(flat >= thresh)
    order = cand[np.lexsort((cand, -flat[cand].astype(np.float64)))]
    big = H * W
    pri = np.full(H * W, big, np.int64)
    pri[order] = np.arange(len(order))
    pri = pri.reshape(H, W)
    open_ = pri < big
    kept = np.zeros((H, W), bool)
    passes = 0
    while open_.any():
        passes += 1
        stronger_kept = _window_min(np.where(kept, pri, big), dist, big) < pri
        stronger_open = _window_min(np.where(open_, pri, big), dist, big) < pri
        now_kept = open_ & ~stronger_kept & ~stronger_open
        kept |= now_kept
        open_ &= ~(stronger_kept | now_kept)
    return passes, kept


def same(a, b):
    """equal bit for bit, except that a NaN equals any NaN at the same place (the sign and payload of an invalid operation's
    NaN are no contract)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def assert_same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if same(got, ref):
        return
    if got.dtype.kind == "f":
        ne = (np.isnan(got) != np.isnan(ref)) | (~np.isnan(ref) & (bits(got) != bits(ref)))
    else:
        ne = got != ref
    at = np.argwhere(ne)[:4].tolist()
    raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {at}: got {[got[tuple(p)] for p in at]}, "
                         f"reference {[ref[tuple(p)] for p in at]}")


# ---- claims -----------------------------------------------------------------------------------------------------------------
RESULT_KEYS = {"nan_rows", "inf_rows", "count", "kept_at_threshold", "first", "absent", "present", "pairs", "winners", "band",
               "sync_passes", "edge_keypoint", "nan_as_zero", "conf_values", "cut_tie", "cells", "heat_cells", "cdesc_cells",
               "all_pixels"}
INPUT_KEYS = {"values", "strict_path", "nan_pixels", "inf_pixel", "zeros_and_denormals", "candidates", "global_max_in_band",
              "norm0_cells", "raw_rows"}


def in_band(c, x, y):
    return not (c.border <= x < c.W - c.border and c.border <= y < c.H - c.border)


def cheb(p, q):
    return max(abs(p[0] - q[0]), abs(p[1] - q[1]))


def assert_inputs(c):
    """what the claim says about the inputs alone"""
    assert (c.heat is None) != (c.semi is None) and c.H % 8 == 0 and c.W % 8 == 0
    Hc, Wc = c.H // 8, c.W // 8
    assert c.desc.shape == (Hc, Wc, 256) and c.desc.dtype == F32
    if c.heat is not None:
        h = c.heat
        assert h.shape == (c.H, c.W) and h.dtype == F32
        ok = np.isnan(h) | (h == np.inf) | ((h >= 0) & (h <= 1) & ~np.signbit(h))
        assert ok.all(), "a heat map outside the contract"
    else:
        assert c.semi.shape == (Hc, Wc, 65) and c.semi.dtype == F32
    assert not set(c.claim) - RESULT_KEYS - INPUT_KEYS, set(c.claim) - RESULT_KEYS - INPUT_KEYS
    for key, v in c.claim.items():
        if key == "values":  # {value: at least this many pixels}, nothing else
            assert set(np.unique(c.heat).tolist()) == {float(x) for x in v}
            for x, least in v.items():
                assert int((c.heat == F32(x)).sum()) >= least, x
        elif key == "strict_path":  # pixel indices: strictly increasing heat along them, consecutive ones adjacent, 0 elsewhere
            flat = c.heat.ravel()
            p = np.asarray(v)
            assert (np.diff(flat[p]) > 0).all() and flat[p[0]] >= c.conf_thresh
            ys, xs = np.divmod(p, c.W)
            assert len(p) == flat.size or (np.maximum(np.abs(np.diff(ys)), np.abs(np.diff(xs))) == 1).all()  # (a ramp covers the image)
            rest = np.ones(flat.size, bool)
            rest[p] = False
            assert (flat[rest] == 0).all()
        elif key == "nan_pixels":
            assert int(np.isnan(c.heat).sum()) == v and v > 0
        elif key == "inf_pixel":
            assert c.heat[v[1], v[0]] == np.inf and int(np.isinf(c.heat).sum()) == 1
        elif key == "zeros_and_denormals":
            assert c.conf_thresh == 0 and int((c.heat == 0).sum()) >= v[0]
            assert int(((c.heat > 0) & (c.heat < FLT_MIN)).sum()) >= v[1]
        elif key == "candidates":
            assert int((c.heat >= F32(c.conf_thresh)).sum()) == v
        elif key == "global_max_in_band":
            y, x = np.unravel_index(np.argmax(c.heat), c.heat.shape)
            assert int((c.heat == c.heat.max()).sum()) == 1 and in_band(c, x, y) == v
        elif key == "norm0_cells":  # {(hc, wc): value}: the whole cell is that value, and its float32 sum of squares is 0
            for (hc, wc), val in v.items():
                assert (c.desc[hc, wc] == F32(val)).all() and F32(val) * F32(val) == 0
        elif key == "raw_rows":  # {(hc, wc): kind}
            for (hc, wc), kind in v.items():
                row = c.desc[hc, wc]
                with np.errstate(all="ignore"):
                    sq = (row * row).astype(F32)
                if kind == "zero":
                    assert (row == 0).all()
                elif kind == "overflow":
                    assert np.isfinite(row).all() and np.isinf(sq).all()
                elif kind == "underflow":
                    assert (row != 0).all() and (sq == 0).all()
                elif kind == "nan":
                    assert int(np.isnan(row).sum()) == 1
                else:
                    assert kind == "ordinary" and np.isfinite(row).all() and 0.1 < float(np.sqrt((row.astype(np.float64) ** 2).sum())) < 100


def classify(a):
    """(NaN, +0, denormal, inf, other) counts of an array"""
    a = np.asarray(a)
    nan, zero, inf = np.isnan(a), a == 0, np.isinf(a)
    den = (np.abs(a) > 0) & (np.abs(a) < FLT_MIN)
    return int(nan.sum()), int(zero.sum()), int(den.sum()), int(inf.sum()), int(a.size - nan.sum() - zero.sum() - den.sum() - inf.sum())


def verify(c, r, orc=None):
    """what the claim says about results, asserted on r (the oracle's reference(c), or the device's results in the same
    form); orc is needed for the claims that compare with another case's results"""
    kp = {(int(x), int(y)) for x, y in r["xy"]}
    assert len(kp) == len(r["xy"])
    assert r["nan_rows"] == c.claim.get("nan_rows", 0), r["nan_rows"]
    assert r["inf_rows"] == c.claim.get("inf_rows", 0), r["inf_rows"]
    assert all(not in_band(c, x, y) for x, y in kp)
    conf = r["conf"]
    assert (conf >= F32(c.conf_thresh)).all() and (np.diff(conf) <= 0).all()
    for key, v in c.claim.items():
        if key == "count":
            assert len(r["xy"]) == v, len(r["xy"])
        elif key == "kept_at_threshold":  # pixels equal to the threshold are candidates, the value below is not
            assert (conf.min() == F32(c.conf_thresh)) == v and BELOW not in conf
            if c.nms_dist == 0:
                inner = c.heat[c.border:c.H - c.border, c.border:c.W - c.border]
                assert len(kp) == int((inner >= THRESH).sum()) and int((inner == THRESH).sum()) == int((conf == THRESH).sum()) > 0
        elif key == "first":
            assert tuple(r["xy"][0]) == v[0] and conf[0] == F32(v[1])
        elif key == "absent":
            assert not kp & set(v), kp & set(v)
        elif key == "present":
            assert set(v) <= kp, set(v) - kp
        elif key == "pairs":  # (p, q, both): equal maxima, p first in row-major order; at distance dist only p survives
            for p, q, both in v:
                assert c.heat[p[1], p[0]] == c.heat[q[1], q[0]] > 0 and p[1] * c.W + p[0] < q[1] * c.W + q[0]
                assert cheb(p, q) == c.nms_dist + (1 if both else 0)
                assert p in kp and (q in kp) == both, (p, q, both)
        elif key == "winners":  # (winner, loser): neighbours one ulp apart, the value decides
            for w, l in v:
                a, b = c.heat[w[1], w[0]], c.heat[l[1], l[0]]
                assert int(bits(a).ravel()[0]) - int(bits(b).ravel()[0]) == 1 and cheb(w, l) == 1
                assert w in kp and l not in kp
        elif key == "band":  # (strong, weak): strong lies in the band, weak inside within the radius: neither is a keypoint
            for s, w in v:
                assert in_band(c, *s) and not in_band(c, *w) and cheb(s, w) <= c.nms_dist
                assert c.heat[s[1], s[0]] > c.heat[w[1], w[0]] >= F32(c.conf_thresh)
                assert not [p for p in kp if cheb(p, s) <= c.nms_dist]
        elif key == "sync_passes":
            passes, kept = sync_fixed_point(heat_of(c, orc), F32(c.conf_thresh), c.nms_dist)
            assert passes == v and passes > 8, passes
            ys, xs = np.nonzero(kept)
            assert {(int(x), int(y)) for x, y in zip(xs, ys) if not in_band(c, x, y)} == kp
        elif key == "edge_keypoint":
            assert any(x < 4 or y < 4 or x >= c.W - 4 or y >= c.H - 4 for x, y in kp) == v
        elif key == "nan_as_zero":
            z = reference(c._replace(heat=np.where(np.isnan(c.heat), F32(0), c.heat)), orc)
            assert np.array_equal(z["xy"], r["xy"]) and np.array_equal(bits(z["conf"]), bits(conf)) and len(kp) > 20
            assert not np.isnan(conf).any()
        elif key == "conf_values":  # every one of these confidences occurs among the keypoints
            assert set(v) <= set(conf.tolist()), set(v) - set(conf.tolist())
        elif key == "cut_tie":  # ranks max_keypoints - 1 and max_keypoints tie, and the row-major earlier one is kept
            full_xy, full_conf = orc.sp_keypoints(heat_of(c, orc), c.conf_thresh, c.nms_dist, c.border)
            k = c.max_keypoints
            assert len(full_xy) > k and len(r["xy"]) == k
            idx = full_xy[:, 1] * c.W + full_xy[:, 0]
            assert (full_conf[k - 1] == full_conf[k]) == v
            if v:
                assert idx[k - 1] < idx[k]
            assert tuple(r["xy"][k - 1]) == tuple(full_xy[k - 1]) and tuple(full_xy[k]) not in kp
        elif key == "cells":
            assert (c.H // 8, c.W // 8) == v and len(kp) > 0
        elif key == "all_pixels":
            assert len(kp) == c.H * c.W == v
        elif key == "heat_cells":  # {(hc, wc): (NaN, zero, denormal) counts of the cell's 64 heat values}
            heat = r["heat"] if "heat" in r else heat_of(c, orc)
            for (hc, wc), want in v.items():
                assert classify(heat[8 * hc:8 * hc + 8, 8 * wc:8 * wc + 8])[:3] == want, ((hc, wc), classify(heat[8 * hc:8 * hc + 8, 8 * wc:8 * wc + 8]))
        elif key == "cdesc_cells":  # {(hc, wc): (NaN, zero, denormal, inf, other) counts of the normalised row}
            for (hc, wc), want in v.items():
                assert classify(r["cdesc"][hc, wc]) == want, ((hc, wc), classify(r["cdesc"][hc, wc]))
        else:
            assert key in INPUT_KEYS or key in ("nan_rows", "inf_rows"), key


# ---- builders ---------------------------------------------------------------------------------------------------------------
def unit_desc(rng, H, W):
    d = rng.standard_normal((H // 8, W // 8, 256))
    return (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(F32)


def random_heat(rng, H, W):
    """softmax-like: most pixels far below the threshold, a few hundred candidates"""
    return (rng.random((H, W)) ** 6).astype(F32)


def case(name, seed, claim, heat=None, semi=None, desc=None, normalize=False, thresh=THRESH, dist=4, border=4, max_keypoints=None):
    a = heat if heat is not None else semi
    H, W = (a.shape[0], a.shape[1]) if heat is not None else (a.shape[0] * 8, a.shape[1] * 8)
    if desc is None:
        desc = unit_desc(np.random.default_rng(1000 + seed), H, W)
    c = Case(name, None if heat is None else np.ascontiguousarray(heat, F32), None if semi is None else np.ascontiguousarray(semi, F32),
             np.ascontiguousarray(desc, F32), bool(normalize), H, W, float(F32(thresh)), dist, border,
             H * W if max_keypoints is None else max_keypoints, claim)
    assert_inputs(c)
    for a in (c.heat, c.semi, c.desc):
        if a is not None:
            a.setflags(write=False)
    return c


def _tie():
    out = []
    vals = np.array([0, BELOW, THRESH, 0.02, 0.02, 0.5], F32)
    for dist in (0, 1, 4):
        rng = np.random.default_rng(10 + dist)
        heat = vals[rng.integers(0, 6, (H0, W0))]
        out.append(case(f"tie-plateaus-r{dist}", 10 + dist, dict(values={0.0: 200, float(BELOW): 200, float(THRESH): 200, float(F32(0.02)): 400, 0.5: 200},
                                                                kept_at_threshold=dist < 4), heat=heat, dist=dist))
    heat = np.full((H0, W0), 0.02, F32)
    for y, x in ((0, 0), (0, W0 - 1), (H0 - 1, 0), (H0 - 1, W0 - 1), (H0 // 2, W0 // 2)):
        heat[y, x] = 0.5
    out.append(case("tie-flat-plus", 14, dict(values={float(F32(0.02)): H0 * W0 - 5, 0.5: 5}, first=((W0 // 2, H0 // 2), 0.5),
                                            absent=[(4, 4), (W0 - 5, 4), (4, H0 - 5), (W0 - 5, H0 - 5)],
                                            present=[(5, 5), (10, 5)]), heat=heat))
    for d in (1, 4):
        for both in (False, True):
            k = d + (1 if both else 0)
            heat = np.zeros((H0, W0), F32)
            # horizontal, vertical, diagonal (the second is below and right), anti-diagonal (the second is below and LEFT:
            # later in row-major order although its x is smaller)
            pairs = [((8, 8), (8 + k, 8), both), ((36, 6), (36, 6 + k), both), ((8, 24), (8 + k, 24 + k), both), ((44, 24), (44 - k, 24 + k), both)]
            for i, (p, q, _) in enumerate(pairs):
                heat[p[1], p[0]] = heat[q[1], q[0]] = F32(0.25 + 0.125 * i)
            out.append(case(f"tie-pair-d{d}-{'past' if both else 'at'}", 15, dict(pairs=pairs, count=8 if both else 4), heat=heat, dist=d))
    heat = np.zeros((H0, W0), F32)
    a = F32(0.3)
    b = np.nextafter(a, F32(1))
    win = []
    for i, (p, q) in enumerate([((8, 8), (9, 8)), ((20, 8), (20, 9)), ((32, 8), (33, 9)), ((45, 9), (44, 10)),   # the later one wins
                                ((9, 24), (8, 24)), ((20, 25), (20, 24)), ((33, 25), (32, 24)), ((44, 26), (45, 25))]):  # the earlier one
        heat[p[1], p[0]], heat[q[1], q[0]] = a, b
        win.append((q, p))
    out.append(case("tie-one-ulp", 16, dict(winners=win, count=8), heat=heat))
    return out


def serpentine_path(H, W):
    """pixel indices of a one-pixel-wide boustrophedon over the even rows, joined through the odd rows at alternating ends"""
    p = []
    for k, y in enumerate(range(0, H, 2)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        p += [y * W + x for x in xs]
        if y + 2 < H:
            p.append((y + 1) * W + (W - 1 if k % 2 == 0 else 0))
    return p


def _chain():
    n = H0 * W0
    up = (F32(0.02) + F32(1e-6) * np.arange(n, dtype=F32)).astype(F32).reshape(H0, W0)
    out = [case("chain-raster-up", 20, dict(strict_path=list(range(n)), sync_passes=38), heat=up),
           case("chain-raster-down", 21, dict(strict_path=list(range(n - 1, -1, -1)), sync_passes=38), heat=up.ravel()[::-1].reshape(H0, W0).copy())]
    path = serpentine_path(H0, W0)
    heat = np.zeros(n, F32)
    heat[path] = (F32(0.02) + F32(1e-5) * np.arange(len(path), dtype=F32)).astype(F32)
    for dist, passes in ((1, 1120), (4, 154)):
        out.append(case(f"chain-serpentine-r{dist}", 22, dict(strict_path=path, sync_passes=passes), heat=heat.reshape(H0, W0).copy(), dist=dist))
    return out


def _band():
    out = []
    heat = np.zeros((H0, W0), F32)
    pairs = [((2, 12), (5, 12)), ((W0 - 2, 20), (W0 - 6, 22)), ((20, 1), (22, 5)), ((36, H0 - 3), (33, H0 - 6))]  # left, right, top, bottom
    for s, w in pairs:
        heat[s[1], s[0]], heat[w[1], w[0]] = 0.5, 0.25
    heat[20, 28] = 0.125  # a control that survives
    out.append(case("band-suppressor-dropped", 30, dict(band=pairs, count=1, present=[(28, 20)]), heat=heat))
    rng = np.random.default_rng(31)
    heat = random_heat(rng, H0, W0)
    heat[1, 30] = 1.0  # a keypoint in the edge rows when there is no border
    for border, extra in ((0, dict(edge_keypoint=True, present=[(30, 1)])), (4, dict(edge_keypoint=False, absent=[(30, 1)])), (20, dict(count=0)), (100, dict(count=0))):
        out.append(case(f"band-border-{border}", 31, extra, heat=heat, border=border))
    for where, (x, y) in (("inner", (30, 17)), ("band", (54, 17))):
        h = np.minimum(heat, F32(0.9))
        h[y, x] = 1.0
        h[1, 30] = 0.9
        out.append(case(f"band-radius-64-max-{where}", 32, dict(global_max_in_band=where == "band", count=0 if where == "band" else 1), heat=h, dist=64))
    return out


def _nonfinite():
    rng = np.random.default_rng(40)
    heat = random_heat(rng, H0, W0)
    heat[rng.random((H0, W0)) < 0.05] = np.nan
    out = [case("nonfinite-nan", 40, dict(nan_pixels=int(np.isnan(heat).sum()), nan_as_zero=True), heat=heat)]
    heat = random_heat(np.random.default_rng(41), H0, W0)
    heat[17, 23] = np.inf
    out.append(case("nonfinite-inf", 41, dict(inf_pixel=(23, 17), first=((23, 17), np.inf)), heat=heat))
    rng = np.random.default_rng(42)
    heat = np.zeros((H0, W0), F32)
    pick = rng.random((H0, W0))
    den = (rng.integers(1, 1 << 23, (H0, W0)).astype(np.uint32)).view(F32)  # every bit pattern below FLT_MIN
    heat[pick < 0.3] = den[pick < 0.3]
    heat[pick < 0.05] = random_heat(rng, H0, W0)[pick < 0.05]
    heat[10:20, 10:24] = 0  # a plateau of zeros wider than the window: its row-major first pixel survives
    heat[14, 14] = F32(1e-45)
    out.append(case("nonfinite-thresh0", 42, dict(zeros_and_denormals=(1000, 300), candidates=H0 * W0, conf_values=[0.0, float(F32(1e-45))],
                                                   present=[(14, 14)]), heat=heat, thresh=0, dist=1))
    return out


COUNT_M = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2240)
CUT_M = (65, 257, 1025)


def _count():
    out = []
    strong = np.array([THRESH, 0.02, 0.25, 1.0], F32)
    weak = np.array([0, BELOW, 0.01], F32)
    for m in COUNT_M:
        rng = np.random.default_rng(50 + m)
        heat = weak[rng.integers(0, 3, H0 * W0)]
        at = rng.choice(H0 * W0, m, replace=False)
        heat[at] = strong[rng.integers(0, 4, m)]
        heat = heat.reshape(H0, W0)
        claim = dict(candidates=m, count=m)
        if m >= 63:
            claim["conf_values"] = strong.tolist()
        out.append(case(f"count-m{m}", 50, claim, heat=heat, dist=0, border=0))
        if m in CUT_M:
            for k in (1, m - 1, m, m + 1):
                claim = dict(candidates=m, count=min(k, m))
                if k < m:
                    claim["cut_tie"] = True
                out.append(case(f"count-m{m}-cut{k}", 50, claim, heat=heat, dist=0, border=0, max_keypoints=k))
    return out


def _size():
    out = []
    for H, W in ((8, 8), (8, 16), (16, 8), (24, 40)):
        heat = random_heat(np.random.default_rng(60 + H + W), H, W)
        heat[H - 1, W - 1] = 1.0  # the last pixel, as far from every window's centre as a pixel gets
        out.append(case(f"size-{H}x{W}", 60 + H, dict(cells=(H // 8, W // 8), present=[(W - 1, H - 1)]), heat=heat, border=0, dist=1))
    return out


def _sample():
    out = []
    # 16 x 24: x = 0, y = 0 reads cell (0, 0) alone, x = 1 .. 12 of row 0 cells (0, 0) and (0, 1) alone; every other pixel
    # mixes in an ordinary cell.
    # 8 x 16 (Hc = 1: the lower taps are the zero padding): x = 0 reads cell (0, 0) alone in all 8 rows, x > 0 mixes it with
    # cell (0, 1).  A cell of zeros alone gives 0 / 0 = NaN; 1e-40 alone, or with zeros, gives values whose squares are 0, so
    # x / 0 = +inf.
    for H, W, tiny, nan_rows, inf_rows in ((16, 24, (0, 1), 1, 12), (8, 16, (0, 1), 8, 120), (16, 8, (1, 0), 8, 120)):
        rng = np.random.default_rng(70 + W)
        desc = unit_desc(rng, H, W).copy()
        desc[0, 0] = 0
        desc[tiny] = F32(1e-40)
        heat = (rng.random((H, W)) * 0.9 + 0.05).astype(F32)
        out.append(case(f"sample-{H}x{W}", 70, dict(norm0_cells={(0, 0): 0.0, tiny: 1e-40}, all_pixels=H * W, nan_rows=nan_rows, inf_rows=inf_rows),
                        heat=heat, desc=desc, thresh=0, dist=0, border=0, max_keypoints=384))
    return out


LOGITS = np.array([-200, -104, -103, -100, -87.4, 0, 88.7, 88.73, 100], F32)
TAME = np.array([-104, -103, -100, -87.4, 0, 0, 1.5, -2.25], F32)  # no overflow of the sum: the cells the float64 softmax is compared on


def _logits():
    rng = np.random.default_rng(80)
    semi = np.zeros((3, 4, 65), F32)
    for hc, wc in ((0, 1), (0, 2), (0, 3), (2, 0), (2, 1), (2, 2)):
        semi[hc, wc] = rng.choice(TAME, 65)
    for hc, wc in ((1, 1), (1, 2), (1, 3)):
        semi[hc, wc] = rng.choice(LOGITS, 65)
    semi[0, 0] = -np.inf      # 64 zeros
    semi[0, 1, 17] = np.inf   # NaN there, 0 in the other 63
    semi[0, 2, 40] = np.nan   # the whole cell NaN
    semi[0, 3, 64] = 100      # the dustbin overflows: all zeros
    semi[1, 0] = -100         # 64 denormal heat values
    semi[2, 3, :64] = -87.4   # exp near FLT_MIN over a sum near 1e-5: normal values out of denormal-range terms
    semi[2, 3, 64] = -90
    claim = dict(heat_cells={(0, 0): (0, 64, 0), (0, 1): (1, 63, 0), (0, 2): (64, 0, 0), (0, 3): (0, 64, 0), (1, 0): (0, 0, 64)})
    return [case("logits-24x32", 80, claim, semi=semi, border=0)]


def _normalise():
    H, W = 16, 24
    rng = np.random.default_rng(90)
    desc = (rng.standard_normal((2, 3, 256)) * 3).astype(F32)
    desc[0, 1] = 0
    desc[0, 2] = (rng.standard_normal(256) * 1e20).astype(F32)
    desc[0, 2][np.abs(desc[0, 2]) < 2e19] = 3e19
    desc[1, 0] = (rng.choice([-1, 1], 256) * 1e-30).astype(F32)
    desc[1, 1, 100] = np.nan
    heat = random_heat(rng, H, W)
    kinds = {(0, 0): "ordinary", (0, 1): "zero", (0, 2): "overflow", (1, 0): "underflow", (1, 1): "nan", (1, 2): "ordinary"}
    cells = {(0, 0): (0, 0, 0, 0, 256), (0, 1): (256, 0, 0, 0, 0), (0, 2): (0, 256, 0, 0, 0), (1, 0): (0, 0, 0, 256, 0), (1, 1): (256, 0, 0, 0, 0),
             (1, 2): (0, 0, 0, 0, 256)}
    return [case("normalise-16x24", 90, dict(raw_rows=kinds, cdesc_cells=cells, all_pixels=H * W, nan_rows=NORMALISE_NAN_ROWS),
                 heat=np.maximum(heat, F32(0.001)), desc=desc, normalize=True, thresh=0, dist=0, border=0)]


# every pixel of 16 x 24 is sampled: a row is free of NaN only where no tap with a non-zero weight reads a NaN cell, and
# inf * 0 or inf - inf make more (counted on the oracle's output; asserted equal on the device's)
NORMALISE_NAN_ROWS = 384

FAMILIES = dict(tie=9, chain=4, band=7, nonfinite=3, count=24, size=4, sample=3, logits=1, normalise=1)
CASES = {}
for _build in (_tie, _chain, _band, _nonfinite, _count, _size, _sample, _logits, _normalise):
    for _c in _build():
        assert _c.name not in CASES
        CASES[_c.name] = _c

# one object created for 40 x 56 serves these in turn: each result must equal a fresh object's
STALE = ["chain-raster-up", "sample-16x24", "size-8x8", "tie-plateaus-r4"]


def names(prefix):
    return [n for n in CASES if n.startswith(prefix + "-")]


# ---- the device against the oracle ------------------------------------------------------------------------------------------
def as_result(xy, conf, desc):
    nan = np.isnan(desc).any(1) if len(desc) else np.zeros(0, bool)
    return dict(xy=xy, conf=conf, desc=desc, nan_rows=int(nan.sum()), inf_rows=int((np.isinf(desc).any(1) & ~nan).sum()) if len(desc) else 0)


def install(sp, c):
    sp.setMaps(c.W, c.H, semi=c.semi, heat=c.heat, desc=c.desc, normalize_desc=c.normalize)


def run_device(sp, c, path):
    """one selection of case c on the installed maps -> (result, status, launches)"""
    if path == "host":
        return as_result(*sp.select(c.conf_thresh, c.nms_dist, c.border)), 0, None
    sp.selectDevice(c.conf_thresh, c.nms_dist, c.border)
    xy, conf, desc, status = sp.lastFeatures()
    return as_result(xy, conf, desc), status, sp.lastLaunches()


def check_case(sp, name, orc, launches=None):
    """case `name` on object sp (whose max_keypoints is the case's, or no cut at all) through both paths, twice each"""
    c, ref = CASES[name], ref_of(name, orc)
    assert sp.max_keypoints == c.max_keypoints or len(ref["full_xy"]) <= min(sp.max_keypoints, c.max_keypoints)
    install(sp, c)
    if c.semi is not None:
        assert_same(sp.download(2, c.W, c.H), ref["heat"], f"{name}: heat map")
    if c.normalize:
        assert_same(sp.download(1, c.W, c.H), ref["cdesc"], f"{name}: normalised descriptor map")
    got = {}
    for path in ("host", "device"):
        r, status, n = run_device(sp, c, path)
        assert status == 0, (name, path, status)
        for k in ("xy", "conf", "desc"):
            assert_same(r[k], ref[k], f"{name}: {k}, {path} path")
        assert (r["nan_rows"], r["inf_rows"]) == (c.claim.get("nan_rows", 0), c.claim.get("inf_rows", 0)), (name, path, r["nan_rows"], r["inf_rows"])
        verify(c, dict(r, cdesc=ref["cdesc"]), orc)  # the case's own claims on the device's results
        again, status2, n2 = run_device(sp, c, path)
        for k in ("xy", "conf", "desc"):
            assert np.array_equal(bits(r[k]), bits(again[k])), f"{name}: {k} differs run to run, {path} path"
        assert status2 == 0 and n2 == n
        if launches is not None and n is not None:
            launches.setdefault((c.H, c.W), set()).add(n)
        got[path] = r
    for k in ("xy", "conf", "desc"):
        assert_same(got["device"][k], got["host"][k], f"{name}: {k}, the two paths")
    return got
