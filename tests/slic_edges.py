"""A plain-Python reference of the super-pixel resampling (mmf_slic_downsample, its thresholded form, mmf_slic_downsample_rgb,
mmf_slic_upsample_u8; csrc/slic_kernels.hpp), the edge cases of test_gpu_slic_edges.py and the device-against-reference check.
test_slic_edges_oracle.py pins the reference to the C oracle where that one is defined and asserts every case's claim.

The reference is the reference program's loops (Core/Segmentation/Slic.h:48-146, Slic.cpp:72-112): one np.float32 addition per
pixel in pixel order, integer RGB sums, the division IN PLACE over ascending index.  Where that program is undefined it follows
the device's rules: a label outside [0, n) takes part in nothing, upsample gives 0 there, a substitute
outside [0, n) leaves the super-pixel its own index, an RGB mean over a zero count is 0.

A case is Case(name, W, H, S, labels, inputs, claim).  inputs: image ([H][W] or [H][W][C] float32), channel, threshold, rgb
([H][W][3 or 4] u8), map (u8, nspix entries): every case runs every function.  claim: what the case is there for, as a dict
that verify() asserts on the reference when the case is built -- a case never claims a property its inputs lack.

numpy only at import; torch and the device bindings are imported where a device context is used."""
import collections

import numpy as np

from helpers import bits, slic_like_labels

F32 = np.float32
INT_MAX = 2 ** 31 - 1
Case = collections.namedtuple("Case", "name W H S labels inputs claim")
VARIANTS = ("round", "spx", "clamp")  # wrong ways to find a substitute, which a claim can name as visible


# ---- the reference ----------------------------------------------------------------------------------------------------------
def resample_empty_index(labels, S, index, variant=None):
    """Slic.h:191-209, literally: mapToHigh(index) divides by spixelY, (int)(h S + S 0.5) truncates.  variant: 'round' rounds
    the centre to nearest, 'spx' divides by spixelX, 'clamp' clamps the row to H - 2."""
    H, W = labels.shape
    spx, spy = W // S, H // S
    hx, hy = index % spx, index // (spx if variant == "spx" else spy)
    extra = 0.5 if variant == "round" else 0.0
    cx, cy = int(hx * S + S * 0.5 + extra), int(hy * S + S * 0.5 + extra)
    if cy >= H:
        cy = H - (2 if variant == "clamp" else 1)
    if cx >= W:
        cx = W - 1
    return int(labels[cy, cx])


def substitute(labels, S, n, index, variant=None):
    r = resample_empty_index(labels, S, index, variant)
    return r if 0 <= r < n else index  # a label the census ignores is no substitute


def census(labels, n):
    counts = [0] * n
    for s in labels.ravel().tolist():
        if 0 <= s < n:
            counts[s] += 1
    return counts


def pixel_order_sums(labels, n, values, threshold):
    """(sums, used): one float32 `+` per pixel that takes part, in pixel order"""
    total, used = [F32(0)] * n, [0] * n
    thr = None if threshold is None else F32(threshold)
    with np.errstate(all="ignore"):
        for s, v in zip(labels.ravel().tolist(), values):  # (v is an np.float32)
            if 0 <= s < n and (thr is None or v > thr):
                total[s] = total[s] + v
                used[s] += 1
    return total, used


def downsample(labels, S, image, channel=0, threshold=None, variant=None):
    """-> (out [H/S][W/S] float32, counts [n] int32, used [n]: the divisor counts of the mode)"""
    H, W = labels.shape
    spx, spy = W // S, H // S
    n = spx * spy
    values = np.ascontiguousarray(image, F32).reshape(H * W, -1)[:, channel]
    counts = census(labels, n)
    out, used = pixel_order_sums(labels, n, values, threshold)
    with np.errstate(all="ignore"):
        for s in range(n):  # in place, ascending: a lower substitute is a mean already, a higher one a raw sum
            cnt, r = used[s], s
            if cnt == 0:
                r = substitute(labels, S, n, s, variant)
                cnt = counts[r]
            out[s] = out[r] / F32(cnt)
    return np.array(out, F32).reshape(spy, spx), np.array(counts, np.int32), used


def downsample_rgb(labels, S, rgb, variant=None):
    """-> [H/S][W/S][3] u8: integer means of input channels (2, 1, 0)"""
    H, W = labels.shape
    spx, spy = W // S, H // S
    n = spx * spy
    counts, sums = [0] * n, [[0, 0, 0] for _ in range(n)]
    for s, px in zip(labels.ravel().tolist(), rgb.reshape(H * W, -1).tolist()):
        if 0 <= s < n:
            counts[s] += 1
            t = sums[s]
            t[0] += px[2]
            t[1] += px[1]
            t[2] += px[0]
    out = np.zeros((n, 3), np.uint8)
    for s in range(n):
        cnt, r = counts[s], s
        if cnt == 0:
            r = substitute(labels, S, n, s, variant)
            cnt = counts[r]
        for k in range(3):
            out[s, k] = min(max(sums[r][k] // cnt, 0), 255) if cnt else 0
    return out.reshape(spy, spx, 3)


def upsample_u8(labels, small):
    m = small.tolist()
    return np.array([m[s] if 0 <= s < len(m) else 0 for s in labels.ravel().tolist()], np.uint8).reshape(labels.shape)


def chains(labels, S, n, used):
    """{s: (depth, end)} of every super-pixel without a divisor of its own: the number of substitutions until a value is
    found, which is 'lower' (a finished mean), 'higher' (a raw sum), 'self' (its own raw sum) or 'none' (no substitute)"""
    out = {}
    for s in range(n):
        depth, idx, end = 0, s, "lower"
        while used[idx] == 0:
            depth += 1
            r = resample_empty_index(labels, S, idx)
            if not 0 <= r < n:
                end = "none"
            elif r == idx:
                end = "self"
            elif r > idx:
                end = "higher"
            if end != "lower":
                break
            idx = r
        if depth:
            out[s] = (depth, end)
    return out


def reference(c, variant=None):
    i = c.inputs
    n = (c.W // c.S) * (c.H // c.S)
    plain, counts, used = downsample(c.labels, c.S, i["image"], i["channel"], None, variant)
    thr, _, used_thr = downsample(c.labels, c.S, i["image"], i["channel"], i["threshold"], variant)
    return dict(plain=plain, counts=counts, thr=thr, used_thr=used_thr, rgb=downsample_rgb(c.labels, c.S, i["rgb"], variant),
                up=upsample_u8(c.labels, i["map"]), chains_plain=chains(c.labels, c.S, n, used),
                chains_thr=chains(c.labels, c.S, n, used_thr))


def same(a, b):
    """equal bit for bit, except that a NaN equals any NaN (sign and payload are no contract)"""
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
def verify(c, ref):
    """assert everything c.claim says, on the reference and the inputs; an unknown key is an error"""
    H, W, S = c.H, c.W, c.S
    spx, spy = W // S, H // S
    n = spx * spy
    lab, flat, img = c.labels, c.labels.ravel(), c.inputs["image"]
    assert lab.shape == (H, W) and lab.dtype == np.int32 and 10 < S < 256 and n >= 1
    assert (img.shape[2] if img.ndim == 3 else 1) > c.inputs["channel"] >= 0 and c.inputs["rgb"].shape[:2] == (H, W)
    in_range = (flat >= 0) & (flat < n)
    counts = np.bincount(flat[in_range], minlength=n)
    assert np.array_equal(counts, ref["counts"])
    for key, v in c.claim.items():
        if key == "n":
            assert n == v
        elif key == "grid":
            assert (spx, spy) == v
        elif key == "wave":  # one wave covers several rows; the last wave is partly dead
            assert (W < 64) == v["rows_per_wave"] and (W * H) % 64 == v["tail"]
        elif key == "thr_chains":
            assert ref["chains_thr"] == v, ref["chains_thr"]
        elif key == "plain_chains":
            assert ref["chains_plain"] == v, ref["chains_plain"]
        elif key == "distinct_counts":  # the divisors of a chain's levels: a wrong level shows
            assert len({int(counts[s]) for s in v}) == len(v) and all(counts[s] for s in v)
        elif key == "absent":
            assert sorted(np.flatnonzero(counts == 0).tolist()) == sorted(v)
        elif key == "differs":  # {variant: modes}: the wrong substitute is visible in these outputs
            for variant, modes in v.items():
                assert variant in VARIANTS
                wrong = reference(c, variant)
                for mode in modes:
                    assert not same(wrong[mode], ref[mode]), (variant, mode)
        elif key == "trunc":  # (s, by truncation, by rounding)
            s, a, b = v
            assert S % 2 == 1 and ref["chains_plain"][s][0] == 1
            assert resample_empty_index(lab, S, s) == a and resample_empty_index(lab, S, s, "round") == b
            assert a != b and 0 <= a < n and 0 <= b < n and counts[a] and counts[b]
            hx, hy = s % spx, s // spy
            assert lab[hy * S + (S - 1) // 2, hx * S + (S - 1) // 2] == a and lab[hy * S + (S - 1) // 2, hx * S + (S + 1) // 2] == b
        elif key == "clamp":  # (s, label in row H - 1, label in the row that index / spx gives)
            s, a, b = v
            hx, hy = s % spx, s // spy
            assert ref["chains_plain"][s][0] == 1 and hy * S + S // 2 >= H and hy >= spy
            assert resample_empty_index(lab, S, s) == a == lab[H - 1, hx * S + S // 2] and resample_empty_index(lab, S, s, "spx") == b
            assert a != b and lab[H - 2, hx * S + S // 2] != a and counts[a] and counts[b]
        elif key == "nan":  # {mode: indices}: NaN exactly there
            for mode, at in v.items():
                assert np.flatnonzero(np.isnan(ref[mode].ravel())).tolist() == sorted(at), (mode, np.flatnonzero(np.isnan(ref[mode].ravel())))
        elif key == "zero":  # {mode: indices}: +0 there (all three channels in 'rgb')
            for mode, at in v.items():
                r = ref[mode].reshape(n, -1)
                assert all((bits(r[s]) == 0).all() for s in at), mode
        elif key == "oob":  # {value: number of pixels}, nothing else out of range
            assert {int(x): int((flat == x).sum()) for x in np.unique(flat[~in_range])} == v
        elif key == "oob_ends":
            assert (int(flat[0]), int(flat[-1])) == v and not in_range[0] and not in_range[-1]
        elif key == "oob_runs":  # (row, x0, x1, value, label on both sides): inside one wave, between two runs of one label
            for y, x0, x1, val, side in v:
                assert (lab[y, x0:x1 + 1] == val).all() and not 0 <= val < n and x1 > x0
                assert lab[y, x0 - 1] == lab[y, x1 + 1] == side and 0 <= side < n
                assert (y * W + x0 - 1) // 64 == (y * W + x1 + 1) // 64
        elif key == "singles":  # (y, x, value): one pixel out of range, in-range neighbours
            for y, x, val in v:
                assert lab[y, x] == val and not 0 <= val < n and 0 <= lab[y, x - 1] < n and 0 <= lab[y, x + 1] < n
        elif key == "run_across":  # pixel indices p: p - 1 and p continue one run
            for p in v:
                assert p % 64 == 0 and p % W != 0 and flat[p - 1] == flat[p] and in_range[p]
        elif key == "box":  # {s: (min_x, min_y, max_x, max_y)}
            for s, box in v.items():
                ys, xs = np.nonzero(lab == s)
                assert (xs.min(), ys.min(), xs.max(), ys.max()) == box, (s, xs.min(), ys.min(), xs.max(), ys.max())
        elif key == "only_last_row_and_column":
            ys, xs = np.nonzero(lab == v)
            assert len(ys) and ((ys == H - 1) | (xs == W - 1)).all() and lab[H - 1, W - 1] == v and (ys == H - 1).any() and (xs == W - 1).any()
        elif key == "order":  # super-pixels whose float32 sum depends on the order of the additions
            for s in v:
                vals = img[lab == s]
                fwd, _ = pixel_order_sums(np.zeros(len(vals), np.int32), 1, vals, None)
                rev, _ = pixel_order_sums(np.zeros(len(vals), np.int32), 1, vals[::-1], None)
                mag = np.abs(vals[vals != 0])
                assert bits(fwd[0]) != bits(rev[0]) and bits(fwd[0]) != bits(vals.sum(dtype=F32)), s
                assert mag.min() < 1e-2 and mag.max() > 1e6 and fwd[0] / F32(len(vals)) == ref["plain"].ravel()[s]
        elif key == "threshold":
            thr = F32(c.inputs["threshold"])
            assert all(img[p] == thr for p in v["at"]) and all(img[p] == np.nextafter(thr, F32(np.inf)) for p in v["above"])
            assert {s: ref["used_thr"][s] for s in v["used"]} == v["used"]
        elif key == "special":  # {kind: pixels}
            test = dict(nan=np.isnan, inf=lambda x: x == np.inf, ninf=lambda x: x == -np.inf, negzero=lambda x: (x == 0) & np.signbit(x))
            for kind, at in v.items():
                assert at and all(test[kind](img[p]) for p in at), kind
        elif key == "all_negzero":  # a super-pixel of -0.0 alone: 0.f + -0.0 is +0
            vals = img[lab == v]
            assert len(vals) and (vals == 0).all() and np.signbit(vals).all() and bits(ref["plain"].ravel()[v]) == 0
        elif key == "channels":
            assert (img.shape[2], c.inputs["channel"]) == v
            others = [downsample(lab, S, img, ch)[0] for ch in range(img.shape[2]) if ch != v[1]]
            assert all(not same(o, ref["plain"]) for o in others)
        elif key == "rgb_channels":
            assert c.inputs["rgb"].shape[2] == v
        elif key == "rgb_all":  # {s: value}: every byte of the super-pixel
            for s, val in v.items():
                px = c.inputs["rgb"][lab == s]
                assert len(px) and (px[:, :3] == val).all() and (ref["rgb"].reshape(n, 3)[s] == val).all()
        elif key == "rgb_mean":  # {s: (out 0, out 1, out 2)}, None = any
            for s, want in v.items():
                assert all(w is None or ref["rgb"].reshape(n, 3)[s, k] == w for k, w in enumerate(want))
        elif key == "map":  # (nspix, pixels that read the map beyond the grid, pixels that get 0)
            nspix, beyond, zeroed = v
            assert c.inputs["map"].size == nspix and (c.inputs["map"] != 0).all()
            assert int(((flat >= n) & (flat < nspix)).sum()) == beyond and int((ref["up"] == 0).sum()) == zeroed
        else:
            raise KeyError(key)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def grid_labels(W, H, S):
    spx, spy = W // S, H // S
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.minimum(yy // S, spy - 1) * spx + np.minimum(xx // S, spx - 1)).astype(np.int32)


def centre(W, H, S, s):
    """(cx, cy): the pixel super-pixel s takes its substitute from"""
    spx, spy = W // S, H // S
    return min(int((s % spx) * S + S * 0.5), W - 1), min(int((s // spy) * S + S * 0.5), H - 1)


def fill(W, H, S, seed, channels=1, channel=0, rgb_channels=3, threshold=0.02, nspix=None):
    rng = np.random.default_rng(seed)
    shape = (H, W) if channels == 1 else (H, W, channels)
    image = (rng.random(shape, dtype=F32) ** 2 * F32(4)).astype(F32)
    image[rng.random(shape) < 0.25] = 0  # invalid depth
    n = (W // S) * (H // S)
    return dict(image=image, channel=channel, threshold=threshold, rgb=rng.integers(0, 256, (H, W, rgb_channels), dtype=np.uint8),
                map=rng.integers(1, 256, n if nspix is None else nspix, dtype=np.uint8))


REF = {}  # name -> reference(case), computed when the case is built


def case(name, S, labels, inputs, claim):
    labels = np.ascontiguousarray(labels, np.int32)
    H, W = labels.shape
    c = Case(name, W, H, S, labels, inputs, claim)
    ref = reference(c)
    verify(c, ref)
    for a in (labels, inputs["image"], inputs["rgb"], inputs["map"]):
        a.setflags(write=False)
    REF[name] = ref
    return c


def drop(labels, s, to):
    labels[labels == s] = to


def paint_centre(labels, S, s, value):
    H, W = labels.shape
    cx, cy = centre(W, H, S, s)
    labels[cy, cx] = value


GW, GH, GS, GN = 160, 128, 16, 80  # the chain cases' image: 10 x 8 super-pixels


def _shapes():
    out = []
    lab = np.zeros((11, 11), np.int32)
    out.append(case("shape-11x11-S11", 11, lab, fill(11, 11, 11, 1), dict(n=1, wave=dict(rows_per_wave=True, tail=57))))
    lab = slic_like_labels(33, 47, 11, seed=5, empty_every=5)
    out.append(case("shape-33x47-S11", 11, lab, fill(33, 47, 11, 2, rgb_channels=4),
                    dict(grid=(3, 4), wave=dict(rows_per_wave=True, tail=1551 % 64), absent=[5, 10], differs=dict(spx=("plain", "thr", "rgb")))))
    lab = slic_like_labels(75, 26, 13, seed=2, empty_every=4)
    out.append(case("shape-75x26-S13", 13, lab, fill(75, 26, 13, 3),
                    dict(grid=(5, 2), wave=dict(rows_per_wave=False, tail=1950 % 64), absent=[4, 8], differs=dict(spx=("plain", "thr", "rgb")))))
    lab = grid_labels(130, 24, 12)
    drop(lab, 17, 16)
    lab[23, :] = 17
    lab[:, 129] = 17
    lab[5:7, :] = 3  # a band as wide as the image: three 64-lane steps per row of the box
    out.append(case("shape-130x24-S12", 12, lab, fill(130, 24, 12, 4, rgb_channels=4),
                    dict(grid=(10, 2), box={3: (0, 0, 129, 11), 17: (0, 0, 129, 23)}, only_last_row_and_column=17,
                         wave=dict(rows_per_wave=False, tail=3120 % 64))))
    lab = slic_like_labels(GW, GH, GS, seed=1, empty_every=7)
    out.append(case("shape-160x128-S16", GS, lab, fill(GW, GH, GS, 5), dict(grid=(10, 8), absent=list(range(7, 80, 7)))))
    inp = fill(255, 255, 255, 6)
    inp["rgb"][..., 2], inp["rgb"][..., 1] = 255, 0
    out.append(case("shape-255x255-S255", 255, np.zeros((255, 255), np.int32), inp,
                    dict(n=1, rgb_mean={0: (255, 0, None)}, wave=dict(rows_per_wave=False, tail=65025 % 64))))
    return out


def _chain(name, links, zeroed, claim, absent=(), seed=10):
    """links: (s, label painted on s's centre pixel); zeroed: labels without a valid depth.  The borders wobble, so the
    super-pixels' counts differ and a divisor taken from the wrong level shows."""
    lab = slic_like_labels(GW, GH, GS, seed=3)
    for s, to in absent:
        drop(lab, s, to)
    for s, to in links:
        paint_centre(lab, GS, s, to)
    inp = fill(GW, GH, GS, seed)
    inp["image"][np.isin(lab, zeroed)] = 0
    return case(name, GS, lab, inp, claim)


def _chains():
    out = [
        _chain("chain-d2-lower", [(50, 30), (30, 12)], [50, 30], dict(thr_chains={50: (2, "lower"), 30: (1, "lower")}, plain_chains={}, distinct_counts=[12, 30])),
        _chain("chain-d3-lower", [(70, 51), (51, 33), (33, 14)], [70, 51, 33],
               dict(thr_chains={70: (3, "lower"), 51: (2, "lower"), 33: (1, "lower")}, plain_chains={}, distinct_counts=[14, 33, 51])),
        _chain("chain-d2-higher", [(40, 20), (20, 60)], [40, 20], dict(thr_chains={40: (2, "higher"), 20: (1, "higher")}, plain_chains={}, distinct_counts=[20, 60])),
        _chain("chain-self", [(45, 3), (3, 3)], [45, 3], dict(thr_chains={3: (1, "self"), 45: (2, "self")}, plain_chains={},
                                                      zero=dict(thr=[3, 45]))),
        _chain("chain-absent", [(37, 5)], [], dict(absent=[37, 62], plain_chains={37: (1, "lower"), 62: (1, "higher")},
                                                   thr_chains={37: (1, "lower"), 62: (1, "higher")}), absent=[(37, 36), (62, 61)]),
        _chain("chain-no-substitute", [(37, -1), (62, GN), (23, INT_MAX), (20, -1)], [20],
               dict(absent=[23, 37, 62], plain_chains={23: (1, "none"), 37: (1, "none"), 62: (1, "none")},
                    thr_chains={20: (1, "none"), 23: (1, "none"), 37: (1, "none"), 62: (1, "none")},
                    nan=dict(plain=[23, 37, 62], thr=[23, 37, 62]), zero=dict(rgb=[23, 37, 62], thr=[20]),
                    oob={-1: 2, GN: 1, INT_MAX: 1}), absent=[(37, 36), (62, 61), (23, 22)]),
    ]
    return out


def _index():
    W, H, S = 75, 26, 13
    lab = grid_labels(W, H, S)
    drop(lab, 3, 2)
    lab[19:21, 46] = 6  # the boundary between x = 3 S + 6 and 3 S + 7 in the row of super-pixel 3's centre
    lab[20, 45] = 6
    trunc = case("index-odd-S-truncation", S, lab, fill(W, H, S, 20), dict(absent=[3], trunc=(3, 8, 6), differs=dict(round=("plain", "thr", "rgb"))))
    lab = grid_labels(W, H, S)
    drop(lab, 4, 3)
    lab[25, 58] = 7  # hy = 4 / spy = 2: the centre row 32 clamps to 25
    clamp = case("index-clamped-row", S, lab, fill(W, H, S, 21),
                 dict(absent=[4], clamp=(4, 7, 3), differs=dict(spx=("plain", "thr", "rgb"), clamp=("plain", "thr", "rgb"))))
    return [trunc, clamp]


def _oob():
    out = []
    lab = grid_labels(GW, GH, GS)
    singles = [(10, 10, -1), (50, 70, GN), (100, 130, INT_MAX), (127, 80, -1), (64, 1, GN)]
    for y, x, v in singles:
        lab[y, x] = v
    out.append(case("oob-single-pixels", GS, lab, fill(GW, GH, GS, 30), dict(singles=singles, oob={-1: 2, GN: 2, INT_MAX: 1})))
    lab = grid_labels(GW, GH, GS)
    runs = [(40, 20, 24, -1, 21), (72, 100, 110, GN, 46), (100, 130, 140, INT_MAX, 68)]
    for y, x0, x1, v, _ in runs:
        lab[y, x0:x1 + 1] = v
    out.append(case("oob-run-between-runs", GS, lab, fill(GW, GH, GS, 31, rgb_channels=4), dict(oob_runs=runs, oob={-1: 5, GN: 11, INT_MAX: 11})))
    for tag, first, last in (("a", -1, INT_MAX), ("b", GN, -1)):
        lab = grid_labels(GW, GH, GS)
        lab[0, 0], lab[-1, -1] = first, last
        out.append(case(f"oob-first-and-last-pixel-{tag}", GS, lab, fill(GW, GH, GS, 32), dict(oob_ends=(first, last), oob={first: 1, last: 1})))
    lab = np.zeros((11, 11), np.int32)
    lab[0, 0], lab[5, 5], lab[10, 10] = -1, 1, INT_MAX
    out.append(case("oob-one-super-pixel", 11, lab, fill(11, 11, 11, 33), dict(n=1, oob={-1: 1, 1: 1, INT_MAX: 1}, oob_ends=(-1, INT_MAX))))
    return out


def _waves():
    lab = grid_labels(GW, GH, GS)
    lab[0, 64:71] = 3   # label 3's run 48 .. 70 crosses pixel 64 (a wave boundary)
    lab[1, 96:101] = 5  # label 5's run crosses pixel 256 (a workgroup boundary)
    a = case("wave-run-across-64-and-256", GS, lab, fill(GW, GH, GS, 40, rgb_channels=4), dict(run_across=[64, 256]))
    b = case("wave-run-across-64-narrow", 11, grid_labels(33, 47, 11), fill(33, 47, 11, 41),
             dict(run_across=[64, 128], wave=dict(rows_per_wave=True, tail=1551 % 64)))
    return [a, b]


def _sums():
    out = []
    lab = grid_labels(GW, GH, GS)
    rng = np.random.default_rng(50)
    inp = fill(GW, GH, GS, 50)
    inp["image"] = (np.where(rng.random((GH, GW)) < 0.3, -1, 1) * 10.0 ** rng.uniform(-3, 7, (GH, GW))).astype(F32)
    out.append(case("sum-order-sensitive", GS, lab, inp, dict(order=[0, 22, 57, 79])))
    thr = F32(0.02)
    inp = fill(GW, GH, GS, 51)
    img = inp["image"]
    img[np.isin(lab, (11, 12))] = 0
    at, above = [(18, 20), (30, 31), (20, 40)], [(25, 25)]  # (y, x): two in label 11, one in label 12; the one above in 11
    for p in at:
        img[p] = thr
    img[above[0]] = np.nextafter(thr, F32(np.inf))
    out.append(case("sum-threshold-met-exactly", GS, lab, inp, dict(threshold=dict(at=at, above=above, used={11: 1, 12: 0}),
                                                                      thr_chains={12: (1, "self")})))
    for name, threshold in (("sum-special-values-thr-0.02", 0.02), ("sum-special-values-thr--1", -1.0)):
        inp = fill(GW, GH, GS, 52, threshold=threshold)
        img = inp["image"]
        img[20, 20] = np.nan                    # label 11
        img[20, 40], img[24, 100] = np.inf, np.inf   # labels 12 and 16
        img[lab == 13] = -0.0
        img[22, 70], img[23, 71] = -0.0, -0.0   # label 14, among positive values
        img[25, 101] = -np.inf                  # label 16: inf + -inf
        plain_nan, thr_nan = [11, 16], []
        out.append(case(name, GS, lab, inp, dict(special=dict(nan=[(20, 20)], inf=[(20, 40), (24, 100)], ninf=[(25, 101)],
                                                              negzero=[(22, 70), (23, 71), (16, 48)]),
                                                 all_negzero=13, nan=dict(plain=plain_nan, thr=thr_nan))))
    lab = slic_like_labels(33, 47, 11, seed=6, empty_every=5)
    for ch in range(4):
        out.append(case(f"sum-4-channels-channel-{ch}", 11, lab.copy(), fill(33, 47, 11, 53, channels=4, channel=ch), dict(channels=(4, ch))))
    return out


def _rgb():
    out = []
    for ch in (3, 4):
        lab = slic_like_labels(75, 26, 13, seed=7, empty_every=3)
        out.append(case(f"rgb-{ch}-channels", 13, lab, fill(75, 26, 13, 60, rgb_channels=ch), dict(rgb_channels=ch, absent=[3, 6, 9])))
    lab = grid_labels(GW, GH, GS)
    inp = fill(GW, GH, GS, 61, rgb_channels=4)
    inp["rgb"][lab == 11] = 255
    inp["rgb"][lab == 12] = 0
    out.append(case("rgb-all-255-and-all-0", GS, lab, inp, dict(rgb_all={11: 255, 12: 0}, rgb_channels=4)))
    return out


def _upsample():
    lab = grid_labels(GW, GH, GS)
    a = case("up-map-of-one", GS, lab, fill(GW, GH, GS, 70, nspix=1), dict(map=(1, 0, GW * GH - 256)))
    lab = grid_labels(GW, GH, GS)
    lab[3, 3:6], lab[60, 60:70], lab[90, 5:9], lab[127, 150:160] = GN, GN + 6, GN + 7, -1
    b = case("up-map-larger-than-the-grid", GS, lab, fill(GW, GH, GS, 71, nspix=GN + 7),
             dict(map=(GN + 7, 13, 14), oob={-1: 10, GN: 3, GN + 6: 10, GN + 7: 4}))
    return [a, b]


FAMILIES = dict(shape=6, chain=6, index=2, oob=5, wave=2, sum=8, rgb=3, up=2)  # prefix -> number of cases
CASES = {}
for _build in (_shapes, _chains, _index, _oob, _waves, _sums, _rgb, _upsample):
    for _c in _build():
        assert _c.name not in CASES
        CASES[_c.name] = _c

# one context, n = 80, 1, 12, 80, 10: modes alternate, and a thresholded call comes directly before a plain one on the same labels
SEQUENCE = [("chain-d3-lower", "thr"), ("chain-d3-lower", "plain"), ("shape-11x11-S11", "rgb"), ("shape-33x47-S11", "thr"),
            ("chain-no-substitute", "rgb"), ("chain-no-substitute", "thr"), ("chain-no-substitute", "plain"),
            ("index-clamped-row", "thr"), ("index-clamped-row", "plain"), ("index-clamped-row", "rgb")]
REFUSALS = ["channel-is-channels", "channel-negative", "rgb-2-channels", "S10", "S256", "nspix0", "null-image", "null-labels"]


def names(prefix):
    return [n for n in CASES if n.startswith(prefix + "-")]


def cells(c):
    return (c.W // c.S) * (c.H // c.S)


def oracle_defined(c):
    """the C oracle indexes by label and divides integers by the count: defined where every label is in [0, n), which also
    gives every substitute pixels"""
    return bool(c.labels.min() >= 0 and c.labels.max() < cells(c))


# ---- the device against the reference ---------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)


def run_device(gpu_ctx, c, mode):
    """one call of `mode` on case c -> {name: numpy array}"""
    from multimotionfusion_amd import slic
    i = c.inputs
    labels = dev(c.labels)
    if mode == "plain":
        out, counts = slic.downsample(gpu_ctx, labels, c.S, dev(i["image"]), channel=i["channel"], with_counts=True)
        return dict(plain=out.cpu().numpy(), counts=counts.cpu().numpy().ravel())
    if mode == "thr":
        return dict(thr=slic.downsample(gpu_ctx, labels, c.S, dev(i["image"]), channel=i["channel"], threshold=i["threshold"]).cpu().numpy())
    if mode == "rgb":
        return dict(rgb=slic.downsample_rgb(gpu_ctx, labels, c.S, dev(i["rgb"])).cpu().numpy())
    assert mode == "up"
    return dict(up=slic.upsample_u8(gpu_ctx, labels, dev(i["map"])).cpu().numpy())


MODES = ("plain", "thr", "rgb", "up")


def check_case(gpu_ctx, name, modes=MODES, twice=True):
    c, ref = CASES[name], REF[name]
    for mode in modes:
        got = run_device(gpu_ctx, c, mode)
        for k, v in got.items():
            assert_same(v, ref[k], f"{name}: {k}")
        if twice:  # the same inputs give the same bytes, NaNs included
            again = run_device(gpu_ctx, c, mode)
            for k, v in got.items():
                assert np.array_equal(bits(v), bits(again[k])), f"{name}: {k} differs run to run"
