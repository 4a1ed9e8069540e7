"""The super-pixel engine's specification restated on the CPU: SLIC as the reference configures gSLICr
(Core/Segmentation/Slic.cpp:33-43 -- RGB colour space, GIVEN_SIZE, coh_weight 0.6, 5 iterations, no connectivity
enforcement), float32 step by step in the written order, integer sums.  numpy's float32 ufuncs round every operation on
its own (no contraction) and np.sqrt is correctly rounded: what the device computes with -ffp-contract=off.

`associate` is vectorised; `associate_scalar` is an independent pixel-by-pixel loop with np.float32 scalars for small
images, which pins the vectorised form (tests/test_slic_engine_oracle.py)."""
import numpy as np

F32 = np.float32
FAR = F32(999999.9999)
COH = F32(0.6)


def check(w, h, S):
    """the sizes the engine takes: S in (10, 256) dividing both sides (gSLICr's map is ceil(W/S) x ceil(H/S), Slic.h sizes
    its arrays by (W/S)(H/S): on a ragged image the reference indexes past its own arrays)"""
    if not (10 < S < 256) or w <= 0 or h <= 0:
        raise ValueError(f"super-pixel size {S} must be in (10, 256)")
    if w % S or h % S:
        raise ValueError(f"super-pixel size {S} must divide {w} x {h}")
    return w // S, h // S


def normalisers(S):
    """(nc, nxy): nxy = t t, t = 1 / (1.4242 S); nc = u u, u = 5 / (1.7321 * 128)"""
    t = F32(1.0) / (F32(1.4242) * F32(S))
    u = F32(5.0) / (F32(1.7321) * F32(128.0))
    return F32(u * u), F32(t * t)


def init_centres(rgb, S):
    """centre k = cy mx + cx at (cx S + S/2, cy S + S/2) (integer division) with that pixel's colour: [n][5] {x, y, c0, c1, c2}"""
    h, w = rgb.shape[:2]
    mx, my = check(w, h, S)
    cy, cx = np.divmod(np.arange(mx * my), mx)
    x, y = cx * S + S // 2, cy * S + S // 2
    out = np.empty((mx * my, 5), F32)
    out[:, 0], out[:, 1] = x, y
    out[:, 2:] = rgb[y, x, :3]
    return out


def associate(rgb, centres, S):
    """labels int32 [h][w]: the nearest of the (up to) nine centres around the pixel's cell; rows i = -1..1, inside them
    columns j = -1..1, strict `<` against 999999.9999f -- the first candidate in scan order wins a tie.  A pixel no
    candidate beats the start value for (centres handed in far away, NaN) keeps its own cell's label."""
    h, w = rgb.shape[:2]
    mx, my = check(w, h, S)
    nc, nxy = normalisers(S)
    p = rgb[..., :3].astype(F32)
    xi, yi = np.meshgrid(np.arange(w), np.arange(h))
    xf, yf = xi.astype(F32), yi.astype(F32)
    cx, cy = xi // S, yi // S
    best = np.full((h, w), FAR, F32)
    lab = np.full((h, w), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                kx, ky = cx + j, cy + i
                valid = (kx >= 0) & (kx < mx) & (ky >= 0) & (ky < my)
                k = np.where(valid, ky * mx + kx, 0)
                c = centres[k]
                e0, e1, e2 = p[..., 0] - c[..., 2], p[..., 1] - c[..., 3], p[..., 2] - c[..., 4]
                dcol = (e0 * e0 + e1 * e1) + e2 * e2
                ex, ey = xf - c[..., 0], yf - c[..., 1]
                dxy = ex * ex + ey * ey
                d = np.sqrt(dcol * nc + (COH * dxy) * nxy)
                better = valid & (d < best)
                best = np.where(better, d, best)
                lab = np.where(better, k, lab).astype(np.int32)
    return np.where(lab < 0, cy * mx + cx, lab).astype(np.int32)


def associate_scalar(rgb, centres, S):
    """the same rule, one pixel and one float32 operation at a time"""
    h, w = rgb.shape[:2]
    mx, my = check(w, h, S)
    nc, nxy = normalisers(S)
    lab = np.empty((h, w), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            for x in range(w):
                best, who = FAR, -1
                p0, p1, p2 = (F32(v) for v in rgb[y, x, :3])
                for i in (-1, 0, 1):
                    for j in (-1, 0, 1):
                        kx, ky = x // S + j, y // S + i
                        if not (0 <= kx < mx and 0 <= ky < my):
                            continue
                        c = centres[ky * mx + kx]
                        e0, e1, e2 = F32(p0 - c[2]), F32(p1 - c[3]), F32(p2 - c[4])
                        dcol = F32(F32(F32(e0 * e0) + F32(e1 * e1)) + F32(e2 * e2))
                        ex, ey = F32(F32(x) - c[0]), F32(F32(y) - c[1])
                        dxy = F32(F32(ex * ex) + F32(ey * ey))
                        d = np.sqrt(F32(F32(dcol * nc) + F32(F32(COH * dxy) * nxy)))
                        if d < best:
                            best, who = d, ky * mx + kx
                lab[y, x] = who if who >= 0 else (y // S) * mx + x // S
    return lab


def sums(rgb, labels, n):
    """integer totals per label: int64 [n][5] {x, y, c0, c1, c2} and counts [n]"""
    h, w = labels.shape
    flat = labels.ravel()
    xi, yi = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    cols = [xi.ravel(), yi.ravel()] + [rgb[..., q].astype(np.int64).ravel() for q in range(3)]
    out = np.zeros((n, 5), np.int64)
    for q, v in enumerate(cols):
        np.add.at(out[:, q], flat, v)
    return out, np.bincount(flat, minlength=n).astype(np.int64)


def update(rgb, labels, centres, S):
    """every centre from the pixels that carry its label: integer sums, converted to float32 once, divided by
    float32(count); a centre without pixels keeps its values.  -> (centres, counts int32, the integer sums)"""
    n = centres.shape[0]
    tot, cnt = sums(rgb, labels, n)
    out = centres.copy()
    nz = cnt > 0
    out[nz] = tot[nz].astype(F32) / cnt[nz].astype(F32)[:, None]
    return out, cnt.astype(np.int32), tot


def segment(rgb, S, iterations=5, centres=None, trace=None):
    """initialise (or `centres`); iterations x (associate, update); associate.  -> labels, the final centres, the counts of
    the last update (zeros without one).  trace: a list that receives (labels, centres, counts, sums) after every update."""
    rgb = np.ascontiguousarray(rgb)
    h, w = rgb.shape[:2]
    mx, my = check(w, h, S)
    c = init_centres(rgb, S) if centres is None else np.array(centres, F32).reshape(mx * my, 5)
    counts = np.zeros(mx * my, np.int32)
    for _ in range(iterations):
        lab = associate(rgb, c, S)
        c, counts, tot = update(rgb, lab, c, S)
        if trace is not None:
            trace.append((lab, c.copy(), counts.copy(), tot))
    return associate(rgb, c, S), c, counts
