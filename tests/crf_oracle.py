"""The dense-CRF motion segmentation (Segmentation::performSegmentationCRF, Core/Segmentation/Segmentation.cpp:159-740)
restated in numpy: the checker of csrc/crf_kernels.hpp.

Stages 2-4 (depth range, average confidences, unaries) run in float32 with the reference's expression order and
literal types (double literals compare and multiply in double), so they are bit-exact to the device.  Stages 5-6
(kernels, mean field) are EXACT Gaussian sums in float64.  Stages 7-13 (argmax, connected components,
largest component per label, size / border rules, depth statistics) replay the reference's loops; float sums run in
cell order.  Stage 1 (super-pixel means) is the oracle's `slic_downsample`.
"""
import numpy as np

F32 = np.float32

# GUI defaults (GUI/Tools/GUI.h:211-226, GUI/MainController.cpp:658-670); the header defaults of Segmentation.h:140-159
# (1/30, 1/0.4, 1/8, 40, 40, 5, 0.01, 40, 10 iterations, 0.07 / 0.4) are what a Segmentation object starts with before the
# GUI pushes these.
DEFAULTS = dict(sigma_rgb=10.0, sigma_depth=0.9, sigma_pos=1.8, weight_appearance=7.0, weight_smoothness=2.0,
                threshold_new=5.5, unary_weight_error=75.0, unary_k_error=0.0375, iterations=10,
                min_rel_size_new=0.005, max_rel_size_new=0.4, spixel_size=16, model_spawn_offset=22, inhibit_new=0)

MAX_DEPTH = F32(100.0)
BORDER = 20


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def grid_labels(W, H, S):
    """B3: the regular grid the product uses when no super-pixel label image is handed in."""
    spx, spy = W // S, H // S
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.minimum(yy // S, spy - 1) * spx + np.minimum(xx // S, spx - 1)).astype(np.int32)


def seq_sum(v):
    """float32 sum in element order (np.add.accumulate is sequential)"""
    v = np.asarray(v, F32)
    return F32(0.0) if v.size == 0 else F32(np.add.accumulate(np.concatenate([[F32(0.0)], v]), dtype=F32)[-1])


def depth_range(low_depth):
    """:198-210"""
    d = np.asarray(low_depth, F32).ravel()
    ok = np.isfinite(d) & (d >= 0) & (d <= MAX_DEPTH)
    dmax = F32(0.0) if not ok.any() else max(F32(0.0), d[ok].max())
    dmin = np.finfo(F32).max if not ok.any() else min(np.finfo(F32).max, d[ok].min())
    return F32(F32(dmax) - F32(dmin))


def avg_confidence(conf):
    """:225-237 -- conf [M][N] float32 is modified in place (non-finite -> 0); returns [M] float32"""
    conf[~np.isfinite(conf)] = 0
    N = conf.shape[1]
    return np.array([F32(seq_sum(conf[i]) / F32(N)) for i in range(conf.shape[0])], F32)


def range_invalid(rng):
    """B4: the product's deviation when the depth range is not a finite positive number"""
    return not (np.isfinite(rng) and rng > 0)


def unaries(err, conf, rng, cfg, allow_new):
    """:271-332 and the clamp of :491-494.  err, conf [M][N] float32 (err is modified in place like lowICP);
    returns U [L][N] float32, L = M + allow_new"""
    M, N = err.shape
    rng = F32(rng)
    wE, kE, thr = F32(cfg["unary_weight_error"]), F32(cfg["unary_k_error"]), F32(cfg["threshold_new"])
    with np.errstate(all="ignore"):
        err[0] = np.where(conf[0].astype(np.float64) < 0.3, F32(np.float64(rng) * 0.01), err[0])
        for i in range(1, M):
            err[i] = np.where(conf[i].astype(np.float64) <= 0.4, F32(rng * kE), err[i])
        e = (err / rng).astype(F32)
        U = np.empty((M + int(bool(allow_new)), N), F32)
        U[:M] = (wE * e).astype(F32)
        lowest = e[0].copy()
        for i in range(M):
            lowest = np.where(e[i] < lowest, e[i], lowest)
        if allow_new:
            a = (thr - (wE * lowest).astype(F32)).astype(F32)
            U[M] = np.where(a < F32(0.01), F32(0.01), a)
        U = np.where(U.astype(np.float64) <= 1e-5, F32(1e-5), U).astype(F32)
    return U


def features(spx, spy, rgb_first, low_depth, cfg):
    """:470-486: smoothness (x/2, y/2) and appearance (x/sp, y/sp, c/srgb x3, min(d/sd, 100)) per cell, float32.
    rgb_first = the first N*3 bytes of the FULL-resolution frame (the reference's quirk)."""
    N = spx * spy
    k = np.arange(N)
    x, y = (k % spx).astype(F32), (k // spx).astype(F32)
    sp, sr, sd = F32(1.0) / F32(cfg["sigma_pos"]), F32(1.0) / F32(cfg["sigma_rgb"]), F32(1.0) / F32(cfg["sigma_depth"])
    fs = np.stack([x / F32(2.0), y / F32(2.0)], 1).astype(F32)
    c = np.asarray(rgb_first, np.uint8).reshape(-1)[:3 * N].reshape(N, 3).astype(F32)
    d = (np.asarray(low_depth, F32).ravel() * sd).astype(F32)
    d = np.where(F32(100.0) < d, F32(100.0), d)
    fa = np.stack([x * sp, y * sp, c[:, 0] * sr, c[:, 1] * sr, c[:, 2] * sr, d], 1).astype(F32)
    return fs, fa


def softmax(v):
    """DenseCRF::expAndNormalize over labels (axis 0), float64, column maximum subtracted"""
    e = np.exp(v - v.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def pair_matrix(fs, fa, cfg, chunk=512):
    """A = w_s Ds Ks Ds + w_a Da Ka Da, float64 [N][N], K_ij = exp(-|f_i - f_j|^2 / 2) (j = i included),
    D_ii = 1 / sqrt(sum_j K_ij + 1e-20) (densecrf 2 DenseKernel, NORMALIZE_SYMMETRIC: B2)"""
    N = fs.shape[0]
    A = np.zeros((N, N))
    for f, w in ((fs, cfg["weight_smoothness"]), (fa, cfg["weight_appearance"])):
        f = f.astype(np.float64)
        K = np.empty((N, N))
        for a in range(0, N, chunk):
            K[a:a + chunk] = np.exp(-0.5 * ((f[a:a + chunk, None, :] - f[None, :, :]) ** 2).sum(-1))
        D = 1.0 / np.sqrt(K.sum(1) + 1e-20)
        A += float(w) * (K * D[:, None] * D[None, :])
    return A


def mean_field(U, fs, fa, cfg, A=None):
    """:496-506: Q = softmax(-U); iterations x Q = softmax(-U + A Q).  Returns Q [L][N] float64."""
    u = -np.asarray(U, np.float64)
    Q = softmax(u)
    if int(cfg["iterations"]) > 0:
        A = pair_matrix(fs, fa, cfg) if A is None else A
        for _ in range(int(cfg["iterations"])):
            Q = softmax(u + (A @ Q.T).T)
    return Q


def argmax_labels(Q):
    """:510-513: first label wins, a later one only if strictly greater (a NaN never wins over label 0)"""
    best = Q[0].copy()
    m = np.zeros(Q.shape[1], np.int64)
    for l in range(1, Q.shape[0]):
        gt = Q[l] > best
        best = np.where(gt, Q[l], best)
        m = np.where(gt, l, m)
    return m


def top_two_margin(Q):
    s = np.sort(Q, axis=0)
    return float((s[-1] - s[-2]).min()) if Q.shape[0] > 1 else float("inf")


def connected_labels(lab):
    """ConnectedLabels.hpp:50-160, literally: 4-connected two-pass labelling; components numbered by the order of
    their first cell in raster order.  lab [H][W] u8 -> comp [H][W] int, stats list of dicts"""
    H, W = lab.shape
    comp = np.zeros((H, W), np.int64)
    roots = []

    def new():
        roots.append(len(roots))
        return len(roots) - 1

    def find(i):
        while roots[i] != i:
            i = roots[i]
        return i

    def merge(a, b):
        r1, r2 = find(a), find(b)
        if r1 < r2:
            roots[r2] = r1
            return r1
        roots[r1] = r2
        return r2

    comp[0, 0] = new()
    for c in range(1, W):
        comp[0, c] = comp[0, c - 1] if lab[0, c] == lab[0, c - 1] else new()
    for r in range(1, H):
        comp[r, 0] = comp[r - 1, 0] if lab[r, 0] == lab[r - 1, 0] else new()
        for c in range(1, W):
            if lab[r, c] == lab[r, c - 1]:
                left, top = comp[r, c - 1], comp[r - 1, c]
                if lab[r, c] == lab[r - 1, c] and left != top:
                    comp[r, c] = merge(top, left)
                else:
                    comp[r, c] = left
            elif lab[r, c] == lab[r - 1, c]:
                comp[r, c] = comp[r - 1, c]
            else:
                comp[r, c] = new()
    mapping = [0] * len(roots)
    cnt = 0
    for i in range(len(roots)):
        rt = find(i)
        if rt == i:
            mapping[rt] = cnt
            cnt += 1
        else:
            roots[i] = rt
    roots = [mapping[c] for c in roots]
    comp = np.array(roots, np.int64)[comp]
    stats = [dict(label=0, size=0, top=2**31 - 1, right=0, bottom=0, left=2**31 - 1) for _ in range(cnt)]
    for y in range(H):
        for x in range(W):
            s = stats[comp[y, x]]
            s["size"] += 1
            s["label"] = int(lab[y, x])
            s["top"], s["bottom"] = min(s["top"], y), max(s["bottom"], y)
            s["left"], s["right"] = min(s["left"], x), max(s["right"], x)
    return comp, stats


def map_to_high(v, S):
    """Slic::mapToHigh (Slic.h:193-195) stored in an unsigned short (ModelData::top ...)"""
    return int(v * S + S * 0.5) & 0xFFFF


def postprocess(raw_ids, spx, spy, W, H, S, ids, next_id, allow_new, low_depth, avg_conf, cfg):
    """Stages 8-13 (:515-679) on the argmax map of model ids.  ids = the existing models' ids in list order.
    Returns (map [N] u8 after relabelling, model_data list of dicts, has_new_label)."""
    N = spx * spy
    lab = np.asarray(raw_ids, np.uint8).reshape(spy, spx)
    comp, stats = connected_labels(lab)
    comp = comp.ravel()
    l2c = {}
    for i, s in enumerate(stats):
        l2c.setdefault(s["label"], []).append(i)
    keys = sorted(l2c)
    for key in keys[1:]:  # keep the largest component of every label but the smallest key (:530-553)
        lst = l2c[key]
        best = lst[0]
        for c in lst[1:]:
            if stats[best]["size"] < stats[c]["size"]:
                stats[best]["label"] = 255
                best = c
            else:
                stats[c]["label"] = 255
        l2c[key] = [best]
    model_ids = [int(i) for i in ids] + ([int(next_id)] if allow_new else [])
    if allow_new:  # :555-563
        mn, mx = int(F32(N) * F32(cfg["min_rel_size_new"])), int(F32(N) * F32(cfg["max_rel_size_new"]))
        for c in l2c.get(int(next_id), []):
            if stats[c]["size"] < mn or stats[c]["size"] > mx:
                stats[c]["label"] = 255
    boxes = []
    for mid in model_ids:  # :565-584
        top, right, bottom, left = 0xFFFF, 0, 0, 0xFFFF
        for c in l2c.get(mid, []):
            s = stats[c]
            top = s["top"] if s["top"] < top else top
            left = s["left"] if s["left"] < left else left
            right = s["right"] if s["right"] > right else right
            bottom = s["bottom"] if s["bottom"] > bottom else bottom
        boxes.append((map_to_high(top, S), map_to_high(right, S), map_to_high(bottom, S), map_to_high(left, S)))
    for mid, (top, right, bottom, left) in zip(model_ids, boxes):  # :586-600
        if mid == 0:
            continue
        hb, wb = (H - BORDER) & 0xFFFFFFFF, (W - BORDER) & 0xFFFFFFFF
        if (top < BORDER and bottom < BORDER) or (left < BORDER and right < BORDER) or \
                (top > hb and bottom > hb) or (left > wb and right > wb):
            for c in l2c.get(mid, []):
                stats[c]["label"] = 255
    out = np.array([stats[c]["label"] for c in comp], np.uint8)  # :602
    # depth statistics (:604-656): float sums in cell order
    d = np.asarray(low_depth, F32).ravel()
    index = {mid: i for i, mid in enumerate(model_ids)}
    L = len(model_ids)
    sel = [np.flatnonzero((out != 255) & (out == mid)) for mid in model_ids]
    for k in range(N):
        assert out[k] == 255 or int(out[k]) in index, ("label without model data", int(out[k]))
    sums = [seq_sum(d[s]) for s in sel]
    cnts = [len(s) for s in sel]
    mean = [F32(sums[i] / F32(cnts[i])) if cnts[i] else F32(0) for i in range(L)]
    devs = [seq_sum(np.abs(mean[i] - d[sel[i]]).astype(F32)) for i in range(L)]
    std = [F32(devs[i] / F32(cnts[i])) if cnts[i] else F32(0) for i in range(L)]
    count = list(cnts)
    for i in range(1, L):
        s, dv, c = sums[i], devs[i], cnts[i]
        lim = 1.1 * np.float64(std[i]) + np.float64(mean[i])
        for k in sel[i]:
            if np.float64(d[k]) > lim:
                s = F32(s - d[k])
                dv = F32(dv - F32(abs(mean[i] - d[k])))
                c -= 1
        sums[i], devs[i], cnts[i] = s, dv, c
    data = []
    for i, mid in enumerate(model_ids):
        data.append(dict(id=mid, super_pixel_count=count[i],
                         avg_confidence=F32(avg_conf[i]) if i < len(ids) else F32(0),
                         depth_mean=F32(sums[i] / F32(cnts[i])) if cnts[i] else F32(0),
                         depth_std=F32(devs[i] / F32(cnts[i])) if cnts[i] else F32(0), box=boxes[i]))
    has_new = False
    if allow_new:
        if data[-1]["super_pixel_count"] > 0:
            has_new = True
        else:
            data.pop()
    return out, data, has_new


def segment(low_depth, low_icp, low_conf, rgb_first, W, H, S, ids, next_id, allow_new, cfg, A=None):
    """Stages 2-13 from the stage-1 maps (low_icp, low_conf [M][N], lowDepth [N]).  Returns a dict."""
    spx, spy = W // S, H // S
    err = np.array(low_icp, F32).reshape(len(ids), -1).copy()
    conf = np.array(low_conf, F32).reshape(len(ids), -1).copy()
    low_depth = np.asarray(low_depth, F32).ravel()
    rng = depth_range(low_depth)
    avg = avg_confidence(conf)
    U = unaries(err, conf, rng, cfg, allow_new)
    bad = range_invalid(rng)
    fs, fa = features(spx, spy, rgb_first, low_depth, cfg)
    if bad:
        Q = np.zeros(U.shape)
        m = np.zeros(U.shape[1], np.int64)
    else:
        Q = mean_field(U, fs, fa, cfg, A)
        m = argmax_labels(Q)
    label_ids = np.array(list(ids) + ([next_id] if allow_new else []), np.uint8)
    raw = label_ids[m]
    out, data, has_new = postprocess(raw, spx, spy, W, H, S, ids, next_id, allow_new, low_depth, avg, cfg)
    return dict(range=rng, range_invalid=bad, avg_conf=avg, unaries=U, q=Q, raw_map=raw, map=out, model_data=data,
                has_new_label=has_new, features=(fs, fa))


def stage1(orc, labels, S, depth, icp_maps, conf_maps):
    """Stage 1 with the oracle's Slic::downsample: lowDepth, and per model {icp, conf} as mmf_shard_gather_maps lays
    them out ([M][2][N])"""
    low_depth = orc.slic_downsample(labels, S, depth, threshold=0.02).ravel()
    maps = np.stack([np.stack([orc.slic_downsample(labels, S, i).ravel(),
                               orc.slic_downsample(labels, S, c, channel=3).ravel()]) for i, c in zip(icp_maps, conf_maps)])
    return low_depth, maps.astype(F32)
