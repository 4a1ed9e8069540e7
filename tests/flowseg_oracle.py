"""The blob stage of the flow_crf segmentation (Core/Segmentation/Segmentation.cpp:1270-1324), restated
literally in plain Python and numpy: cv::findContours' border following (icvFetchContour, outer borders), cv::contourArea's
shoelace, the polygon fill of cv::drawContours(FILLED), rint, the ascending-id overwrite, the nearest resize, a float64
meanStdDev and the 5 % rule.  This is the judge of the device engine (csrc/flowseg_kernels.hpp); `closed_form` is the
independent rule the issue of this stage states, held against the literal version by tests/test_flowseg_oracle.py.

What is pinned here is this restatement.  OpenCV itself is not: that its contour list holds later-found contours first
(so that a tie goes to the component found last) and that FILLED covers exactly the cells the border polygon winds around
are assumptions."""
from collections import deque

import numpy as np

# cv::findContours' eight directions: E, NE, N, NW, W, SW, S, SE (y grows downwards)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)


def components(mask):
    """8-connected components of a boolean image in the order a raster scan meets them: a list of (first_index, cells)
    with cells a list of (y, x)"""
    h, w = mask.shape
    seen = np.zeros((h, w), bool)
    out = []
    for y, x in zip(*(a.tolist() for a in np.nonzero(mask))):  # raster order
        if seen[y, x]:
            continue
        cells, q = [], deque([(y, x)])
        seen[y, x] = True
        while q:
            cy, cx = q.popleft()
            cells.append((cy, cx))
            for s in range(8):
                ny, nx = cy + DY[s], cx + DX[s]
                if 0 <= ny < h and 0 <= nx < w and mask[ny, nx] and not seen[ny, nx]:
                    seen[ny, nx] = True
                    q.append((ny, nx))
        out.append((y * w + x, cells))
    return out


def follow_border(img, x0, y0):
    """icvFetchContour for an outer border that starts at (x0, y0), whose west neighbour is 0: the points (x, y) in the
    order OpenCV stores them (CHAIN_APPROX_NONE).  `img` is a boolean image; outside it everything is 0."""
    h, w = img.shape

    def at(x, y):
        return 0 <= x < w and 0 <= y < h and bool(img[y, x])

    s_end = s = 4
    while True:
        s = (s - 1) & 7
        if at(x0 + DX[s], y0 + DY[s]) or s == s_end:
            break
    if s == s_end:
        return [(x0, y0)]
    x1, y1 = x0 + DX[s], y0 + DY[s]
    x3, y3 = x0, y0
    pts = []
    while True:
        while True:
            s += 1
            x4, y4 = x3 + DX[s & 7], y3 + DY[s & 7]
            if at(x4, y4):
                break
        s &= 7
        pts.append((x3, y3))
        if (x4, y4) == (x0, y0) and (x3, y3) == (x1, y1):
            break
        x3, y3 = x4, y4
        s = (s + 4) & 7
    return pts


def contour_area2(pts):
    """2 cv::contourArea: |sum prev.x cur.y - prev.y cur.x| with prev starting at the last point"""
    a, (px, py) = 0, pts[-1]
    for x, y in pts:
        a += px * y - py * x
        px, py = x, y
    return abs(a)


def fill_polygon(pts, h, w):
    """the cells a FILLED drawing of the closed polygon through `pts` covers: its points, and every cell centre the even-odd
    rule puts inside (the crossing test of a ray to the right: an edge counts for the rows ymin <= y < ymax)"""
    out = np.zeros((h, w), bool)
    tog = np.zeros((h, w + 1), np.int64)
    n = len(pts)
    for k in range(n):
        (xa, ya), (xb, yb) = pts[k], pts[(k + 1) % n]
        out[ya, xa] = True
        if ya != yb:  # unit steps: the edge crosses the one row min(ya, yb), at the x of its end there
            if ya < yb:
                tog[ya, xa] += 1
            else:
                tog[yb, xb] += 1
    # crossings strictly right of the cell
    right = np.cumsum(tog[:, ::-1], axis=1)[:, ::-1][:, 1:]
    out |= (right[:, :w] & 1).astype(bool)
    return out


def closed_form(cells, h, w):
    """the rule without a border: F = the component plus every cell that cannot reach the outside of the image by
    4-connected steps through cells that are not the component's; area2 = over all 2 x 2 blocks of cells, 2 where four are in
    F and 1 where three are.  Returns (area2, F)."""
    comp = np.zeros((h + 2, w + 2), bool)
    for y, x in cells:
        comp[y + 1, x + 1] = True
    out = np.zeros_like(comp)
    q = deque([(0, 0)])
    out[0, 0] = True
    while q:
        y, x = q.popleft()
        for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            ny, nx = y + dy, x + dx
            if 0 <= ny < h + 2 and 0 <= nx < w + 2 and not comp[ny, nx] and not out[ny, nx]:
                out[ny, nx] = True
                q.append((ny, nx))
    F = ~out
    n = F[:-1, :-1].astype(int) + F[:-1, 1:] + F[1:, :-1] + F[1:, 1:]
    return int(2 * (n == 4).sum() + (n == 3).sum()), F[1:-1, 1:-1]


def rint_half(area2):
    """rint(area2 / 2), half to even"""
    return int(np.rint(area2 / 2.0))


def segment(ids, depth, table_ids, allow_new=False, new_id=0, new_model_size=0.05, avg_confidence=0.4):
    """ids [h,w] uint8, depth [4h,4w] float32, table_ids = the models' ids in list order.  Returns a dict: the stage images
    component / area2 int32 [h,w], winner / segm uint8 [h,w], full uint8 [4h,4w]; per table entry (the new label last)
    area2 and first_cell; models = [(id, super_pixel_count, avg_confidence, depth_mean, depth_std)] after the new label's
    entry has been dropped; has_new_label, new_cells, n_entries."""
    ids = np.asarray(ids, np.uint8)
    h, w = ids.shape
    table = [int(i) for i in table_ids] + ([int(new_id)] if allow_new else [])
    assert len(set(table)) == len(table)
    component = np.full((h, w), -1, np.int32)
    area2_img = np.zeros((h, w), np.int32)
    winner = np.zeros((h, w), np.uint8)
    segm = np.zeros((h, w), np.uint8)
    segm_count, win_area2, win_first = {}, {}, {}
    for m in sorted(table):  # idx_map is a std::map: ascending ids
        mask = ids == m
        contours = []
        for first, cells in components(mask):
            for y, x in cells:
                component[y, x] = first
            # (in `mask` as the reference does: a set cell next to a cell of the component is the component's)
            pts = follow_border(mask, first % w, first // w)
            a2 = contour_area2(pts)
            for y, x in cells:
                area2_img[y, x] = a2
            contours.append((first, cells, pts, a2))
        contours.reverse()  # OpenCV's list: later-found contours first
        max_a, max_i = 0, 0
        for j, c in enumerate(contours):
            if c[3] > max_a:  # (:1280: strict)
                max_a, max_i = c[3], j
        segm_count[m], win_area2[m], win_first[m] = rint_half(max_a), 0, -1
        if contours:
            first, cells, pts, a2 = contours[max_i]
            win_area2[m], win_first[m] = a2, first
            for y, x in cells:
                winner[y, x] = 1
            segm[fill_polygon(pts, h, w)] = m  # ascending ids: the highest id that covers a cell stays
    full = np.repeat(np.repeat(segm, 4, axis=0), 4, axis=1)
    depth = np.asarray(depth, np.float32)
    assert depth.shape == full.shape
    models = []
    for m in table:
        sel = full == m
        n = int(sel.sum())
        mean = std = np.float32(0)
        if n:
            d = depth[sel].astype(np.float64)
            mu = d.sum() / n
            var = (d * d).sum() / n - mu * mu
            mean, std = np.float32(mu), np.float32(np.sqrt(max(var, 0.0)))
        spc = int(np.uint32(np.float32(segm_count[m]) * np.float32(16.0)))
        models.append((m, spc, np.float32(avg_confidence), mean, std))
    has_new, new_cells = False, 0
    if allow_new:
        new_cells = int((segm == new_id).sum())
        has_new = bool(np.float32(new_cells) / np.float32(w * h) > np.float32(new_model_size))
        if not has_new:
            models.pop()
    return dict(component=component, area2=area2_img, winner=winner, segm=segm, full=full,
                entry_area2=[win_area2[m] for m in table], entry_first=[win_first[m] for m in table], models=models,
                has_new_label=has_new, new_cells=new_cells, n_entries=len(models))
