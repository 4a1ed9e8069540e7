"""The id images tests/test_gpu_flowseg.py runs the blob engine on.  A case is (ids uint8 [h,w], table ids, allow_new, new_id);
`depth(h, w)` is the matching depth image: k / 1024 with k < 8192, so that every float64 sum over it is exact whatever its
order and the oracle's mean and std are the one right answer."""
import numpy as np

SIZES = ((8, 6), (20, 20), (33, 25))  # cells: w, h (frames 32 x 24, 80 x 80, 132 x 100)
LARGE = (320, 240)                    # (1280 x 960)


def depth(h, w, seed=0):
    return (np.random.default_rng(seed).integers(0, 8192, (4 * h, 4 * w)) / 1024.0).astype(np.float32)


def table_of(L, seed):
    """L distinct ids with 0 first; 255 among them from three labels on"""
    rng = np.random.default_rng(1000 + seed)
    rest = rng.choice(np.arange(1, 255), size=L - 1, replace=False).tolist()
    if L >= 3:
        rest[-1] = 255
    return [0] + rest


def random_case(w, h, L, density, coarse, seed):
    """every cell one of the table's ids: the first with probability 1 - density; `coarse`: in blocks of that many cells"""
    rng = np.random.default_rng(seed)
    table = table_of(L, seed)
    hh, ww = -(-h // coarse), -(-w // coarse)
    pick = np.where(rng.random((hh, ww)) < density, rng.integers(1, L, (hh, ww)) if L > 1 else 0, 0)
    ids = np.asarray(table, np.uint8)[pick]
    ids = np.repeat(np.repeat(ids, coarse, axis=0), coarse, axis=1)[:h, :w]
    allow_new = L >= 2
    return np.ascontiguousarray(ids), table[:-1] if allow_new else table, allow_new, table[-1]


def checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, 3, 8).astype(np.uint8), [3, 8], False, 0


def nested_rings(w, h, outer_high):
    y, x = np.mgrid[0:h, 0:w]
    ring = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y))
    a, b = (9, 4) if outer_high else (4, 9)
    return np.where(ring % 2 == 0, a, b).astype(np.uint8), [4, 9], False, 0


def diagonal_ring(w, h):
    """a ring whose inside meets the outside only across diagonal gaps, with another id inside and around it"""
    ids = np.full((h, w), 1, np.uint8)
    for yy, row in enumerate((".##.", "#..#", "#.#.", ".#..")):
        for xx, c in enumerate(row):
            if c == "#":
                ids[1 + yy, 2 + xx] = 6
    return ids, [1, 6], False, 0


def edge_blob(w, h):
    """a frame along all four image edges with a bar across: its holes hold another id, which disappears"""
    ids = np.full((h, w), 2, np.uint8)
    ids[0, :] = ids[-1, :] = ids[:, 0] = ids[:, -1] = 5
    ids[:, w // 2] = 5
    return ids, [2, 5], False, 0


def singles(w, h):
    """only single-cell components of id 7: all areas 0, the last in raster order wins"""
    ids = np.zeros((h, w), np.uint8)
    ids[1::2, 1::2] = 7
    return ids, [0, 7], False, 0


def tie(w, h):
    ids = np.zeros((h, w), np.uint8)
    ids[0:2, 0:2] = 1
    ids[3:5, 4:6] = 1
    ids[3:5, 0:2] = 1  # three of area 1; the one that starts last in raster order is (3, 4)'s
    return ids, [0, 1], False, 0


def table_edges(w, h):
    """an id of the table without a cell (77), an id of the image that is not in the table (13), ids 0 and 255"""
    ids = np.zeros((h, w), np.uint8)
    ids[1:4, 1:5] = 255
    ids[2, 2] = 13       # a hole of 255 holding a foreign id: filled
    ids[4:6, 5:8] = 13   # a foreign blob: never drawn
    ids[0, w - 1] = 255
    return ids, [255, 77, 0], True, 200


def serpentine(w, h):
    """a one-cell-wide line of id 1 through the whole image, on id 0: the longest border, the deepest union chains"""
    ids = np.zeros((h, w), np.uint8)
    ids[0::2, :] = 1
    ids[1::4, w - 1] = 1
    ids[3::4, 0] = 1
    return ids, [0, 1], True, 2


def empty(w, h):
    return np.zeros((h, w), np.uint8), [0, 1], True, 2


def new_label(cells):
    """20 x 20 cells with `cells` of them the new label's (a 4 x 5 block and one more): 20 / 400 is not > 0.05, 21 / 400 is"""
    ids = np.zeros((20, 20), np.uint8)
    ids[0:4, 0:5] = 9
    if cells == 21:
        ids[4, 0] = 9
    assert int((ids == 9).sum()) == cells
    return ids, [0], True, 9


STRUCTURED = {
    "checkerboard": checkerboard, "rings_outer_high": lambda w, h: nested_rings(w, h, True),
    "rings_outer_low": lambda w, h: nested_rings(w, h, False), "diagonal_ring": diagonal_ring, "edge_blob": edge_blob,
    "singles": singles, "tie": tie, "table_edges": table_edges, "serpentine": serpentine, "empty": empty,
}
RANDOM = [(L, density, coarse) for L in (2, 5, 32) for density, coarse in ((0.15, 1), (0.5, 1), (0.9, 1), (0.5, 3))]
