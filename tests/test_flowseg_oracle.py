"""tests/flowseg_oracle.py against hand-computed blobs and against the closed form of the contour area and the fill (CPU).

The oracle is a literal restatement of cv::findContours' border following, cv::contourArea and a polygon fill; the closed
form needs no border at all (flood fill from outside the image, then a count over 2 x 2 blocks).  That the two agree on
seeded random images is what makes either believable without OpenCV at hand."""
import numpy as np
import pytest

import flowseg_cases as fc
import flowseg_oracle as fo


def blob(rows):
    return np.array([[c == "#" for c in r] for r in rows], bool)


def only(mask):
    comps = fo.components(mask)
    assert len(comps) == 1
    first, cells = comps[0]
    h, w = mask.shape
    pts = fo.follow_border(mask, first % w, first // w)
    return first, cells, pts, fo.contour_area2(pts), fo.fill_polygon(pts, h, w)


KNOWN = {
    # name: (rows, area2, cells that the fill adds to the component)
    "single": ([".....", "..#..", "....."], 0, []),
    "block2x2": (["....", ".##.", ".##.", "...."], 2, []),
    "L3": (["....", ".#..", ".##.", "...."], 1, []),
    "plus5": ([".....", "..#..", ".###.", "..#..", "....."], 4, []),
    "diamond_ring": ([".....", "..#..", ".#.#.", "..#..", "....."], 4, [(2, 2)]),
    "ring3x3": ([".....", ".###.", ".#.#.", ".###.", "....."], 8, [(2, 2)]),
    "line": (["#####"], 0, []),
    "diagonal": (["#..", ".#.", "..#"], 0, []),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_hand_computed(name):
    rows, area2, extra = KNOWN[name]
    m = blob(rows)
    _, cells, pts, a2, fill = only(m)
    assert a2 == area2
    want = m.copy()
    for y, x in extra:
        want[y, x] = True
    assert np.array_equal(fill, want)
    ca2, F = fo.closed_form(cells, *m.shape)
    assert ca2 == area2 and np.array_equal(F, want)


def test_border_points_of_a_block():
    """the order OpenCV stores: from the first cell down the west side, counter-clockwise on the screen"""
    _, _, pts, _, _ = only(blob(["##", "##"]))
    assert pts == [(0, 0), (0, 1), (1, 1), (1, 0)]
    _, _, pts, _, _ = only(blob(["###"]))
    assert pts == [(0, 0), (1, 0), (2, 0), (1, 0)]  # out and back along the line


def test_rint_is_half_to_even():
    assert [fo.rint_half(a) for a in (0, 1, 2, 3, 4, 5, 7)] == [0, 0, 1, 2, 2, 2, 4]


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_equals_literal_on_random_images(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(3, 13)), int(rng.integers(3, 13))
    checked = 0
    for density in (0.3, 0.5, 0.65, 0.8):
        for _ in range(8):
            m = rng.random((h, w)) < density
            for first, cells in fo.components(m):
                pts = fo.follow_border(m, first % w, first // w)
                a2, F = fo.closed_form(cells, h, w)
                assert fo.contour_area2(pts) == a2
                assert np.array_equal(fo.fill_polygon(pts, h, w), F)
                checked += 1
    assert checked > 30


def test_hole_that_touches_the_outside_diagonally_is_a_hole():
    m = blob([".##.",
              "#..#",
              "#.#.",
              ".#.."])
    _, cells, _, a2, fill = only(m)
    # the two inner cells (1,1), (1,2) and (2,1) meet the outside only across the diagonal gaps of the ring
    assert fill[1, 1] and fill[1, 2] and fill[2, 1] and not fill[3, 3] and not fill[0, 0]
    ca2, F = fo.closed_form(cells, *m.shape)
    assert ca2 == a2 and np.array_equal(F, fill)


def depth_of(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 8192, (4 * h, 4 * w)) / 1024.0).astype(np.float32)


def test_ties_go_to_the_component_found_last():
    ids = np.zeros((6, 8), np.uint8)
    ids[0:2, 0:2] = 1
    ids[3:5, 4:6] = 1  # the same area, later in raster order
    r = fo.segment(ids, depth_of(6, 8, 0), [0, 1])
    assert r["entry_area2"] == [r["entry_area2"][0], 2] and r["entry_first"][1] == 3 * 8 + 4
    assert (r["segm"] == 1).sum() == 4 and r["segm"][3, 4] == 1 and r["segm"][0, 0] == 0
    single = np.zeros((6, 8), np.uint8)
    single[1, 1] = single[4, 6] = single[2, 5] = 1  # all areas 0: max_i stays 0, the head of OpenCV's list
    r = fo.segment(single, depth_of(6, 8, 0), [0, 1])
    assert r["entry_first"][1] == 4 * 8 + 6 and (r["segm"] == 1).sum() == 1 and r["segm"][4, 6] == 1
    assert r["models"][1][1] == 0


def test_highest_id_overwrites_and_enclosed_ids_disappear():
    ids = np.zeros((9, 9), np.uint8)
    ids[1:8, 1:8] = 3
    ids[2:7, 2:7] = 2
    ids[3:6, 3:6] = 3
    ids[4, 4] = 7
    r = fo.segment(ids, depth_of(9, 9, 1), [0, 2, 3, 7])
    want = np.zeros((9, 9), np.uint8)
    want[1:8, 1:8] = 3  # the outer ring of 3 is filled last but one; 2 lies inside it and is covered
    want[4, 4] = 7
    assert np.array_equal(r["segm"], want)
    assert r["entry_area2"][1] == 2 * 16 and r["entry_area2"][2] == 2 * 36 and r["models"][1][1] == 16 * 16
    assert np.array_equal(r["full"], np.kron(want, np.ones((4, 4), np.uint8)))


def test_model_data_and_the_new_label_rule():
    ids = np.zeros((20, 20), np.uint8)
    ids[0:4, 0:5] = 9  # 20 of 400 cells: 0.05 is not > 0.05
    d = depth_of(20, 20, 2)
    r = fo.segment(ids, d, [0], allow_new=True, new_id=9)
    assert r["new_cells"] == 20 and not r["has_new_label"] and r["n_entries"] == 1 and len(r["models"]) == 1
    ids[4, 0] = 9
    r = fo.segment(ids, d, [0], allow_new=True, new_id=9)
    assert r["new_cells"] == 21 and r["has_new_label"] and r["n_entries"] == 2
    mid, spc, conf, mean, std = r["models"][1]
    sel = np.kron(ids == 9, np.ones((4, 4), bool)).astype(bool)
    assert mid == 9 and conf == np.float32(0.4)
    assert spc == 16 * 12  # the border polygon of 4 x 5 cells and one more: area 3 x 4 = 12
    assert mean == np.float32(d[sel].astype(np.float64).mean()) and std == np.float32(d[sel].astype(np.float64).std())
    # an id without a cell, and an id of the image that is not in the table
    r = fo.segment(ids, d, [0, 5])
    assert r["models"][1] == (5, 0, np.float32(0.4), np.float32(0), np.float32(0)) and r["entry_first"][1] == -1
    assert not (r["segm"] == 9).any() and (r["component"][ids == 9] == -1).all()


def test_what_the_cases_exercise():
    """the properties the cases of tests/test_gpu_flowseg.py were built for, read off the oracle"""
    def case(kind, w, h):
        ids, table, allow_new, new_id = fc.STRUCTURED[kind](w, h)
        return None, None, None, None, None, fo.segment(ids, fc.depth(h, w), table, allow_new, new_id)

    r = case("checkerboard", 8, 6)[5]
    assert len(np.unique(r["component"])) == 2  # every id one diagonally connected component
    r = case("rings_outer_high", 20, 20)[5]
    assert (r["segm"] == 9).all()  # the outermost ring of the highest id covers everything
    r = case("rings_outer_low", 20, 20)[5]
    assert (r["segm"][1:-1, 1:-1] == 9).all() and (r["segm"][0] == 4).all()
    r = case("diagonal_ring", 8, 6)[5]
    assert r["segm"][2, 3] == 6 and r["segm"][2, 4] == 6 and r["segm"][3, 3] == 6  # the hole is filled
    r = case("edge_blob", 20, 20)[5]
    assert (r["segm"] == 5).all()
    r = case("singles", 8, 6)[5]
    assert r["entry_area2"][1] == 0 and r["entry_first"][1] == 5 * 8 + 7 and (r["segm"] == 7).sum() == 1
    r = case("tie", 8, 6)[5]
    assert r["entry_area2"][1] == 2 and r["entry_first"][1] == 3 * 8 + 4
    r = case("table_edges", 8, 6)[5]
    assert r["entry_first"][1] == -1 and r["segm"][2, 2] == 255 and not (r["segm"] == 13).any() and r["segm"][0, 7] == 0
    r = case("serpentine", 33, 25)[5]
    line = fc.serpentine(33, 25)[0] == 1
    assert (r["component"][line] == 0).all() and r["entry_area2"][1] == 24  # one component; its 24 turns are half a cell each
