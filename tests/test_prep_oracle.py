"""CPU: the crafted inputs of the batched-preparation tests (tests/prep_oracle.py) exercise what they claim, and the numpy
restatements in it (source choice, extents, the decoder of the extent words) say what csrc/extent.hpp and
csrc/prep_batch.hpp document.  No device."""
import numpy as np
import pytest

import prep_oracle as po
from multimotionfusion_amd import synth

SIZES = [(32, 32), (68, 36), (100, 52), (132, 44), (260, 36)]


def model_of(orc, w, h, pred):
    pred = dict(pred)
    pred.setdefault("pose", po.general_pose())
    return po.prepare_model(orc, synth.intrinsics(w, h), pred)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("channels", [3, 4])
def test_crafted_scene_has_valid_and_invalid_pixels_at_every_level(orc, w, h, channels):
    K = synth.intrinsics(w, h)
    pred = po.crafted_prediction(w, h, channels=channels)
    m = model_of(orc, w, h, pred)
    s = po.crafted_sensor(w, h, channels=channels)
    sb = po.prepare_sensor(orc, K, s["depth"], s["cutoff"], s["rgb"])
    for lvl in range(3):
        rows = h >> lvl
        for name, a in (("last_depth", m["last_depth"][lvl]), ("vertex", m["prev_packed"][lvl][..., 0]), ("normal", m["prev_packed"][lvl][..., 3]),
                        ("vmaps_curr", sb["vmaps_curr"][lvl][:rows]), ("nmaps_curr", sb["nmaps_curr"][lvl][:rows])):
            bad = np.isnan(a)
            assert bad.any() and not bad.all(), (name, lvl)
        for name, a in (("last_image", m["last_image"][lvl]), ("next_image", sb["next_image"][lvl])):
            assert (a == 0).any() and (a != 0).any(), (name, lvl)  # an all-zero 5 x 5 window gives a zero one level up
        assert np.isfinite(m["prev_packed"][lvl][~np.isnan(m["prev_packed"][lvl][..., 3])][:, 3:]).all()  # no normal of zero length
    # what the crafted texels are there for
    v, d0 = pred["vertex"], m["last_depth"][0]
    assert (v[..., 2] == 0).any() and (v[v[..., 2] == 0][:, :2] != 0).all()  # empty, x and y not
    beyond = v[..., 2] > po.MAX_DEPTH_RGB
    assert beyond.sum() > 4 and np.isnan(d0[beyond]).all() and not np.isnan(m["prev_packed"][0][..., 0][beyond]).any()
    assert not np.isnan(d0[v[..., 2] == np.float32(po.MAX_DEPTH_RGB)]).any()  # the cut-off itself is kept
    assert np.isnan(d0[v[..., 2] < 0]).all() and (v[..., 2] < 0).any()
    # 2 x 2 blocks with exactly one empty texel exist, and their vertex one level up is invalid
    empty = (v[..., 2] == 0).reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3))
    assert (empty == 1).sum() >= 3 and np.isnan(m["prev_packed"][1][..., 0][empty == 1]).all()
    assert not np.isnan(m["prev_packed"][1][..., 0][empty == 0]).any()
    # the sensor depth: the cut-off and its upper neighbour are invalid, its lower neighbour is not
    c = np.float32(s["cutoff"])
    vx = sb["vmaps_curr"][0][:h]
    for value, ok in ((c, False), (np.nextafter(c, np.float32(100)), False), (np.nextafter(c, np.float32(0)), True), (np.float32(0), False)):
        at = s["depth"] == value
        assert at.any() and (np.isnan(vx[at]) != ok).all(), value
    assert np.isnan(vx[np.isnan(s["depth"])]).all() and np.isnan(s["depth"]).any()


@pytest.mark.parametrize("w,h", SIZES)
def test_last_column_scene_needs_the_two_extra_extent_boxes(orc, w, h):
    """A depth that is a number makes its parent a number EXCEPT in the last column and row, which the parent's window
    [max(0, 2x - 2), min(2x + 3, cols - 1)) leaves out: the scene with texels in the last column only has a valid level-0
    depth and no valid level-1 depth at all."""
    col = po.sparse_prediction(w, h, [(w - 1, y, 1.0 + 0.01 * y) for y in range(h - 1)])
    m = model_of(orc, w, h, col)
    assert not np.isnan(m["last_depth"][0][:h - 1, w - 1]).any()
    assert np.isnan(m["last_depth"][1]).all() and np.isnan(m["last_depth"][2]).all()
    e = po.expected_extents(m, col)
    assert e["depth0"] == (w - 1, 0, w - 1, h - 2) and e["depth1"] is None and e["depth2"] is None
    row = po.sparse_prediction(w, h, [(x, h - 1, 2.0) for x in range(3, w - 1)])
    m = model_of(orc, w, h, row)
    e = po.expected_extents(m, row)
    assert e["depth0"] == (3, h - 1, w - 2, h - 1) and e["depth1"] is None and e["depth2"] is None
    # one row higher the parents are numbers, and the level-1 box of the last row appears
    row2 = po.sparse_prediction(w, h, [(x, h - 2, 2.0) for x in range(w)])
    e = po.expected_extents(model_of(orc, w, h, row2), row2)
    assert e["depth0"] == (w - 1, h - 2, w - 1, h - 2) and e["depth1"] == (0, h // 2 - 2, w // 2 - 1, h // 2 - 1) and e["depth2"] is not None


@pytest.mark.parametrize("w,h", SIZES)
def test_vertex_box_is_larger_than_the_depth_box_beyond_max_depth_rgb(orc, w, h):
    texels = [(w // 2 + dx, h // 2 + dy, 2.0) for dx in range(6) for dy in range(6)] + [(2, 1, 7.5), (w - 3, h - 2, 6.25)]
    pred = po.sparse_prediction(w, h, texels)
    m = model_of(orc, w, h, pred)
    e = po.expected_extents(m, pred)
    lo, hi = e["vertex"]
    depth_box = po.box_of(~np.isnan(m["last_depth"][0]))
    assert depth_box == (w // 2, h // 2, w // 2 + 5, h // 2 + 5)
    assert (lo[0], lo[1], hi[0], hi[1]) == (2, 1, w - 3, h - 2) and lo[2] == 2.0 and hi[2] == 7.5
    assert lo[0] < depth_box[0] and lo[1] < depth_box[1] and hi[0] > depth_box[2] and hi[1] > depth_box[3]


def test_source_choice_boundary_sits_exactly_on_the_ratio():
    assert [po.takes_alt(c, 12, 0.75) for c in (0, 8, 9, 12)] == [True, True, False, False]  # 9 / 12 == 0.75 exactly: not below
    assert np.float32(9) / np.float32(12) == np.float32(0.75)
    assert [po.takes_alt(s) for s in (0, 1, 7, None)] == [False, True, True, False]
    p = po.crafted_prediction(32, 32)
    p.update(po.alt_of(p))
    for name in ("vertex", "normal", "image"):
        differs = (p[name][..., :3] != p["alt_" + name][..., :3]).any(-1)
        assert differs.all(), name  # a job that read the wrong source is wrong at every pixel
    assert ((p["vertex"][..., 2] == 0) != (p["alt_vertex"][..., 2] == 0)).mean() > 0.5
    p.update(sel=8, sel_total=12, sel_ratio=0.75)
    assert po.chosen(p)[0] is p["alt_vertex"]
    p.update(sel=9)
    assert po.chosen(p)[0] is p["vertex"]


@pytest.mark.parametrize("w,h", [(100, 52), (132, 44)])
def test_box_sequence_empties_regions_and_stays_inside_its_boxes(w, h):
    seq = po.box_sequence(w, h)
    assert ((1, 1, 0, 0), None) in seq and ((w - 1, h - 1, w - 1, h - 1), None) in seq and ((0, 0, w - 1, h - 1), None) in seq
    assert any(b[0] == 64 for b, _ in seq) and any(b[2] == 63 for b, _ in seq) and any(b[1] % 16 == 0 and b[1] for b, _ in seq)
    assert any(b[0] % 2 == 1 and b[1] % 2 == 1 for b, _ in seq if b[2] >= b[0])
    before = None
    part = emptied = 0
    for box, fill in seq:
        p = po.crafted_prediction(w, h, box=box, fill=fill)
        nz = (p["vertex"] != 0).any(-1) | (p["normal"] != 0).any(-1) | (p["image"] != 0).any(-1)
        got = po.box_of(nz)
        x0, y0, x1, y1 = box
        if x1 < x0:
            assert got is None
        else:
            assert got is not None and got[0] >= x0 and got[1] >= y0 and got[2] <= x1 and got[3] <= y1
            if fill is None:
                assert got == box  # non-zero right up to the box's edges
            else:
                assert got == fill and got != box
                part += 1
        if before is not None and before.any():
            assert (before & ~nz).any() or fill is None and box == (0, 0, w - 1, h - 1)  # something that was there is gone
            emptied += int((before & ~nz).any())
        before = nz
    assert part == 1 and emptied >= 5
    (a, _), (b, _) = seq[0], seq[1]
    assert b[0] > a[2] and b[1] > a[3]  # disjoint


def test_extent_words_decode_and_ignore_other_generations():
    def key(f):
        b = int(np.array([f], np.float32).view(np.uint32)[0])
        return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)
    g = 7
    words = np.zeros(po.EXTENT_WORDS, np.uint64)
    box = (5, 3, 99, 51)
    for lvl in (0, 2):
        words[4 * lvl:4 * lvl + 4] = [(g << 32) | (0xFFFF - box[0]), (g << 32) | box[2], (g << 32) | (0xFFFF - box[1]), (g << 32) | box[3]]
    words[4:8] = [((g - 1) << 32) | 1, ((g - 1) << 32) | 2, ((g - 1) << 32) | 3, ((g - 1) << 32) | 4]  # an older frame's
    lo, hi = (2.0, 1.0, -1.5), (97.0, 50.0, 60.0)
    for k in range(3):
        words[12 + k] = (g << 32) | (0xFFFFFFFF - key(lo[k]))
        words[15 + k] = (g << 32) | key(hi[k])
    words[18 + (4 & 1)] = (4 << 32) | (0xFFFFFFFF - key(0.351))
    e = po.decode_extents(words, g)
    assert e["depth0"] == box and e["depth2"] == box and e["depth1"] is None
    assert e["vertex"] == (tuple(np.float32(x) for x in lo), tuple(np.float32(x) for x in hi))
    other = po.decode_extents(words, g + 1)
    assert all(v is None for v in other.values()) and all(v is None for v in po.decode_extents(words, 0).values())
    assert po.decode_zmin(words, 4) == np.float32(0.351) and po.decode_zmin(words, 5) is None and po.decode_zmin(words, 6) is None
    assert po.generations(words)[:4] == [g] * 4 and po.generations(words)[4:8] == [g - 1] * 4


def test_expected_zmin_follows_create_vmap(orc):
    w, h = 68, 36
    s = po.crafted_sensor(w, h)
    vm = orc.create_vmap(s["depth"], *po.level_intr(synth.intrinsics(w, h), 0), s["cutoff"])
    ok = ~np.isnan(vm[:h])
    assert po.expected_zmin(s["depth"], s["cutoff"]) == vm[2 * h:][ok].min()
    assert po.expected_zmin(po.crafted_sensor(w, h, mode="none")["depth"], 3.0) is None
    e = po.crafted_sensor(w, h, mode="edge")
    vm = orc.create_vmap(e["depth"], *po.level_intr(synth.intrinsics(w, h), 0), e["cutoff"])
    edge = np.zeros((h, w), bool)
    edge[:, -1] = edge[-1, :] = True
    assert (~np.isnan(vm[:h]) == edge).all()
