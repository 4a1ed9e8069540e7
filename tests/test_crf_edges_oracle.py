"""CPU: the cases of test_gpu_crf_edges.py (tests/crf_edges.py) reach the edges they are named for -- asserted on the oracle
alone (tests/crf_oracle.py), with the scenes the device tests use.

Every case whose argmax map is compared has an oracle top-two margin >= 1e-3 (the rule of test_gpu_crf.py).  Every case that
runs the mean field is evaluated once in float32 numpy and must stay within 2.5e-5 of the float64 oracle, a quarter of the
device tolerance of 1e-4.  Every soft case moves at least one label, has an unsaturated Q after one iteration, and sees each
of three damaged oracles (cell N - 1 missing from both kernels, the last chunk of 128 cells missing, the appearance kernel
missing) by at least 1e-3, ten times the tolerance.

Measured: float32 evaluation 2.9e-6 at worst (I-41x25-L17; A-L32 2.3e-6), at most 6e-7 in groups B, F, G and H; smallest soft
margin 5.4e-3 (A-L32-new-soft); smallest damage 1.6e-3 (B-41x25-soft, one cell of 1025), 3.1e-3 in group A.

Two cases cannot move a label and are exempt from that one condition: N = 1 has a single depth, so its range is 0 and the
frame is all background, and at N = 2 each cell's own unary (a gap above 2) outweighs what one neighbour sends."""
import functools

import numpy as np
import pytest

import crf_edges as ce
import crf_oracle as co

F32 = np.float32
_orc = None


@functools.lru_cache(maxsize=None)
def ref(name):
    return ce.reference(_orc, name)


@pytest.fixture(autouse=True)
def _oracle(orc):
    global _orc
    _orc = orc


def iterations(c):
    return c["cfg"].get("iterations", co.DEFAULTS["iterations"])


def components(c, raw):
    spy, spx = c["owner"].shape
    return co.connected_labels(np.asarray(raw, np.uint8).reshape(spy, spx))


@pytest.mark.parametrize("name", list(ce.CASES))
def test_case_is_well_posed(name):
    """the margin of every compared map, the float32 headroom of every mean field, the soft conditions"""
    c = ce.CASES[name]
    r = ref(name)
    spy, spx = c["owner"].shape
    N = spx * spy
    assert (spx, spy) == (c["W"] // c["S"], c["H"] // c["S"]) and r["q"].shape == (c["M"] + int(c["allow_new"]), N)
    assert 10 < c["S"] < 256 and N <= 16384
    if r["range_invalid"]:
        assert not c["need_margin"] or N == 1, "a compared case must have a depth range"
        return
    if c["need_margin"]:
        assert co.top_two_margin(r["q"]) >= 1e-3, co.top_two_margin(r["q"])
    if iterations(c) == 0:
        return
    fs, fa = r["features"]
    _, cfg = ce.oracle_inputs(_orc, name)
    q32 = ce.mean_field_f32(r["unaries"], fs, fa, cfg)
    d32 = float(np.abs(q32.astype(np.float64) - r["q"]).max())
    assert d32 <= 2.5e-5, d32
    if not c["soft"]:
        return
    if N > 2:
        assert (ce.reference(_orc, name, iterations=0)["raw_map"] != r["raw_map"]).any(), "the mean field moves no label"
    q1 = ce.reference(_orc, name, iterations=1)["q"]
    assert ((q1 > 0.05) & (q1 < 0.95)).any()
    Ks, Ka = ce.gauss_kernels(fs, fa)
    whole = co.mean_field(r["unaries"], fs, fa, cfg, A=ce.assemble(Ks, Ka, cfg))
    assert np.abs(whole - r["q"]).max() <= 1e-12  # (assemble without damage is crf_oracle.pair_matrix)
    for damage in ce.DAMAGES:
        moved = float(np.abs(co.mean_field(r["unaries"], fs, fa, cfg, A=ce.assemble(Ks, Ka, cfg, damage)) - r["q"]).max())
        assert moved >= 1e-3, (damage, moved)


def test_float32_mean_field_is_the_oracles():
    """the float32 evaluation against the oracle's hand-checked two-cell case (test_crf_oracle.py)"""
    cfg = co.config(iterations=1, weight_smoothness=2.0, weight_appearance=3.0)
    fs = np.array([[0.0, 0.0], [0.5, 0.0]], F32)
    fa = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 1]], F32)
    U = np.array([[1.0, 2.0], [2.0, 1.0]], F32)
    np.testing.assert_allclose(ce.mean_field_f32(U, fs, fa, cfg), co.mean_field(U, fs, fa, cfg), rtol=0, atol=5e-7)
    assert list(ce.dropped_cells(1025, "chunk")) == [1024] and list(ce.dropped_cells(1024, "chunk")) == list(range(896, 1024))
    assert list(ce.dropped_cells(7, "cell")) == [6] and len(ce.dropped_cells(7, "appearance")) == 0


# ---- A ----------------------------------------------------------------------------------------------------------------------
def instantiation(L):
    return next(k for k in (1, 2, 4, 8, 16, 32) if L <= k)


def test_label_counts_sit_on_both_ends_of_every_instantiation():
    seen = {}
    for name in ce.names("A-"):
        c = ce.CASES[name]
        L = c["M"] + int(c["allow_new"])
        seen.setdefault(instantiation(L), set()).add(L)
        assert c["owner"].shape == (30, 40) and (c["W"], c["H"], c["S"]) == (640, 480, 16)
        for m in range(c["M"]):  # a 3 x 3 block of its own away from the border
            own = c["owner"] == m
            assert any(own[y:y + 3, x:x + 3].all() for y in range(1, 27) for x in range(1, 37)), (name, m)
        if c["allow_new"]:
            assert (c["owner"] == -1).sum() >= 16
    assert seen == {2: {2}, 4: {4}, 8: {5, 8}, 16: {9, 16}, 32: {17, 32}}
    assert len(ce.names("A-")) == 32 and max(ce.LABEL_COUNTS) == 32  # kCrfMaxLabels
    for soft in (False, True):
        assert sum(ce.CASES[n]["soft"] == soft for n in ce.names("A-")) == 16


# ---- B ----------------------------------------------------------------------------------------------------------------------
def test_cell_counts_sit_on_the_tiles():
    want = {1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 40}
    got, no_labels, sizes = set(), 0, set()
    for name in ce.names("B-"):
        c = ce.CASES[name]
        spy, spx = c["owner"].shape
        got.add(spx * spy)
        sizes.add(c["S"])
        assert c["W"] == spx * c["S"] + c["S"] - 1 and c["H"] == spy * c["S"] + c["S"] - 1  # the last cell's largest remainder
        assert c["M"] == 1 and c["allow_new"]
        no_labels += c["labels"] is None
        labels = ce.scene(name)[0]
        assert (labels is None) == (c["labels"] is None)
        g = ce.oracle_labels(c, labels)
        assert g.shape == (c["H"], c["W"]) and g.min() >= 0 and g.max() <= spx * spy - 1
    assert got == want and sizes == {11, 16, 255} and no_labels == len(ce.names("B-")) // 2
    shapes = {ce.CASES[n]["owner"].shape for n in ce.names("B-")}
    assert (40, 1) in shapes and (1, 40) in shapes  # one column, one row
    assert ref("B-1x1-default")["range_invalid"]  # one cell has one depth: B4


# ---- C ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ncomp", [("C-checkerboard", 16384), ("C-comb", 2)])
def test_cell_limit_cases(name, ncomp):
    c = ce.CASES[name]
    r = ref(name)
    assert c["owner"].size == 16384 and (c["W"], c["H"], c["S"]) == (1408, 1408, 11) and iterations(c) == 0
    assert np.array_equal(r["raw_map"], ce.intended_map(c))
    comp, stats = components(c, r["raw_map"])
    assert len(stats) == ncomp
    if ncomp == 2:  # each comb is one cell wide and reaches every second column
        assert sorted(s["size"] for s in stats) == [8192, 8192]
        assert all(s["right"] - s["left"] >= 126 and s["bottom"] - s["top"] >= 126 for s in stats)


# ---- D ----------------------------------------------------------------------------------------------------------------------
def test_id_cases_tell_positions_from_values():
    for name in ce.names("D-"):
        c = ce.CASES[name]
        r = ref(name)
        ids = c["ids"]
        assert ids != list(range(c["M"])) and c["next_id"] != c["M"]
        assert np.array_equal(r["raw_map"], ce.intended_map(c))
        data = {d["id"]: d for d in r["model_data"]}
        assert [d["id"] for d in r["model_data"]] == ids + [c["next_id"]] and r["has_new_label"]
        # trimming is visible: position 0 keeps its outliers, position 1 loses some
        low = ce.oracle_inputs(_orc, name)[0]
        for pos in (0, 1):
            d = data[ids[pos]]
            sel = low[r["map"] == ids[pos]]
            if len(sel) == 0:  # (D-ids-7-2-9: the border rule leaves position 0 without a cell)
                assert name == "D-ids-7-2-9" and pos == 0
                continue
            untrimmed = co.seq_sum(sel) / F32(len(sel))
            assert (d["depth_mean"] == untrimmed) == (pos == 0), (name, pos, d, untrimmed)
    r = ref("D-ids-0-200-3-254-64")
    assert r["model_data"][2]["id"] == 3 and r["model_data"][2]["super_pixel_count"] == 0 and (r["raw_map"] == 3).sum() == 6
    r = ref("D-ids-7-2-9")  # no id 0: position 0 (id 7) is removed by the border rule; the smallest key (2) keeps two components
    assert r["model_data"][0]["id"] == 7 and r["model_data"][0]["super_pixel_count"] == 0 and (r["raw_map"] == 7).any()
    assert r["model_data"][1]["super_pixel_count"] == 16 + 9 and min(c for c in (7, 2, 9, 5)) == 2
    r = ref("D-ids-0-253")
    assert (r["map"] == 255).sum() == 3 and r["model_data"][1]["super_pixel_count"] == 9
    r = ref("D-ids-5-0-1")  # id 0 at position 1 lies in row 0 and stays; it is the smallest key
    assert r["model_data"][1]["id"] == 0 and r["model_data"][1]["super_pixel_count"] == 7
    assert r["model_data"][2]["super_pixel_count"] == 16  # (id 1: the larger of its two components)


# ---- E ----------------------------------------------------------------------------------------------------------------------
def e_case(name):
    c = ce.CASES[name]
    r = ref(name)
    assert iterations(c) == 0 and c["owner"].shape == (30, 40) and c["labels"] == "grid"
    assert np.array_equal(r["raw_map"], ce.intended_map(c))
    comp, stats = components(c, r["raw_map"])
    return c, r, comp, stats, r["map"].reshape(30, 40)


def test_checkerboard_has_1200_components():
    c, r, comp, stats, out = e_case("E-checkerboard")
    assert len(stats) == 1200 and (out[c["owner"] == 0] == 0).all()
    ones = out[c["owner"] == 1]
    assert ones[0] == 1 and (ones[1:] == 255).all()


def test_serpentine_is_one_long_component():
    c, r, comp, stats, out = e_case("E-serpentine")
    assert len(stats) == 2 and sorted(s["size"] for s in stats) == [14 * 38 + 13, 1200 - 14 * 38 - 13]
    assert np.array_equal(out, r["raw_map"].reshape(30, 40))
    own = c["owner"]  # one cell wide: no 2 x 2 block of label 1
    assert not (own[:-1, :-1] & own[1:, :-1] & own[:-1, 1:] & own[1:, 1:]).any()


def test_u_shape_takes_the_number_of_its_first_cell():
    c, r, comp, stats, out = e_case("E-u-shape")
    assert len(stats) == 3 and comp[2, 5] == comp[2, 30] == comp[27, 17] == 1 and comp[2, 8] == 2
    assert stats[1]["size"] == stats[2]["size"] == 76
    assert (out[c["owner"] == 1][comp[c["owner"] == 1] == 1] == 1).all() and (out[2:6, 8:27] == 255).all()
    # the arms meet in the last row of the U only
    assert (c["owner"][2:27, 6:30] == 1).sum() == 76


def test_rings_are_nested_components():
    c, r, comp, stats, out = e_case("E-rings")
    assert len(stats) == 13 and [s["label"] for s in stats] == [0, 1] * 6 + [0]
    assert (out[2, 2:38] == 1).all() and (out[c["owner"] == 0] == 0).all()
    assert (out[c["owner"] == 1] == 255).sum() == sum(s["size"] for s in stats[3::2])


def test_ties_straddle_component_1024():
    c, r, comp, stats, out = e_case("E-ties")
    numbers = [int(comp[y, x]) for y, x in ce.TIE_CELLS]
    assert len(stats) > 1024 and numbers[:3] == [1, 2, 3] and numbers[3] > 1024 and numbers[4] > 1024, numbers
    assert all(stats[n]["size"] == 3 and stats[n]["label"] == 1 for n in numbers)
    assert max(s["size"] for s in stats if s["label"] == 1) == 3
    for n, (y, x) in enumerate(ce.TIE_CELLS):  # the earliest one wins
        assert (out[y, x:x + 3] == (1 if n == 0 else 255)).all()
    # more than 1024 components of one label too: model 2's checkerboard cells, all of one size
    assert sum(s["label"] == 2 for s in stats) > 500


BORDER_REMOVED = {"E-border-S11": {1, 2, 3, 4}, "E-border-S16": {1, 3, 4}, "E-border-S39": {1}, "E-border-S40": set(),
                  "E-border-S16-H495": {1, 4}}


@pytest.mark.parametrize("name", list(BORDER_REMOVED))
def test_border_rule_cases(name):
    """mapToHigh(v) = int(v S + S / 2): row 0 gives 5, 8, 19, 20 and row 1 gives 16, 24, 58, 60 at S = 11, 16, 39, 40 against the
    band of 20; the last row and column give exactly H - 20 and W - 20 at S = 39 and 40 (not above: kept)"""
    c, r, comp, stats, out = e_case(name)
    assert len(stats) == 6
    removed = {m for m in range(1, 6) if (out[c["owner"] == m] == 255).all()}
    assert removed == BORDER_REMOVED[name] and (out[c["owner"] == 5] == 5).all()
    assert all((out[c["owner"] == m] == m).all() for m in set(range(1, 6)) - removed)
    s5 = stats[int(comp[0, 0])]
    assert (s5["top"], s5["left"], s5["bottom"], s5["right"]) == (0, 0, 29, 39)  # touches all four borders
    assert co.map_to_high(0, 40) == 20 and co.map_to_high(1, 11) == 16 and co.map_to_high(0, 39) == 19
    if name == "E-border-S16-H495":
        assert c["H"] // 16 == 30 and co.map_to_high(29, 16) <= c["H"] - 20
    if name == "E-border-S39":
        assert co.map_to_high(29, 39) == c["H"] - 20 and co.map_to_high(39, 39) == c["W"] - 20


@pytest.mark.parametrize("cells,keep", [(5, False), (6, True), (480, True), (481, False)])
def test_new_label_size_cases(cells, keep):
    c, r, comp, stats, out = e_case(f"E-new-{cells}")
    cfg = co.config()
    mn, mx = int(F32(1200) * F32(cfg["min_rel_size_new"])), int(F32(1200) * F32(cfg["max_rel_size_new"]))
    assert (mn, mx) == (6, 480) and cells in (mn - 1, mn, mx, mx + 1)
    new = [s for s in stats if s["label"] == c["next_id"]]
    assert len(new) == 1 and new[0]["size"] == cells
    assert r["has_new_label"] == keep and (out[c["owner"] == -1] == (c["next_id"] if keep else 255)).all()


# ---- F ----------------------------------------------------------------------------------------------------------------------
def test_confidence_thresholds_fall_between_the_float_and_the_double():
    c = ce.CASES["F-conf"]
    labels, depth, rgb, maps = ce.scene("F-conf")
    r = ref("F-conf")
    c0, c2 = ce.conf_edge_cells(c)
    own = c["owner"].ravel()
    assert (own[c0] == 0).all() and (own[c2] == 2).all()
    rng, cfg = r["range"], co.config()
    U = r["unaries"]
    low0 = co.unaries(np.array([[F32(np.float64(rng) * 0.01)]], F32), np.ones((1, 1), F32), rng, cfg, False)[0, 0]
    lowk = co.unaries(np.array([[F32(rng * F32(cfg["unary_k_error"]))]], F32), np.ones((1, 1), F32), rng, cfg, False)[0, 0]
    # model 0: f32(0.3) > 0.3 keeps the error, one ulp below, -inf (-> 0) and -0.5 replace it; f32(0.4) is above 0.3
    assert [bool(U[0, k] == low0) for k in c0] == [False, True, False, False, True, True]
    # a later model: f32(0.4) > 0.4 keeps the error, one ulp below replaces it, and so does everything smaller
    for cells in (c0, c2):
        assert [bool(U[2, k] == lowk) for k in cells] == [True, True, False, True, True, True]
    assert np.float64(ce.F_CONF[0]) > 0.3 > np.float64(ce.F_CONF[1]) and np.float64(ce.F_CONF[2]) > 0.4 > np.float64(ce.F_CONF[3])
    assert np.array_equal(maps[0, 1, c0], np.array(ce.F_CONF, F32))


@pytest.mark.parametrize("name", ["F-err-default", "F-err-soft"])
def test_error_edges(name):
    r = ref(name)
    labels, depth, rgb, maps = ce.scene(name)
    U = r["unaries"]
    zero = maps[:, 0] == 0
    assert zero.sum() == 6 and (U[:3][zero] == F32(1e-5)).all()          # the clamp with an error of exactly 0
    assert np.isinf(maps[:, 0]).sum() == 6 and (np.isinf(U) == np.pad(np.isinf(maps[:, 0]), ((0, 1), (0, 0)))).all()
    assert (U[3] == F32(0.01)).sum() >= 12 and (U[3] > F32(0.01)).any()  # the new label's floor, reached and not
    assert np.isfinite(r["q"]).all() and (r["q"][np.isinf(U)] == 0).all()


def test_depth_edges():
    low, _ = ce.oracle_inputs(_orc, "F-depth-95")
    r = ref("F-depth-95")
    assert ((low > 94.9) & (low < 100)).sum() == 13 and 92.5 < r["range"] < 93.5
    assert (r["features"][1][:, 5] == 100.0).sum() == 13  # inside the range, the feature on its clamp
    low, _ = ce.oracle_inputs(_orc, "F-depth-150")
    r = ref("F-depth-150")
    assert (low > 100).sum() == 13 and 0.9 < r["range"] < 1.1 and (r["features"][1][:, 5] == 100.0).sum() == 13
    assert any(d["depth_mean"] > 3.0 or d["depth_std"] > 1.0 for d in r["model_data"])  # the statistics do see them
    low, _ = ce.oracle_inputs(_orc, "F-depth-equal")
    r = ref("F-depth-equal")
    assert (low == 2.0).all() and r["range"] == 0 and r["range_invalid"]  # B4 through range 0, with every depth valid
    low, _ = ce.oracle_inputs(_orc, "F-depth-one-valid")
    r = ref("F-depth-one-valid")
    assert (low <= 100).sum() == 1 and r["range"] == 0 and r["range_invalid"]


# ---- G, H, I ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G-tie-default", "G-tie-soft"])
def test_twin_models_tie_exactly(name):
    c = ce.CASES[name]
    maps = ce.scene(name)[3]
    r = ref(name)
    assert c["M"] == 3 and np.array_equal(maps[1], maps[2], equal_nan=True) and not c["need_margin"]
    assert np.array_equal(r["q"][1], r["q"][2]) and (r["raw_map"] == 1).any() and not (r["raw_map"] == 2).any()
    assert iterations(c) == 10


def test_iteration_cases_differ():
    maps = [ref(f"H-iterations-{it}")["q"] for it in ce.ITERATIONS]
    assert ce.ITERATIONS == (0, 1, 2) and all(ce.CASES[f"H-iterations-{it}"]["soft"] for it in ce.ITERATIONS)
    assert np.abs(maps[0] - maps[1]).max() > 0.1 and np.abs(maps[1] - maps[2]).max() > 0.01
    assert maps[0].shape == (3, 1200)


def test_reuse_sequence_shrinks_and_grows():
    dims = [(ce.CASES[n]["owner"].size, ce.CASES[n]["M"] + int(ce.CASES[n]["allow_new"])) for n in ce.REUSE_ORDER]
    assert dims == [(1200, 32), (64, 2), (1200, 3), (1025, 17)]
    assert [ce.CASES[n]["cfg"].get("iterations", 10) for n in ce.REUSE_ORDER] == [10, 10, 0, 10]
