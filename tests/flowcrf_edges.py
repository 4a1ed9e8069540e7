"""Scenes, cases and the device-against-oracle check shared by the flow-CRF inference tests: test_gpu_flowcrf.py
and test_gpu_flowcrf_edges.py run them on the device, test_flowcrf_edges_oracle.py asserts on the oracle alone
(tests/flowcrf_oracle.py) that every case reaches the edge it is named for.

numpy only at import; torch and the package's device bindings are imported where a device context is used.

The cases, by the part of the engine they pin:
  PAIR     fcrf_pair_kernel where a workgroup takes several chunks of 256 cells j (per = ceil(nchunk / nsplit) >= 2) and
           trailing ranges are empty -- the geometry of every production size, never that of fo.GPU_CASES
  WIDTH8   the label width 8 (5 to 8 labels), with and without zero columns
  DEGENERATE  images of one cell, 2 x 2 cells, one row and one column
  ties     models with the same vertex image and motion = 0: prob is proj alone, and the first maximum must win
  gates    the strict comparisons of fcrf_prep_kernel at their values, the depth image's pathologies, the pixels not to read"""
import functools
import hashlib

import numpy as np

import flowcrf_oracle as fo
from helpers import assert_bit_equal, bits

F32 = np.float32
STAGES = ("E", "U", "proj", "Q", "prob", "label", "ids", "ids_full", "invalid")
WIDTHS = (1, 2, 4, 8, 16, 32)

# (w, h, labels, allow_new): two mean-field iterations each (fo.case_scene: more than 2000 cells).
#   100 x 76, 2 labels: 7600 cells = 30 chunks in 26 ranges of 2, 11 of them empty, at width 1 (the normalisation) and width 2;
#                       100 > 89 columns: the row blur of the middle cells ends at the radius 44 on both sides
#   60 x 92, 17 labels: 5520 cells = 22 chunks in 18 ranges of 2 at width 32 (15 zero columns, IPL = 2), 7 of them empty, the
#                       last non-empty one holds two chunks; 92 > 89 rows: the same for the column blur
# The smallest images at which flowcrf_nsplit leaves per == 1: from about 7200 cells below width 32, about 5100 at width 32.
PAIR_CASES = [(100, 76, 2, False), (60, 92, 17, True)]
PAIR_SOFT = [(100, 76, 2, False)]  # the cases that also run with soft pairwise weights (pair_case says why)
PAIR_WIDTHS = {(100, 76, 2, False): (1, 2), (60, 92, 17, True): (32,)}  # the widths at which the case has per >= 2
WIDTH8_CASES = [(44, 12, 5, False), (43, 25, 8, True)]
DEGENERATE_SIZES = [(1, 1), (2, 2), (70, 1), (1, 70)]
TIE_SIZES = [(8, 8), (43, 25)]
PRODUCTION_CELLS = [160 * 120, 320 * 240]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sampled_mask(H, W):
    """[H][W] bool: the pixels (4x, 4y) the engine reads of the depth and vertex images"""
    m = np.zeros((H, W), bool)
    m[::4, ::4] = True
    return m


def vertex_images(vz, seed=0, poison=False):
    """[H][W][4] per model: channel 2 is z; the others hold numbers the engine must not read.  poison: every pixel that is not
    sampled is NaN in all four channels"""
    rng = np.random.default_rng(seed)
    out = []
    for z in vz:
        v = rng.normal(0, 100, z.shape + (4,)).astype(F32)
        v[..., 2] = z
        if poison:
            v[~sampled_mask(*z.shape)] = np.nan
        out.append(dev(v))
    return out


def engine(gpu_ctx, sc, cfg, **kw):
    from multimotionfusion_amd.flowcrf import FlowCrf
    n = len(sc["tracks"]["ts_cur"]) if sc["tracks"] is not None else 0
    kw.setdefault("max_tracks", n + 7)
    kw.setdefault("max_labels", len(sc["ids"]) + int(sc["allow_new"]))
    return FlowCrf(gpu_ctx, sc["W"], sc["H"], sc["cam"], **kw, **{k: v for k, v in cfg.items()})


def infer(e, sc, tracks="scene", poison=False):
    tr = sc["tracks"] if tracks == "scene" else tracks
    if isinstance(tr, dict):
        tr = {k: dev(v) for k, v in tr.items()}
    depth = sc["depth"]
    if poison:
        depth = np.where(sampled_mask(*depth.shape), depth, F32(np.nan)).astype(F32)
    return e.infer(sc["ids"], sc["T_start"], sc["T_end"], vertex_images(sc["vertex_z"], poison=poison), dev(depth), dev(sc["flow"]),
                   dev(sc["motion"]), tracks=tr, allow_new=sc["allow_new"], new_id=sc["new_id"])


def same_bits_nan_as_nan(got, want, what):
    """bit for bit; a NaN equals a NaN (the sign of 0 / 0 is the processor's choice)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    ne = (bits(got) != bits(want)) & ~nan
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[:4].tolist()}"


def describe(sc):
    return f"{sc['w']}x{sc['h']} L={len(sc['ids']) + int(sc['allow_new'])} new={sc['allow_new']}"


def download(e, n_tracks):
    got = {name: e.download(name) for name in STAGES}
    got["cell"] = e.download("cell")[:, :n_tracks]
    return got


def assert_same_run(got, want, what):
    """two device runs: every stage image and the tracks' cells, bit for bit"""
    for name in STAGES + ("cell",):
        assert_bit_equal(got[name], want[name], f"{what}: {name}")


def replay_fusion(got, sc, what):
    """stage (e) from the device's own Q and proj: products and differences of float32, rounded one by one on both sides, so
    prob is the oracle's bit for bit and the label is the first maximum at EVERY cell, ties included; the ids follow"""
    L, h, w = got["Q"].shape
    prob, label = fo.fuse(got["Q"].reshape(L, -1), sc["motion"], got["proj"].reshape(L, -1))
    assert_bit_equal(got["prob"], prob.reshape(L, h, w), what + ": prob replayed from the device's Q and proj")
    label = label.reshape(h, w).astype(np.int32)
    ne = got["label"] != label
    assert not ne.any(), f"{what}: {int(ne.sum())} labels are not the first maximum of prob, first at {np.argwhere(ne)[:4].tolist()}"
    all_ids = np.array(list(sc["ids"]) + ([sc["new_id"]] if sc["allow_new"] else []), np.uint8)
    assert np.array_equal(got["ids"], all_ids[label]) and np.array_equal(got["ids_full"], fo.upscale4(all_ids[label])), what


def check_against_oracle(gpu_ctx, sc, cfg, want, need_clear=True, **engine_kw):
    """One engine (engine_kw: max_labels, max_tracks) on the scene against want = fo.run_scene(sc, cfg): stages (a) to (e), the
    replay of (e), the structure of the result, the launch count and a second run with the same bits.  need_clear = False
    for a scene made of ties: the labels are then held by the replay alone, not compared with the oracle's.  Returns the
    device's stage images (and "cell")."""
    L = len(sc["ids"]) + int(sc["allow_new"])
    N = sc["w"] * sc["h"]
    e = engine(gpu_ctx, sc, cfg, **engine_kw)
    ids_t, full_t = infer(e, sc)
    n = len(sc["tracks"]["ts_cur"]) if sc["tracks"] is not None else 0
    got = download(e, n)
    what = describe(sc)
    # (a): bit for bit
    same_bits_nan_as_nan(got["E"], want["E"], what + ": E")
    cell = e.download("cell")
    assert np.array_equal(cell[:, :n], want["cell"]) and (cell[:, n:] == -1).all(), what  # (rows past the table: no sample)
    assert np.array_equal(got["invalid"].astype(bool), want["invalid"]), what
    # (b), (c): a few ulp of expf / logf / a division over at most 32 terms
    U, Uo = got["U"], want["U"]
    assert np.array_equal(np.isposinf(U), np.isposinf(Uo)) and not np.isnan(U).any(), what
    fin = np.isfinite(Uo)
    errU = np.abs(U[fin] - Uo[fin]) / np.maximum(1, np.abs(Uo[fin]))
    near = np.abs(want["proj64"] - cfg["min_proj_prob"]) < 1e-5
    assert near.mean() < 0.01
    errP = np.abs(got["proj"] - want["proj"])[~near]
    # (d), (e)
    errQ = np.abs(got["Q"].astype(np.float64) - want["Q"])
    errProb = np.abs(got["prob"].astype(np.float64) - want["prob"])
    print(f"{what}: max |dU| {errU.max():.3g}  |dproj| {errP.max():.3g}  |dQ| {errQ.max():.3g}  |dprob| {errProb.max():.3g}")
    assert errU.max() <= 1e-5 and errP.max() <= 1e-5, what
    assert errQ.max() <= 1e-4 and errProb.max() <= 1e-4, what
    clear = want["margin"] >= 1e-3
    if need_clear:
        # (fewer than ten cells: one cell near a tie is more than a tenth of the image; the clear ones are still compared)
        assert L == 1 or N < 10 or clear.mean() >= 0.9, f"{what}: {int(clear.sum())} clear cells of {N}"
        same = (got["label"][clear] == want["label"][clear]) & (got["ids"][clear] == want["ids"][clear])
        assert same.all(), f"{what}: {int((~same).sum())} of {int(clear.sum())} clear cells (of {N}) have another label"
    replay_fusion(got, sc, what)
    # structure: the ids follow the labels, the large image is the nearest x4 of the small one, the tensors are the images
    all_ids = np.array(sc["ids"] + ([sc["new_id"]] if sc["allow_new"] else []), np.uint8)
    assert np.array_equal(got["ids"], all_ids[got["label"]])
    assert np.array_equal(got["ids_full"], fo.upscale4(got["ids"]))
    assert np.array_equal(ids_t.cpu().numpy(), got["ids"]) and np.array_equal(full_t.cpu().numpy(), got["ids_full"])
    assert np.abs(got["Q"].sum(0) - 1).max() <= 1e-5 and got["prob"].min() >= 0 and got["prob"].max() <= 1
    assert e.last_launches() == (5 + 3 * cfg["iterations"] if cfg["iterations"] > 0 else 4)
    # a second run on the same input: the same bits in every stage
    infer(e, sc)
    assert_same_run(download(e, n), got, what + ": second run")
    e.close()
    return got


def run_once(gpu_ctx, sc, cfg, poison=False, **engine_kw):
    """the device's stage images of one inference on a fresh engine"""
    e = engine(gpu_ctx, sc, cfg, **engine_kw)
    infer(e, sc, poison=poison)
    got = download(e, len(sc["tracks"]["ts_cur"]) if sc["tracks"] is not None else 0)
    e.close()
    return got


# ---- the launch geometry of the pair pass --------------------------------------------------------------------------------------
def pair_geometry(n_cells, width):
    """(nsplit, nchunk, per) as flowcrf_launch_pair launches it (mmf_debug_flowcrf_pair_geometry; a host function)"""
    from multimotionfusion_amd.flowcrf import pair_geometry as query
    return query(n_cells, width)


def empty_ranges(nsplit, nchunk, per):
    return sum(1 for s in range(nsplit) if s * per >= nchunk)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def freeze(sc):
    for v in list(sc.values()) + list((sc["tracks"] or {}).values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def case(w, h, L, allow_new):
    """(scene, configuration, oracle) of fo.case_scene; computed once per process, not to be modified"""
    sc, cfg = fo.case_scene(w, h, L, allow_new)
    return freeze(sc), cfg, fo.run_scene(sc, cfg)


SOFT = 1.0 / 40.0  # the factor on both pairwise weights of a pair case's second configuration


@functools.lru_cache(maxsize=None)
def pair_case(w, h, L, allow_new):
    """(scene, cfg, oracle, soft cfg, soft oracle or None, moved) of a PAIR case; moved = {"default", "soft"}: max |dQ| of the
    oracle when the cells j of the second chunk are left out of every sum.  At the default weights (40, 40) two iterations saturate Q in
    all but a few cells of a two-label scene, and a softmax that is saturated hides an error of the pair sums: leaving a chunk
    of 256 cells j out moves Q by less than 1e-5 there (test_flowcrf_edges_oracle.py).  With both weights at 1 the messages
    are of the order of the unaries, Q stays soft and follows the pair sums: the cases of PAIR_SOFT run that way as well.  (The
    17-label case needs no such run -- a chunk left out moves its Q by 1 -- and would not bear one: under soft weights a
    third of its cells have no clear winner.)  The mean field is linear in the pair matrix, so one N x N matrix serves both:
    A(soft) = SOFT * A"""
    sc, cfg = fo.case_scene(w, h, L, allow_new)
    A = fo.pair_matrix(*fo.features(w, h, sc["flow"]), cfg)
    want = fo.run_scene(sc, cfg, A)
    soft = fo.config(iterations=cfg["iterations"], weight_smoothness=SOFT * cfg["weight_smoothness"],
                     weight_appearance=SOFT * cfg["weight_appearance"])
    moved = {}
    n_labels = want["Q"].shape[0]

    def leave_a_chunk_out(c, r, M):
        M[:, 256:512] = 0
        return float(np.abs(fo.mean_field(r["U"].reshape(n_labels, -1), None, None, c, A=M) - r["Q"].reshape(n_labels, -1)).max())

    want_soft = None
    if (w, h, L, allow_new) in PAIR_SOFT:
        A *= SOFT
        want_soft = fo.run_scene(sc, soft, A)
        moved["soft"] = leave_a_chunk_out(soft, want_soft, A)
        A *= 1.0 / SOFT
    moved["default"] = leave_a_chunk_out(cfg, want, A)
    return freeze(sc), cfg, want, soft, want_soft, moved


def scene_checksum(sc):
    """sha256 over every array of a scene, in a fixed order"""
    hsh = hashlib.sha256()
    for key in ("depth", "vertex_z", "flow", "motion"):
        hsh.update(np.ascontiguousarray(sc[key]).tobytes())
    for key in sorted(sc["tracks"]):
        hsh.update(np.ascontiguousarray(sc["tracks"][key]).tobytes())
    for T in sc["T_start"] + sc["T_end"]:
        hsh.update(np.ascontiguousarray(T).tobytes())
    hsh.update(repr((sc["W"], sc["H"], sc["ids"], sc["new_id"], sc["allow_new"], [float(v) for v in sc["cam"]])).encode())
    return hsh.hexdigest()


@functools.lru_cache(maxsize=None)
def degenerate(w, h, with_tracks):
    """w x h cells, two models and the new label.  The jittered grid of fo.make_scene is empty at these sizes and most of its
    edge tracks end outside the frame, so with_tracks appends a still track on cell 0 (an inlier of model 0) and three that
    move like model 1: at the middle of the frame, in the last column (which wraps past the last cell of a single row: dropped)
    and in the last row; without: tracks = None"""
    sc = fo.make_scene(w, h, 3, True, seed=w + 3 * h)
    if with_tracks:
        W, H, cam, tr = sc["W"], sc["H"], sc["cam"], sc["tracks"]
        for (ex, ey), (sx, sy) in (((1, 1), (1, 1)), ((W // 2, H // 2), (W // 2 - 2, H // 2)), ((W - 1, 2), (W - 3, 2)),
                                   ((2, H - 1), (0, H - 1))):
            c1 = fo.back_project(np.float64(ex), np.float64(ey), np.float64(1.5), cam)
            c0 = fo.back_project(np.float64(sx), np.float64(sy), np.float64(1.5), cam)
            for key, val in (("xy_cur", [ex, ey]), ("xy_prev", [sx, sy]), ("co_cur", c1), ("co_prev", c0), ("ts_prev", 1_000_000_000),
                             ("ts_cur", 1_000_000_000 + fo.DT), ("ok_cur", 1), ("ok_prev", 1)):
                tr[key] = np.concatenate([tr[key], np.asarray(val, tr[key].dtype)[None]])
    else:
        sc["tracks"] = None
    cfg = fo.config()
    return freeze(sc), cfg, fo.run_scene(sc, cfg)


@functools.lru_cache(maxsize=None)
def tie_scene(w, h, kind):
    """motion = 0, so prob = 1 - (1 - 0)(1 - proj) depends on proj alone.  kind "three": models 1 and 2 share a vertex image
    2 mm behind the depth and model 0 lies 25 mm behind it: proj = (0, p, p) with the same bits twice, the label is 1 at every
    valid cell.  "two": two identical models, proj = (0.5, 0.5), label 0.  "two-new": the same with the new label, whose proj
    and prob are 0: never chosen.  Holes (3 % of the pixels, frame and models alike) are `invalid`: prob = 0, label 0."""
    M = 3 if kind == "three" else 2
    sc = fo.make_scene(w, h, M + int(kind == "two-new"), kind == "two-new", seed=11 + w)
    sc["depth"][4 * 2, 4 * 3] = 0  # (the small image has no hole of its own at a sampled pixel)
    hole = sc["depth"] == 0
    near = np.where(hole, 0, sc["depth"] + F32(0.002)).astype(F32)
    vz = np.stack([near] * M)
    if kind == "three":
        vz[0] = np.where(hole, 0, sc["depth"] + F32(0.025))
    sc["vertex_z"] = vz
    sc["motion"] = np.zeros_like(sc["motion"])
    cfg = fo.config()
    return freeze(sc), cfg, fo.run_scene(sc, cfg)


@functools.lru_cache(maxsize=None)
def threshold_scene():
    """fo.rectangle_scene(False) and v, the largest finite track error of its one model: the three thresholds one float
    below v, v and one float above it turn the cells that carry v from outliers (e > threshold) into neither (not e > threshold,
    not e < threshold) into inliers (e < threshold)"""
    sc, _ = fo.rectangle_scene(False)
    E, _ = fo.track_errors(sc["W"], sc["H"], sc["cam"], sc["T_start"], sc["T_end"], sc["tracks"], 2)
    v = E[0][np.isfinite(E[0])].max()
    at = (E[0] == v).reshape(sc["h"], sc["w"])
    return freeze(sc), F32(v), at


def thresholds(v):
    return [("below", float(np.nextafter(F32(v), F32(0)))), ("at", float(v)), ("above", float(np.nextafter(F32(v), F32(np.inf))))]


@functools.lru_cache(maxsize=None)
def threshold_reference(which):
    sc, v, at = threshold_scene()
    cfg = fo.config(iterations=0, threshold=dict(thresholds(v))[which])
    return cfg, fo.run_scene(sc, cfg)


@functools.lru_cache(maxsize=None)
def twin_scene():
    """two identical models on 8 x 8 cells: proj is exactly 0.5 (e / (e + e), whatever expf returns), 0 in the holes"""
    sc = fo.make_scene(8, 8, 2, False, seed=21)
    sc["vertex_z"] = np.stack([sc["vertex_z"][0]] * 2)
    return freeze(sc)


# the depth classes of fcrf_prep_kernel: (name, d, (z of model 0, 1, 2), invalid).  `tiny` = 1e-6f, the bound of both tests.
# The finite distances differ from model to model (4, 12 and 50 mm: the last one beyond max_err = 30 mm), so that a class which
# clamps one model and not another shows in proj.
TINY = F32(1e-6)
TINY_LO, TINY_HI = np.nextafter(TINY, F32(0)), np.nextafter(TINY, F32(1))
NAN, INF = F32(np.nan), F32(np.inf)
Z3 = (F32(1.504), F32(1.512), F32(1.55))
DEPTH_CLASSES = [
    ("d=0, every z>0", F32(0), (F32(0.004), F32(0.012), F32(0.05)), False),
    ("d>0, one z=0", F32(1.5), (F32(0), Z3[0], Z3[1]), False),
    ("d=0, one z=0", F32(0), (F32(0.004), F32(0), F32(0.012)), True),
    ("d<0, every z>0", F32(-0.001), (F32(0.004), F32(0.012), F32(0.05)), False),
    ("d<0, one z<0", F32(-0.001), (F32(0.004), F32(0.012), F32(-0.002)), True),
    ("d=tiny-, z=0", TINY_LO, (Z3[0], F32(0), Z3[1]), True),
    ("d=tiny, z=0", TINY, (Z3[0], F32(0), Z3[1]), False),
    ("d=tiny+, z=0", TINY_HI, (Z3[0], F32(0), Z3[1]), False),
    ("d=0, z=tiny-", F32(0), (F32(0.004), TINY_LO, F32(0.012)), True),
    ("d=0, z=tiny", F32(0), (F32(0.004), TINY, F32(0.012)), False),
    ("d=0, z=tiny+", F32(0), (F32(0.004), TINY_HI, F32(0.012)), False),
    ("d=NaN", NAN, Z3, False),
    ("d=NaN, one z=0", NAN, (F32(0), Z3[0], Z3[1]), False),
    ("d=+inf, z finite", INF, Z3, False),
    ("d=+inf, one z=+inf", INF, (INF, Z3[0], Z3[1]), False),
    ("d>0, one z=NaN", F32(1.5), (NAN, Z3[0], Z3[1]), False),
    ("d>0, one z=+inf", F32(1.5), (Z3[0], INF, Z3[1]), False),
    ("d=0, one z=NaN", F32(0), (F32(0.004), NAN, F32(0.012)), False),
]


def depth_class_cells():
    """the cell (x, y) of every class: rows 1 to 6 of the 8 x 8 image, columns 1, 3, 5"""
    return [(1 + 2 * (k % 3), 1 + k // 3) for k in range(len(DEPTH_CLASSES))]


@functools.lru_cache(maxsize=None)
def depth_class_scene():
    sc = fo.make_scene(8, 8, 3, False, seed=31)
    for (x, y), (_, d, zs, _) in zip(depth_class_cells(), DEPTH_CLASSES):
        sc["depth"][4 * y, 4 * x] = d
        for m in range(3):
            sc["vertex_z"][m, 4 * y, 4 * x] = zs[m]
    cfg = fo.config(iterations=0)
    return freeze(sc), cfg, fo.run_scene(sc, cfg)
