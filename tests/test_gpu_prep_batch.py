"""-m gpu: the batched frame preparation (csrc/prep_batch.hpp: prep_batch_kernel, prep_batch_wide_kernel) against the oracle's
per-stage functions chained in the reference's order (tests/prep_oracle.py), bit for bit, on stand-alone odometries
(mmf_debug_odom_prepare: the collectors processFrame fills its stages with).

Every downloadable buffer of levels 0, 1 and 2 is compared, and the extent words and the stored box are decoded and compared
with what numpy finds in the reference buffers.  An invalid vector is NaN in x; what its y and z hold is not defined (every
reader tests x), so validity must match exactly and the components are compared where the vector is valid.  The sizes are
the smallest at which the geometry can go wrong: narrower than a 64-lane tile (32 x 32), a 4-pixel group past a tile with odd
coarse levels (68 x 36), rows no multiple of the tile (100 x 52), a tile + 2 and an odd level (132 x 44), five tiles and a
remainder (260 x 36); the shipped 640 x 480 once."""
import numpy as np
import pytest
import torch

import prep_oracle as po
from helpers import assert_bit_equal
from multimotionfusion_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (68, 36), (100, 52), (132, 44), (260, 36)]
MODEL_BUFFERS = ("prev_packed", "cloud4", "last_depth", "last_image")
SENSOR_BUFFERS = {2: ("vmaps_curr", "nmaps_curr", "depth_pyr"), 1: ("next_image", "dIdx", "dIdy")}  # by side
PRED_IMAGES = ("vertex", "normal", "image", "alt_vertex", "alt_normal", "alt_image")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Rig:
    """n stand-alone odometries of one size, the preparations they went through, and the comparison with the oracle."""

    def __init__(self, ctx, orc, w, h, n=1):
        from multimotionfusion_amd.odometry import RGBDOdometry
        self.ctx, self.orc, self.w, self.h, self.K = ctx, orc, w, h, synth.intrinsics(w, h)
        self.odoms = [RGBDOdometry(ctx, w, h, self.K["cx"], self.K["cy"], self.K["fx"], self.K["fy"]) for _ in range(n)]
        self.gen = 40          # the frame number the extents are noted under
        self.sensor_gen = 0    # depth-side preparations of odoms[0]
        self.boxed = [0] * n   # boxed preparations of each odometry (the slot its box is stored in)
        self.keep = None

    def close(self):
        for o in self.odoms:
            o.close()

    def prepare(self, preds, sensor=None, sides=3, rect=True):
        """preds: host dicts (prep_oracle) with "pose" and optionally "sel", "sel_total", "sel_ratio", "box"."""
        from multimotionfusion_amd.odometry import debugPrepare
        self.gen += 1
        up = []
        for k, p in enumerate(preds):
            d = {name: dev(p[name]) for name in PRED_IMAGES if name in p}
            d["pose"], d["ext_gen"] = p["pose"], self.gen
            if p.get("sel") is not None:
                d["sel"] = dev(np.array([p["sel"]], np.int32))
                d["sel_total"], d["sel_ratio"] = p.get("sel_total", 0), p.get("sel_ratio", 0.0)
            if p.get("box") is not None:
                d["pred_box"] = dev(np.array(p["box"], np.int32))
                self.boxed[k] += int(rect and p.get("sel") is None)
            up.append(d)
        s = None
        if sensor is not None:
            s = {"depth": dev(sensor["depth"]), "rgb": dev(sensor["rgb"]), "cutoff": sensor["cutoff"]}
            self.sensor_gen += int(bool(sides & 2))
        self.keep = (up, s)  # (the odometries alias nothing, but the inputs live until the next preparation all the same)
        debugPrepare(self.odoms, up, s, sides)

    def download(self, k=0, sides=0):
        o = self.odoms[k]
        names = MODEL_BUFFERS + tuple(n for side, ns in SENSOR_BUFFERS.items() if sides & side for n in ns)
        out = {name: [o.download(name, lvl) for lvl in range(3)] for name in names}
        out["extent"], out["prep_box"] = o.download("extent", 0), o.download("prep_box", 0)
        return out

    def check_model(self, k, pred, what):
        """Odometry k's model side against the oracle's for `pred`, the extents included."""
        ref = po.prepare_model(self.orc, self.K, pred)
        o = self.odoms[k]
        for lvl in range(3):
            pk = o.download("prev_packed", lvl)
            for first in (0, 3):
                ok = ~np.isnan(ref["prev_packed"][lvl][..., first])
                assert_bit_equal(~np.isnan(pk[..., first]), ok, f"{what}: prev_packed[{lvl}] validity of vector {first // 3}")
                assert_bit_equal(pk[..., first:first + 3][ok], ref["prev_packed"][lvl][..., first:first + 3][ok], f"{what}: prev_packed[{lvl}] vector {first // 3}")
            for name in ("last_depth", "cloud4", "last_image"):
                assert_bit_equal(o.download(name, lvl), ref[name][lvl], f"{what}: {name}[{lvl}]")
        words = o.download("extent", 0)
        want, got = po.expected_extents(ref, pred), po.decode_extents(words, self.gen)
        assert got == want, (what, got, want)
        if all(v is None for v in want.values()):
            assert self.gen not in po.generations(words)[:18], (what, po.generations(words))
        return ref

    def check_box(self, k, box, what):
        got = self.odoms[k].download("prep_box", 0)[self.boxed[k] & 1]
        want = (1, 1, 0, 0) if box[2] < box[0] or box[3] < box[1] else box
        assert tuple(int(v) for v in got) == tuple(want), (what, got, want)

    def check_sensor(self, sensor, sides, what):
        ref = po.prepare_sensor(self.orc, self.K, sensor["depth"], sensor["cutoff"], sensor["rgb"])
        o = self.odoms[0]
        for lvl in range(3):
            rows = self.h >> lvl
            if sides & 2:
                for name in ("vmaps_curr", "nmaps_curr"):
                    a, b = o.download(name, lvl), ref[name][lvl]
                    ok = ~np.isnan(b[:rows])
                    assert_bit_equal(~np.isnan(a[:rows]), ok, f"{what}: {name}[{lvl}] validity")
                    for p in range(3):
                        assert_bit_equal(a[p * rows:(p + 1) * rows][ok], b[p * rows:(p + 1) * rows][ok], f"{what}: {name}[{lvl}] plane {p}")
                if lvl:  # (level 0 of the depth pyramid is the input itself)
                    assert_bit_equal(o.download("depth_pyr", lvl), ref["depth_pyr"][lvl], f"{what}: depth_pyr[{lvl}]")
            if sides & 1:
                for name in ("next_image", "dIdx", "dIdy"):
                    assert_bit_equal(o.download(name, lvl), ref[name][lvl], f"{what}: {name}[{lvl}]")
        if sides & 2:
            words = o.download("extent", 0)
            want, got = po.expected_zmin(sensor["depth"], sensor["cutoff"]), po.decode_zmin(words, self.sensor_gen)
            assert (got is None and want is None) or (got is not None and want is not None and got == want), (what, got, want)
            if want is None:
                assert self.sensor_gen not in po.generations(words)[18:], what


@pytest.fixture
def prep_big(gpu_ctx):
    """Sets the pixel threshold of the four-tile workgroups for one test; the tunable again afterwards."""
    def set_big(n):
        assert gpu_ctx.lib.mmf_debug_set_prep_big(n) == 0
    try:
        yield set_big
    finally:
        gpu_ctx.lib.mmf_debug_set_prep_big(-1)
        gpu_ctx.lib.mmf_debug_set_prep_rect(-1)


def with_pose(pred, pose):
    pred = dict(pred)
    pred["pose"] = pose
    return pred


#        prediction channels, sensor channels (None: no sensor frame), sides, general pose
CASES = [(4, 3, 3, True), (3, 4, 3, False), (4, None, 0, False), (3, None, 0, True), (4, 3, 2, True), (3, 4, 1, False)]


def run_every_job(gpu_ctx, orc, w, h):
    rig = Rig(gpu_ctx, orc, w, h)
    try:
        for k, (pch, sch, sides, general) in enumerate(CASES):
            pred = with_pose(po.crafted_prediction(w, h, seed=k, channels=pch), po.general_pose() if general else np.eye(4, dtype=np.float32))
            sensor = po.crafted_sensor(w, h, seed=k, channels=sch) if sch else None
            what = f"{w}x{h} case {k}"
            rig.prepare([pred], sensor, sides)
            rig.check_model(0, pred, what)
            if sensor:
                rig.check_sensor(sensor, sides, what)
    finally:
        rig.close()


@pytest.mark.parametrize("big", [1, 0], ids=["reps4", "reps1"])
@pytest.mark.parametrize("w,h", SIZES)
def test_every_job_on_crafted_inputs(gpu_ctx, orc, prep_big, w, h, big):
    """All jobs of prep_collect_all (a sensor frame and one model in the same four launches), of prep_collect_model alone and
    of prep_collect_sensor + prep_collect_model (one side of the sensor frame), 3- and 4-channel images on both sides, a
    general pose and the identity -- with every job's workgroups four tiles tall (rows 52 / 26 / 13 and 36 / 18 / 9 are no
    multiple of that 16-row group) and one tile tall."""
    prep_big(big)
    run_every_job(gpu_ctx, orc, w, h)


def test_the_shipped_geometry(gpu_ctx, orc, prep_big):
    """640 x 480 with the tunable left alone: four tiles per workgroup at level 0, one below."""
    prep_big(-1)
    w, h = 640, 480
    rig = Rig(gpu_ctx, orc, w, h)
    try:
        pred = with_pose(po.crafted_prediction(w, h, seed=3, channels=4), po.general_pose())
        sensor = po.crafted_sensor(w, h, seed=3, channels=3)
        rig.prepare([pred], sensor, 3)
        rig.check_model(0, pred, "640x480")
        rig.check_sensor(sensor, 3, "640x480")
    finally:
        rig.close()


@pytest.mark.parametrize("big", [1, 0], ids=["reps4", "reps1"])
@pytest.mark.parametrize("w,h", [(68, 36), (100, 52)])
def test_source_choice_on_the_device(gpu_ctx, orc, prep_big, w, h, big):
    """*sel as a flag (sel_total == 0) and as a count of sel_total == 12 samples against the ratio 0.75, which 9 / 12 sits on
    exactly: the prediction's images or the alt images, which differ at every pixel."""
    prep_big(big)
    rig = Rig(gpu_ctx, orc, w, h)
    taken = []
    try:
        for k, (total, sel) in enumerate([(0, 0), (0, 1), (12, 0), (12, 8), (12, 9), (12, 12)]):
            pred = with_pose(po.crafted_prediction(w, h, seed=10 + k, channels=4 if k % 2 else 3), po.general_pose())
            pred.update(po.alt_of(pred, seed=k))
            pred.update(sel=sel, sel_total=total, sel_ratio=0.75)
            sensor = po.crafted_sensor(w, h, seed=k) if k % 3 == 0 else None  # with a sensor side in the same launches, and alone
            rig.prepare([pred], sensor, 3)
            rig.check_model(0, pred, f"total {total} sel {sel}")
            taken.append(po.takes_alt(sel, total, 0.75))
    finally:
        rig.close()
    assert taken == [False, True, True, True, False, False]  # both outcomes, in both forms


def extent_scenes(w, h):
    corners = [(0, 0, 1.0), (w - 1, 0, 1.5), (0, h - 1, 2.0), (w - 1, h - 1, 2.5)]
    scenes = {"each corner alone": None,
              "four corners": corners,
              "last column only": [(w - 1, y, 1.0 + 0.01 * y) for y in range(h)],
              "last row only": [(x, h - 1, 3.0 - 0.001 * x) for x in range(w)],
              "nothing valid": [],
              "beyond the cut-off only": [(w // 2, h // 2, 6.5), (3, h - 1, 9.0)]}
    if w > 64:  # both sides of the ballot's wave boundary, in the rows the jobs of levels 0 and 1 note
        scenes["lanes 63 and 64"] = [(63, h - 1, 1.0), (64, h - 1, 1.25)] + [(x, h - 2, 2.0) for x in (126, 127, 128, 129) if x < w]
    out = []
    for name, texels in scenes.items():
        if texels is None:
            out += [(f"corner {c[:2]}", [c]) for c in corners]
        else:
            out.append((name, texels))
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_extents_of_sparse_scenes(gpu_ctx, orc, prep_big, w, h):
    """The extent words against the boxes numpy finds in the reference buffers: single texels in the corners, the last column
    and the last row alone (the boxes of levels 0 and 1 exist for them), both sides of a wave boundary, nothing at all."""
    prep_big(-1)
    rig = Rig(gpu_ctx, orc, w, h)
    try:
        for name, texels in extent_scenes(w, h):
            pred = with_pose(po.sparse_prediction(w, h, texels), po.general_pose())
            rig.prepare([pred])
            rig.check_model(0, pred, f"{w}x{h} {name}")
    finally:
        rig.close()


@pytest.mark.parametrize("w,h", [(68, 36), (132, 44)])
def test_a_newer_generation_supersedes_the_extents(gpu_ctx, orc, prep_big, w, h):
    """Two preparations of one odometry under generations g and g + 1, a large box first and a small one second: the second
    frame's words are its own, not the hull.  And the sensor frame's smallest depth in both of its slots; a frame with nothing
    valid notes nothing."""
    prep_big(-1)
    rig = Rig(gpu_ctx, orc, w, h)
    try:
        big_scene = with_pose(po.crafted_prediction(w, h, seed=1), po.general_pose())
        small = with_pose(po.sparse_prediction(w, h, [(w // 2 + dx, h // 2 + dy, 2.0 + 0.1 * dx) for dx in range(5) for dy in range(5)]), po.general_pose())
        frames = [po.crafted_sensor(w, h, seed=1), po.crafted_sensor(w, h, seed=2, cutoff=2.5), po.crafted_sensor(w, h, seed=3, mode="none"),
                  po.crafted_sensor(w, h, seed=4, mode="edge")]
        frames[1]["depth"][h - 1, w - 1] = 0.125  # (the smallest of its frame, below the first frame's)
        for k, (pred, sensor) in enumerate(zip([big_scene, small, big_scene, small], frames)):
            rig.prepare([pred], sensor, 3)
            ref = rig.check_model(0, pred, f"generation {k}")
            rig.check_sensor(sensor, 3, f"sensor frame {k}")
            if k == 1:
                e = po.expected_extents(ref, pred)
                assert e["depth2"] is not None and e["depth2"][2] - e["depth2"][0] < 8 and e["vertex"][0][0] == w // 2  # (the small one)
        assert rig.sensor_gen == 4
    finally:
        rig.close()


def boxed_prediction(w, h, step, box, fill, channels):
    p = with_pose(po.crafted_prediction(w, h, seed=20 + step, channels=channels, box=box, fill=fill), po.general_pose())
    p["box"] = box
    return p


@pytest.mark.parametrize("big", [1, 0], ids=["reps4", "reps1"])
@pytest.mark.parametrize("w,h", [(100, 52), (132, 44)])
def test_boxed_walk_leaves_whole_frame_buffers(gpu_ctx, orc, prep_big, w, h, big):
    """An object model's preparation covers the hull of the box its prediction is non-zero in now and of the box of its previous
    preparation, taken to each level with the pyramid windows' reach.  After every step of a sequence of boxes (interior,
    disjoint, empty, the last pixel, edges on x = 63 | 64 and on tile edges, the whole image, odd-aligned, shrinking) all
    buffers must be what the oracle makes of the WHOLE frame, and the box is stored for the next step."""
    prep_big(big)
    gpu_ctx.lib.mmf_debug_set_prep_rect(1)
    rig = Rig(gpu_ctx, orc, w, h)
    try:
        for step, (box, fill) in enumerate(po.box_sequence(w, h)):
            pred = boxed_prediction(w, h, step, box, fill, 4 if step % 3 else 3)
            rig.prepare([pred])
            rig.check_model(0, pred, f"{w}x{h} step {step} box {box}")
            rig.check_box(0, box, f"step {step}")
        assert rig.boxed[0] == len(po.box_sequence(w, h))
    finally:
        rig.close()


def test_boxed_walk_equals_the_whole_frame_walk(gpu_ctx, orc, prep_big):
    """The same sequence with mmf_debug_set_prep_rect(0): every job covers the frame.  Identical buffers, all bits."""
    w, h = 100, 52
    prep_big(-1)
    runs = []
    for rect in (1, 0):
        gpu_ctx.lib.mmf_debug_set_prep_rect(rect)
        rig = Rig(gpu_ctx, orc, w, h)
        try:
            steps = []
            for step, (box, fill) in enumerate(po.box_sequence(w, h)):
                rig.prepare([boxed_prediction(w, h, step, box, fill, 4)], rect=bool(rect))
                steps.append(rig.download())
            runs.append(steps)
            if not rect:  # nothing was boxed: no box was stored
                assert not steps[-1]["prep_box"].any()
        finally:
            rig.close()
    for step, (a, b) in enumerate(zip(*runs)):
        for name in MODEL_BUFFERS:
            for lvl in range(3):
                assert_bit_equal(a[name][lvl], b[name][lvl], f"step {step}: {name}[{lvl}]")
        assert_bit_equal(a["extent"], b["extent"], f"step {step}: extent words")


def several(w, h, n, boxed=False):
    preds = []
    for k in range(n):
        pose = synth.make_pose((0.05 * k, -0.2 + 0.03 * k, 0.1), (0.1 * k, -0.05 * k, 0.3)).astype(np.float32)
        box = None
        if boxed:  # each odometry its own box
            box = [(3, 2, w // 2, h // 2), (w // 2 + 1, 5, w - 1, h - 3), (1, 1, 0, 0), (7, h // 2 - 3, w - 9, h - 1)][k % 4]
        p = with_pose(po.crafted_prediction(w, h, seed=30 + k, channels=3 if k % 2 else 4, box=box), pose)
        if boxed:
            p["box"] = box
        preds.append(p)
    return preds


@pytest.mark.parametrize("n", [4, 10])
@pytest.mark.parametrize("w,h", [(32, 32), (68, 36)])
def test_several_models_in_one_stage(gpu_ctx, orc, prep_big, w, h, n):
    """Four models put 32 jobs into the last stage, which goes out as one launch of the wide kernel; ten put 80 there, two
    wide launches.  Different inputs and poses per odometry: each must hold its own oracle result.  With four, the sensor frame
    is prepared in the same stages."""
    prep_big(-1)
    rig = Rig(gpu_ctx, orc, w, h, n)
    try:
        preds = several(w, h, n)
        sensor = po.crafted_sensor(w, h, seed=n) if n == 4 else None
        rig.prepare(preds, sensor, 3)
        for k, p in enumerate(preds):
            rig.check_model(k, p, f"{w}x{h} model {k} of {n}")
        if sensor:
            rig.check_sensor(sensor, 3, f"{w}x{h} sensor")
    finally:
        rig.close()


def test_several_boxed_models_in_one_stage(gpu_ctx, orc, prep_big):
    """Four object models, each with its own box, in the same launches -- twice, so that the second preparation walks hulls."""
    w, h, n = 68, 36, 4
    prep_big(-1)
    gpu_ctx.lib.mmf_debug_set_prep_rect(1)
    rig = Rig(gpu_ctx, orc, w, h, n)
    try:
        preds = several(w, h, n, boxed=True)
        for turn in range(2):
            preds = preds[1:] + preds[:1] if turn else preds  # every odometry moves on to its neighbour's box and images
            rig.prepare(preds)
            for k, p in enumerate(preds):
                rig.check_model(k, p, f"turn {turn} model {k}")
                rig.check_box(k, p["box"], f"turn {turn} model {k}")
    finally:
        rig.close()


@pytest.mark.parametrize("w,h", [(100, 52)])
def test_run_to_run(gpu_ctx, orc, prep_big, w, h):
    """One case executed twice, on two fresh odometries: the same bits everywhere, the extent words included."""
    prep_big(1)
    got = []
    for _ in range(2):
        rig = Rig(gpu_ctx, orc, w, h)
        try:
            pred = with_pose(po.crafted_prediction(w, h, seed=5), po.general_pose())
            rig.prepare([pred], po.crafted_sensor(w, h, seed=5), 3)
            got.append(rig.download(0, sides=3))
        finally:
            rig.close()
    a, b = got
    for name in a:
        if name in ("extent", "prep_box"):
            assert_bit_equal(a[name], b[name], name)
        else:
            for lvl in range(3):
                assert_bit_equal(a[name][lvl], b[name][lvl], f"{name}[{lvl}]")
