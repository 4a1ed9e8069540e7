"""The cases of the back-dating tests (tests/test_backdate_oracle.py on the CPU, tests/test_gpu_backdate.py on the device):
each is a short script of tracker calls that ends in one backdate(label, history), the smallest that reaches the edge it is
named for.  A script is a list of steps a driver replays: ("log", frames), ("add", xy, desc, timestamp, depth),
("associate", mask, ids), ("prune", min_kps, min_time), ("reset",).

A scene is made of PHYSICAL keypoints: keypoint k has one unit descriptor (random unit rows are far beyond the matching gate
from each other, an exact repeat continues its track), a pixel of its own in every frame and the depth there; `seen[k]` says
in which frames it is visible, `nan[k]` in which of those its depth is 0 (a non-null keypoint with NaN coordinates), `label[k]`
what the id image holds at its pixel in the last frame."""
import numpy as np

import viewlog_oracle as vo

W, H = 64, 48
K = (52.0, 51.5, 31.5, 23.25)


class Case:
    def __init__(self, name, steps, label, history, capacity=64, max_keypoints=32, max_points=1024, expect=None):
        self.name, self.steps, self.label, self.history = name, steps, label, history
        self.capacity, self.max_keypoints, self.max_points = capacity, max_keypoints, max_points
        self.expect = expect or {}  # field -> the list over the entries the oracle must give (the edge the case is named for)


def frames_of(rng, n_frames, seen, nan=None, label=None, t0=1_000_000, first_stamp_index=0):
    """-> the add steps of n_frames frames and the last frame's id image.  seen: {k: frames}, nan: {k: frames}, label: {k: id}"""
    nan, label = nan or {}, label or {}
    keys = sorted(seen)
    desc = {k: d for k, d in zip(keys, vo.unit_rows(np.random.default_rng(1234), len(keys)))}  # (the same rows in every case)
    steps, mask = [], np.zeros((H, W), np.uint8)
    for f in range(n_frames):
        vis = [k for k in keys if f in seen[k]]
        flat = rng.choice(W * H, len(vis), replace=False)
        xy = np.stack([flat % W, flat // W], 1).astype(np.int32).reshape(-1, 2)
        depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
        for q, k in enumerate(vis):
            if f in nan.get(k, ()):
                depth[xy[q, 1], xy[q, 0]] = 0.0
        d = np.stack([desc[k] for k in vis]).astype(np.float32) if vis else np.zeros((0, 256), np.float32)
        steps.append(("add", xy, d, t0 + 33_000 * (f + first_stamp_index), depth))
        if f == n_frames - 1:
            for q, k in enumerate(vis):
                mask[xy[q, 1], xy[q, 0]] = label.get(k, 0)
    return steps, mask


def simple(name, n_frames, n_tracks, history, log_frames=8, seen=None, nan=None, label=None, expect=None, seed=0, ids=(1, 2), **kw):
    rng = np.random.default_rng(seed)
    seen = seen or {k: range(n_frames) for k in range(n_tracks)}
    label = label if label is not None else {k: 1 for k in seen}
    adds, mask = frames_of(rng, n_frames, seen, nan, label)
    return Case(name, [("log", log_frames)] + adds + [("associate", mask, list(ids))], 1, history, expect=expect, **kw)


def all_cases():
    every = lambda n, f: {k: range(f) for k in range(n)}
    cases = [
        simple("history_2", 4, 5, 2, expect={"from": [-1, 0], "nvalid": [0, 5], "stamp": [3, 4]}),
        simple("history_3", 4, 5, 3, expect={"from": [-1, 0, 1], "nvalid": [0, 5, 5], "stamp": [2, 3, 4]}),
        # history = F = 4 after 6 adds: the ring has wrapped (s > F), every slot of it is in the window
        simple("history_F_wrapped", 6, 5, 4, log_frames=4, expect={"stamp": [3, 4, 5, 6], "nvalid": [0, 5, 5, 5]}),
        simple("cut_by_F", 5, 5, 8, log_frames=3, expect={"stamp": [3, 4, 5], "from": [-1, 0, 1]}),
        simple("nvalid_2", 3, 2, 2, expect={"nvalid": [0, 2], "both": [0, 2], "status": [0, 1]}),
        simple("nvalid_3", 3, 3, 2, expect={"nvalid": [0, 3], "status": [0, 0]}),
        # track 0 has depth 0 in frame 1: non-null, not finite -- it counts in both, not in nvalid
        simple("nan_track", 3, 4, 3, nan={0: [1]}, expect={"both": [0, 4, 4], "nvalid": [0, 3, 3], "from": [-1, 0, 1]}),
        # frame 2 (of 0 .. 3) shows one track only: from[3] skips it and pair (1, 3) spans two frames
        simple("gap_frame", 4, 4, 4, seen={0: range(4), 1: [0, 1, 3], 2: [0, 1, 3], 3: [0, 1, 3]},
               expect={"from": [-1, 0, 1, 1], "nvalid": [0, 4, 1, 4], "status": [0, 0, 1, 0]}),
        simple("two_gap_frames", 5, 4, 5, seen={0: range(5), 1: [0, 1, 4], 2: [0, 1, 4], 3: [0, 1, 4]},
               expect={"from": [-1, 0, 1, 1, 1], "nvalid": [0, 4, 1, 1, 4], "status": [0, 0, 1, 1, 0]}),
        # keypoints 0 .. 3 carry label 1; 4, 5 label 2; 6 lies on label 0; 7 is not visible in the last frame (unlabelled)
        simple("other_labels", 3, 8, 2, seen={**every(7, 3), 7: [0, 1]}, label={0: 1, 1: 1, 2: 1, 3: 1, 4: 2, 5: 2, 6: 0},
               expect={"nvalid": [0, 4], "both": [0, 4]}),
        # frame 1 (of 0 .. 2) has no keypoint at all: an empty slot, a gap
        simple("empty_slot", 3, 4, 3, seen={k: [0, 2] for k in range(4)}, expect={"both": [0, 0, 4], "from": [-1, 0, 0], "status": [0, 1, 0]}),
        # 9 rows against a batch object of max_points 8: the host core estimates the problem
        simple("host_fallback", 2, 9, 2, max_points=8, expect={"nvalid": [0, 9], "host_estimated": [0, 1], "status": [0, 0]}),
    ]
    # len cut by L: the table is emptied by a prune (length 0), two adds follow -- L = 2 while the ring holds 4 frames
    rng = np.random.default_rng(20)
    a, _ = frames_of(rng, 2, every(4, 2))
    b, mask = frames_of(rng, 2, every(4, 2), label={k: 1 for k in range(4)}, first_stamp_index=2)
    cases.append(Case("cut_by_L", [("log", 8)] + a + [("prune", 99, 1 << 40)] + b + [("associate", mask, [1])], 1, 4,
                      expect={"stamp": [3, 4], "nvalid": [0, 4]}))
    # the log switched on two frames ago: three adds without it, two with it
    rng = np.random.default_rng(21)
    adds, mask = frames_of(rng, 5, every(4, 5), label={k: 1 for k in range(4)})
    cases.append(Case("log_on_two_frames_ago", adds[:3] + [("log", 8)] + adds[3:] + [("associate", mask, [1])], 1, 4,
                      expect={"stamp": [4, 5], "nvalid": [0, 4]}))
    # len 1: the log was switched on one frame ago
    cases.append(Case("len_1", adds[:4] + [("log", 8)] + adds[4:] + [("associate", mask, [1])], 1, 4,
                      expect={"stamp": [5], "from": [-1], "status": [0]}))
    # a track pruned since: keypoint 4 was seen in frame 0 only; the prune behind frame 2 removes it, its uid stays in the log
    rng = np.random.default_rng(22)
    adds, mask = frames_of(rng, 3, {**every(4, 3), 4: [0]}, label={k: 1 for k in range(4)})
    cases.append(Case("pruned_track", [("log", 8)] + adds + [("prune", 2, 1 << 40), ("associate", mask, [1])], 1, 3,
                      expect={"nvalid": [0, 4, 4]}))
    # a tracker reset between frames: the stamps restart, what was logged before is gone
    rng = np.random.default_rng(23)
    a, _ = frames_of(rng, 3, every(4, 3))
    b, mask = frames_of(rng, 2, every(4, 2), label={k: 1 for k in range(4)}, first_stamp_index=3)
    cases.append(Case("reset_between_frames", [("log", 8)] + a + [("reset",)] + b + [("associate", mask, [1])], 1, 4,
                      expect={"stamp": [1, 2], "nvalid": [0, 4]}))
    # a table of 1025 rows, the segment = rows 1020 .. 1024: it straddles the second pass of the 1024 lanes
    rng = np.random.default_rng(24)
    adds, mask = frames_of(rng, 2, every(1025, 2), label={k: 1 for k in range(1020, 1025)})
    cases.append(Case("table_1025_rows", [("log", 2)] + adds + [("associate", mask, [1])], 1, 2, capacity=1100, max_keypoints=1025,
                      expect={"nvalid": [0, 5], "both": [0, 5]}))
    return cases


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = all_cases()
    return CASES


def replay(case, driver):
    """the case's script through a driver with log / add / associate / prune / reset"""
    for step in case.steps:
        getattr(driver, step[0])(*step[1:])
