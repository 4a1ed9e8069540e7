"""Cases of the fern keyframe database worked by hand (tests/test_ferns_oracle.py checks the oracle against them,
tests/test_gpu_ferns.py runs them through the device).  A case is a table, a configuration and a list of steps on SMALL images;
`expect` holds the fields of the result record that the step pins, `codes` the expected codes.  full_size() turns a small image
into the frame-size image whose nearest sample is that small image (every small pixel repeated 8 x 8)."""
import numpy as np

F = np.float32
NAN = F(np.nan)
FLT_MAX = np.finfo(np.float32).max
FIND, ADD = 1, 2
IDENT = np.eye(4, dtype=F).reshape(16)


def full_size(small):
    return np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=0), 8, axis=1))


def pose(k):
    p = np.eye(4, dtype=F)
    p[:3, 3] = (k, 2 * k, -k)
    return p.reshape(16)


# ---- codes: one fern per line, the pixel's (r, g, b, z) beside it -------------------------------------------------------------
# small image 3 x 2: (x, y) -> r, g, b, z
CODE_PIXELS = {
    (0, 0): (100, 50, 200, F(1.0)),              # z * 1000 = 1000 exactly
    (1, 0): (255, 255, 255, F(0.0)),             # z == 0: bad
    (2, 0): (0, 0, 0, F(3.0e6)),                 # z * 1000 = 3e9 >= 2^31: counts as greater
    (0, 1): (255, 255, 255, F(-1.0)),            # negative: bad
    (1, 1): (255, 255, 255, NAN),                # NaN: bad
    (2, 1): (7, 8, 9, F(1.0) + F(2.0) ** -10),   # z * 1000 = 1000.9765625 exactly: truncates to 1000
}
CODE_TABLE = np.array([
    # x  y  t_r  t_g  t_b  t_d
    [0, 0, 100, 49, 199, 1000],   # r == t_r: 0;  g, b one above: 1, 1;  int(z 1000) == t_d: 0   -> 0110 = 6
    [0, 0, 99, 50, 200, 999],     # r above: 1;  g == t_g, b == t_b: 0, 0;  1000 > 999: 1       -> 1001 = 9
    [1, 0, 0, 0, 0, 400],         # z == 0                                                         -> 255
    [2, 0, 0, 0, 0, 15000],       # 0 > 0 three times: 0;  2^31 rule: 1                           -> 0001 = 1
    [0, 1, 0, 0, 0, 400],         # z < 0                                                          -> 255
    [1, 1, 0, 0, 0, 400],         # z NaN                                                          -> 255
    [2, 1, 6, 8, 8, 1000],        # 7 > 6: 1;  8 > 8: 0;  9 > 8: 1;  int(1000.97..) = 1000 > 1000: 0 -> 1010 = 10
    [2, 1, 7, 7, 9, 999],         # 0;  1;  0;  1000 > 999: 1                                      -> 0101 = 5
], np.int32)
CODE_EXPECT = np.array([6, 9, 255, 1, 255, 255, 10, 5], np.uint8)
CODE_GOOD = 5


def code_images():
    image = np.zeros((2, 3, 4), np.uint8)
    vert = np.zeros((2, 3, 4), F)
    for (x, y), (r, g, b, z) in CODE_PIXELS.items():
        image[y, x] = (r, g, b, 255)
        vert[y, x] = (0.25 * x, 0.5 * y, z, 1)
    return image, vert, np.full((2, 3, 4), 0.5, F)


# ---- decisions: four ferns, one per pixel of a 2 x 2 image, thresholds (127, 127, 127, 1000) -------------------------------------
DECISION_TABLE = np.array([[0, 0, 127, 127, 127, 1000], [1, 0, 127, 127, 127, 1000], [0, 1, 127, 127, 127, 1000],
                           [1, 1, 127, 127, 127, 1000]], np.int32)


def frame_from_codes(codes):
    """the 2 x 2 small images on which DECISION_TABLE yields `codes` (255: a pixel without depth)"""
    image = np.zeros((2, 2, 4), np.uint8)
    vert = np.zeros((2, 2, 4), F)
    norm = np.zeros((2, 2, 4), F)
    for i, c in enumerate(codes):
        y, x = divmod(i, 2)
        if c == 255:
            image[y, x] = (200, 200, 200, 255)  # colour alone makes no code
            continue
        image[y, x] = (255 if c & 8 else 0, 255 if c & 4 else 0, 255 if c & 2 else 0, 255)
        vert[y, x] = (x, y, 2.0 if c & 1 else 0.5, 1)
        norm[y, x] = (0, 0, -1, c)
    return image, vert, norm


def step(codes, time, flags=FIND | ADD, **expect):
    return dict(codes=list(codes), time=time, flags=flags, expect=expect)


DECISION_CASES = [
    # the first frame: without a good code it is not added, with one it is -- whatever the threshold
    dict(name="first_frame", config=dict(threshold=10.0, min_time_gap=0), steps=[
        step([255] * 4, 1, added=0, count=0, good_codes=0, add_minimum=FLT_MAX, closest=-1, candidate=0),
        step([255, 3, 255, 255], 2, added=1, count=1, good_codes=1, add_minimum=FLT_MAX, closest=-1),
        # ... the second never is under this threshold: dissim (1 - 0) / 1 = 1 is not above 10
        step([255, 4, 255, 255], 9, added=0, count=1, add_minimum=F(1.0), closest=0, closest_dissim=F(1.0), closest_similarity=F(0.0),
             candidate=0, closest_time=2),
    ]),
    # two keyframes at the same dissimilarity: the lowest j; dissim = (4 - 2) / 4 = 0.5 for both
    dict(name="tie", config=dict(min_time_gap=0), steps=[
        step([1, 2, 3, 4], 1, added=1, count=1),
        step([1, 2, 5, 6], 2, added=1, count=2, add_minimum=F(0.5), closest=0, closest_dissim=F(0.5), closest_similarity=F(0.5), candidate=1),
        step([1, 2, 7, 8], 3, added=1, count=3, add_minimum=F(0.5), closest=0, closest_dissim=F(0.5), closest_similarity=F(0.5), candidate=1,
             closest_time=1),
    ]),
    # minimum == threshold: strict >, not added
    dict(name="minimum_equals_threshold", config=dict(threshold=0.5, min_time_gap=0), steps=[
        step([1, 2, 3, 4], 1, added=1, count=1),
        step([1, 2, 7, 8], 2, added=0, count=1, add_minimum=F(0.5)),
        step([1, 7, 8, 9], 3, added=1, count=2, add_minimum=F(0.75)),
    ]),
    # the time gap is strict: time - srcTime == min_time_gap is excluded, one more is included
    dict(name="time_gap", config=dict(min_time_gap=3), steps=[
        step([1, 2, 3, 4], 10, added=1, count=1),
        step([1, 2, 3, 4], 13, flags=FIND, added=0, count=1, closest=-1, closest_dissim=FLT_MAX, candidate=0, add_minimum=FLT_MAX),
        step([1, 2, 3, 4], 14, flags=FIND, added=0, count=1, closest=0, closest_dissim=F(0.0), closest_similarity=F(1.0), candidate=1,
             closest_time=10),
        # ADD alone finds nothing, and an equal frame is not added (0 is not above the threshold)
        step([1, 2, 3, 4], 20, flags=ADD, added=0, count=1, closest=-1, add_minimum=F(0.0)),
    ]),
    # no fern good in both: dissim (2 - 0) / 2 = 1, similarity 0 / 0 = NaN, no candidate
    dict(name="no_common_fern", config=dict(min_time_gap=0), steps=[
        step([1, 2, 255, 255], 1, added=1, count=1, good_codes=2),
        step([255, 255, 3, 4], 2, added=1, count=2, good_codes=2, add_minimum=F(1.0), closest=0, closest_dissim=F(1.0), closest_similarity=NAN,
             candidate=0),
    ]),
    # a current frame without a good code: every dissim is 0 / 0, find has no keyframe, add does not look
    dict(name="good_cur_zero", config=dict(min_time_gap=0), steps=[
        step([1, 2, 3, 4], 1, added=1, count=1),
        step([255] * 4, 2, added=0, count=1, good_codes=0, add_minimum=FLT_MAX, closest=-1, closest_dissim=FLT_MAX, candidate=0),
    ]),
    # a capacity of 2: the third accepted frame is dropped and counted, a rejected one is not
    dict(name="capacity", config=dict(min_time_gap=0, capacity=2), steps=[
        step([1, 1, 1, 1], 1, added=1, count=1, dropped_total=0),
        step([2, 2, 2, 2], 2, added=1, count=2, dropped_total=0),
        step([3, 3, 3, 3], 3, added=0, count=2, dropped_total=1, add_minimum=F(1.0)),
        step([1, 1, 1, 1], 4, added=0, count=2, dropped_total=1, add_minimum=F(0.0), closest=0, candidate=1),
        step([4, 4, 4, 4], 5, added=0, count=2, dropped_total=2),
    ]),
]
