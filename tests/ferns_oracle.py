"""The arithmetic of the fern keyframe database (Core/Ferns.cpp:21-143, 145-203, 322-337) restated in numpy,
float32 wherever the reference uses `float`.  The device engine (csrc/ferns_kernels.hpp) equals this bit for bit.

Small images: w = width // 8, h = height // 8; small pixel (i, j) is the source texel (texel((i + 0.5f) / w, width),
texel((j + 0.5f) / h, height)), texel(c, n) = clamp((int)floorf(c * (float)n), 0, n - 1) (GPUResize as oracle/mmf_oracle_surfel.c
restates it, assumption A3); rows are not flipped."""
import numpy as np

F = np.float32
BAD = 255
FIND, ADD = 1, 2
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(num=500, max_depth_mm=15000, capacity=1024, min_time_gap=300, threshold=F(0.3095), min_similarity=F(0.3))
MASK64 = (1 << 64) - 1


def texel(c, n):
    """c float32 array of normalised coordinates -> int texel in [0, n - 1]"""
    t = np.floor(np.asarray(c, F) * F(n)).astype(np.int64)
    return np.clip(t, 0, n - 1)


def small_indices(width, height):
    """(ty [h], tx [w]): the source row of every small row, the source column of every small column"""
    w, h = width // 8, height // 8
    tx = texel((np.arange(w, dtype=F) + F(0.5)) / F(w), width)
    ty = texel((np.arange(h, dtype=F) + F(0.5)) / F(h), height)
    return ty, tx


def resize(img):
    """[height, width, C] -> [h, w, C] by the nearest-sample rule above"""
    ty, tx = small_indices(img.shape[1], img.shape[0])
    return np.ascontiguousarray(img[ty][:, tx])


def _splitmix(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, z ^ (z >> 31)


def make_table(seed, num, w, h, max_depth_mm):
    """mmf_ferns_make_table: per fern x, y, t_r, t_g, t_b, t_d, each lo + next % (hi - lo + 1) of a splitmix64 sequence"""
    state = seed & MASK64
    out = np.zeros((num, 6), np.int32)
    for i in range(num):
        for k, (lo, hi) in enumerate(((0, w - 1), (0, h - 1), (0, 255), (0, 255), (0, 255), (400, max_depth_mm))):
            state, r = _splitmix(state)
            out[i, k] = lo + r % (hi - lo + 1)
    return out


def encode(table, image_small, vert_small):
    """(codes uint8 [num], good): Ferns.cpp:90-110.  image_small uint8 [h, w, >= 3], vert_small float32 [h, w, 4]"""
    codes = np.full(len(table), BAD, np.uint8)
    for i, (x, y, tr, tg, tb, td) in enumerate(np.asarray(table, np.int64)):
        z = F(vert_small[y, x, 2])
        if not z > 0:  # (a NaN compares false)
            continue
        p = image_small[y, x]
        mm = F(z * F(1000.0))  # one float multiplication
        deep = True if mm >= F(2147483648.0) else int(np.trunc(mm)) > td  # (2^31 or more counts as greater)
        codes[i] = (int(p[0]) > tr) << 3 | (int(p[1]) > tg) << 2 | (int(p[2]) > tb) << 1 | int(deep)
    return codes, int(np.count_nonzero(codes != BAD))


def co_occurrence(cur, db):
    return int(np.count_nonzero((cur != BAD) & (db == cur)))


def dissimilarity(good_cur, good_j, co):
    max_co = F(min(good_cur, good_j))
    with np.errstate(invalid="ignore", divide="ignore"):
        return F(F(max_co - F(co)) / max_co)  # (0 / 0: NaN)


def block_hd_aware(a, b):
    """Ferns.cpp:322-337: equal codes among the ferns good in both / their number; NaN when there are none"""
    both = (a != BAD) & (b != BAD)
    with np.errstate(invalid="ignore", divide="ignore"):
        return F(F(np.count_nonzero(both & (a == b))) / F(np.count_nonzero(both)))


class Database:
    """The database with a capacity; process() is one mmf_ferns_process + mmf_ferns_result."""

    def __init__(self, width, height, table, **config):
        self.cfg = dict(DEFAULTS, **config)
        self.cfg["threshold"], self.cfg["min_similarity"] = F(self.cfg["threshold"]), F(self.cfg["min_similarity"])
        self.width, self.height, self.w, self.h = width, height, width // 8, height // 8
        self.table = np.asarray(table, np.int32).reshape(-1, 6)
        assert len(self.table) == self.cfg["num"]
        self.reset()

    def reset(self):
        self.frames, self.dropped = [], 0
        self.cur = None

    def process_small(self, image, vert, norm, pose, time, flags=FIND | ADD):
        """the same on small images (the hand-worked cases)"""
        cfg = self.cfg
        codes, good = encode(self.table, image, vert)
        n = len(self.frames)
        co = np.array([co_occurrence(codes, f["codes"]) for f in self.frames], np.int32)
        dis = np.array([dissimilarity(good, f["good"], c) for f, c in zip(self.frames, co)], F)
        self.cur = dict(image=image, vert=vert, norm=norm, codes=codes, good=good, co=co, dissim=dis)
        add_min = FLT_MAX
        if flags & ADD and good > 0:
            for d in dis:
                if d < add_min:
                    add_min = d
        wanted = bool(flags & ADD) and (add_min > cfg["threshold"] or n == 0) and good > 0
        added = wanted and n < cfg["capacity"]
        if wanted and not added:
            self.dropped += 1
        closest, closest_d = -1, FLT_MAX
        if flags & FIND:
            for j, d in enumerate(dis):
                if d < closest_d and time - self.frames[j]["time"] > cfg["min_time_gap"]:
                    closest_d, closest = d, j
        sim = block_hd_aware(codes, self.frames[closest]["codes"]) if closest >= 0 else F(0)
        res = dict(added=int(added), dropped_total=self.dropped, count=n + int(added), good_codes=good, add_minimum=F(add_min),
                   closest=closest, closest_dissim=F(closest_d), closest_similarity=F(sim),
                   candidate=int(closest >= 0 and bool(sim > cfg["min_similarity"])),
                   closest_pose=(self.frames[closest]["pose"] if closest >= 0 else np.zeros(16, F)),
                   closest_time=(self.frames[closest]["time"] if closest >= 0 else 0))
        if added:
            self.frames.append(dict(codes=codes, good=good, pose=np.asarray(pose, F).reshape(16).copy(), time=int(time),
                                    image=image.copy(), vert=vert.copy(), norm=norm.copy()))
        return res

    def process(self, image, vert, norm, pose, time, flags=FIND | ADD):
        """image uint8 [height, width, 4], vert / norm float32 [height, width, 4]"""
        return self.process_small(resize(image), resize(vert), resize(norm), pose, time, flags)
