"""The scene of the back-dating fusion tests: the 320 x 240 scene of tests/test_gpu_viewlog_fusion.py (a box that is segmented
from frame SPAWN on, leaves after LAST_SEEN and 100 static landmarks), with the OBJECT's keypoints added from frame 0 on
instead of from SPAWN -- the box is in view before it is segmented, which is what refineTrackSubset back-dates over."""
import numpy as np

import viewlog_oracle as vo
from test_gpu_redetect_fusion import BACK, H, LAST_SEEN, N_FRAMES, SPAWN, W, gap_scene, physical_keypoints

SEED = 21
LOST = LAST_SEEN + 1  # the frame in which model 1 is found lost


def build():
    """-> K, per frame the rendering it shows, per frame the keypoints (xy [m,2], descriptor [m,256])"""
    K, poses, objs, traj, with_obj, without = gap_scene(SEED)
    obj_kps, obj_desc = physical_keypoints(SEED, K, poses, traj, with_obj)
    rng = np.random.default_rng(SEED)
    f0 = with_obj[0]
    ys, xs = np.nonzero((f0["ids"] == 0) & (f0["depth"] > 0))
    pick = rng.choice(len(ys), 100, replace=False)
    cam = f0["vertex"][ys[pick], xs[pick], :3].astype(np.float64)
    world = cam @ poses[0][:3, :3].T + poses[0][:3, 3]
    land_desc = vo.unit_rows(rng, 100)
    frames, kps = [], []
    for i in range(LOST + 1):
        hidden = LAST_SEEN < i < BACK
        frames.append(without[i] if hidden else with_obj[i])
        Pi = np.linalg.inv(poses[i])
        x = world @ Pi[:3, :3].T + Pi[:3, 3]
        u = np.rint(x[:, 0] / x[:, 2] * K["fx"] + K["cx"]).astype(np.int64)
        v = np.rint(x[:, 1] / x[:, 2] * K["fy"] + K["cy"]).astype(np.int64)
        ok = (x[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        xy, desc = np.stack([u[ok], v[ok]], 1).astype(np.int32), land_desc[ok]
        if not hidden:  # (from frame 0 on)
            idx, oxy, _ = obj_kps[i]
            xy, desc = np.concatenate([xy, oxy]), np.concatenate([desc, obj_desc[idx]])
        kps.append((xy, desc))
    return K, frames, kps


def frame_mask(frames, i, label=1):
    """the id image frame i brings: the box carries `label` from SPAWN on while it is in view"""
    mask = np.zeros((H, W), np.uint8)
    if SPAWN <= i <= LAST_SEEN:
        mask[frames[i]["ids"] == 1] = label
    return mask
