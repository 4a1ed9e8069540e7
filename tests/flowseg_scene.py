"""The sequence tests/test_gpu_flowseg_fusion.py and tests/test_gpu_flowseg_shim.py run the flow_crf mode on: a static
camera in front of a textured relief, and in its middle a patch whose texture starts to slide in frame 2.  The patch's
inner part R returns no depth in frames 0 and 1 (so the camera's model has no surfel there) and, from frame 2 on, the
depth of an object in front of the relief, except on the pixels (4x, 4y) the inference samples.

With ONE model the inference's projection probability is 1 wherever the frame or the model has depth, so
the new label can win only where both have none and the flow says "moving": R in frame 2.  The landmarks on the patch's
rim -- which has depth throughout -- slide with it (8 pixels in 33 ms: 240 px/s against the threshold of 20) and make the
patch's cells the new label's; the landmarks on the relief stand still.  flowseg_scene.predict() restates the frame-2
segmentation on the CPU with tests/flow_oracle.py, tests/flowcrf_oracle.py and tests/flowseg_oracle.py (identity poses,
the model's prediction taken as frame 1's depth): R is about 12 % of the cells."""
import numpy as np

F32 = np.float32
DT = 33_000_000
N_FRAMES = 5
SHIFT = 8  # pixels per frame, from frame 2 on


def _smooth(rng, h, w, passes=3, k=5):
    a = rng.random((h + 2 * k * passes, w + 2 * k * passes, 3))
    ker = np.ones(k) / k
    for _ in range(passes):
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="valid"), 0, a)
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="valid"), 1, a)
    a = a[:h, :w]
    a = (a - a.min()) / (a.max() - a.min())
    return a


def geometry(W, H):
    """the patch P and its depth-less inner part R, in pixels: (x0, y0, x1, y1) each, multiples of 4"""
    px0, py0 = (W // 4) // 4 * 4, (H // 4) // 4 * 4
    px1, py1 = px0 + (W * 9 // 20) // 4 * 4, py0 + (H * 7 // 15) // 4 * 4
    return (px0, py0, px1, py1), (px0 + 8, py0 + 8, px1 - 8, py1 - 8)


def make(W, H, seed=5):
    """K, frames [{rgb uint8 [H,W,3], depth float32 [H,W]}], keypoints per frame (xy int32 [n,2], descriptor float32 [n,256])"""
    rng = np.random.default_rng(seed)
    K = dict(fx=float(W), fy=float(W), cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    P, R = geometry(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    # depth in steps of 1 / 1024 m: every float64 sum over it is exact, so depth_mean and depth_std have one right answer
    relief = (np.rint((2.0 + 0.15 * np.sin(xx / 23.0) * np.cos(yy / 17.0)) * 1024) / 1024).astype(F32)
    back = _smooth(rng, H, W)
    slide = _smooth(rng, P[3] - P[1], P[2] - P[0] + SHIFT * N_FRAMES)
    in_r = (xx >= R[0]) & (xx < R[2]) & (yy >= R[1]) & (yy < R[3])
    lattice = (xx % 4 == 0) & (yy % 4 == 0)
    # landmarks: a grid on the relief outside the patch, two rows on the patch's rim
    gx, gy = np.meshgrid(np.arange(6, W - 6, 13), np.arange(6, H - 6, 11))
    gx, gy = gx.ravel(), gy.ravel()
    out = (gx < P[0] - 4) | (gx >= P[2] + 4) | (gy < P[1] - 4) | (gy >= P[3] + 4)
    static = np.stack([gx[out], gy[out]], 1)
    # ... and one in the middle of every second cell of the left part of R: these slide with the patch
    ix, iy = np.meshgrid(np.arange(R[0] + 2, R[2] - SHIFT - 2, 8), np.arange(R[1] + 2, R[3] - 2, 8))
    rim = np.stack([ix.ravel(), iy.ravel()], 1)
    desc = rng.normal(size=(len(static) + len(rim), 256))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    frames, kps = [], []
    for i in range(N_FRAMES):
        off = SHIFT * max(i - 1, 0)
        img = back.copy()
        img[P[1]:P[3], P[0]:P[2]] = slide[:, SHIFT * N_FRAMES - off:SHIFT * N_FRAMES - off + P[2] - P[0]]  # moves to the right
        moved = rim + np.array([off, 0])
        depth = relief.copy()
        obj = relief - F32(0.375)
        if i < 2:  # no return from R but at the landmarks
            depth[in_r] = 0
            depth[moved[:, 1], moved[:, 0]] = obj[moved[:, 1], moved[:, 0]]
        else:
            depth[in_r] = obj[in_r]
            depth[in_r & lattice] = 0
        frames.append(dict(rgb=np.ascontiguousarray((img * 255).astype(np.uint8)), depth=depth))
        kps.append((np.concatenate([static, moved]).astype(np.int32), desc))
    return K, frames, kps


def predict(W, H, frame=2, crf=None):
    """the flow_crf segmentation of `frame` as the CPU oracles compute it from the scene alone (see the module's text):
    (inference ids [h,w], flowseg_oracle.segment's result)"""
    import flow_oracle
    import flowcrf_oracle
    import flowseg_oracle
    K, frames, kps = make(W, H)
    cam = (F32(K["fx"]), F32(K["fy"]), F32(K["cx"]), F32(K["cy"]))
    flow = flow_oracle.pair(frames[frame - 1]["rgb"], frames[frame]["rgb"], flow_oracle.config())["flow"]
    xy0, xy1 = kps[frame - 1][0], kps[frame][0]

    def coords(xy, depth):
        z = depth[xy[:, 1], xy[:, 0]].astype(np.float64)
        return flowcrf_oracle.back_project(xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), z, cam)

    n = len(xy1)
    ts0 = np.full(n, 1000 + DT * (frame - 1), np.int64)
    tracks = dict(xy_cur=xy1, co_cur=coords(xy1, frames[frame]["depth"]), ts_cur=ts0 + DT, ok_cur=np.ones(n, np.int32),
                  xy_prev=xy0, co_prev=coords(xy0, frames[frame - 1]["depth"]), ts_prev=ts0, ok_prev=np.ones(n, np.int32))
    eye = [np.eye(4, dtype=F32)]
    cfg = flowcrf_oracle.config(**(crf or {}))
    r = flowcrf_oracle.infer(W, H, cam, [0], eye, eye, frames[frame - 1]["depth"][None], frames[frame]["depth"],
                             flow, flowcrf_oracle.motion_of(flow), tracks, True, 1, cfg)
    return r["ids"], flowseg_oracle.segment(r["ids"], frames[frame]["depth"], [0], True, 1)
