"""numpy restatement of the model database's arithmetic and files: the export of a model's stable surfels
(Core/Model/Model.cpp:1547-1594), `cloud.ply` (:1516-1537) and `tracks.ply` (:1386-1498 with descriptors, binary).  Test
infrastructure only: float32 operations in the stated order, the bytes of both files built from plain arrays."""
import struct

import numpy as np

DIM = 256
NO_KEYPOINT = 0xFFFFFFFF
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                        ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("radius", "<f4")])

CLOUD_PROPERTIES = ("property float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                    "property float nx\nproperty float ny\nproperty float nz\n"
                    "property float radius\n")


def f32(a):
    return np.asarray(a, np.float32)


def apply_pose(pose, xyz):
    """((p0 x + p1 y) + p2 z) + p3 per row p of the pose, every operation rounded to float32"""
    P, v = f32(pose).reshape(4, 4), f32(xyz).reshape(-1, 3)
    with np.errstate(all="ignore"):
        cols = [((P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2]) + P[r, 3] for r in range(3)]
    return np.stack(cols, 1).astype(np.float32)


def rotate_negated(pose, n):
    """-((r0 nx + r1 ny) + r2 nz) per row r of the pose's upper-left 3 x 3"""
    P, v = f32(pose).reshape(4, 4), f32(n).reshape(-1, 3)
    with np.errstate(all="ignore"):
        cols = [-((P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2]) for r in range(3)]
    return np.stack(cols, 1).astype(np.float32)


def export_cloud(surfels, pose, conf_threshold):
    """surfels [n,12] (Model.downloadMap's layout) -> the records of the surfels with conf > threshold, ascending"""
    s = f32(surfels).reshape(-1, 12)
    with np.errstate(invalid="ignore"):
        keep = s[:, 3] > np.float32(conf_threshold)  # strict: NaN is dropped
    s = s[keep]
    out = np.zeros(len(s), CLOUD_DTYPE)
    p, n = apply_pose(pose, s[:, 0:3]), rotate_negated(pose, s[:, 8:11])
    out["x"], out["y"], out["z"] = p[:, 0], p[:, 1], p[:, 2]
    c = s[:, 4].astype(np.int64)  # integer-valued floats in [0, 2^24)
    out["red"], out["green"], out["blue"] = (c >> 16) & 255, (c >> 8) & 255, c & 255
    out["nx"], out["ny"], out["nz"] = n[:, 0], n[:, 1], n[:, 2]
    out["radius"] = s[:, 11]
    return out


def cloud_header(n):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + CLOUD_PROPERTIES + "end_header\n").encode()


def cloud_bytes(records):
    r = np.ascontiguousarray(records, CLOUD_DTYPE).reshape(-1)
    return cloud_header(len(r)) + r.tobytes()


def records_equal(a, b):
    """bit for bit, except that a float component that is NaN in both counts as equal"""
    if a.shape != b.shape:
        return False
    for name in CLOUD_DTYPE.names:
        x, y = a[name], b[name]
        if x.dtype.kind == "f":
            same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            same = x == y
        if not same.all():
            return False
    return True


def tracks_header(vertices, tracks):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
            "property float32 x\nproperty float32 y\nproperty float32 z\nproperty list uint16 float32 descriptor\n"
            "element edge 0\nproperty uint32 vertex1\nproperty uint32 vertex2\n"
            "element track %d\nproperty list uint32 uint32 vertex_index\nend_header\n" % (vertices, tracks)).encode()


def tracks_bytes(views, pose):
    """views = [(descriptor [n,256], coordinate [n,3])] per time index.  Track t = row t of every view; vertices numbered track
    by track, then time index by time index; a vertex = pose * coordinate, uint16 256, the descriptor."""
    views = [(f32(d).reshape(-1, DIM), apply_pose(pose, f32(c).reshape(-1, 3))) for d, c in views]
    T = max([len(d) for d, _ in views], default=0)
    vert, trk, vid = [], [], 0
    for t in range(T):
        trk.append(struct.pack("<I", len(views)))
        for d, c in views:
            if t < len(d):
                vert.append(c[t].astype("<f4").tobytes() + struct.pack("<H", DIM) + d[t].astype("<f4").tobytes())
                trk.append(struct.pack("<I", vid))
                vid += 1
            else:
                trk.append(struct.pack("<I", NO_KEYPOINT))
    return tracks_header(vid, T) + b"".join(vert) + b"".join(trk)


def load_views(data):
    """Model::load (Model.cpp:1658-1691) on the bytes of a well-formed tracks.ply, then the views of its tracks: view i = the
    tracks with a keypoint at time index i, in track order"""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().split("\n")
    V = int([ln for ln in head if ln.startswith("element vertex")][0].split()[2])
    T = int([ln for ln in head if ln.startswith("element track")][0].split()[2])
    stride = 12 + 2 + 4 * DIM
    body = data[end:]
    verts = [(np.frombuffer(body, "<f4", DIM, v * stride + 14).copy(), np.frombuffer(body, "<f4", 3, v * stride).copy()) for v in range(V)]
    at, tracks = V * stride, []
    for _ in range(T):
        nk = struct.unpack_from("<I", body, at)[0]
        tracks.append(struct.unpack_from("<%dI" % nk, body, at + 4))
        at += 4 + 4 * nk
    assert at == len(body)
    n_views = len(tracks[0]) if tracks else 0
    out = []
    for i in range(n_views):
        ids = [t[i] for t in tracks if t[i] != NO_KEYPOINT]
        out.append((np.array([verts[k][0] for k in ids], np.float32).reshape(-1, DIM),
                    np.array([verts[k][1] for k in ids], np.float32).reshape(-1, 3)))
    return out


def make_views(counts, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        d = rng.normal(size=(n, DIM)).astype(np.float32)
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6).astype(np.float32)
        out.append((d, rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)))
    return out


def make_pose(seed):
    """a rotation that is no axis permutation, with a translation"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = q.astype(np.float32), rng.uniform(-2, 2, 3).astype(np.float32)
    return P
