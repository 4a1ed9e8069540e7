"""The files of the model database through the C ABI (csrc/modeldb_io.hpp): `cloud.ply`, a model's stable surfels as
Model::exportModelPLY writes them (Core/Model/Model.cpp:1510-1598), and `tracks.ply`, its keypoint views in the layout
Model::load reads (:1386-1498, :1658-1691).  Host code in libmmf_hip.so; no device is touched."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, fptr

DIM = 256
# one record of cloud.ply / Model.exportCloud: 31 packed little-endian bytes
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                        ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("radius", "<f4")])
assert CLOUD_DTYPE.itemsize == 31


def writeCloud(path, records):
    r = np.ascontiguousarray(records, CLOUD_DTYPE).reshape(-1)
    check(_capi.load().mmf_ply_write_cloud(str(path).encode(), r.ctypes.data if r.size else None, r.size))


def readCloud(path):
    lib = _capi.load()
    n = C.c_uint()
    lib.mmf_ply_read_cloud(str(path).encode(), None, 0, C.byref(n))  # the count (the status speaks of the capacity)
    out = np.zeros(max(n.value, 1), CLOUD_DTYPE)
    check(lib.mmf_ply_read_cloud(str(path).encode(), out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]


def _pack(views):
    counts = np.array([len(d) for d, _ in views], np.int32)
    total = int(counts.sum())
    desc, coord = np.zeros((total, DIM), np.float32), np.zeros((total, 3), np.float32)
    o = 0
    for d, c in views:
        n = len(d)
        if n:
            desc[o:o + n], coord[o:o + n] = np.asarray(d, np.float32).reshape(n, DIM), np.asarray(c, np.float32).reshape(n, 3)
        o += n
    return counts, desc, coord


def writeTracks(path, views, pose=None):
    """views = [(descriptor [n,256], coordinate [n,3])] per time index (redetection.ViewStore's form); every coordinate is
    written as pose * coordinate"""
    counts, desc, coord = _pack(views)
    p = np.ascontiguousarray(np.eye(4) if pose is None else pose, np.float32).reshape(16)
    check(_capi.load().mmf_tracks_ply_write(str(path).encode(), len(views), counts.ctypes.data, desc.ctypes.data, coord.ctypes.data,
                                            fptr(p)))


def readTracks(path):
    """-> the views Model::load rebuilds from the file, [(descriptor [n,256], coordinate [n,3])]"""
    lib = _capi.load()
    nv, nr = C.c_int(), C.c_int()
    check(lib.mmf_tracks_ply_read(str(path).encode(), 0, C.byref(nv), None, 0, C.byref(nr), None, None))
    counts = np.zeros(max(nv.value, 1), np.int32)
    desc, coord = np.zeros((max(nr.value, 1), DIM), np.float32), np.zeros((max(nr.value, 1), 3), np.float32)
    check(lib.mmf_tracks_ply_read(str(path).encode(), nv.value, C.byref(nv), counts.ctypes.data, nr.value, C.byref(nr),
                                  desc.ctypes.data, coord.ctypes.data))
    out, o = [], 0
    for n in counts[: nv.value]:
        out.append((desc[o:o + n].copy(), coord[o:o + n].copy()))
        o += int(n)
    return out
