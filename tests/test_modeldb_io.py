"""CPU: the files of the model database (csrc/modeldb_io.hpp through the C ABI) against tests/modeldb_oracle.py: cloud.ply and
tracks.ply byte for byte, the readers' round trips, and every malformed file refused with MMF_ERR_INVALID."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import modeldb_oracle as mo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
GUARD = 0xA5

CLOUD_HEADER_5 = (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\n"
                  b"property float x\nproperty float y\nproperty float z\n"
                  b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  b"property float nx\nproperty float ny\nproperty float nz\n"
                  b"property float radius\nend_header\n")


@pytest.fixture(scope="module")
def lib():
    from multimotionfusion_amd import _capi, build
    build.build(verbose=False)
    return _capi.load()


def some_records(n, seed=3):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, mo.CLOUD_DTYPE)
    for name in mo.CLOUD_DTYPE.names:
        r[name] = rng.integers(0, 256, n) if r[name].dtype.kind == "u" else rng.normal(size=n).astype(np.float32)
    return r


def read_cloud(lib, path, capacity):
    """-> (status, n, the destination: capacity records and a guard record behind them)"""
    buf = np.full((capacity + 1) * 31, GUARD, np.uint8)
    n = C.c_uint(12345)
    rc = lib.mmf_ply_read_cloud(str(path).encode(), buf.ctypes.data, capacity, C.byref(n))
    assert (buf[capacity * 31:] == GUARD).all(), "a write past capacity"
    return rc, n.value, buf


@pytest.mark.parametrize("n", [0, 1, 5])
def test_cloud_file_is_the_oracles_bytes_and_reads_back(lib, tmp_path, n):
    from multimotionfusion_amd import modeldb
    r = some_records(n)
    path = tmp_path / "cloud.ply"
    assert lib.mmf_ply_write_cloud(str(path).encode(), r.ctypes.data if n else None, n) == 0
    data = path.read_bytes()
    assert data == mo.cloud_bytes(r)
    if n == 5:
        assert data[:len(CLOUD_HEADER_5)] == CLOUD_HEADER_5 and len(data) == len(CLOUD_HEADER_5) + 5 * 31
    rc, got, buf = read_cloud(lib, path, n + 2)
    assert rc == 0 and got == n and buf[:n * 31].tobytes() == r.tobytes() and (buf[n * 31:] == GUARD).all()
    back = modeldb.readCloud(path)
    assert back.dtype == mo.CLOUD_DTYPE and back.tobytes() == r.tobytes()
    modeldb.writeCloud(tmp_path / "again.ply", back)
    assert (tmp_path / "again.ply").read_bytes() == data


def test_cloud_reader_refuses_what_is_not_exactly_the_file(lib, tmp_path):
    r = some_records(5)
    good = mo.cloud_bytes(r)
    bad = {
        "short": good[:-1],
        "long": good + b"\0",
        "count": good.replace(b"element vertex 5\n", b"element vertex 6\n"),
        "property": good.replace(b"property uchar green", b"property uchar greem"),
        "ascii": good.replace(b"binary_little_endian", b"ascii"),
        "empty": b"",
        "huge": good.replace(b"element vertex 5\n", b"element vertex 4294967295\n"),
        "overflow": good.replace(b"element vertex 5\n", b"element vertex 99999999999\n"),
    }
    for name, data in bad.items():
        path = tmp_path / (name + ".ply")
        path.write_bytes(data)
        rc, _, buf = read_cloud(lib, path, 8)
        assert rc == INVALID and (buf == GUARD).all(), name
        assert b"mmf_ply_read_cloud" in lib.mmf_last_error(), name
    path = tmp_path / "good.ply"
    path.write_bytes(good)
    rc, n, buf = read_cloud(lib, path, 4)  # capacity < n
    assert rc == INVALID and n == 5 and (buf == GUARD).all()
    rc, n, buf = read_cloud(lib, path, 5)
    assert rc == 0 and n == 5
    assert read_cloud(lib, tmp_path / "missing.ply", 4)[0] == INVALID


def write_tracks(lib, path, views, pose):
    from multimotionfusion_amd import modeldb
    modeldb.writeTracks(path, views, pose)
    return path.read_bytes()


def read_tracks(lib, path, cap_views, cap_rows):
    counts = np.full(cap_views + 1, -77, np.int32)
    desc = np.full((cap_rows + 1, mo.DIM), np.float32(-77), np.float32)
    coord = np.full((cap_rows + 1, 3), np.float32(-77), np.float32)
    nv, nr = C.c_int(-1), C.c_int(-1)
    rc = lib.mmf_tracks_ply_read(str(path).encode(), cap_views, C.byref(nv), counts.ctypes.data, cap_rows, C.byref(nr),
                                 desc.ctypes.data, coord.ctypes.data)
    assert counts[cap_views] == -77 and (desc[cap_rows] == -77).all() and (coord[cap_rows] == -77).all(), "a write past capacity"
    return rc, nv.value, nr.value, counts, desc, coord


@pytest.mark.parametrize("counts", [[3, 0, 5], [4], [0, 0, 0], []])
def test_tracks_file_is_the_oracles_bytes_and_reads_back(lib, tmp_path, counts):
    """A file without tracks (every view empty, or no view) has nowhere to say how many views there were: it reads back as no
    views at all -- as Model::load leaves tracks_local empty.  Every other case reads back counts and rows bit for bit."""
    from multimotionfusion_amd import modeldb
    views, pose = mo.make_views(counts, seed=7), mo.make_pose(5)
    path = tmp_path / "tracks.ply"
    data = write_tracks(lib, path, views, pose)
    assert data == mo.tracks_bytes(views, pose)
    want = mo.load_views(data)
    if max(counts, default=0) == 0:
        assert want == [] and data == mo.tracks_header(0, 0)
    else:
        assert [len(d) for d, _ in want] == counts
        for (d, c), (d0, c0) in zip(want, views):  # the oracle's reader against what went in
            assert np.array_equal(d, d0) and np.array_equal(c.view(np.uint32), mo.apply_pose(pose, c0).view(np.uint32))
    nv, nr = C.c_int(-1), C.c_int(-1)
    assert lib.mmf_tracks_ply_read(str(path).encode(), 0, C.byref(nv), None, 0, C.byref(nr), None, None) == 0  # sizes only
    assert nv.value == len(want) and nr.value == sum(len(d) for d, _ in want)
    rc, n_views, n_rows, got_counts, desc, coord = read_tracks(lib, path, nv.value + 1, nr.value + 2)
    assert rc == 0 and n_views == len(want) and list(got_counts[:n_views]) == [len(d) for d, _ in want]
    o = 0
    for d, c in want:
        assert np.array_equal(desc[o:o + len(d)].view(np.uint32), d.view(np.uint32))
        assert np.array_equal(coord[o:o + len(d)].view(np.uint32), c.view(np.uint32))
        o += len(d)
    assert o == n_rows
    back = modeldb.readTracks(path)
    assert len(back) == len(want) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(back, want))
    if nr.value:  # too small a destination is refused, untouched
        assert read_tracks(lib, path, nv.value - 1, nr.value)[0] == INVALID
        rc, _, _, _, desc, coord = read_tracks(lib, path, nv.value, nr.value - 1)
        assert rc == INVALID and (desc == -77).all() and (coord == -77).all()
    # identity pose: the coordinates come back as they went in
    data_id = write_tracks(lib, tmp_path / "identity.ply", views, np.eye(4, dtype=np.float32))
    for (d, c), (d0, c0) in zip(mo.load_views(data_id), views):
        assert np.array_equal(c, c0) and np.array_equal(d, d0)


def test_tracks_reader_refuses_malformed_files(lib, tmp_path):
    views, pose = mo.make_views([3, 0, 5], seed=9), mo.make_pose(2)
    good = bytearray(mo.tracks_bytes(views, pose))
    hdr = len(mo.tracks_header(8, 5))
    stride = 12 + 2 + 4 * mo.DIM
    tracks_at = hdr + 8 * stride

    def patched(at, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    bad = {
        "descriptor_255": patched(hdr + 2 * stride + 12, "<H", 255),
        "descriptor_257": patched(hdr + 12, "<H", 257),
        "descriptor_huge": patched(hdr + 12, "<H", 65535),
        "track_len_2": patched(tracks_at + 16, "<I", 2),
        "track_len_4": patched(tracks_at, "<I", 4),
        "track_len_huge": patched(tracks_at, "<I", 0xFFFFFFF0),
        "index_V": patched(tracks_at + 4, "<I", 8),
        "index_big": patched(tracks_at + 4, "<I", 0xFFFFFFFE),
        "cut_descriptor": bytes(good[:hdr + 3 * stride + 500]),
        "cut_vertex": bytes(good[:hdr + 3 * stride + 6]),
        "cut_track": bytes(good[:tracks_at + 16 + 6]),
        "cut_track_length": bytes(good[:tracks_at + 2]),
        "one_short": bytes(good[:-1]),
        "trailing": bytes(good) + b"\0",
        "more_vertices": bytes(good).replace(b"element vertex 8\n", b"element vertex 9\n"),
        "vertices_huge": bytes(good).replace(b"element vertex 8\n", b"element vertex 4294967295\n"),
        "more_tracks": bytes(good).replace(b"element track 5\n", b"element track 6\n"),
        "edges": bytes(good).replace(b"element edge 0\n", b"element edge 1\n"),
        "no_descriptor": bytes(good).replace(b"property list uint16 float32 descriptor\n", b""),
        "empty": b"",
    }
    for name, data in bad.items():
        path = tmp_path / (name + ".ply")
        path.write_bytes(data)
        rc, _, _, counts, desc, coord = read_tracks(lib, path, 3, 8)
        assert rc == INVALID, name
        assert (desc == -77).all() and (coord == -77).all(), name
        assert b"mmf_tracks_ply_read" in lib.mmf_last_error(), name
        nv, nr = C.c_int(), C.c_int()
        assert lib.mmf_tracks_ply_read(str(path).encode(), 0, C.byref(nv), None, 0, C.byref(nr), None, None) == INVALID, name
    path = tmp_path / "good.ply"
    path.write_bytes(bytes(good))
    assert read_tracks(lib, path, 3, 8)[0] == 0


def test_modeldb_io_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/modeldb_io_sanitized.cpp: host code only, its own main, built with -fsanitize=address,undefined and run
    directly.  It writes and reads both files (the round trips above) and feeds the readers the malformed files, into
    destinations allocated at exactly their capacity."""
    exe = tmp_path / "modeldb_io_sanitized"
    src = os.path.join(REPO, "tests", "cpp", "modeldb_io_sanitized.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    assert out.stdout.strip().startswith("ok ") and out.stderr == "", (out.stdout, out.stderr)
