"""The layout of an odometry's slab, as mmf_odom_buffer shows it: names, byte counts and offsets.

Batched chains address model m at slab(m) - slab(0), and several launch paths are chosen by pointer alignment, so the
order of the buffers, the 256-byte rounding of each and their sizes are part of what the library computes.  The offsets
expected here are worked out from that order alone.  Allocation only: no kernel runs.
"""
import ctypes as C

import pytest

from multimotionfusion_amd import _capi
from multimotionfusion_amd._capi import MMF_NUM_PYRS, MmfError
from multimotionfusion_amd.odometry import RGBDOdometry

pytestmark = pytest.mark.gpu

ALIGN = 256
DATATERM = C.sizeof(_capi.mmf_dataterm)
EXTENT_BYTES = 20 * 8  # extent.hpp: kExtentWords 64-bit words
MMF_ERR_INVALID = -1

# The carve order of one pyramid level: (name mmf_odom_buffer knows it by or None, bytes per pixel).
PER_LEVEL = [("vmaps_g_prev", 12), ("nmaps_g_prev", 12), ("vmaps_curr", 12), ("nmaps_curr", 12),
             ("last_depth", 4), ("next_depth", 4), ("depth_pyr", 4),
             ("last_image", 1), ("next_image", 1), ("last_next_image", 1),
             ("dIdx", 2), ("dIdy", 2), (None, 2), (None, 2),  # (the write side of the double-buffered gradients)
             ("cloud", 12), ("cloud4", 16), ("corres", DATATERM), ("prev_packed", 24)]
SINGLE = ["icp_error", "rgb_error", "extent", "prep_box"]

SIZES = [(32, 32),    # the smallest the constructor takes: level 2 is 8 x 8, its 64-byte images are below the alignment
         (36, 44),    # level 2 is 9 x 11: ragged against the alignment
         (640, 480)]


def _up(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def _buffer(odom, name, level=0):
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    _capi.check(odom.ctx.lib.mmf_odom_buffer(odom.handle, name.encode(), level, C.byref(ptr), C.byref(nbytes)))
    return ptr.value, nbytes.value


def _expected(width, height):
    """{(name, level): (offset from vmaps_g_prev level 0, bytes)} and the offset behind prev_packed level 2."""
    out, off = {}, 0
    for level in range(MMF_NUM_PYRS):
        n = (width >> level) * (height >> level)
        for name, per_px in PER_LEVEL:
            if name:
                out[(name, level)] = (off, n * per_px)
            off = _up(off + n * per_px)
    return out, off


@pytest.fixture(params=SIZES, ids=lambda s: "%dx%d" % s)
def odom(request, gpu_ctx):
    w, h = request.param
    o = RGBDOdometry(gpu_ctx, w, h, w / 2.0, h / 2.0, 1.1 * w, 1.1 * w)
    yield o
    o.close()


def test_names_and_byte_counts(odom):
    expected, _ = _expected(odom.width, odom.height)
    assert len({name for name, _ in expected}) + len(SINGLE) == 20
    for (name, level), (_, nbytes) in expected.items():
        assert _buffer(odom, name, level)[1] == nbytes, (name, level)
    image = odom.width * odom.height * 4
    for level in range(MMF_NUM_PYRS):  # `level` is ignored for the single buffers
        assert _buffer(odom, "icp_error", level)[1] == image
        assert _buffer(odom, "rgb_error", level)[1] == image
        assert _buffer(odom, "extent", level)[1] == EXTENT_BYTES
        assert _buffer(odom, "prep_box", level)[1] == 8 * 4


def test_per_level_offsets(odom):
    expected, _ = _expected(odom.width, odom.height)
    base = _buffer(odom, "vmaps_g_prev", 0)[0]
    assert base % ALIGN == 0
    for (name, level), (off, _) in expected.items():
        assert _buffer(odom, name, level)[0] - base == off, (name, level)


def test_single_buffers(odom):
    _, end = _expected(odom.width, odom.height)
    base = _buffer(odom, "vmaps_g_prev", 0)[0]
    image = odom.width * odom.height * 4
    at = {name: _buffer(odom, name)[0] - base for name in SINGLE}
    for name in ("icp_error", "rgb_error", "extent"):
        assert at[name] >= end, name
        assert at[name] % ALIGN == 0, name
    assert at["prep_box"] >= end
    assert at["rgb_error"] - at["icp_error"] == _up(image)
    assert at["extent"] > at["rgb_error"]
    assert at["prep_box"] - at["extent"] == EXTENT_BYTES


def test_unknown_name(odom):
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    rc = odom.ctx.lib.mmf_odom_buffer(odom.handle, b"grad_w_dx", 0, C.byref(ptr), C.byref(nbytes))
    assert rc == MMF_ERR_INVALID
    assert "grad_w_dx" in odom.ctx.lib.mmf_last_error().decode()
    with pytest.raises(MmfError, match="no_such_buffer"):
        _buffer(odom, "no_such_buffer")
