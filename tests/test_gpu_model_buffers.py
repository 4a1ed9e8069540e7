"""The layout of a surfel model's slab, as mmf_model_texture and mmf_model_surfel_arrays show it: byte counts and offsets.

The slab's buffers are carved in one order, each rounded up to 256 bytes; the offsets expected here are worked out from that
order alone, written down below, not read from the library.  Allocation only, but for the four tiny launches that copy the
(transposed) index-map images row-major into the export area when mmf_model_texture is asked for them.
"""
import ctypes as C

import pytest

from multimotionfusion_amd import _capi
from multimotionfusion_amd.model import Model

pytestmark = pytest.mark.gpu

ALIGN = 256
MMF_ERR_INVALID = -1

# The carve order: (key, bytes per surfel of capacity, bytes per pixel, bytes per 256 surfels + pixels, fixed bytes).
# A key in TEXTURES is the name mmf_model_texture knows the buffer by; in EXPORTED it is handed out as a copy inside "export".
SOA = ["pos", "col", "nrm"]
CARVE = ([("set0." + k, 16, 0, 0, 0) for k in SOA] + [("set1." + k, 16, 0, 0, 0) for k in SOA]
         + [("meas." + k, 0, 16, 0, 0) for k in SOA] + [("cand2." + k, 0, 16, 0, 0) for k in SOA]
         + [("flags_a", 4, 4, 0, 0), ("flags_b", 0, 4, 0, 0), ("prefix_a", 4, 4, 0, 0), ("prefix_b", 0, 4, 0, 0),
            ("block_sums", 0, 0, 4, 8), ("totals", 0, 0, 0, 64), ("winner", 4, 0, 0, 0), ("conf_time", 8, 8, 0, 0),
            ("keys", 0, 8, 0, 0), ("rays", 0, 16, 0, 0),
            ("index", 0, 4, 0, 0), ("vertConf", 0, 16, 0, 0), ("colorTime", 0, 16, 0, 0), ("normRad", 0, 16, 0, 0),
            ("image", 0, 4, 0, 0), ("vertexConf", 0, 16, 0, 0), ("normalRadius", 0, 16, 0, 0), ("time", 0, 2, 0, 0),
            ("depth", 0, 4, 0, 0), ("export", 0, 52, 0, 0),
            ("fillVertex", 0, 16, 0, 0), ("fillNormal", 0, 16, 0, 0), ("fillImage", 0, 4, 0, 0)])
EXPORTED = ["index", "vertConf", "colorTime", "normRad"]  # in the export area one behind the other, unrounded
TEXTURES = EXPORTED + ["image", "vertexConf", "normalRadius", "time", "depth", "fillVertex", "fillNormal", "fillImage"]

SIZES = [(32, 32),    # the smallest the constructor takes
         (36, 44),    # npix * 2 and npix * 4 are no multiples of the alignment: the roundings show
         (640, 480)]
CAPACITIES = [1000,   # 1000 * 16 bytes is ragged against the alignment: the store arrays' spacing shows the rounding
              4096]


def _up(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def _expected(width, height, cap):
    """{key: (offset from set0.pos, bytes)} for every buffer of the carve order."""
    npix, out, off = width * height, {}, 0
    for key, per_surfel, per_pixel, per_block, fixed in CARVE:
        nbytes = per_surfel * cap + per_pixel * npix + per_block * ((cap + npix) // 256) + fixed
        out[key] = (off, nbytes)
        off = _up(off + nbytes)
    return out


def _texture(model, name):
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    _capi.check(model.ctx.lib.mmf_model_texture(model.handle, name.encode(), C.byref(ptr), C.byref(nbytes)))
    return ptr.value, nbytes.value


def _surfel_arrays(model):
    pos, col, nrm, count = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint()
    _capi.check(model.ctx.lib.mmf_model_surfel_arrays(model.handle, C.byref(pos), C.byref(col), C.byref(nrm), C.byref(count)))
    assert count.value == 0
    return pos.value, col.value, nrm.value


@pytest.fixture(params=[(w, h, cap) for w, h in SIZES for cap in CAPACITIES], ids=lambda p: "%dx%d-%d" % p)
def model(request, gpu_ctx):
    w, h, cap = request.param
    m = Model(gpu_ctx, w, h, w / 2.0, h / 2.0, 1.1 * w, 1.1 * w, max_surfels=cap)
    m.capacity = cap
    yield m
    m.close()  # (waits for the export launches)


def test_byte_counts(model):
    expected = _expected(model.width, model.height, model.capacity)
    assert len(TEXTURES) == 12
    for name in TEXTURES:
        assert _texture(model, name)[1] == expected[name][1], name
    assert expected["export"][1] == sum(expected[name][1] for name in EXPORTED)


def test_store_spacing(model):
    expected = _expected(model.width, model.height, model.capacity)
    pos, col, nrm = _surfel_arrays(model)  # (a fresh model: the first of the two stores)
    assert pos % ALIGN == 0
    assert col - pos == expected["set0.col"][0] == _up(model.capacity * 16)
    assert nrm - pos == expected["set0.nrm"][0] == 2 * _up(model.capacity * 16)


def test_texture_offsets(model):
    expected = _expected(model.width, model.height, model.capacity)
    pos = _surfel_arrays(model)[0]
    inside = 0  # of the export area
    for name in TEXTURES:
        at = _texture(model, name)[0] - pos
        if name in EXPORTED:
            assert at == expected["export"][0] + inside, name
            inside += expected[name][1]
        else:
            assert at == expected[name][0], name
            assert at % ALIGN == 0, name
    assert expected["export"][0] % ALIGN == 0


def test_unknown_name(model):
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    rc = model.ctx.lib.mmf_model_texture(model.handle, b"flags_a", C.byref(ptr), C.byref(nbytes))
    assert rc == MMF_ERR_INVALID
    assert "flags_a" in model.ctx.lib.mmf_last_error().decode()
    with pytest.raises(_capi.MmfError, match="no_such_texture"):
        _texture(model, "no_such_texture")
