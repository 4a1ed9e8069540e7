// superpoint_f16_host.hpp -- host side of the f16 forward pass (included by superpoint_host.hpp): the f16 rounding,
// the weight packing and the launches of superpoint_f16_kernels.hpp.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "superpoint_f16_kernels.hpp"

namespace mmf {

// f32 -> f16 bits, round to nearest, ties to even; overflow (|x| >= 65520) to inf, NaN kept (payload's top bits, never
// turned into inf), results below 2^-14 subnormal.  The rounding of the packer and of mmf_f16_round.
static inline uint16_t sp_f16_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    uint32_t a = x & 0x7fffffffu;
    if (a > 0x7f800000u) {  // NaN
        uint16_t r = (uint16_t)(0x7c00u + ((a & 0x007fffffu) >> 13));
        if (r == 0x7c00u) r = 0x7c01u;
        return sign | r;
    }
    if (a >= 0x477ff000u) return sign | 0x7c00u;  // 65520 = the midpoint of 65504 and 2^16, tie to even = inf
    if (a < 0x38800000u) {                        // below 2^-14: a multiple of 2^-24, 1024 = the smallest normal
        float m;
        std::memcpy(&m, &a, 4);
        return sign | (uint16_t)std::nearbyintf(m * 16777216.0f);  // the product is exact; default rounding = to even
    }
    a += 0xfffu + ((a >> 13) & 1u);
    return sign | (uint16_t)((a - 0x38000000u) >> 13);
}

static inline bool sp_f16_finite(float f) { return std::isfinite(f) && std::fabs(f) < 65520.0f; }

// packed order = the order the lanes of sp_conv_f16_kernel read: [z][step][half][t][kh][n][j] with
// step = block * taps + tap, input channel = 32*block + 16*half + 8*kh + j, output channel = (z*nt + t)*32 + n
static std::vector<uint16_t> sp_pack_weights_f16(const float* w, int cin, int cout, int taps, int nt) {
    const int chunks = cin / kSpKBlock, steps = chunks * taps, zt = (cout + 32 * nt - 1) / (32 * nt);
    std::vector<uint16_t> out((size_t)zt * steps * 2 * nt * 512, 0);
    for (int z = 0; z < zt; ++z)
        for (int chunk = 0; chunk < chunks; ++chunk)
            for (int tap = 0; tap < taps; ++tap)
                for (int half = 0; half < 2; ++half)
                    for (int t = 0; t < nt; ++t)
                        for (int kh = 0; kh < 2; ++kh)
                            for (int n = 0; n < 32; ++n)
                                for (int j = 0; j < 8; ++j) {
                                    const int ci = 32 * chunk + 16 * half + 8 * kh + j, co = (z * nt + t) * 32 + n;
                                    if (co >= cout) continue;
                                    const size_t idx =
                                        ((((((size_t)z * steps + chunk * taps + tap) * 2 + half) * nt + t) * 2 + kh) * 32 + n) * 8 + j;
                                    out[idx] = sp_f16_bits(w[((size_t)co * cin + ci) * taps + tap]);
                                }
    return out;
}

template <int NT, bool OUTF32>
static void sp_launch_f16_nt(hipStream_t s, dim3 grid, int taps, bool pool, const SpConvArgsH& a) {
    if (taps == 9 && pool)
        hipLaunchKernelGGL((sp_conv_f16_kernel<NT, 9, true, OUTF32>), grid, dim3(256), 0, s, a);
    else if (taps == 9)
        hipLaunchKernelGGL((sp_conv_f16_kernel<NT, 9, false, OUTF32>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((sp_conv_f16_kernel<NT, 1, false, OUTF32>), grid, dim3(256), 0, s, a);
}

static SpConvArgsH sp_conv_args_f16(const SpLayer& L, const _Float16* in, int in_stride, void* out, int out_stride, int H, int W) {
    SpConvArgsH a;
    a.in = in, a.wpack = reinterpret_cast<const _Float16*>(L.wpack16), a.bias = L.bias, a.out = out;
    a.in_stride = in_stride, a.out_stride = out_stride;
    a.H = H, a.W = W, a.cin = L.cin, a.cout = L.cout, a.relu = L.relu ? 1 : 0;
    return a;
}

template <bool OUTF32>
static void sp_launch_conv_f16_as(hipStream_t s, const SpLayer& L, const SpConvArgsH& a) {
    const dim3 grid((a.W + kSpTileW - 1) / kSpTileW, (a.H + kSpTileH - 1) / kSpTileH, (L.cout + 32 * L.nt - 1) / (32 * L.nt));
    if (L.nt == 4)
        sp_launch_f16_nt<4, OUTF32>(s, grid, L.taps, L.pool, a);
    else if (L.nt == 2)
        sp_launch_f16_nt<2, OUTF32>(s, grid, L.taps, L.pool, a);
    else
        sp_launch_f16_nt<1, OUTF32>(s, grid, L.taps, L.pool, a);
}

static void sp_launch_conv_f16(hipStream_t s, const SpLayer& L, const _Float16* in, int in_stride, void* out, int out_stride, int H,
                               int W, bool out_f32) {
    const SpConvArgsH a = sp_conv_args_f16(L, in, in_stride, out, out_stride, H, W);
    if (out_f32)
        sp_launch_conv_f16_as<true>(s, L, a);
    else
        sp_launch_conv_f16_as<false>(s, L, a);
}

// the two 1x1 heads (both NT = 1, no ReLU, same image, f32 out) as one launch
static void sp_launch_head_pair_f16(hipStream_t s, const SpConvArgsH& a, const SpConvArgsH& b) {
    SpConvPairH q;
    q.a = a, q.b = b, q.za = (a.cout + 31) / 32;
    const dim3 grid((a.W + kSpTileW - 1) / kSpTileW, (a.H + kSpTileH - 1) / kSpTileH, q.za + (b.cout + 31) / 32);
    hipLaunchKernelGGL(sp_conv_f16_pair_kernel, grid, dim3(256), 0, s, q);
}

}  // namespace mmf

extern "C" int mmf_f16_round(const float* src, size_t n, uint16_t* dst) {
    MMF_REQUIRE((src && dst) || n == 0, "mmf_f16_round: null argument");
    for (size_t k = 0; k < n; ++k) dst[k] = mmf::sp_f16_bits(src[k]);
    return MMF_OK;
}
