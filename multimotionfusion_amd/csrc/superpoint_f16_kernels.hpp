// superpoint_f16_kernels.hpp -- the f16 forward pass of the SuperPoint network on gfx950 (MMF_SP_F16).
//
// The implicit GEMM of superpoint_kernels.hpp with f16 operands and f32 accumulation on
// v_mfma_f32_32x32x16_f16 (1/16 of the f32 instruction's cycles per multiply-add).  What carries over: the 8 x 16
// pixel tile per four-wave workgroup, wave w owning rows 2w, 2w+1 as eight 2x2 blocks (MFMA row = 4*block + 2*dy + dx,
// so the pool is a 4-way max in the epilogue), K blocks of 32 input channels x taps, weights pre-packed on the host
// in the order the lanes consume them and streamed from L2/L1 into registers a few MFMA groups ahead.  What differs:
//   * activations are f16 channels-last; a lane's A operand of one MFMA is eight consecutive channels of its pixel
//     (k = 8*(lane>>5) + j), one ds_read_b128.  An LDS pixel is 5 x 16 B (32 f16 + 16 B pad), a halo row 104 x 16 B
//     (18 pixels = 90 used; 104 = 8 mod 16): the 16 lanes of every b128 group (rows {0-3,12-15,20-27} or the rest)
//     then hit 16 distinct 16-byte slots.  The halo is 16.6 KB and there are two of them: the next K block is stored
//     while this one is read, one barrier per K block;
//   * one MFMA group is (tap, 16-channel half): NT MFMAs, one per output tile;
//   * the arithmetic: ONE f32 accumulator per output, walked over K blocks, taps and the two
//     16-channel halves of a block, each ascending -- the same for every NT, z slice and for the paired head launch;
//     what the instruction does inside its 16 products is the hardware's.  Then + bias (f32), ReLU, the 2x2 maximum
//     (NaN kept), and one round-to-nearest-even conversion to f16 (v_cvt_f16_f32: overflow to inf) -- or, for the
//     two 1x1 heads, the f32 value as it is.
#pragma once
#include "superpoint_kernels.hpp"

namespace mmf {

typedef _Float16 sp_f16x8 __attribute__((ext_vector_type(8)));

constexpr int kSpHPixU = 5;    // 16-byte units per LDS pixel (32 f16 + 16 B pad)
constexpr int kSpHRowU = 104;  // 16-byte units per halo row (18 pixels use 90; 104 = 8 mod 16)

struct SpConvArgsH {
    const _Float16* in;     // [H][W][in_stride], first `cin` channels used
    const _Float16* wpack;  // packed f16 weights (sp_pack_weights_f16 on the host)
    const float* bias;      // [cout]
    void* out;              // [H or H/2][W or W/2][out_stride], f16 or f32
    int in_stride, out_stride;
    int H, W, cin, cout;
    int relu;
};

// NaN-keeping maximum (a > b is false for either NaN: the plain select would drop a NaN in a)
__device__ __forceinline__ float sp_max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

template <int NT, int TAPS, bool POOL, bool OUTF32>
__device__ __forceinline__ void sp_conv_f16_body(const SpConvArgsH& p, const int z) {
    constexpr int HALO = TAPS == 9 ? 1 : 0;
    constexpr int HR = kSpTileH + 2 * HALO, HC = kSpTileW + 2 * HALO;
    constexpr int UNITS = HR * HC * 4;  // (pixel, 8-channel group) staging units of one K block, 16 B each
    constexpr int UPT = (UNITS + 255) / 256;
    constexpr int GROUPS = TAPS * 2;  // MFMA groups (16 channels of one tap) per K block
    constexpr int IMG = HR * kSpHRowU;
    // operand rings: a group is NT MFMAs = 32 NT cycles, so the narrower the output tile, the more groups ahead its
    // weights (RB - 1 groups) and its LDS reads (RA - 1 groups) are issued -- about 256 and 128 cycles for every NT.
    // RA divides GROUPS; where RB does not (the 1x1 layers) the ring is rotated back at the end of a K block
    constexpr int RB = TAPS == 9 ? (NT == 1 ? 9 : NT == 2 ? 6 : 3) : 3;
    constexpr int RA = TAPS == 9 ? (NT == 1 ? 6 : NT == 2 ? 3 : 2) : 2;
    static_assert(GROUPS % RA == 0, "the LDS read ring must divide a K block");
    __shared__ uint4 lds_a[2][IMG];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kSpTileW, y0 = blockIdx.y * kSpTileH;
    const int chunks = p.cin / kSpKBlock;
    const int last_group = chunks * GROUPS - 1;
    // this lane's weight operands: 16 B per (group, output tile), 1 KB contiguous per wave and load
    const uint4* __restrict__ wp = reinterpret_cast<const uint4*>(p.wpack) + (size_t)z * chunks * GROUPS * NT * 64 + lane;

    // staging addresses of this thread's units (the same for every K block, which only shifts the channel)
    int a_src[UPT], a_dst[UPT];
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
        const int u = tid + 256 * j;
        const int pix = u >> 2, q = u & 3;
        const int r = pix / HC, c = pix - r * HC;
        const int gy = y0 - HALO + r, gx = x0 - HALO + c;
        const bool inside = u < UNITS && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        a_src[j] = inside ? (gy * p.W + gx) * p.in_stride + 8 * q : -1;
        a_dst[j] = u < UNITS ? r * kSpHRowU + c * kSpHPixU + q : -1;
    }
    uint4 a_stage[UPT];
#define SP_LOAD_A(chunk)                                                                                        \
    _Pragma("unroll") for (int j = 0; j < UPT; ++j) {                                                           \
        a_stage[j] = make_uint4(0u, 0u, 0u, 0u);                                                                \
        if (a_src[j] >= 0) a_stage[j] = *reinterpret_cast<const uint4*>(p.in + a_src[j] + (chunk) * kSpKBlock); \
    }
#define SP_STORE_A(buf) \
    _Pragma("unroll") for (int j = 0; j < UPT; ++j) if (a_dst[j] >= 0) lds_a[buf][a_dst[j]] = a_stage[j];

    // MFMA row of this lane: i = 4*block + 2*dy + dx; the lane half kh supplies channels 8*kh .. 8*kh+7 of a half
    const int i = lane & 31, kh = lane >> 5;
    const int a_base = (2 * wave + ((i >> 1) & 1)) * kSpHRowU + (2 * (i >> 2) + (i & 1)) * kSpHPixU + kh;

    sp_f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

    uint4 b[RB][NT];
#pragma unroll
    for (int r = 0; r < RB - 1; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t) b[r][t] = wp[(size_t)(min(r, last_group) * NT + t) * 64];
    SP_LOAD_A(0);
    SP_STORE_A(0);
    __syncthreads();

    for (int chunk = 0; chunk < chunks; ++chunk) {
        const bool more = chunk + 1 < chunks;
        if (more) SP_LOAD_A(chunk + 1);  // lands during this block's MFMAs
        const uint4* la = lds_a[chunk & 1];
        uint4 a[RA];
#pragma unroll
        for (int r = 0; r < RA - 1; ++r) {
            const int tap = r >> 1, half = r & 1;
            a[r] = la[a_base + (TAPS == 9 ? (tap / 3) * kSpHRowU + (tap % 3) * kSpHPixU : 0) + 2 * half];
        }
#pragma unroll
        for (int q = 0; q < GROUPS; ++q) {
            const int gi = chunk * GROUPS + q;
            const int gn = min(gi + RB - 1, last_group);
#pragma unroll
            for (int t = 0; t < NT; ++t) b[(q + RB - 1) % RB][t] = wp[(size_t)(gn * NT + t) * 64];
            if (q + RA - 1 < GROUPS) {
                const int tap = (q + RA - 1) >> 1, half = (q + RA - 1) & 1;
                const int tap_off = TAPS == 9 ? (tap / 3) * kSpHRowU + (tap % 3) * kSpHPixU : 0;
                a[(q + RA - 1) % RA] = la[a_base + tap_off + 2 * half];
            }
            // the scheduling fences keep the operand loads above ahead of this group's MFMAs
            __builtin_amdgcn_sched_barrier(0);
            const sp_f16x8 av = __builtin_bit_cast(sp_f16x8, a[q % RA]);
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, __builtin_bit_cast(sp_f16x8, b[q % RB][t]), acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (GROUPS % RB != 0) {  // the group that is next sits in slot GROUPS % RB: bring it back to slot 0
            uint4 old[RB][NT];
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int t = 0; t < NT; ++t) old[r][t] = b[r][t];
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int t = 0; t < NT; ++t) b[r][t] = old[(r + GROUPS) % RB][t];
        }
        if (more) {
            SP_STORE_A((chunk + 1) & 1);  // the other halo: every wave left it before the previous barrier
            __syncthreads();
        }
    }
#undef SP_LOAD_A
#undef SP_STORE_A

    // epilogue: accumulator register v of lane (n, kh) is MFMA row (v&3) + 8*(v>>2) + 4*kh = pixel block
    // 2*(v>>2) + kh, (dy, dx) = ((v>>1)&1, v&1); column n = output channel (the layout does not depend on the dtype)
    _Float16* const out16 = static_cast<_Float16*>(p.out);
    float* const out32 = static_cast<float*>(p.out);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = (z * NT + t) * 32 + i;
        const bool co_ok = co < p.cout;
        const float bias = co_ok ? p.bias[co] : 0.f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            const int bx = 2 * blk + kh;
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = acc[t][4 * blk + k] + bias;
                if (p.relu) o[k] = o[k] < 0.f ? 0.f : o[k];
            }
            if (POOL) {
                const int py = (y0 >> 1) + wave, px = (x0 >> 1) + bx;
                const float m = sp_max_nan(sp_max_nan(o[0], o[1]), sp_max_nan(o[2], o[3]));
                if (co_ok && py < (p.H >> 1) && px < (p.W >> 1)) {
                    const size_t at = ((size_t)py * (p.W >> 1) + px) * p.out_stride + co;
                    if (OUTF32)
                        out32[at] = m;
                    else
                        out16[at] = (_Float16)m;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int oy = y0 + 2 * wave + (k >> 1), ox = x0 + 2 * bx + (k & 1);
                    if (co_ok && oy < p.H && ox < p.W) {
                        const size_t at = ((size_t)oy * p.W + ox) * p.out_stride + co;
                        if (OUTF32)
                            out32[at] = o[k];
                        else
                            out16[at] = (_Float16)o[k];
                    }
                }
            }
        }
    }
}

template <int NT, int TAPS, bool POOL, bool OUTF32>
__global__ __launch_bounds__(256) void sp_conv_f16_kernel(SpConvArgsH p) {
    sp_conv_f16_body<NT, TAPS, POOL, OUTF32>(p, blockIdx.z);
}

// the two 1x1 heads in one launch, as sp_conv_mfma_pair_kernel: f16 in, f32 out
struct SpConvPairH {
    SpConvArgsH a, b;
    int za;
};

__global__ __launch_bounds__(256) void sp_conv_f16_pair_kernel(SpConvPairH q) {
    if ((int)blockIdx.z < q.za)  // workgroup uniform
        sp_conv_f16_body<1, 1, false, true>(q.a, blockIdx.z);
    else
        sp_conv_f16_body<1, 1, false, true>(q.b, blockIdx.z - q.za);
}

// ---- conv1a with an f16 store: the arithmetic of sp_conv1a_kernel (grey conversion, one fmaf chain per output over
// the taps, + bias, ReLU) in f32 with f32 weights, rounded to nearest-even f16 when it is stored; four lanes per pixel,
// 16 output channels = 32 B each ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_conv1a_f16_kernel(const uint8_t* __restrict__ img, int channels, int H, int W,
                                                            const float* __restrict__ w_tap_co /* [9][64] */,
                                                            const float* __restrict__ bias, _Float16* __restrict__ out) {
    __shared__ float4 wl[9 * 16];
    if (threadIdx.x < 9 * 16) wl[threadIdx.x] = reinterpret_cast<const float4*>(w_tap_co)[threadIdx.x];
    __syncthreads();
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int pix = gid >> 2, q = gid & 3;
    if (pix >= H * W) return;
    const int y = pix / W, x = pix - y * W;
    float v[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
        v[tap] = inside ? sp_grey(img, (size_t)yy * W + xx, channels) : 0.f;
    }
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int c = 0; c < 16; c += 4) {
            const float4 w = wl[tap * 16 + 4 * q + (c >> 2)];
            acc[c] = fmaf(v[tap], w.x, acc[c]), acc[c + 1] = fmaf(v[tap], w.y, acc[c + 1]);
            acc[c + 2] = fmaf(v[tap], w.z, acc[c + 2]), acc[c + 3] = fmaf(v[tap], w.w, acc[c + 3]);
        }
    sp_f16x8* o = reinterpret_cast<sp_f16x8*>(out + (size_t)pix * 64 + 16 * q);
#pragma unroll
    for (int c = 0; c < 16; c += 8) {
        sp_f16x8 r;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float s = acc[c + k] + bias[16 * q + c + k];
            s = s < 0.f ? 0.f : s;
            r[k] = (_Float16)s;
        }
        o[c >> 3] = r;
    }
}

}  // namespace mmf
