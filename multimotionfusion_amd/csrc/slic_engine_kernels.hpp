// slic_engine_kernels.hpp -- the SLIC super-pixel engine on the device: what the reference gets from
// gSLICr every frame (Core/Segmentation/Slic.cpp:23-47, 72-80) in the variant its settings pick -- RGB colour space,
// GIVEN_SIZE, coh_weight 0.6, 5 iterations, no connectivity enforcement.  gSLICr's source is not in the reference tree;
// the arithmetic below follows the specification written down in DESIGN.md B5, and tests/slic_oracle.py restates the same
// text on the CPU.  Everything is float32 in the written order (this translation unit is built with -ffp-contract=off,
// sqrtf is correctly rounded: device_math.hpp) or integer, so the label image, the centres and the counts are bit exact
// against the oracle whatever the order the pixels are visited in:
//   * associate: one thread per four consecutive pixels; the nine candidate centres are read once per thread, all loads
//     ahead of the arithmetic, when the four pixels share a cell (the rule), scan order rows i = -1..1, columns
//     j = -1..1, strict `<`: first candidate wins a tie;
//   * update: GATHERED -- one workgroup per centre walks the 3S x 3S window its pixels lie in and reduces integer sums
//     (64 bit) over the workgroup: no atomics of any kind, no float sums, one conversion to float per total.
// Centres live in a workspace of eight floats each {x, y, c0, c1, c2, -, -, -}: two 16-byte loads per candidate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmf {

constexpr int kSlicCentreStride = 8;  // floats per centre in the workspace

struct SlicEngineGeom {
    int W, H, S, mx, my;  // mx = W / S, my = H / S (W % S == 0 and H % S == 0)
    float nc, nxy;        // colour and distance normalisers (mmf_slic_segment computes them once, in float32)
};

// centres_in == nullptr: centre k = cy * mx + cx at (cx S + S/2, cy S + S/2) with that pixel's colour; else a copy of
// centres_in [n][5].  counts start at 0.
__global__ __launch_bounds__(256) void slic_engine_init_kernel(SlicEngineGeom g, const uint8_t* __restrict__ rgb,
                                                               const float* __restrict__ centres_in,
                                                               float* __restrict__ centres, int* __restrict__ counts) {
    const int k = blockIdx.x * 256 + threadIdx.x, n = g.mx * g.my;
    if (k >= n) return;
    float v[5];
    if (centres_in != nullptr) {
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = centres_in[5 * k + q];
    } else {
        const int cy = k / g.mx, cx = k - cy * g.mx;
        const int x = cx * g.S + g.S / 2, y = cy * g.S + g.S / 2;  // inside the image: S divides W and H
        const uint8_t* px = rgb + ((size_t)y * g.W + x) * 3;
        v[0] = (float)x, v[1] = (float)y, v[2] = (float)px[0], v[3] = (float)px[1], v[4] = (float)px[2];
    }
    float4* out = reinterpret_cast<float4*>(centres + (size_t)k * kSlicCentreStride);
    out[0] = make_float4(v[0], v[1], v[2], v[3]);
    out[1] = make_float4(v[4], 0.f, 0.f, 0.f);
    counts[k] = 0;
}

struct SlicCentre {
    float x, y, c0, c1, c2;
};

__device__ __forceinline__ SlicCentre slic_engine_load_centre(const float* __restrict__ centres, int k) {
    const float4* p = reinterpret_cast<const float4*>(centres + (size_t)k * kSlicCentreStride);
    const float4 a = p[0], b = p[1];
    return SlicCentre{a.x, a.y, a.z, a.w, b.x};
}

// d = sqrtf(dcol nc + (0.6 dxy) nxy), every step rounded to float32 in this order
__device__ __forceinline__ float slic_engine_distance(const SlicCentre& k, float x, float y, float p0, float p1, float p2,
                                                      float nc, float nxy) {
    const float e0 = p0 - k.c0, e1 = p1 - k.c1, e2 = p2 - k.c2;
    const float dcol = e0 * e0 + e1 * e1 + e2 * e2;
    const float ex = x - k.x, ey = y - k.y;
    const float dxy = ex * ex + ey * ey;
    return sqrtf(dcol * nc + (0.6f * dxy) * nxy);
}

constexpr float kSlicEngineFar = 999999.9999f;

// One thread: the four pixels 4 t .. 4 t + 3 of the flattened image.  `vec`: rgb is 4-byte and labels 16-byte aligned
// (three dword loads, one 16-byte store); the last thread of an image whose size is not a multiple of four, and unaligned
// buffers, go pixel by pixel.
__global__ __launch_bounds__(256) void slic_engine_associate_kernel(SlicEngineGeom g, const uint8_t* __restrict__ rgb,
                                                                    const float* __restrict__ centres,
                                                                    int* __restrict__ labels, int vec) {
    const int npix = g.W * g.H;
    const int base = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (base >= npix) return;
    const int cnt = npix - base < 4 ? npix - base : 4;
    float p[4][3];
    if (vec && cnt == 4) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(rgb + (size_t)base * 3);
        const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
        p[0][0] = (float)(w0 & 255u), p[0][1] = (float)((w0 >> 8) & 255u), p[0][2] = (float)((w0 >> 16) & 255u);
        p[1][0] = (float)(w0 >> 24), p[1][1] = (float)(w1 & 255u), p[1][2] = (float)((w1 >> 8) & 255u);
        p[2][0] = (float)((w1 >> 16) & 255u), p[2][1] = (float)(w1 >> 24), p[2][2] = (float)(w2 & 255u);
        p[3][0] = (float)((w2 >> 8) & 255u), p[3][1] = (float)((w2 >> 16) & 255u), p[3][2] = (float)(w2 >> 24);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) p[q][ch] = q < cnt ? (float)rgb[(size_t)(base + q) * 3 + ch] : 0.f;
    }
    int px[4], py[4];
    py[0] = base / g.W, px[0] = base - py[0] * g.W;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        const bool wrap = px[q - 1] + 1 == g.W;
        px[q] = wrap ? 0 : px[q - 1] + 1, py[q] = py[q - 1] + (wrap ? 1 : 0);
    }
    float best[4] = {kSlicEngineFar, kSlicEngineFar, kSlicEngineFar, kSlicEngineFar};
    int lab[4] = {-1, -1, -1, -1};
    const int cx0 = px[0] / g.S, cy0 = py[0] / g.S;
    const bool shared = cnt == 4 && py[3] == py[0] && px[3] / g.S == cx0;
    if (shared) {  // the four pixels lie in one cell: nine candidates, each read once
        // every load is issued before the first distance (clamped indices; nine dependent L2 round trips otherwise)
        SlicCentre c[9];
        int ck[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            const int cy = cy0 + m / 3 - 1, cx = cx0 + m % 3 - 1;
            const bool inside = cy >= 0 && cy < g.my && cx >= 0 && cx < g.mx;
            ck[m] = inside ? cy * g.mx + cx : -1;
            c[m] = slic_engine_load_centre(centres, inside ? ck[m] : cy0 * g.mx + cx0);
        }
#pragma unroll
        for (int m = 0; m < 9; ++m) {  // scan order: rows i = m / 3 - 1, columns j = m % 3 - 1
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d = slic_engine_distance(c[m], (float)px[q], (float)py[q], p[q][0], p[q][1], p[q][2], g.nc, g.nxy);
                if (ck[m] >= 0 && d < best[q]) best[q] = d, lab[q] = ck[m];
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q >= cnt) continue;
            const int cxq = px[q] / g.S, cyq = py[q] / g.S;
            for (int i = -1; i <= 1; ++i) {
                const int cy = cyq + i;
                if (cy < 0 || cy >= g.my) continue;
                for (int j = -1; j <= 1; ++j) {
                    const int cx = cxq + j;
                    if (cx < 0 || cx >= g.mx) continue;
                    const int k = cy * g.mx + cx;
                    const SlicCentre c = slic_engine_load_centre(centres, k);
                    const float d = slic_engine_distance(c, (float)px[q], (float)py[q], p[q][0], p[q][1], p[q][2], g.nc, g.nxy);
                    if (d < best[q]) best[q] = d, lab[q] = k;
                }
            }
        }
    }
    // (a pixel whose nine distances are all NaN or beyond the start value -- centres handed in far away -- has no nearer
    // centre than its own cell's: the label stays inside [0, n))
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (lab[q] < 0) lab[q] = (py[q] / g.S) * g.mx + px[q] / g.S;
    if (vec && cnt == 4) {
        *reinterpret_cast<int4*>(labels + base) = make_int4(lab[0], lab[1], lab[2], lab[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < cnt) labels[base + q] = lab[q];
    }
}

__device__ __forceinline__ long long slic_engine_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// One workgroup per centre k: the pixels labelled k lie in the cells (cx - 1 .. cx + 1) x (cy - 1 .. cy + 1).  Integer
// sums of x, y and the three channels in 64 bits (585 225 pixels at S = 255 times a coordinate overflows 32), converted
// to float once and divided by (float)count; a centre without pixels keeps its values.
__global__ __launch_bounds__(256) void slic_engine_update_kernel(SlicEngineGeom g, const uint8_t* __restrict__ rgb,
                                                                 const int* __restrict__ labels,
                                                                 float* __restrict__ centres, int* __restrict__ counts) {
    const int k = blockIdx.x;  // grid = n
    const int cy = k / g.mx, cx = k - cy * g.mx;
    const int x0 = (cx > 0 ? cx - 1 : 0) * g.S, x1 = (cx + 2 < g.mx ? cx + 2 : g.mx) * g.S;
    const int y0 = (cy > 0 ? cy - 1 : 0) * g.S, y1 = (cy + 2 < g.my ? cy + 2 : g.my) * g.S;
    const int ww = x1 - x0, total = ww * (y1 - y0);
    long long s[5] = {0, 0, 0, 0, 0};
    long long cnt = 0;
    int wy = (int)threadIdx.x / ww, wx = (int)threadIdx.x - wy * ww;
    const int dy = 256 / ww, dx = 256 - dy * ww;  // the step of 256 window pixels, without a division per pixel
    for (int t = threadIdx.x; t < total; t += 4 * 256) {
        // four steps' labels are loaded before the first is looked at; the colours only where the label matches (runs of
        // a label: a wave's lanes agree almost everywhere)
        int lab[4];
        size_t at[4];
        int xs[4], ys[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            xs[u] = x0 + wx, ys[u] = y0 + wy;
            at[u] = (size_t)ys[u] * g.W + xs[u];
            lab[u] = t + u * 256 < total ? labels[at[u]] : -1;
            wx += dx, wy += dy;
            if (wx >= ww) wx -= ww, ++wy;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (lab[u] != k) continue;
            const uint8_t* px = rgb + at[u] * 3;
            s[0] += xs[u], s[1] += ys[u], s[2] += px[0], s[3] += px[1], s[4] += px[2];
            ++cnt;
        }
    }
    __shared__ long long part[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] = slic_engine_wave_sum(s[q]);
    cnt = slic_engine_wave_sum(cnt);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) part[wave][q] = s[q];
        part[wave][5] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) tot[q] = part[0][q] + part[1][q] + part[2][q] + part[3][q];
        counts[k] = (int)tot[5];
        if (tot[5] > 0) {
            const float c = (float)tot[5];
            float4* out = reinterpret_cast<float4*>(centres + (size_t)k * kSlicCentreStride);
            out[0] = make_float4((float)tot[0] / c, (float)tot[1] / c, (float)tot[2] / c, (float)tot[3] / c);
            out[1] = make_float4((float)tot[4] / c, 0.f, 0.f, 0.f);
        }
    }
}

// the workspace's centres as the interface has them: [n][5]
__global__ __launch_bounds__(256) void slic_engine_export_kernel(int n, const float* __restrict__ centres,
                                                                 float* __restrict__ centres_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const SlicCentre c = slic_engine_load_centre(centres, k);
    float* o = centres_out + (size_t)5 * k;
    o[0] = c.x, o[1] = c.y, o[2] = c.c0, o[3] = c.c1, o[4] = c.c2;
}

}  // namespace mmf
