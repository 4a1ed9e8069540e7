// flow_kernels.hpp -- dense optical flow after Farneback on the device: the stage the reference runs as
// cv::calcOpticalFlowFarneback(gprev, gnext, flow, 0.2, 1, 20, 2, 5, 15/50.0, 0) on a frame pair scaled down by four
// (Core/Segmentation/Segmentation.cpp:779-804).  OpenCV is not part of this project and its source is not in the reference
// tree: the arithmetic below follows the specification written down in DESIGN.md 4.8 (Farneback's published algorithm in the
// box-window, single-level form), and tests/flow_oracle.py restates the same text on the CPU.  Parity with OpenCV itself is
// NOT pinned.  Everything is integer, or float32 in the written order (this translation unit is built with
// -ffp-contract=off; `/` and sqrtf are correctly rounded: device_math.hpp), no sum depends on the order pixels are visited
// in, no atomics: every stage image is bit exact against the oracle.
//   * flow_expand_kernel: stages 1-4 for one or two frames (blockIdx.z) in ONE launch.  A 32 x 8 tile stages the grey values
//     of its pixels and a halo of poly_n + 1 in LDS (area mean of div x div RGB pixels, integer), smooths them there
//     ([1 2 1]/4 twice, reflect-101) and expands them (vertical then horizontal pass, clamped) into the five coefficient
//     channels.
//   * flow_matrices_kernel: stage 5, one thread per pixel.
//   * flow_blur_solve_kernel: stage 6 (and 8 behind the last iteration): the (2m+1)^2 box sums of the five channels through
//     LDS -- horizontal taps in ascending x, then vertical taps in ascending y -- and the 2 x 2 solve.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmf {

constexpr int kFlowTX = 32, kFlowTY = 8;  // the tile: 256 threads, four waves
constexpr int kFlowMaxN = 7;              // poly_n <= 7
constexpr int kFlowMaxM = 16;             // winsize / 2 <= 16
constexpr int kFlowBorder = 5;

struct FlowTables {
    float g[kFlowMaxN + 1], xg[kFlowMaxN + 1], xxg[kFlowMaxN + 1];
    float ig[4];  // ig11, ig03, ig33, ig55
};

struct FlowGeom {
    int width, height;  // the frame
    int div;            // 1, 2 or 4
    int W, H;           // the flow image: width / div, height / div
    int n;              // poly_n
    int m;              // winsize / 2
};

// what stages 1-4 write for one frame
struct FlowFrameOut {
    const uint8_t* rgb;  // [height][width][3]
    uint8_t* gray;       // [H][W]
    float* smooth;       // [H][W]
    float* R;            // [H][W][5]
};

__device__ __forceinline__ int flow_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int flow_reflect101(int v, int size) { return v < 0 ? -v : (v >= size ? 2 * size - 2 - v : v); }

// stages 1-2 at flow-image pixel (x, y): the per-channel area mean (exact integer rounding), then the grey value.  The
// reference hands RGB data to COLOR_BGR2GRAY, so channel 0 gets the 0.114 weight (1868 / 16384).
__device__ __forceinline__ int flow_gray_at(const uint8_t* __restrict__ rgb, int width, int div, int x, int y, bool aligned4) {
    int c0, c1, c2;
    if (div == 4) {
        int s0 = 0, s1 = 0, s2 = 0;
        const uint8_t* p = rgb + ((size_t)(4 * y) * width + 4 * x) * 3;
        if (aligned4) {  // (width is a multiple of four: every row of twelve bytes starts on a dword)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p + (size_t)j * width * 3);
                const uint32_t a = q[0], b = q[1], c = q[2];  // r g b r | g b r g | b r g b
                s0 += (a & 255u) + (a >> 24) + ((b >> 16) & 255u) + ((c >> 8) & 255u);
                s1 += ((a >> 8) & 255u) + (b & 255u) + (b >> 24) + ((c >> 16) & 255u);
                s2 += ((a >> 16) & 255u) + ((b >> 8) & 255u) + (c & 255u) + (c >> 24);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t* q = p + (size_t)j * width * 3;
#pragma unroll
                for (int i = 0; i < 4; ++i) s0 += q[3 * i], s1 += q[3 * i + 1], s2 += q[3 * i + 2];
            }
        }
        // sum / 16, half to even
        c0 = (s0 >> 4) + (((s0 & 15) > 8 || ((s0 & 15) == 8 && ((s0 >> 4) & 1))) ? 1 : 0);
        c1 = (s1 >> 4) + (((s1 & 15) > 8 || ((s1 & 15) == 8 && ((s1 >> 4) & 1))) ? 1 : 0);
        c2 = (s2 >> 4) + (((s2 & 15) > 8 || ((s2 & 15) == 8 && ((s2 >> 4) & 1))) ? 1 : 0);
    } else if (div == 2) {
        const uint8_t* p = rgb + ((size_t)(2 * y) * width + 2 * x) * 3;
        const uint8_t* q = p + (size_t)width * 3;
        c0 = (p[0] + p[3] + q[0] + q[3] + 2) >> 2;
        c1 = (p[1] + p[4] + q[1] + q[4] + 2) >> 2;
        c2 = (p[2] + p[5] + q[2] + q[5] + 2) >> 2;
    } else {
        const uint8_t* p = rgb + ((size_t)y * width + x) * 3;
        c0 = p[0], c1 = p[1], c2 = p[2];
    }
    return (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14;
}

// LDS extents of a tile at the largest radius
constexpr int kFlowGW = kFlowTX + 2 * kFlowMaxN + 2, kFlowGH = kFlowTY + 2 * kFlowMaxN + 2;  // grey: halo n + 1
constexpr int kFlowSW = kFlowTX + 2 * kFlowMaxN, kFlowSH = kFlowTY + 2 * kFlowMaxN;          // smooth: halo n

// Stages 1-4.  grid = (ceil(W / 32), ceil(H / 8), frames), block = 256.
// LDS slot (j, i) of `sg` holds the grey value at (clamp(x0 - n - 1 + i), clamp(y0 - n - 1 + j)); slot (j, i) of `ss` the
// smoothed value at (clamp(x0 - n + i), clamp(y0 - n + j)): the expansion's clamped taps are plain slot offsets.
__global__ __launch_bounds__(256) void flow_expand_kernel(FlowGeom geo, FlowTables tab, FlowFrameOut f0, FlowFrameOut f1) {
    __shared__ float sg[kFlowGH][kFlowGW];
    __shared__ float sh[kFlowGH][kFlowSW];  // horizontal smoothing pass: grey rows, smooth columns
    __shared__ float ss[kFlowSH][kFlowSW];
    __shared__ float sr[3][kFlowTY][kFlowSW];  // the expansion's vertical pass

    const FlowFrameOut f = blockIdx.z == 0 ? f0 : f1;
    const int W = geo.W, H = geo.H, n = geo.n;
    const int x0 = blockIdx.x * kFlowTX, y0 = blockIdx.y * kFlowTY;
    const int tid = threadIdx.y * kFlowTX + threadIdx.x;
    const int gw = kFlowTX + 2 * n + 2, gh = kFlowTY + 2 * n + 2, sw = kFlowTX + 2 * n, shh = kFlowTY + 2 * n;
    const int gx0 = x0 - n - 1, gy0 = y0 - n - 1;
    const bool aligned4 = (reinterpret_cast<uintptr_t>(f.rgb) & 3u) == 0;

    for (int s = tid; s < gw * gh; s += 256) {
        const int j = s / gw, i = s - j * gw;
        const int x = flow_clamp(gx0 + i, W - 1), y = flow_clamp(gy0 + j, H - 1);
        sg[j][i] = (float)flow_gray_at(f.rgb, geo.width, geo.div, x, y, aligned4);
    }
    __syncthreads();
    // stage 3, horizontal: 0.5 c + 0.25 (l + r), reflect-101 (W >= 8: the reflected column is inside the halo)
    for (int s = tid; s < sw * gh; s += 256) {
        const int j = s / sw, i = s - j * sw;
        const int cx = flow_clamp(x0 - n + i, W - 1);
        const float c = sg[j][cx - gx0], l = sg[j][flow_reflect101(cx - 1, W) - gx0], r = sg[j][flow_reflect101(cx + 1, W) - gx0];
        sh[j][i] = 0.5f * c + 0.25f * (l + r);
    }
    __syncthreads();
    // stage 3, vertical
    for (int s = tid; s < sw * shh; s += 256) {
        const int j = s / sw, i = s - j * sw;
        const int cy = flow_clamp(y0 - n + j, H - 1);
        const float c = sh[cy - gy0][i], u = sh[flow_reflect101(cy - 1, H) - gy0][i], d = sh[flow_reflect101(cy + 1, H) - gy0][i];
        ss[j][i] = 0.5f * c + 0.25f * (u + d);
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    const bool inside = x < W && y < H;
    if (inside) {
        f.gray[(size_t)y * W + x] = (uint8_t)(int)sg[n + 1 + threadIdx.y][n + 1 + threadIdx.x];
        f.smooth[(size_t)y * W + x] = ss[n + threadIdx.y][n + threadIdx.x];
    }
    // stage 4, vertical pass over the tile's rows and every column of the halo
    for (int s = tid; s < sw * kFlowTY; s += 256) {
        const int j = s / sw, i = s - j * sw;
        const float c = ss[n + j][i];
        float r0 = tab.g[0] * c, r1 = 0.f, r2 = 0.f;
        for (int k = 1; k <= n; ++k) {
            const float t0 = ss[n + j - k][i], t1 = ss[n + j + k][i];
            r0 += tab.g[k] * (t0 + t1);
            r1 += tab.xg[k] * (t1 - t0);
            r2 += tab.xxg[k] * (t0 + t1);
        }
        sr[0][j][i] = r0, sr[1][j][i] = r1, sr[2][j][i] = r2;
    }
    __syncthreads();
    if (!inside) return;
    const int ty = threadIdx.y, cx = n + threadIdx.x;
    float b1 = sr[0][ty][cx] * tab.g[0], b3 = sr[1][ty][cx] * tab.g[0], b5 = sr[2][ty][cx] * tab.g[0];
    float b2 = 0.f, b4 = 0.f, b6 = 0.f;
    for (int k = 1; k <= n; ++k) {
        const float r0p = sr[0][ty][cx + k], r0m = sr[0][ty][cx - k];
        const float r1p = sr[1][ty][cx + k], r1m = sr[1][ty][cx - k];
        const float r2p = sr[2][ty][cx + k], r2m = sr[2][ty][cx - k];
        const float tg = r0p + r0m;
        b1 += tg * tab.g[k];
        b2 += (r0p - r0m) * tab.xg[k];
        b4 += tg * tab.xxg[k];
        b3 += (r1p + r1m) * tab.g[k];
        b6 += (r1p - r1m) * tab.xg[k];
        b5 += (r2p + r2m) * tab.g[k];
    }
    float* out = f.R + ((size_t)y * W + x) * 5;
    out[0] = b3 * tab.ig[0];
    out[1] = b2 * tab.ig[0];
    out[2] = b1 * tab.ig[1] + b5 * tab.ig[2];
    out[3] = b1 * tab.ig[1] + b4 * tab.ig[2];
    out[4] = b6 * tab.ig[3];
}

// the border factor of coordinate v on an axis of `size` pixels: the product over the (up to two) edges it is within 5 of
__device__ __forceinline__ float flow_border_scale(int v, int size) {
    const float border[kFlowBorder] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    const float lo = v < kFlowBorder ? border[v] : 1.f;
    const float hi = v >= size - kFlowBorder ? border[size - v - 1] : 1.f;
    return lo * hi;
}

// Stage 5.  flow == nullptr: the zero flow of the first iteration.  One thread per pixel, grid = ceil(W H / 256).
__global__ __launch_bounds__(256) void flow_matrices_kernel(FlowGeom geo, const float* __restrict__ R0, const float* __restrict__ R1,
                                                            const float* __restrict__ flow, float* __restrict__ M) {
    const int W = geo.W, H = geo.H;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    float dx = 0.f, dy = 0.f;
    if (flow != nullptr) dx = flow[2 * (size_t)idx], dy = flow[2 * (size_t)idx + 1];
    const float* a = R0 + (size_t)idx * 5;
    const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4];
    float fx = (float)x + dx, fy = (float)y + dy;
    const float x1f = floorf(fx), y1f = floorf(fy);
    float r2, r3, r4, r5, r6;
    if (x1f >= 0.f && x1f < (float)(W - 1) && y1f >= 0.f && y1f < (float)(H - 1)) {  // (a NaN flow takes the other branch)
        const int x1 = (int)x1f, y1 = (int)y1f;
        fx -= x1f, fy -= y1f;
        const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
        const float* p = R1 + ((size_t)y1 * W + x1) * 5;
        const float* q = p + (size_t)W * 5;
        r2 = p[0] * w00 + p[5] * w01 + q[0] * w10 + q[5] * w11;
        r3 = p[1] * w00 + p[6] * w01 + q[1] * w10 + q[6] * w11;
        r4 = p[2] * w00 + p[7] * w01 + q[2] * w10 + q[7] * w11;
        r5 = p[3] * w00 + p[8] * w01 + q[3] * w10 + q[8] * w11;
        r6 = p[4] * w00 + p[9] * w01 + q[4] * w10 + q[9] * w11;
        r4 = (a2 + r4) * 0.5f;
        r5 = (a3 + r5) * 0.5f;
        r6 = (a4 + r6) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = a2;
        r5 = a3;
        r6 = a4 * 0.5f;
    }
    r2 = (a0 - r2) * 0.5f;
    r3 = (a1 - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    const float scale = flow_border_scale(x, W) * flow_border_scale(y, H);  // 1 away from the edges: an exact multiplication
    r2 *= scale, r3 *= scale, r4 *= scale, r5 *= scale, r6 *= scale;
    float* out = M + (size_t)idx * 5;
    out[0] = r4 * r4 + r6 * r6;
    out[1] = (r4 + r5) * r6;
    out[2] = r5 * r5 + r6 * r6;
    out[3] = r4 * r2 + r6 * r3;
    out[4] = r6 * r2 + r5 * r3;
}

// Stage 6, and stage 8 when magnitude != nullptr (the last iteration).  grid = (ceil(W / 32), ceil(H / 8)), block = 256.
// Per channel: the tile and its halo of m (coordinates clamped to the image) into LDS, then the horizontal sums of every row
// of the halo; behind the five channels the vertical sums of the tile's pixels.  Every sum starts at 0.f and adds its 2m + 1
// taps in ascending order.  45 KiB of LDS, 110 VGPRs.
__global__ __launch_bounds__(256) void flow_blur_solve_kernel(FlowGeom geo, const float* __restrict__ M, float* __restrict__ flow,
                                                              float* __restrict__ magnitude, float* __restrict__ motion) {
    constexpr int kTH = kFlowTY + 2 * kFlowMaxM, kTW = kFlowTX + 2 * kFlowMaxM;
    constexpr int kRows = kTH / kFlowTY;  // rows of the halo per thread in the horizontal pass: row threadIdx.y + 8 r
    __shared__ float st[2][kTH][kTW];     // the tile of one channel; two, so that a channel costs one barrier
    __shared__ float sx[5][kTH][kFlowTX];
    const int W = geo.W, H = geo.H, m = geo.m;
    const int x0 = blockIdx.x * kFlowTX, y0 = blockIdx.y * kFlowTY;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kFlowTX + tx;
    const int tw = kFlowTX + 2 * m, th = kFlowTY + 2 * m;
    const float inv = 1.f / (float)((2 * m + 1) * (2 * m + 1));
    // A sum's taps are added one after the other, so a thread runs several sums side by side to have something to do while
    // an add waits for its tap: its (up to five) rows in the horizontal pass, the five channels in the vertical one.
    // The five channels of a thread's (up to ten) slots of the tile are read into registers at once, ahead of the channel
    // loop: one wait for global memory per launch, not one per channel.
    constexpr int kSlots = (kTH * kTW + 255) / 256;
    float tap[kSlots][5];
    int slot[kSlots];  // the slot's offset in a tile, -1 past the halo
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
        const int s = tid + 256 * q;
        slot[q] = -1;
#pragma unroll
        for (int c = 0; c < 5; ++c) tap[q][c] = 0.f;
        if (s < tw * th) {
            const int j = s / tw, i = s - j * tw;
            const int x = flow_clamp(x0 - m + i, W - 1), y = flow_clamp(y0 - m + j, H - 1);
            const float* p = M + ((size_t)y * W + x) * 5;
#pragma unroll
            for (int c = 0; c < 5; ++c) tap[q][c] = p[c];
            slot[q] = j * kTW + i;
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        float(*t)[kTW] = st[c & 1];
#pragma unroll
        for (int q = 0; q < kSlots; ++q)
            if (slot[q] >= 0) (&t[0][0])[slot[q]] = tap[q][c];
        __syncthreads();  // (the tile written two channels ago was last read in front of the previous channel's barrier)
        float acc[kRows];
        int row[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = 0.f, row[r] = min(ty + kFlowTY * r, th - 1);  // (a row past the halo: computed, not stored)
#pragma unroll 4
        for (int k = 0; k <= 2 * m; ++k) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] += t[row[r]][tx + k];
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (ty + kFlowTY * r < th) sx[c][ty + kFlowTY * r][tx] = acc[r];
    }
    __syncthreads();
    float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k <= 2 * m; ++k) {
#pragma unroll
        for (int c = 0; c < 5; ++c) sum[c] += sx[c][ty + k][tx];
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) sum[c] *= inv;
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const float g11 = sum[0], g12 = sum[1], g22 = sum[2], h1 = sum[3], h2 = sum[4];
    const float idet = (float)(1.0 / ((double)(g11 * g22 - g12 * g12) + 1e-3));
    const float u = (g11 * h2 - g12 * h1) * idet, v = (g22 * h1 - g12 * h2) * idet;
    const size_t idx = (size_t)y * W + x;
    flow[2 * idx] = u, flow[2 * idx + 1] = v;
    if (magnitude != nullptr) {
        const float mag = sqrtf(u * u + v * v);
        float mo = (mag - 0.2f) / 4.8f;
        mo = mo > 0.f ? mo : 0.f;
        mo = mo < 1.f ? mo : 1.f;
        magnitude[idx] = mag, motion[idx] = mo;
    }
}

}  // namespace mmf
