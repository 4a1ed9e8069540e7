// flowcrf_kernels.hpp -- the inference of the reference's flow_crf segmentation (Core/Segmentation/Segmentation.cpp:819-1263)
// on the device; DESIGN.md 4.9 writes the arithmetic out, tests/flowcrf_oracle.py restates it.  Textually included from
// mmf_hip.hip.
//
//   fcrf_track_kernel    (a) every model's start / end projection of every track (Model::computeTrackProjectionStartEnd,
//                        Model.cpp:524-579, length 2), its speed in pixels per second and its CRF cell; the track with the
//                        highest table index claims the cell (an integer atomicMax: the reference overwrites in order)
//   fcrf_prep_kernel     per cell: E from the claims, (b) norm01 / softmax / -log, (c) the projection probabilities, the
//                        appearance features
//   fcrf_pair_kernel     (d) sum_j K_a(i, j) X_j, the exact sum over every pair; once with X = 1 for the normalisation and
//                        once per mean-field iteration with X = D_a Q
//   fcrf_hblur_kernel    (d) the row half of the separable smoothness sum, sum_dx g(dx) X(x + dx, y); fcrf_update_kernel
//                        does the column half
//   fcrf_update_kernel   D = 1/sqrt(sum + 1e-20); Q = softmax(-U + w_s D_s S_s + w_a D_a S_a); X = D Q for the next pass
//   fcrf_fuse_kernel     (e) prob = 1 - (1 - Q motion)(1 - proj), the first maximum, the id image and its x4 copy
//
// Determinism: no float atomics; every float sum has a fixed order.  A cell's pair sum runs over j in `nsplit` contiguous
// ranges of whole chunks (one workgroup each; inside it four waves take a quarter of every chunk, j ascending, and are
// added ((w0 + w1) + w2) + w3); fcrf_update_kernel adds the ranges in range order.  nsplit depends on N alone.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crf_kernels.hpp"

namespace mmf {

constexpr int kFcrfTJ = 256;     // cells j of one staged chunk of fcrf_pair_kernel (64 per wave)
constexpr int kFcrfRadius = 44;  // g(d) = exp(-d d / 18) rounds to 0 in float from d = 44 on (1.9e-47 < 2^-150)
constexpr int kFcrfMaxModels = kCrfMaxLabels;

struct FcrfGeom {
    int W, H, w, h, N;  // the frame, the CRF image (W / 4 x H / 4), its cells
    float fx, fy, cx, cy;
};

struct FcrfModels {  // per call
    int M, L, allow_new;
    float T_start[kFcrfMaxModels][12], T_end[kFcrfMaxModels][12];  // rows 0-2 of the row-major 4 x 4
};

struct FcrfTracks {  // slot 1 = prev = the start, slot 0 = cur = the end
    const int* xy[2];
    const float* co[2];
    const long long* ts[2];
    const int* ok[2];
    const int* n_dev;  // the number of tracks on the device (the tracker's head), or null
    int n;             // ... on the host; an upper bound of it when n_dev is given
};

struct FcrfVertexList {
    const float* v[kFcrfMaxModels];  // [H][W][4] each
};

struct FcrfTable {
    float g[kFcrfRadius + 1];  // exp(-d d / 18): the smoothness kernel of features (x / 3, y / 3), one axis
};

// Isometry3d * point as Eigen's coefficient-wise product writes it: ((r0 x + r1 y) + r2 z) + t, every product and sum rounded
__device__ __forceinline__ double fcrf_row(const float* __restrict__ p, int r, double x, double y, double z) {
    const double a = __dmul_rn((double)p[4 * r], x), b = __dmul_rn((double)p[4 * r + 1], y), c = __dmul_rn((double)p[4 * r + 2], z);
    return __dadd_rn(__dadd_rn(__dadd_rn(a, b), c), (double)p[4 * r + 3]);
}

// one end of a track in a model's frame: false = no keypoint (null slot, stamp 0, non-finite coordinate: make_kp returns
// nullptr, Model.cpp:544-569) ; *inside = the transformed coordinate is finite and the pixel lies in the frame
__device__ __forceinline__ bool fcrf_project(const FcrfGeom& g, const float* __restrict__ T, const FcrfTracks& tr, int slot, int k,
                                             int* px, int* py, bool* inside) {
    if (!tr.ok[slot][k] || tr.ts[slot][k] == 0) return false;
    const float* c = tr.co[slot] + 3 * (size_t)k;
    if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) return false;
    const double x = (double)c[0], y = (double)c[1], z = (double)c[2];
    const double X = fcrf_row(T, 0, x, y, z), Y = fcrf_row(T, 1, x, y, z), Z = fcrf_row(T, 2, x, y, z);
    const double u = __dadd_rn((double)g.cx, __dmul_rn(__ddiv_rn(X, Z), (double)g.fx));
    const double v = __dadd_rn((double)g.cy, __dmul_rn(__ddiv_rn(Y, Z), (double)g.fy));
    *inside = false;
    // (a pixel that is not a number, or beyond int, is undefined in the reference's cast<int>: it counts as outside)
    if (isfinite(X) && isfinite(Y) && isfinite(Z) && fabs(u) < 1e9 && fabs(v) < 1e9) {
        *px = (int)round(u), *py = (int)round(v);  // half away from zero
        *inside = *px >= 0 && *px < g.W && *py >= 0 && *py < g.H;
    }
    return true;
}

// grid (ceil(n / 256), M).  speed[m][k], cell[m][k] (-1: the track gives model m no sample), claim[m][cell] = max k
__global__ __launch_bounds__(256) void fcrf_track_kernel(FcrfGeom g, FcrfModels md, FcrfTracks tr, int stride, float* __restrict__ speed,
                                                         int* __restrict__ cell, int* __restrict__ claim) {
    const int k = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    int n = tr.n;
    if (tr.n_dev) n = min(n, *tr.n_dev);
    if (k >= n) {
        if (k < stride) cell[(size_t)m * stride + k] = -1;
        return;
    }
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    bool in0 = false, in1 = false;
    const bool has0 = fcrf_project(g, md.T_start[m], tr, 1, k, &x0, &y0, &in0);
    const bool has1 = fcrf_project(g, md.T_end[m], tr, 0, k, &x1, &y1, &in1);
    int idx = -1;
    float v = 0.f;
    if (has0 && has1 && in0 && in1) {
        // cv::norm(Point2f(kp1) - Point2f(kp0)) is a double; (t1 - t0) is a uint64_t difference (:1002)
        const float dx = (float)x1 - (float)x0, dy = (float)y1 - (float)y0;
        const double len = sqrt(__dadd_rn(__dmul_rn((double)dx, (double)dx), __dmul_rn((double)dy, (double)dy)));
        const unsigned long long dt = (unsigned long long)tr.ts[0][k] - (unsigned long long)tr.ts[1][k];
        v = (float)__ddiv_rn(len, __dmul_rn((double)dt, 1e-9));
        // `s * kp1->xy` saturates to cv::Point: cvRound, half to even; the linear index as the reference writes it (:1026)
        const int ccx = (int)rint(0.25 * (double)x1), ccy = (int)rint(0.25 * (double)y1);
        idx = ccy * g.w + ccx;
        if (idx >= g.N) idx = -1;  // (the reference writes past the matrix there)
    }
    speed[(size_t)m * stride + k] = v;
    cell[(size_t)m * stride + k] = idx;
    if (idx >= 0) atomicMax(&claim[(size_t)m * g.N + idx], k);
}

struct FcrfPrepArgs {
    FcrfGeom g;
    int M, L, allow_new, stride;
    float threshold, max_err, min_proj;
    const int* claim;     // [M][N], null: no tracks at all
    const float* speed;   // [M][stride]
    const float* depth;   // [H][W]
    FcrfVertexList vert;
    const float* flow;    // [h][w][2]
    float *E, *U, *proj;  // [L][N]
    uint8_t* invalid;     // [N]
    float4* feat;         // [N] {x / 40, y / 40, 10 flow.x, 10 flow.y}
};

__global__ __launch_bounds__(256) void fcrf_prep_kernel(FcrfPrepArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, N = a.g.N;
    if (i >= N) return;
    const int y = i / a.g.w, x = i - y * a.g.w;
    const float inf = __builtin_inff();
    // (a), (b): the errors of this cell, norm01 (:1055-1069), softmax of -E (:1125-1136), -log (:1139)
    bool all_finite = true, any_below = false;
    float tot = 0.f;
    for (int m = 0; m < a.M; ++m) {
        const int k = a.claim ? a.claim[(size_t)m * N + i] : -1;
        const float e = k >= 0 ? a.speed[(size_t)m * a.stride + k] : inf;
        a.E[(size_t)m * N + i] = e;
        const bool fin = isfinite(e);
        all_finite = all_finite && fin;
        any_below = any_below || e < a.threshold;
        const float u = fin ? (e > a.threshold ? 1.f : 0.f) : e;
        const float ex = expf(-u);
        a.U[(size_t)m * N + i] = ex;
        tot = tot + ex;
    }
    if (a.allow_new) {
        a.E[(size_t)a.M * N + i] = inf;
        const float u = all_finite ? (any_below ? 1.f : 0.f) : inf;
        const float ex = expf(-u);
        a.U[(size_t)a.M * N + i] = ex;
        tot = tot + ex;
    }
    const bool soft = tot > 0.f;  // (false for a NaN as well: equal timestamps and equal pixels, 0 / 0)
    for (int l = 0; l < a.L; ++l) {
        const float p = soft ? a.U[(size_t)l * N + i] / tot : 1.f / (float)a.L;
        a.U[(size_t)l * N + i] = -logf(p);
    }
    // (c): the projection probabilities (:819-862, :1169), nearest sample at (4x, 4y)
    const size_t px = (size_t)(4 * y) * a.g.W + 4 * x;
    const float d = a.depth[px];
    bool inv = false;
    float sum = 0.f;
    for (int m = 0; m < a.M; ++m) {
        const float z = a.vert.v[m][4 * px + 2];
        inv = inv || (d < 1e-6f && z < 1e-6f);
        float dist = fabsf(d - z);
        dist = dist < a.max_err ? dist : a.max_err;  // (a NaN becomes max_err)
        const float e = expf(-1.f * (dist / a.max_err));
        a.proj[(size_t)m * N + i] = e;
        sum = sum + e;
    }
    for (int m = 0; m < a.M; ++m) {
        float p = a.proj[(size_t)m * N + i] / sum;
        if (inv) p = 0.f;
        if (p < a.min_proj) p = 0.f;
        a.proj[(size_t)m * N + i] = p;
    }
    if (a.allow_new) a.proj[(size_t)a.M * N + i] = 0.f;
    a.invalid[i] = inv ? 1 : 0;
    // (d): the appearance features; `v / 40` is an integer division in the reference (:1151-1152)
    a.feat[i] = make_float4((float)(x / 40), (float)(y / 40), a.flow[2 * (size_t)i] * 10.f, a.flow[2 * (size_t)i + 1] * 10.f);
}

// The pair sums of the appearance kernel, K(i, j) = exp(-|f_i - f_j|^2 / 2), every pair evaluated.
// Grid (ceil(N / (64 IPL)), nsplit), 256 lanes.  All four waves hold the SAME 64 IPL cells i (IPL per lane, LMAX accumulators
// each, in registers) and each takes a quarter of every staged chunk of kFcrfTJ cells j: a j's features and its X row are one
// wave-uniform LDS address, read once for the lane's IPL cells.  x = [N][LMAX] (rows padded with zeros), null: X = 1.
// partial = [nsplit][N][LMAX].
template <int LMAX, int IPL>
__global__ __launch_bounds__(256) void fcrf_pair_kernel(const float4* __restrict__ feat, const float* __restrict__ x, int N, int nsplit,
                                                        float* __restrict__ partial) {
    constexpr int kStage = kFcrfTJ * (4 + LMAX), kRed = 3 * LMAX * IPL * 64;
    __shared__ __attribute__((aligned(16))) float s_buf[kStage > kRed ? kStage : kRed];
    float4* s_f = reinterpret_cast<float4*>(s_buf);
    float* s_x = s_buf + 4 * kFcrfTJ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * (64 * IPL) + lane, split = blockIdx.y;
    const int nchunk = (N + kFcrfTJ - 1) / kFcrfTJ, per = (nchunk + nsplit - 1) / nsplit;
    const int c0 = split * per, c1 = min(nchunk, c0 + per);
    float4 fi[IPL];
    float acc[IPL][LMAX];
#pragma unroll
    for (int q = 0; q < IPL; ++q) {
        const int i = i0 + 64 * q;
        fi[q] = i < N ? feat[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int l = 0; l < LMAX; ++l) acc[q][l] = 0.f;
    }
    for (int c = c0; c < c1; ++c) {
        __syncthreads();  // the chunk before this one has been read
        const int jb = c * kFcrfTJ;
        s_f[tid] = jb + tid < N ? feat[jb + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = tid; t < kFcrfTJ * LMAX; t += 256) {
            const bool in = jb + t / LMAX < N;
            s_x[t] = in ? (x ? x[(size_t)jb * LMAX + t] : (t % LMAX == 0 ? 1.f : 0.f)) : 0.f;
        }
        __syncthreads();
        for (int jj = wave * 64; jj < wave * 64 + 64; ++jj) {
            const float4 fj = s_f[jj];
            float xv[LMAX];
#pragma unroll
            for (int l = 0; l < LMAX; ++l) xv[l] = s_x[jj * LMAX + l];
#pragma unroll
            for (int q = 0; q < IPL; ++q) {
                const float d0 = fi[q].x - fj.x, d1 = fi[q].y - fj.y, d2 = fi[q].z - fj.z, d3 = fi[q].w - fj.w;
                const float s = __builtin_fmaf(d3, d3, __builtin_fmaf(d2, d2, __builtin_fmaf(d1, d1, d0 * d0)));
                const float k = __builtin_amdgcn_exp2f(s * -0.72134752f);  // exp(-s / 2)
#pragma unroll
                for (int l = 0; l < LMAX; ++l) acc[q][l] = __builtin_fmaf(k, xv[l], acc[q][l]);
            }
        }
    }
    __syncthreads();
    float* s_red = s_buf;  // [3][LMAX][IPL][64]
    if (wave > 0) {
#pragma unroll
        for (int l = 0; l < LMAX; ++l)
#pragma unroll
            for (int q = 0; q < IPL; ++q) s_red[(((wave - 1) * LMAX + l) * IPL + q) * 64 + lane] = acc[q][l];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < IPL; ++q) {
            const int i = i0 + 64 * q;
            if (i >= N) continue;
#pragma unroll
            for (int l = 0; l < LMAX; ++l) {
                const float s = ((acc[q][l] + s_red[((0 * LMAX + l) * IPL + q) * 64 + lane]) + s_red[((1 * LMAX + l) * IPL + q) * 64 + lane]) +
                                s_red[((2 * LMAX + l) * IPL + q) * 64 + lane];
                partial[((size_t)split * N + i) * LMAX + l] = s;
            }
        }
    }
}

// hb[i][l] = sum_dx g(|dx|) xs[(x + dx, y)][l], dx ascending over the columns of the image.  One lane per (cell, label).
__global__ __launch_bounds__(256) void fcrf_hblur_kernel(FcrfTable tab, int w, int N, int LMAX, const float* __restrict__ xs,
                                                         float* __restrict__ hb) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)N * LMAX) return;
    const int i = (int)(t / LMAX), l = (int)(t % LMAX);
    const int y = i / w, x = i - y * w;
    const int a = max(-kFcrfRadius, -x), b = min(kFcrfRadius, w - 1 - x);
    float s = 0.f;
    for (int dx = a; dx <= b; ++dx) s = __builtin_fmaf(tab.g[dx < 0 ? -dx : dx], xs[(size_t)(i + dx) * LMAX + l], s);
    hb[t] = s;
}

struct FcrfUpdateArgs {
    FcrfTable tab;
    int mode;  // 0: the normalisation and Q = softmax(-U); 1: one mean-field update
    int w, h, N, L, nsplit;
    float w_smooth, w_app;  // 4 weight_smoothness, weight_appearance
    const float* partial;   // mode 0: [nsplit][N][1] of the pass with X = 1 (null: no mean field, D = 0); mode 1: [nsplit][N][LMAX]
    const float* hb;        // mode 1: [N][LMAX]
    const float* U;
    float *Ds, *Da, *Q;     // Q [L][N]
    float *xs, *xa;         // [N][LMAX]
};

template <int LMAX>
__global__ __launch_bounds__(256) void fcrf_update_kernel(FcrfUpdateArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, N = a.N;
    if (i >= N) return;
    const int y = i / a.w, x = i - y * a.w;
    float ds, da;
    float v[LMAX];
    if (a.mode == 0) {
        ds = da = 0.f;
        if (a.partial) {
            float sa = 0.f, sx = 0.f, sy = 0.f;
            for (int s = 0; s < a.nsplit; ++s) sa = sa + a.partial[(size_t)s * N + i];
            for (int d = max(-kFcrfRadius, -x); d <= min(kFcrfRadius, a.w - 1 - x); ++d) sx = sx + a.tab.g[d < 0 ? -d : d];
            for (int d = max(-kFcrfRadius, -y); d <= min(kFcrfRadius, a.h - 1 - y); ++d) sy = sy + a.tab.g[d < 0 ? -d : d];
            ds = 1.f / sqrtf(sx * sy + 1e-20f), da = 1.f / sqrtf(sa + 1e-20f);
        }
        a.Ds[i] = ds, a.Da[i] = da;
#pragma unroll
        for (int l = 0; l < LMAX; ++l) v[l] = l < a.L ? -a.U[(size_t)l * N + i] : 0.f;
    } else {
        ds = a.Ds[i], da = a.Da[i];
        float ss[LMAX], sa[LMAX];
#pragma unroll
        for (int l = 0; l < LMAX; ++l) ss[l] = 0.f, sa[l] = 0.f;
        for (int s = 0; s < a.nsplit; ++s) {
            const float* p = a.partial + ((size_t)s * N + i) * LMAX;
#pragma unroll
            for (int l = 0; l < LMAX; ++l) sa[l] = sa[l] + p[l];
        }
        for (int d = max(-kFcrfRadius, -y); d <= min(kFcrfRadius, a.h - 1 - y); ++d) {
            const float gd = a.tab.g[d < 0 ? -d : d];
            const float* p = a.hb + (size_t)(i + d * a.w) * LMAX;
#pragma unroll
            for (int l = 0; l < LMAX; ++l) ss[l] = __builtin_fmaf(gd, p[l], ss[l]);
        }
#pragma unroll
        for (int l = 0; l < LMAX; ++l)
            v[l] = l < a.L ? (-a.U[(size_t)l * N + i] + a.w_smooth * (ds * ss[l])) + a.w_app * (da * sa[l]) : 0.f;
    }
    float m = v[0];
#pragma unroll
    for (int l = 1; l < LMAX; ++l) m = (l < a.L && m < v[l]) ? v[l] : m;
    float tot = 0.f;
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < a.L) v[l] = expf(v[l] - m), tot = tot + v[l];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
        const float q = l < a.L ? v[l] / tot : 0.f;
        if (l < a.L) a.Q[(size_t)l * N + i] = q;
        a.xs[(size_t)i * LMAX + l] = ds * q, a.xa[(size_t)i * LMAX + l] = da * q;
    }
}

struct FcrfFuseArgs {
    FcrfGeom g;
    int L;
    uint8_t id[kCrfMaxLabels];
    const float *Q, *proj, *motion;
    float* prob;       // [L][N]
    int* label;        // [N]
    uint8_t* ids;      // [h][w]
    uint8_t* ids_full; // [H][W]
};

// (e) :1193-1263.  One lane per cell; it writes the cell's 4 x 4 block of the full-resolution image (one 32-bit store a row).
__global__ __launch_bounds__(256) void fcrf_fuse_kernel(FcrfFuseArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, N = a.g.N;
    if (i >= N) return;
    const float mo = a.motion[i];
    int best_l = 0;
    float best = 0.f;
    for (int l = 0; l < a.L; ++l) {
        const float pf = a.Q[(size_t)l * N + i] * mo;
        const float p = 1.f - ((1.f - pf) * (1.f - a.proj[(size_t)l * N + i]));
        a.prob[(size_t)l * N + i] = p;
        if (l == 0 || p > best) best = p, best_l = l;  // the first maximum
    }
    a.label[i] = best_l;
    const unsigned id = a.id[best_l];
    a.ids[i] = (uint8_t)id;
    const int y = i / a.g.w, x = i - y * a.g.w;
    const unsigned four = id * 0x01010101u;
    for (int r = 0; r < 4; ++r) *reinterpret_cast<unsigned*>(a.ids_full + (size_t)(4 * y + r) * a.g.W + 4 * x) = four;
}

}  // namespace mmf
