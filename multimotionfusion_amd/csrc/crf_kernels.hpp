// crf_kernels.hpp -- the dense-CRF motion segmentation of Segmentation::performSegmentationCRF
// (Core/Segmentation/Segmentation.cpp:159-740) on the device, stages 2-13 of DESIGN.md section 4 (stage 1 and 14 are the
// super-pixel kernels of slic_kernels.hpp).  Textually included from mmf_hip.hip.
//
//   crf_prep_kernel      one workgroup: depth range (:198-210), average confidences (:225-237), unaries (:271-332, clamp
//                        :491-494), the two feature vectors of every cell (:470-486)
//   crf_pair_kernel      sum_j K(f_i, f_j) X_j for both Potts kernels, exact Gaussian sums (no lattice: DESIGN.md B1); used
//                        once with X = 1 for the normalisation and once per mean-field iteration with X = D Q
//   crf_softmax_kernel   D = 1/sqrt(sum + 1e-20), Q = softmax(-U + w_s D sum_s + w_a D sum_a) per cell (:496-506)
//   crf_post_kernel      one workgroup: argmax (:510-513), connected components (ConnectedLabels.hpp:50-160), the
//                        largest component per label, size and border rules, relabelling, depth statistics (:515-679)
//
// Determinism: no float atomics anywhere; every float sum has a fixed order.  The pair sums of a cell run over j in
// chunks of kCrfTJ per workgroup (four waves a quarter each, added ((w0 + w1) + w2) + w3) and the chunks are added in
// chunk order by crf_softmax_kernel.  Every label goes through the same operations in the same order, so labels that are
// exactly tied stay tied.  The float sums the reference runs in cell order (confidences, depth statistics) run in cell
// order here too, one lane per label, and are bit-exact.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

namespace mmf {

constexpr int kCrfMaxLabels = 32;       // models + the new label
constexpr int kCrfMaxCells = 16384;     // (W/S) x (H/S): the post kernel holds comp (int) + map (u8) of every cell in LDS
constexpr int kCrfTJ = 128;             // cells j per workgroup of crf_pair_kernel
constexpr int kCrfTI = 64;              // cells i per workgroup of crf_pair_kernel (one per lane)

struct CrfParams {
    float scale_rgb, scale_depth, scale_pos;  // 1.0f / sigma (Segmentation.h:123-125)
    float w_app, w_smooth;
    float thr_new, w_err, k_err;
    float min_rel, max_rel;
};

// what the host reads back (one pinned copy per call)
struct CrfSummary {
    float range;
    int range_invalid;
    int has_new_label;
    int n_models_out;   // entries of `models` that belong to the result (the new label's is dropped when it has no cell)
    int n_labels, n_cells, allow_new, n_components;
    float avg_conf[kCrfMaxLabels];
    mmf_segmentation_model models[kCrfMaxLabels];
};

// B3: the regular grid when no super-pixel engine hands labels in
__global__ __launch_bounds__(256) void crf_grid_labels_kernel(int W, int H, int S, int spx, int spy, int* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W * H) return;
    const int y = i / W, x = i - y * W;
    const int cy = y / S < spy - 1 ? y / S : spy - 1, cx = x / S < spx - 1 ? x / S : spx - 1;
    out[i] = cy * spx + cx;
}

// :491-494 -- `unary(j, i) <= 1e-5` compares in double
__device__ __forceinline__ float crf_clamp_unary(float v) { return (double)v <= 1e-5 ? (float)1e-5 : v; }

// One workgroup of 1024.  maps = [M][2][N] {icp, conf} (mmf_shard_gather_maps' layout); U = [L][N]; feat = [N][8]
// {x/2, y/2, x*sp, y*sp, r*srgb, g*srgb, b*srgb, min(d*sd, 100)}; rgb = the frame (u8 x 3), of which the first N pixels
// are the colour features (the reference's quirk, :477-479).
__global__ __launch_bounds__(1024) void crf_prep_kernel(const float* __restrict__ low_depth, const float* __restrict__ maps,
                                                        const uint8_t* __restrict__ rgb, int N, int spx, int M, int allow_new,
                                                        CrfParams p, float* __restrict__ U, float* __restrict__ feat,
                                                        CrfSummary* __restrict__ sum) {
    __shared__ float s_max[16], s_min[16];
    __shared__ float s_range;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float dmax = 0.f, dmin = FLT_MAX;
    for (int k = tid; k < N; k += 1024) {
        const float d = low_depth[k];
        if (d > 100.f || d < 0.f || !isfinite(d)) continue;
        dmax = dmax < d ? d : dmax;
        dmin = dmin > d ? d : dmin;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float a = __shfl_xor(dmax, o), b = __shfl_xor(dmin, o);
        dmax = dmax < a ? a : dmax;
        dmin = dmin > b ? b : dmin;
    }
    if (lane == 0) s_max[wave] = dmax, s_min[wave] = dmin;
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, b = FLT_MAX;
        for (int w = 0; w < 16; ++w) a = a < s_max[w] ? s_max[w] : a, b = b > s_min[w] ? s_min[w] : b;
        const float r = a - b;
        s_range = r;
        sum->range = r;
        sum->range_invalid = !(r > 0.f && r <= FLT_MAX);
        sum->n_cells = N, sum->n_labels = M + (allow_new ? 1 : 0), sum->allow_new = allow_new ? 1 : 0;
    }
    __syncthreads();
    const float range = s_range;
    const float err0_low_conf = (float)((double)range * 0.01);  // :276, a double literal
    const float err_k = range * p.k_err;                        // :282
    for (int k = tid; k < N; k += 1024) {
        float lowest = 0.f;
        for (int i = 0; i < M; ++i) {
            float c = maps[((size_t)i * 2 + 1) * N + k];
            if (!isfinite(c)) c = 0.f;  // :230-232 (in place: the unaries see 0)
            float e = maps[((size_t)i * 2) * N + k];
            if (i == 0 && (double)c < 0.3) e = err0_low_conf;
            if (i >= 1 && (double)c <= 0.4) e = err_k;
            const float en = e / range;
            if (i == 0 || en < lowest) lowest = en;
            U[(size_t)i * N + k] = crf_clamp_unary(p.w_err * en);
        }
        if (allow_new) {
            const float a = p.thr_new - p.w_err * lowest;
            U[(size_t)M * N + k] = crf_clamp_unary(a < 0.01f ? 0.01f : a);  // std::max(a, 0.01f)
        }
        const int y = k / spx, x = k - y * spx;
        const float fx = (float)x, fy = (float)y;
        float d = low_depth[k] * p.scale_depth;
        d = 100.f < d ? 100.f : d;  // std::min(d, 100.0f)
        float* f = feat + (size_t)k * 8;
        f[0] = fx / 2.f, f[1] = fy / 2.f;
        f[2] = fx * p.scale_pos, f[3] = fy * p.scale_pos;
        f[4] = (float)rgb[3 * k + 0] * p.scale_rgb, f[5] = (float)rgb[3 * k + 1] * p.scale_rgb;
        f[6] = (float)rgb[3 * k + 2] * p.scale_rgb, f[7] = d;
    }
    // average confidence (:225-237): one lane per model, float sum in cell order
    if (wave == 0 && lane < M) {
        const float* c = maps + ((size_t)lane * 2 + 1) * N;
        float s = 0.f;
        int k = 0;
        for (; k + 4 <= N; k += 4) {
            const float4 v = make_float4(c[k], c[k + 1], c[k + 2], c[k + 3]);
            s = s + (isfinite(v.x) ? v.x : 0.f);
            s = s + (isfinite(v.y) ? v.y : 0.f);
            s = s + (isfinite(v.z) ? v.z : 0.f);
            s = s + (isfinite(v.w) ? v.w : 0.f);
        }
        for (; k < N; ++k) s = s + (isfinite(c[k]) ? c[k] : 0.f);
        sum->avg_conf[lane] = s / (float)(unsigned)N;
    }
}

// partial[split][2][L][N]: sum over this workgroup's chunk of j of K_s(i, j) xs[l][j] and K_a(i, j) xa[l][j].
// K(i, j) = exp(-|f_i - f_j|^2 / 2), no truncation: every pair is evaluated.
template <int LMAX>
__global__ __launch_bounds__(256) void crf_pair_kernel(const float* __restrict__ feat, int N, int L, const float* __restrict__ xs,
                                                       const float* __restrict__ xa, float* __restrict__ partial) {
    __shared__ float s_f[kCrfTJ][8];
    __shared__ float s_xs[LMAX][kCrfTJ], s_xa[LMAX][kCrfTJ];
    __shared__ float s_red[3][2][LMAX][kCrfTI];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.y * kCrfTJ, split = blockIdx.y;
    for (int t = tid; t < kCrfTJ * 8; t += 256) {
        const int j = j0 + t / 8;
        s_f[t / 8][t % 8] = j < N ? feat[(size_t)j * 8 + (t % 8)] : 0.f;
    }
    for (int t = tid; t < LMAX * kCrfTJ; t += 256) {
        const int l = t / kCrfTJ, jj = t % kCrfTJ, j = j0 + jj;
        const bool ok = l < L && j < N;
        s_xs[l][jj] = ok ? xs[(size_t)l * N + j] : 0.f;
        s_xa[l][jj] = ok ? xa[(size_t)l * N + j] : 0.f;
    }
    __syncthreads();
    const int i = blockIdx.x * kCrfTI + lane;
    float fi[8];
    if (i < N) {
#pragma unroll
        for (int q = 0; q < 8; ++q) fi[q] = feat[(size_t)i * 8 + q];
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) fi[q] = 0.f;
    }
    float as[LMAX], aa[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) as[l] = 0.f, aa[l] = 0.f;
    const int jb = wave * (kCrfTJ / 4), je = min(jb + kCrfTJ / 4, N - j0);
    for (int jj = jb; jj < je; ++jj) {
        const float dx = fi[0] - s_f[jj][0], dy = fi[1] - s_f[jj][1];
        const float ks = __expf(-0.5f * (dx * dx + dy * dy));
        float d2 = 0.f;
#pragma unroll
        for (int q = 2; q < 8; ++q) {
            const float t = fi[q] - s_f[jj][q];
            d2 = d2 + t * t;
        }
        const float ka = __expf(-0.5f * d2);
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            as[l] = as[l] + ks * s_xs[l][jj];
            aa[l] = aa[l] + ka * s_xa[l][jj];
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int l = 0; l < LMAX; ++l) s_red[wave - 1][0][l][lane] = as[l], s_red[wave - 1][1][l][lane] = aa[l];
    }
    __syncthreads();
    if (wave == 0 && i < N) {
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            if (l >= L) break;
            const float s = ((as[l] + s_red[0][0][l][lane]) + s_red[1][0][l][lane]) + s_red[2][0][l][lane];
            const float a = ((aa[l] + s_red[0][1][l][lane]) + s_red[1][1][l][lane]) + s_red[2][1][l][lane];
            partial[(((size_t)split * 2 + 0) * L + l) * N + i] = s;
            partial[(((size_t)split * 2 + 1) * L + l) * N + i] = a;
        }
    }
}

// mode 0: the normalisation (partials of the pass with x = 1, one label) -> Ds, Da; Q = softmax(-U).
// mode 1: Q = softmax(-U + w_s Ds sum_s + w_a Da sum_a) (the partials of the pass with x = D Q).
// Both write xs = Ds Q and xa = Da Q for the next pass.  Under B4 Q = 0.
template <int LMAX>
__global__ __launch_bounds__(256) void crf_softmax_kernel(int mode, int N, int L, int nsplit, const float* __restrict__ partial,
                                                          const float* __restrict__ U, float w_smooth, float w_app,
                                                          float* __restrict__ Ds, float* __restrict__ Da, float* __restrict__ Q,
                                                          float* __restrict__ xs, float* __restrict__ xa,
                                                          const CrfSummary* __restrict__ sum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const bool invalid = sum->range_invalid != 0;
    float ds, da;
    float v[LMAX];  // (every index below is a compile-time one: the label loops are unrolled, v stays in registers)
    if (mode == 0) {
        if (partial) {
            float ss = 0.f, sa = 0.f;
            for (int s = 0; s < nsplit; ++s) ss = ss + partial[((size_t)s * 2 + 0) * N + i], sa = sa + partial[((size_t)s * 2 + 1) * N + i];
            ds = 1.f / sqrtf(ss + 1e-20f), da = 1.f / sqrtf(sa + 1e-20f);
            Ds[i] = ds, Da[i] = da;
        } else {
            ds = da = 0.f;
        }
#pragma unroll
        for (int l = 0; l < LMAX; ++l) v[l] = l < L ? -U[(size_t)l * N + i] : 0.f;
    } else {
        ds = Ds[i], da = Da[i];
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            v[l] = 0.f;
            if (l >= L) continue;
            float ss = 0.f, sa = 0.f;
            for (int s = 0; s < nsplit; ++s)
                ss = ss + partial[(((size_t)s * 2 + 0) * L + l) * N + i], sa = sa + partial[(((size_t)s * 2 + 1) * L + l) * N + i];
            // tmp1 = -unary; tmp1 -= (-w_s Kt_s Q); tmp1 -= (-w_a Kt_a Q) (PottsCompatibility::apply = -w Q)
            v[l] = (-U[(size_t)l * N + i] - -(w_smooth * (ds * ss))) - -(w_app * (da * sa));
        }
    }
    float m = v[0];
#pragma unroll
    for (int l = 1; l < LMAX; ++l) m = (l < L && m < v[l]) ? v[l] : m;
    float tot = 0.f;
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) v[l] = expf(v[l] - m), tot = tot + v[l];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
        if (l >= L) break;
        const float q = invalid ? 0.f : v[l] / tot;
        Q[(size_t)l * N + i] = q;
        xs[(size_t)l * N + i] = ds * q, xa[(size_t)l * N + i] = da * q;
    }
}

// Stages 7-13 in one workgroup of 1024.  Dynamic LDS: comp[N] int + map[N] u8.  Global scratch: cstat[N][6] ints
// {size, label, top, left, bottom, right} per component, cid[N] (component of every cell), flabel[N] (final label per
// component).  ids = the labels' model ids (the new label's last).
struct CrfPostArgs {
    const float* Q;
    const float* low_depth;
    int N, spx, spy, W, H, S, L, M, allow_new;
    unsigned next_id;
    unsigned ids[kCrfMaxLabels];
    float min_rel, max_rel;
    int* cstat;
    int* cid;
    int* flabel;
    uint8_t* raw_map;
    uint8_t* map;
    CrfSummary* sum;
};

__global__ __launch_bounds__(1024) void crf_post_kernel(CrfPostArgs a) {
    extern __shared__ int s_dyn[];
    int* comp = s_dyn;
    uint8_t* lab = reinterpret_cast<uint8_t*>(s_dyn + a.N);
    __shared__ unsigned long long s_best[256];
    __shared__ int s_box[256][4];  // top left bottom right of the components in a label's list
    __shared__ int s_kill[256];
    __shared__ int s_scan[1024];
    __shared__ int s_changed, s_smallest, s_ncomp;
    const int tid = threadIdx.x, N = a.N, spx = a.spx;
    const bool invalid = a.sum->range_invalid != 0;
    if (tid < 256) {
        s_best[tid] = 0ull;
        s_box[tid][0] = s_box[tid][1] = 0xFFFF, s_box[tid][2] = s_box[tid][3] = 0;
        s_kill[tid] = 0;
    }
    if (tid == 0) s_smallest = 256;
    // 7: argmax (:510-513): the first label wins, a later one only when strictly greater
    for (int k = tid; k < N; k += 1024) {
        int m = 0;
        if (!invalid) {
            float best = a.Q[k];
            for (int l = 1; l < a.L; ++l) {
                const float q = a.Q[(size_t)l * N + k];
                if (q > best) best = q, m = l;
            }
        }
        const uint8_t id = (uint8_t)a.ids[m];
        lab[k] = id, a.raw_map[k] = id;
        comp[k] = k;
    }
    // 8: 4-connected components.  Every cell's comp only decreases and always names a cell of its component; the fixed
    // point is the component's first cell in raster order (= ConnectedLabels.hpp's numbering, by rank below)
    for (;;) {
        __syncthreads();
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int k = tid; k < N; k += 1024) {
            const int y = k / spx, x = k - y * spx;
            const uint8_t l = lab[k];
            int c = comp[k];
            if (x > 0 && lab[k - 1] == l) c = min(c, comp[k - 1]);
            if (x + 1 < spx && lab[k + 1] == l) c = min(c, comp[k + 1]);
            if (y > 0 && lab[k - spx] == l) c = min(c, comp[k - spx]);
            if (y + 1 < a.spy && lab[k + spx] == l) c = min(c, comp[k + spx]);
            c = min(c, comp[c]);
            if (c < comp[k]) {
                atomicMin(&comp[k], c);
                s_changed = 1;
            }
        }
        __syncthreads();
        if (!s_changed) break;
    }
    // component numbers: rank of the root among the roots (block scan over contiguous chunks)
    const int chunk = (N + 1023) / 1024, k0 = min(N, tid * chunk), k1 = min(N, k0 + chunk);
    int cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += comp[k] == k;
    s_scan[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int r = s_scan[tid] - cnt;
    for (int k = k0; k < k1; ++k)
        if (comp[k] == k) a.cid[k] = r++;  // (root cells hold their own number first)
    if (tid == 1023) s_ncomp = s_scan[1023];
    __syncthreads();
    const int ncomp = s_ncomp;
    for (int c = tid; c < ncomp; c += 1024) {
        int* st = a.cstat + (size_t)c * 6;
        st[0] = 0, st[1] = 0, st[2] = INT_MAX, st[3] = INT_MAX, st[4] = 0, st[5] = 0;
    }
    __syncthreads();
    for (int k = tid; k < N; k += 1024) {
        const int c = a.cid[comp[k]];
        const int y = k / spx, x = k - y * spx;
        int* st = a.cstat + (size_t)c * 6;
        atomicAdd(&st[0], 1);
        if (comp[k] == k) st[1] = lab[k];
        atomicMin(&st[2], y), atomicMin(&st[3], x), atomicMax(&st[4], y), atomicMax(&st[5], x);
        atomicMin(&s_smallest, (int)lab[k]);
    }
    __syncthreads();
    for (int k = tid; k < N; k += 1024) comp[k] = a.cid[comp[k]];  // comp now holds component numbers
    // 9: the largest component of every label (ties: the earlier one); the smallest key keeps all (:530-553)
    for (int c = tid; c < ncomp; c += 1024) {
        const int* st = a.cstat + (size_t)c * 6;
        atomicMax(&s_best[st[1]], ((unsigned long long)(unsigned)st[0] << 32) | (0xFFFFFFFFu - (unsigned)c));
    }
    __syncthreads();
    const int mn = (int)((float)(unsigned)N * a.min_rel), mx = (int)((float)(unsigned)N * a.max_rel);
    for (int c = tid; c < ncomp; c += 1024) {
        const int* st = a.cstat + (size_t)c * 6;
        const int l = st[1];
        const bool in_list = l == s_smallest || (0xFFFFFFFFu - (unsigned)(s_best[l] & 0xFFFFFFFFull)) == (unsigned)c;
        int fl = in_list ? l : 255;
        // 10: the new label's size (:555-563)
        if (a.allow_new && in_list && (unsigned)l == a.next_id && (st[0] < mn || st[0] > mx)) fl = 255;
        a.flabel[c] = fl;
        if (in_list) {  // 11: the boxes over the label's list (:565-584)
            atomicMin(&s_box[l][0], st[2]), atomicMin(&s_box[l][1], st[3]);
            atomicMax(&s_box[l][2], st[4]), atomicMax(&s_box[l][3], st[5]);
        }
    }
    __syncthreads();
    if (tid < a.L) {  // border rule (:586-600), the boxes mapped to full resolution as unsigned short
        const unsigned id = a.ids[tid];
        if (id != 0) {
            const int S = a.S;
            auto hi = [S](int v) -> unsigned { return (unsigned)(int)(v * S + S * 0.5) & 0xFFFFu; };
            const unsigned top = hi(s_box[id][0]), left = hi(s_box[id][1]), bottom = hi(s_box[id][2]), right = hi(s_box[id][3]);
            const unsigned B = 20, hb = (unsigned)a.H - B, wb = (unsigned)a.W - B;
            if ((top < B && bottom < B) || (left < B && right < B) || (top > hb && bottom > hb) || (left > wb && right > wb))
                s_kill[id] = 1;
        }
    }
    __syncthreads();
    for (int c = tid; c < ncomp; c += 1024) {
        const int* st = a.cstat + (size_t)c * 6;
        const int l = st[1];
        const bool in_list = l == s_smallest || (0xFFFFFFFFu - (unsigned)(s_best[l] & 0xFFFFFFFFull)) == (unsigned)c;
        if (in_list && s_kill[l]) a.flabel[c] = 255;
    }
    __syncthreads();
    for (int k = tid; k < N; k += 1024) {  // :602
        const uint8_t v = (uint8_t)a.flabel[comp[k]];
        lab[k] = v, a.map[k] = v;
    }
    __syncthreads();
    float* depth = reinterpret_cast<float*>(comp);  // (comp is done with: the depth statistics read the depths from LDS)
    for (int k = tid; k < N; k += 1024) depth[k] = a.low_depth[k];
    __syncthreads();
    // 12, 13: depth statistics and counts (:604-679), one lane per label, float sums in cell order
    if (tid < a.L) {
        const uint8_t id = (uint8_t)a.ids[tid];
        const float* d = depth;
        float s = 0.f, dv = 0.f;
        unsigned n = 0;
        for (int k = 0; k < N; ++k) {
            const bool hit = lab[k] == id;
            const float x = d[k];
            s = hit ? s + x : s;
            n += hit;
        }
        const float mean = n ? s / (float)n : 0.f;
        for (int k = 0; k < N; ++k) {
            const bool hit = lab[k] == id;
            const float x = d[k];
            dv = hit ? dv + fabsf(mean - x) : dv;
        }
        const float stdv = n ? dv / (float)n : 0.f;
        const unsigned count = n;
        if (tid != 0) {
            const double lim = 1.1 * (double)stdv + (double)mean;
            for (int k = 0; k < N; ++k) {
                const float x = d[k];
                const bool hit = lab[k] == id && (double)x > lim;
                s = hit ? s - x : s;
                dv = hit ? dv - fabsf(mean - x) : dv;
                n -= hit;
            }
        }
        mmf_segmentation_model& md = a.sum->models[tid];
        md.id = a.ids[tid];
        md.super_pixel_count = count;
        md.avg_confidence = tid < a.M ? a.sum->avg_conf[tid] : 0.f;
        md.depth_mean = n ? s / (float)n : 0.f;
        md.depth_std = n ? dv / (float)n : 0.f;
        if (tid == a.L - 1) {
            const bool has_new = a.allow_new && count > 0;
            a.sum->has_new_label = has_new ? 1 : 0;
            a.sum->n_models_out = a.allow_new ? (has_new ? a.L : a.L - 1) : a.L;
            a.sum->n_components = ncomp;
        }
    }
}

}  // namespace mmf
