// ransac_kernels.hpp -- RigidRANSAC::estimate for many independent problems on the device: the geometric verification of
// the redetection candidates (Model::getBestMatch, Core/Model/Model.cpp:845-873), one wave per problem.
//
// The arithmetic is rigid_ransac.hpp's, compiled for the device: the same functions the host class runs, with
// -ffp-contract=off and correctly rounded sqrt and division, so that a problem's result equals, bit for bit, what a FRESH
// RigidRANSAC(cfg).estimate(p0, p1, N) returns on the host.  Fresh is the one deviation from the host path of
// mmf_viewstore_best_match, where one engine runs on from view to view: with a fresh engine and no mask
// the three rows of hypothesis `it` depend on (N, it) only, the host tabulates them with the real std::shuffle
// (ransac_triple_table) and the device needs no random numbers.
//
//   ransac_wave     the five steps of one problem, for 64 lanes:
//                     1. keys = hash_row of every correspondence; rank by (key, index) -- a total order, so any sort gives
//                        the rows of the host's std::sort; the points go to LDS in that order
//                     2. lane = hypothesis: the three-point fit
//                     3. lanes = points, loop over the hypotheses: distances, __ballot gives the inlier words and __popcll
//                        the counts (integers, order-free)
//                     4. lane = hypothesis that passed the candidate test: refit and the float error sum, both sequential
//                        in row order (what makes the doubles equal); lane 32 fits all rows, the result when none passed
//                     5. every lane scans the errors in iteration order with a strict < (first of equals wins, NaN never)
//   ransac_batch_kernel    grid = problems of a ragged batch, points packed in device arrays
//   rd_verify_kernel       grid = (views, query sets): the matches of a view against a set are the problem
//   rd_pick_kernel         grid = (asked models, query sets): the smallest error over a model's views, ascending, first wins
//   ransac_ops_kernel      sqrt and division as the code above spells them, for the test that pins their rounding
//
// All loops are bounded (Jacobi: 60 sweeps; the rank: N compares per row); nothing polls.  LDS per wave:
// ransac_lds_bytes(cap): 38.5 KB at cap = 1024 (46.7 KB with rd_verify_kernel's gather lists), three waves per CU at the least.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rigid_ransac.hpp"

namespace mmf {

constexpr int kRansacMaxPoints = 1024;
constexpr int kRansacMaxIterations = 32;
constexpr int kRansacAllLane = 32;  // the lane that fits all rows; hypotheses are lanes 0 .. iterations - 1

struct RansacDeviceConfig {
    int iterations;
    float inlier_threshold, inlier_fraction;
    int max_points;               // the table's last N; larger problems are refused
    int cap;                      // LDS capacity in points: max_points rounded up to a multiple of 64
    const unsigned short* table;  // ransac_triple_table(iterations, max_points)
};

// keys [cap] u64 | inlier words [cap / 64][32] u64 | p0s, p1s [cap][3] f32 | hypothesis transforms [32][12] f32 |
// errors [32] f32 | gather lists [2][cap] i32 (rd_verify_kernel only)
__host__ __device__ inline size_t ransac_lds_bytes(int cap, bool lists) {
    return (size_t)cap * 8 + (size_t)cap / 64 * 32 * 8 + (size_t)cap * 24 + 32 * 12 * 4 + 32 * 4 + (lists ? (size_t)cap * 8 : 0);
}

struct RansacLds {
    unsigned long long *keys, *words;
    float *p0s, *p1s, *th, *err;
    int* lists;
    __device__ RansacLds(unsigned char* base, int cap) {
        keys = reinterpret_cast<unsigned long long*>(base);
        words = keys + cap;
        p0s = reinterpret_cast<float*>(words + cap / 64 * 32);
        p1s = p0s + 3 * cap;
        th = p1s + 3 * cap;
        err = th + 32 * 12;
        lists = reinterpret_cast<int*>(err + 32);
    }
};

struct SelBitsOrAll {
    const unsigned long long* words;
    int stride;
    bool all;
    __host__ __device__ bool operator()(int i) const { return all || ((words[(size_t)(i >> 6) * stride] >> (i & 63)) & 1ull); }
};

__device__ inline void ransac_write_identity(mmf_ransac_result* out, int status) {
    for (int k = 0; k < 16; ++k) out->T[k] = (k % 5 == 0) ? 1.f : 0.f;
    out->error = __builtin_inff();
    out->n_inliers = 0, out->has_inlier = 0, out->status = status;
}

// One problem of 3 <= N <= cfg.cap correspondences, all 64 lanes of the wave.  src.row(i, a, b) gives correspondence i
// (p0 row, p1 row).  out and inlier (N bytes, over the hash-sorted rows) may be anywhere the device can write.
template <class Src>
__device__ inline void ransac_wave(const Src& src, int N, const RansacDeviceConfig& cfg, const RansacLds& L, mmf_ransac_result* out,
                                   unsigned char* inlier) {
    using namespace ransac_core;
    const int lane = threadIdx.x;
    // 1. keys, ranks, points in key order
    for (int i = lane; i < N; i += 64) {
        float a[3], b[3];
        src.row(i, a, b);
        L.keys[i] = hash_row(a, b);
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        const unsigned long long k = L.keys[i];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const unsigned long long kj = L.keys[j];
            rank += (kj < k || (kj == k && j < i)) ? 1 : 0;
        }
        float a[3], b[3];
        src.row(i, a, b);
        for (int c = 0; c < 3; ++c) L.p0s[3 * rank + c] = a[c], L.p1s[3 * rank + c] = b[c];
    }
    __syncthreads();
    // 2. the hypotheses
    if (lane < cfg.iterations) {
        const unsigned short* tr = cfg.table + 3 * ((size_t)(N - 3) * cfg.iterations + lane);
        const Isometry3f T = fit_triple(L.p0s, L.p1s, tr[0], tr[1], tr[2]);
        for (int k = 0; k < 9; ++k) L.th[12 * lane + k] = T.R[k];
        for (int k = 0; k < 3; ++k) L.th[12 * lane + 9 + k] = T.t[k];
    }
    __syncthreads();
    // 3. inlier words and counts
    int count = 0;
    for (int h = 0; h < cfg.iterations; ++h) {
        Isometry3f T;
        for (int k = 0; k < 9; ++k) T.R[k] = L.th[12 * h + k];
        for (int k = 0; k < 3; ++k) T.t[k] = L.th[12 * h + 9 + k];
        int c = 0;
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            const bool in = i < N && rigid_distance(T, L.p0s + 3 * i, L.p1s + 3 * i) < cfg.inlier_threshold;
            const unsigned long long w = __ballot(in);
            if (lane == 0) L.words[(size_t)(base >> 6) * 32 + h] = w;
            c += __popcll(w);
        }
        if (lane == h) count = c;
    }
    __syncthreads();
    // 4. refits of the candidates, and the fit to all rows
    const bool candidate = lane < cfg.iterations && count > candidate_floor(cfg.inlier_fraction, N);
    float error = __builtin_inff();
    Isometry3f T;
    if (candidate || lane == kRansacAllLane) {
        float e;
        T = refit_score(L.p0s, L.p1s, N, SelBitsOrAll{L.words + (lane & 31), 32, !candidate}, candidate ? count : N, &e);
        if (candidate) error = e;
    }
    if (lane < 32) L.err[lane] = error;
    __syncthreads();
    // 5. the first smallest error
    int best = -1;
    float best_error = __builtin_inff();
    for (int h = 0; h < cfg.iterations; ++h) {
        const float e = L.err[h];
        if (e < best_error) best_error = e, best = h;
    }
    if (lane == (best < 0 ? kRansacAllLane : best)) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) out->T[4 * r + c] = T.R[3 * r + c];
            out->T[4 * r + 3] = T.t[r];
        }
        out->T[12] = out->T[13] = out->T[14] = 0.f, out->T[15] = 1.f;
        out->error = best_error;
        out->n_inliers = best < 0 ? 0 : count;
        out->has_inlier = best < 0 ? 0 : 1;
        out->status = MMF_RANSAC_OK;
    }
    if (inlier)
        for (int i = lane; i < N; i += 64)
            inlier[i] = best < 0 ? 0 : (unsigned char)((L.words[(size_t)(i >> 6) * 32 + best] >> (i & 63)) & 1ull);
}

struct RansacPackedSrc {
    const float *p0, *p1;  // the problem's first rows
    __device__ void row(int i, float* a, float* b) const {
        for (int c = 0; c < 3; ++c) a[c] = p0[3 * (size_t)i + c], b[c] = p1[3 * (size_t)i + c];
    }
};

// problem p = rows offsets[p] .. offsets[p + 1] of p0 / p1; results[p], inlier[offsets[p] ..]
__global__ __launch_bounds__(64) void ransac_batch_kernel(const float* __restrict__ p0, const float* __restrict__ p1,
                                                          const int* __restrict__ offsets, RansacDeviceConfig cfg,
                                                          mmf_ransac_result* __restrict__ results, unsigned char* __restrict__ inlier) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ransac_smem[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int o = offsets[p], N = offsets[p + 1] - o;
    if (N < 3 || N > cfg.max_points) {  // (uniform)
        if (lane == 0) ransac_write_identity(results + p, N < 3 ? MMF_RANSAC_TOO_FEW : MMF_RANSAC_TOO_MANY);
        for (int i = lane; i < N; i += 64) inlier[(size_t)o + i] = 0;
        return;
    }
    const RansacLds L(ransac_smem, cfg.cap);
    ransac_wave(RansacPackedSrc{p0 + 3 * (size_t)o, p1 + 3 * (size_t)o}, N, cfg, L, results + p, inlier + o);
}

// ---- the view store's verification (redetect_host.hpp) ------------------------------------------------------------------------
struct RdViewDev {
    int model, index, rows;  // as RdView; model < 0: forgotten
    int row0, coord0;
};
struct RdVerifySet {  // one query set of a frame
    const float* coordinate;  // DEVICE [nq][3]
    int nq;
    int q0;  // the set's first query row in the match results
};
struct RdViewResult {
    mmf_ransac_result r;
    int n_matches;
};
struct RdRecord {  // Model::getBestMatch of one (set, model)
    float T[16];
    float error;
    int inliers, view, n_matches, found, model_id;
};
struct RdListSrc {
    const float *query, *train;
    const int *qi, *ti;
    __device__ void row(int k, float* a, float* b) const {
        const size_t q = (size_t)qi[k], t = (size_t)ti[k];
        for (int c = 0; c < 3; ++c) a[c] = query[3 * q + c], b[c] = train[3 * t + c];
    }
};

// block (v, s): view v of the store against set s.  train_row = rd_cross_kernel's rows ([view][query row] per set, at
// V * q0).  Views of models that are not asked for, empty views and views with fewer than 3 matches leave has_inlier = 0
// and return at once.  per_view[s * V + v]; inlier[(s * V + v) * stride ..] over the hash-sorted matches.
__global__ __launch_bounds__(64) void rd_verify_kernel(const RdViewDev* __restrict__ views, int V, const RdVerifySet* __restrict__ sets,
                                                       const int* __restrict__ asked, int n_asked, const int* __restrict__ train_row,
                                                       const float* __restrict__ coords, RansacDeviceConfig cfg,
                                                       RdViewResult* __restrict__ per_view, unsigned char* __restrict__ inlier, int stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ransac_smem[];
    const int v = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const RdViewDev view = views[v];
    const RdVerifySet set = sets[s];
    RdViewResult* out = per_view + (size_t)s * V + v;
    bool wanted = false;
    for (int a = 0; a < n_asked; ++a) wanted = wanted || asked[a] == view.model;
    if (view.model < 0 || view.rows == 0 || !wanted || set.nq < 3 || set.nq > cfg.max_points) {  // (uniform)
        if (lane == 0) out->r.has_inlier = 0, out->r.n_inliers = 0, out->r.error = __builtin_inff(), out->r.status = MMF_RANSAC_TOO_FEW, out->n_matches = 0;
        return;
    }
    const RansacLds L(ransac_smem, cfg.cap);
    int* qi = L.lists;
    int* ti = L.lists + cfg.cap;
    const int* rows = train_row + (size_t)V * set.q0 + (size_t)v * set.nq;
    int N = 0;  // the matched query rows, ascending (Model.cpp:848-856)
    for (int base = 0; base < set.nq; base += 64) {
        const int i = base + lane;
        const int row = i < set.nq ? rows[i] : -1;
        const unsigned long long w = __ballot(row >= 0);
        if (row >= 0) {
            const int k = N + __popcll(w & ((1ull << lane) - 1ull));
            qi[k] = i, ti[k] = view.coord0 + (row - view.row0);
        }
        N += __popcll(w);
    }
    __syncthreads();
    if (N < 3) {
        if (lane == 0) out->r.has_inlier = 0, out->r.n_inliers = 0, out->r.error = __builtin_inff(), out->r.status = MMF_RANSAC_TOO_FEW, out->n_matches = N;
        return;
    }
    if (lane == 0) out->n_matches = N;
    ransac_wave(RdListSrc{set.coordinate, coords, qi, ti}, N, cfg, L, &out->r, inlier + ((size_t)s * V + v) * stride);
}

// block (a, s): Model::getBestMatch of model asked[a] for set s from the per-view estimates: views ascending, estimates
// without inliers dropped (:859), the smallest error, the first of equals (:870-873).  One record per (set, model) and the
// winner's inlier flags go to memory the host reads.
__global__ __launch_bounds__(64) void rd_pick_kernel(const RdViewDev* __restrict__ views, int V, const int* __restrict__ asked, int n_asked,
                                                     const RdViewResult* __restrict__ per_view, const unsigned char* __restrict__ inlier,
                                                     int stride, RdRecord* __restrict__ records,
                                                     unsigned char* __restrict__ record_inlier) {
    const int a = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const int model = asked[a];
    // the wave's lanes take the views 64 at a time; per chunk the first smallest error by a scan of the ballot's lanes
    int best = -1;
    float best_error = 0.f;
    for (int base = 0; base < V; base += 64) {
        const int v = base + lane;
        bool ok = false;
        float e = 0.f;
        if (v < V && model >= 0 && views[v].model == model) {
            const RdViewResult& r = per_view[(size_t)s * V + v];
            ok = r.r.has_inlier != 0 && r.r.n_inliers > 0;
            e = r.r.error;
        }
        unsigned long long w = __ballot(ok);
        while (w) {  // (at most 64 turns, uniform)
            const int l = __ffsll((long long)w) - 1;
            w &= w - 1;
            const float el = __shfl(e, l);
            if (best < 0 || el < best_error) best = base + l, best_error = el;
        }
    }
    RdRecord* rec = records + (size_t)s * n_asked + a;
    if (best < 0) {
        if (lane == 0) {
            for (int k = 0; k < 16; ++k) rec->T[k] = (k % 5 == 0) ? 1.f : 0.f;
            rec->error = __builtin_inff();
            rec->inliers = 0, rec->view = -1, rec->n_matches = 0, rec->found = 0, rec->model_id = model;
        }
        return;
    }
    const RdViewResult& r = per_view[(size_t)s * V + best];
    if (lane == 0) {
        for (int k = 0; k < 16; ++k) rec->T[k] = r.r.T[k];
        rec->error = r.r.error;
        rec->inliers = r.r.n_inliers, rec->view = views[best].index, rec->n_matches = r.n_matches, rec->found = 1, rec->model_id = model;
    }
    const unsigned char* src = inlier + ((size_t)s * V + best) * stride;
    unsigned char* dst = record_inlier + ((size_t)s * n_asked + a) * stride;
    for (int i = lane; i < r.n_matches; i += 64) dst[i] = src[i];
}

// out[i] = op(a[i], b[i]) spelled as rigid_ransac.hpp spells it: 0 sqrt (double), 1 / (double), 2 sqrt (float), 3 rintf,
// 4 / (float), 5 float / int as the error's mean (b holds the ints)
__global__ __launch_bounds__(256) void ransac_ops_kernel(int op, const void* __restrict__ a, const void* __restrict__ b, size_t n,
                                                         void* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *ad = static_cast<const double*>(a), *bd = static_cast<const double*>(b);
    const float *af = static_cast<const float*>(a), *bf = static_cast<const float*>(b);
    if (op == 0) static_cast<double*>(out)[i] = std::sqrt(ad[i]);
    else if (op == 1) static_cast<double*>(out)[i] = ad[i] / bd[i];
    else if (op == 2) static_cast<float*>(out)[i] = std::sqrt(af[i]);
    else if (op == 3) static_cast<float*>(out)[i] = rintf(af[i]);
    else if (op == 4) static_cast<float*>(out)[i] = af[i] / bf[i];
    else static_cast<float*>(out)[i] = af[i] / static_cast<const int*>(b)[i];
}

}  // namespace mmf
