// redetect_kernels.hpp -- one query set against EVERY stored keypoint view, in a constant number of launches (gfx950).
//
// Model::getBestMatch (Core/Model/Model.cpp:832-844) calls cv::BFMatcher(cv::NORM_L2, true).match(query, view) once per
// stored view of an inactive model: a model that lived 300 frames has 300 views of a few dozen descriptors, and
// MultiMotionFusion.cpp:494-551 does that for every segment and every inactive model of every frame.  Each of those matches
// is far too small for the device (one or two 32 x 32 tiles), so here they are ONE problem: the views of all models lie in
// one descriptor buffer (the view store, mmf_hip.hip: mmf_viewstore), every view padded to a multiple of 32 rows, so that a
// 32-row train tile belongs to exactly one view and a per-tile table {view, valid rows} is all the kernel needs to know.
//
//   rd_begin_kernel   |q_i|^2 of the query rows (diagonal MFMA tiles, as row_norms_kernel) + reset of the arg-min keys
//   rd_tile_kernel    one wave per (train tile, 32 query rows): the Gram tile by gram_tile (match_kernels.hpp), so every
//                     d2 = (|q|^2 + |t|^2) - 2 <q, t> is the fmaf chain of oracle/mmf_oracle_match.c; row minima per
//                     (view, query row), column minima per train row, as 64-bit atomicMin keys (smallest index wins a tie)
//   rd_cross_kernel   crossCheck per (view, query row), no distance gate (getBestMatch uses none); the result goes to
//                     host memory the device writes
//
// Three launches per query set whatever the number of views or models.  |t_j|^2 of the train rows is computed once, when a
// view is stored (rd_train_norms_kernel).  Rows of padding are masked to +inf before the minima: they never win.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hpp"

namespace mmf {

struct RdTile {
    int view;   // index of the view in the store (all models)
    int valid;  // rows of this tile that hold a descriptor (1 .. 32; the rest is padding)
};

// |t_j|^2 of `nrows` (a multiple of 32) freshly stored train rows; one wave per 32 rows.  Padding rows are zeros: norm 0.
__global__ __launch_bounds__(64) void rd_train_norms_kernel(const float* __restrict__ t, int nrows, int dim, float* __restrict__ tn) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * 32;
    if (i0 + 32 > nrows) return;  // (uniform; nrows % 32 == 0)
    const float* row = t + (size_t)(i0 + r) * dim;
    const f32x16 acc = gram_tile(row, row, dim, h);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int lr = (v & 3) + 8 * (v >> 2) + 4 * h;
        if (lr == r) tn[i0 + r] = acc[v];
    }
}

// blocks [0, qblocks): the query norms; the other blocks: row_best[n_views * nq] and col_best[n_rows] = empty (grid stride)
__global__ __launch_bounds__(64) void rd_begin_kernel(const float* __restrict__ q, int nq, int dim, float* __restrict__ qn,
                                                      unsigned long long* __restrict__ row_best, size_t n_row_keys,
                                                      unsigned long long* __restrict__ col_best, size_t n_col_keys) {
    const int qblocks = (nq + 31) / 32;
    if ((int)blockIdx.x >= qblocks) {
        const size_t stride = (size_t)(gridDim.x - qblocks) * 64;
        for (size_t i = (size_t)(blockIdx.x - qblocks) * 64 + threadIdx.x; i < n_row_keys + n_col_keys; i += stride) {
            if (i < n_row_keys)
                row_best[i] = kNoMatchKey;
            else
                col_best[i - n_row_keys] = kNoMatchKey;
        }
        return;
    }
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * 32;
    const float* row = q + (size_t)min(i0 + r, nq - 1) * dim;
    const f32x16 acc = gram_tile(row, row, dim, h);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int lr = (v & 3) + 8 * (v >> 2) + 4 * h;
        if (lr == r && i0 + r < nq) qn[i0 + r] = acc[v];
    }
}

// grid = (train tiles, ceil(nq / 32)); one wave per 32 x 32 tile of the distance matrix; train tile j covers the store's rows
// [32 j, 32 j + 32), of which the first tiles[j].valid belong to view tiles[j].view.  Keys: row_best[view * nq + i] holds the
// STORE row of the nearest train row (rows of a view are contiguous and ascending: the smallest store row is the smallest
// row of the view), col_best[store row] the nearest query row.
__global__ __launch_bounds__(64) void rd_tile_kernel(const float* __restrict__ q, const float* __restrict__ t,
                                                     const float* __restrict__ qn, const float* __restrict__ tn,
                                                     const RdTile* __restrict__ tiles, int nq, int dim,
                                                     unsigned long long* __restrict__ row_best,
                                                     unsigned long long* __restrict__ col_best) {
    __shared__ float tile[32][33];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const RdTile tl = tiles[blockIdx.x];
    // (train rows of a tile all exist: the padding rows are zeros inside the buffer; query rows past the end are clamped)
    const f32x16 acc = gram_tile(q + (size_t)min(i0 + r, nq - 1) * dim, t + (size_t)(j0 + r) * dim, dim, h);
    const float tnc = tn[j0 + r];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int lr = (v & 3) + 8 * (v >> 2) + 4 * h, row = i0 + lr;
        const float d2 = (qn[min(row, nq - 1)] + tnc) - 2.0f * acc[v];
        tile[lr][r] = (row < nq && r < tl.valid) ? d2 : __builtin_inff();
    }
    __syncthreads();
    float best = __builtin_inff();
    int arg = -1;
#pragma unroll 8
    for (int s = 0; s < 32; ++s) {
        const float d = h ? tile[s][r] : tile[r][s];
        if (d < best) best = d, arg = s;  // first minimum
    }
    if (arg < 0) return;
    if (!h) {
        if (i0 + r < nq)
            atomicMin(&row_best[(size_t)tl.view * nq + i0 + r], ((unsigned long long)ordered_bits(best) << 32) | (unsigned)(j0 + arg));
    } else {
        if (r < tl.valid) atomicMin(&col_best[j0 + r], ((unsigned long long)ordered_bits(best) << 32) | (unsigned)(i0 + arg));
    }
}

// crossCheck for every (view, query row): train_row[v * nq + i] = STORE row of the match or -1, distance = sqrt(max(d2, 0));
// train_row_dev (null unless a verifier is attached to the store): the rows again, in device memory, for rd_verify_kernel
__global__ __launch_bounds__(256) void rd_cross_kernel(const unsigned long long* __restrict__ row_best,
                                                       const unsigned long long* __restrict__ col_best, int nq, size_t n,
                                                       int* __restrict__ train_row, float* __restrict__ distance,
                                                       int* __restrict__ train_row_dev) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int i = (int)(e % (size_t)nq);
    const unsigned long long key = row_best[e];
    int j = -1;
    float d = 0.f;
    if (key != kNoMatchKey) {
        const int cand = (int)(unsigned)key;
        if ((int)(unsigned)col_best[cand] == i) {
            const float d2 = from_ordered_bits((unsigned)(key >> 32));
            d = sqrtf(d2 > 0.f ? d2 : 0.f);
            j = cand;
        }
    }
    train_row[e] = j;
    distance[e] = d;
    if (train_row_dev) train_row_dev[e] = j;
}

// label of every keypoint = the id image at its pixel (MultiMotionFusion.cpp:428-434); -1: outside the image (:432)
__global__ __launch_bounds__(256) void rd_gather_labels_kernel(const uint8_t* __restrict__ mask, int width, int height,
                                                               const int* __restrict__ xy, int n, int* __restrict__ label) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = xy[2 * i], y = xy[2 * i + 1];
    label[i] = (x >= 0 && x < width && y >= 0 && y < height) ? (int)mask[(size_t)y * width + x] : -1;
}

// the packed rows of a model's views (DEVICE, one view after the other) to their places in the store: workgroup = one tile
// of 32 rows, four waves of 64 lanes x 16 B; row j of the tile comes from packed row src0[tile] + j, the rows past the
// tile's valid ones are the zero padding.  dim = 256.
__global__ __launch_bounds__(256) void rd_scatter_views_kernel(const float* __restrict__ packed, const RdTile* __restrict__ tiles,
                                                               const int* __restrict__ src0, float* __restrict__ dst) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tile = blockIdx.x;
    const int valid = tiles[tile].valid;
    const size_t s0 = (size_t)src0[tile];
    for (int j = w; j < 32; j += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < valid) v = reinterpret_cast<const float4*>(packed + (s0 + j) * 256)[lane];
        reinterpret_cast<float4*>(dst + ((size_t)tile * 32 + j) * 256)[lane] = v;
    }
}

}  // namespace mmf
