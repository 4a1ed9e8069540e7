// flowseg_kernels.hpp -- the blob stage of the flow_crf segmentation (Core/Segmentation/Segmentation.cpp:1270-1324; DESIGN.md
// 4.10): from the MAP id image of the flow-CRF inference (flowcrf_kernels.hpp) to the largest blob per model, the filled
// contours, the full-size id image and the model data.  Textually included from mmf_hip.hip.
//
//   fseg_init_kernel     label[i] = i for a cell whose id is in the table, -1 else; ring[i] = its neighbours of the same id
//   fseg_merge_kernel    8-connected cells of one id are united (lock-free union by the smaller index, global memory)
//   fseg_flatten_kernel  label[i] = its root = the component's first cell in raster order ("component")
//   fseg_trace_kernel    one lane per component follows its outer border from that cell exactly as cv::findContours does
//                        (icvFetchContour) and sums the integer shoelace: area2 = 2 contourArea.  The winner of an id is the
//                        maximum of (area2, first cell), one 64-bit integer atomicMax
//   fseg_mark_kernel     one lane per table entry follows the winner's border again and leaves the signed crossings of its
//                        edges with the rows (an edge between rows y and y + 1 counts at its end in row y)
//   fseg_compose_kernel  one wave per row: the winding number of a cell is the sum of the crossings left of it; a cell is in
//                        the filled blob when it is the winner's or its winding number is not 0; ids in ascending order, the
//                        highest wins ("segm"); the stage images "area2" and "winner"
//   fseg_stats_kernel    "full" = segm scaled by 4, cells per entry, and per entry the sums of depth and depth^2 in float64
//   fseg_finish_kernel   the model data, has_new_label and the summary
//
// Everything that decides is an integer.  The two float64 sums per entry follow mask_kernels.hpp (B7): a butterfly over the
// wave, one lane adds to the wave's LDS bin in program order, the four bins are added in wave order into the workgroup's row
// and the rows in workgroup order by the finish launch; the geometry depends on the frame size alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mask_kernels.hpp"  // mask_wave_sum

namespace mmf {

constexpr int kFsegThreads = 256;
constexpr int kFsegStatPix = 4;                                // pixels per thread and load: one cell's row of `full`
constexpr int kFsegStatIters = 4;
constexpr int kFsegStatTile = kFsegThreads * kFsegStatPix * kFsegStatIters;
constexpr uint8_t kFsegNoEntry = 0xff;

struct FsegTable {
    int L;                        // entries: the models in list order, then the new label
    int allow_new;                // the last entry is the new label's
    uint8_t id[kCrfMaxLabels];    // per entry
    uint8_t order[kCrfMaxLabels]; // entries by ascending id (idx_map is a std::map)
    uint8_t entry[256];           // id -> entry, kFsegNoEntry: not in the table
};

// what the host reads back (one pinned copy per run); the public mmf_flowseg_summary
using FsegSummary = mmf_flowseg_summary;

__device__ __forceinline__ int fseg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int fseg_find(const int* label, int a) {
    for (int p = fseg_load(label + a); p != a; p = fseg_load(label + a)) a = p;
    return a;
}
// the set of the larger root is hung under the smaller: a root is its set's smallest index
__device__ __forceinline__ void fseg_unite(int* label, int a, int b) {
    bool done = false;
    while (!done) {
        a = fseg_find(label, a), b = fseg_find(label, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(label + a, b);  // (a > b)
        done = old == a;
        a = old;
    }
}

// label, and ring[i]: which of the eight neighbours carry the cell's id, bit s = direction s in cv::findContours' order: E, NE,
// N, NW, W, SW, S, SE (y grows downwards).  Cells of one id that touch are one component, so this is all a border walk reads.
__global__ __launch_bounds__(kFsegThreads) void fseg_init_kernel(const uint8_t* __restrict__ ids, FsegTable tab, int w, int h,
                                                                 int* __restrict__ label, uint8_t* __restrict__ ring) {
    const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    const uint8_t me = ids[i];
    const bool listed = tab.entry[me] != kFsegNoEntry;
    const int x = i % w, y = i / w;
    unsigned m = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int nx = x + DX[s], ny = y + DY[s];
        if (listed && nx >= 0 && nx < w && ny >= 0 && ny < h && ids[ny * w + nx] == me) m |= 1u << s;
    }
    label[i] = listed ? i : -1;
    ring[i] = (uint8_t)m;
}

__global__ __launch_bounds__(kFsegThreads) void fseg_merge_kernel(const uint8_t* __restrict__ ids, int w, int N, int* label) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (fseg_load(label + i) < 0) return;
    const int x = i % w, y = i / w;
    const uint8_t me = ids[i];
    if (x > 0 && ids[i - 1] == me) fseg_unite(label, i, i - 1);
    if (y > 0) {
        if (ids[i - w] == me) fseg_unite(label, i, i - w);
        if (x > 0 && ids[i - w - 1] == me) fseg_unite(label, i, i - w - 1);
        if (x + 1 < w && ids[i - w + 1] == me) fseg_unite(label, i, i - w + 1);
    }
}

__global__ __launch_bounds__(kFsegThreads) void fseg_flatten_kernel(int N, const int* label, int* __restrict__ comp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    comp[i] = fseg_load(label + i) < 0 ? -1 : fseg_find(label, i);
}

// icvFetchContour (outer border) from the component's first cell.  MARK: leave the crossings in `cross` instead of returning
// the area.  Returns |sum (x_k y_k+1 - x_k+1 y_k)| = 2 contourArea.
template <bool MARK>
__device__ __forceinline__ int fseg_follow(const uint8_t* __restrict__ ring8, int w, int n, int root, int8_t* cross) {
    const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    const int x0 = root % w, y0 = root / w;
    unsigned ring = ring8[root];
    if (ring == 0u) return 0;  // a single cell: one point, area 0, no edge
    int s = 4;                 // clockwise from the west neighbour, which is no cell of the component
    do s = (s - 1) & 7;
    while (!(ring >> s & 1u));
    const int x1 = x0 + DX[s], y1 = y0 + DY[s];
    int x3 = x0, y3 = y0;
    long long sum = 0;
    const long long limit = 8ll * n + 8;  // (a cell is left in a direction once: the guard never fires)
    for (long long step = 0; step < limit; ++step) {
        do s = (s + 1) & 7;  // counter-clockwise from the direction after the one it came from
        while (!(ring >> s & 1u));
        const int x4 = x3 + DX[s], y4 = y3 + DY[s];
        sum += (long long)x3 * y4 - (long long)x4 * y3;
        if (MARK && y4 != y3) {
            if (y4 > y3) cross[y3 * w + x3] += 1;
            else cross[y4 * w + x4] -= 1;
        }
        if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
        x3 = x4, y3 = y4, s = (s + 4) & 7;
        ring = ring8[y3 * w + x3];
    }
    return (int)(sum < 0 ? -sum : sum);
}

// best[e] = max over the components of entry e of ((area2 << 32 | first cell) + 1); 0: the id has no cell
__global__ __launch_bounds__(64) void fseg_trace_kernel(const uint8_t* __restrict__ ids, const int* __restrict__ comp,
                                                        const uint8_t* __restrict__ ring, FsegTable tab, int w, int h,
                                                        int* __restrict__ area2, unsigned long long* best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h || comp[i] != i) return;
    const int a2 = fseg_follow<false>(ring, w, w * h, i, nullptr);
    area2[i] = a2;
    atomicMax(best + tab.entry[ids[i]], ((unsigned long long)(unsigned)a2 << 32 | (unsigned)i) + 1ull);
}

__global__ __launch_bounds__(64) void fseg_mark_kernel(const uint8_t* __restrict__ ring, int L, int w, int h,
                                                       const unsigned long long* __restrict__ best, int8_t* cross) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L || best[e] == 0ull) return;
    const int root = (int)(unsigned)((best[e] - 1ull) & 0xffffffffull);
    (void)fseg_follow<true>(ring, w, w * h, root, cross + (size_t)e * w * h);
}

// One wave per row.
__global__ __launch_bounds__(64) void fseg_compose_kernel(const uint8_t* __restrict__ ids, const int* __restrict__ comp,
                                                          const int* __restrict__ area2, FsegTable tab, int w, int h,
                                                          const unsigned long long* __restrict__ best, const int8_t* __restrict__ cross,
                                                          uint8_t* segm, int* __restrict__ area2_cell, uint8_t* __restrict__ winner) {
    const int y = blockIdx.x, lane = threadIdx.x, N = w * h;
    for (int x = lane; x < w; x += 64) {
        const int i = y * w + x, c = comp[i];
        segm[i] = 0;
        area2_cell[i] = c >= 0 ? area2[c] : 0;
        winner[i] = c >= 0 && (int)(unsigned)((best[tab.entry[ids[i]]] - 1ull) & 0xffffffffull) == c ? 1 : 0;
    }
    for (int k = 0; k < tab.L; ++k) {
        const int e = tab.order[k];
        const unsigned long long b = best[e];
        if (b == 0ull) continue;  // (uniform: the whole wave)
        const int root = (int)(unsigned)((b - 1ull) & 0xffffffffull);
        const int8_t* cr = cross + (size_t)e * N + (size_t)y * w;
        int carry = 0;
        for (int x0 = 0; x0 < w; x0 += 64) {
            const int x = x0 + lane;
            const int c = x < w ? (int)cr[x] : 0;
            int incl = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off);
                if (lane >= off) incl += up;
            }
            const int wind = carry + incl - c;  // crossings strictly left of the cell
            if (x < w && (comp[y * w + x] == root || wind != 0)) segm[y * w + x] = tab.id[e];
            carry += __shfl(incl, 63);
        }
    }
}

// `full` and the per-entry cells and depth sums.  A thread takes the four pixels of one cell's row.  slab: [workgroup][2][32].
template <bool VEC>
__global__ __launch_bounds__(kFsegThreads) void fseg_stats_kernel(const uint8_t* __restrict__ segm, const float* __restrict__ depth,
                                                                  FsegTable tab, int W, int H, uint8_t* __restrict__ full,
                                                                  double* __restrict__ slab, unsigned* g_pix) {
    __shared__ double s_sum[kFsegThreads / 64][2][kCrfMaxLabels];
    __shared__ unsigned s_pix[kCrfMaxLabels];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2 * kCrfMaxLabels)
        for (int v = 0; v < kFsegThreads / 64; ++v) s_sum[v][tid / kCrfMaxLabels][tid % kCrfMaxLabels] = 0.0;
    if (tid < kCrfMaxLabels) s_pix[tid] = 0u;
    __syncthreads();
    const long long n = (long long)W * H, tile0 = (long long)blockIdx.x * kFsegStatTile;
    const int w = W / 4;
#pragma unroll 1
    for (int it = 0; it < kFsegStatIters; ++it) {
        const long long p0 = tile0 + (long long)it * (kFsegThreads * kFsegStatPix) + (long long)tid * kFsegStatPix;
        int e = -1;
        double s1 = 0.0, s2 = 0.0;
        if (p0 < n) {  // (4 divides W: the four pixels are one row's)
            const int y = (int)(p0 / W), x = (int)(p0 % W);
            const uint8_t id = segm[(y / 4) * w + x / 4];
            float d[4];
            if (VEC) {
                const float4 d4 = *reinterpret_cast<const float4*>(depth + p0);
                d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
                *reinterpret_cast<uchar4*>(full + p0) = make_uchar4(id, id, id, id);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = depth[p0 + k], full[p0 + k] = id;
            }
            const int ent = tab.entry[id];
            if (ent != kFsegNoEntry) {
                e = ent;
                const double a = d[0], b = d[1], c = d[2], g = d[3];
                s1 = ((a + b) + c) + g;
                s2 = ((a * a + b * b) + c * c) + g * g;
            }
        }
        unsigned long long todo = __ballot(e >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int cur = __shfl(e, leader);
            const bool mine = e == cur;
            const unsigned long long who = __ballot(mine);
            const double t1 = mask_wave_sum(mine ? s1 : 0.0), t2 = mask_wave_sum(mine ? s2 : 0.0);
            if (lane == leader) {
                s_sum[wave][0][cur] += t1, s_sum[wave][1][cur] += t2;
                atomicAdd(&s_pix[cur], (unsigned)__popcll(who) * 4u);
            }
            todo &= ~who;
        }
    }
    __syncthreads();
    if (tid < 2 * kCrfMaxLabels) {
        const int q = tid / kCrfMaxLabels, l = tid % kCrfMaxLabels;
        slab[(size_t)blockIdx.x * 2 * kCrfMaxLabels + tid] = ((s_sum[0][q][l] + s_sum[1][q][l]) + s_sum[2][q][l]) + s_sum[3][q][l];
    }
    if (tid < kCrfMaxLabels && s_pix[tid]) atomicAdd(g_pix + tid, s_pix[tid]);
}

// One wave, lane = entry.
__global__ __launch_bounds__(64) void fseg_finish_kernel(FsegTable tab, int w, int h, float new_model_size, float avg_confidence,
                                                         const double* __restrict__ slab, int nwg, const unsigned* __restrict__ g_pix,
                                                         const unsigned long long* __restrict__ best, FsegSummary* __restrict__ out) {
    const int l = threadIdx.x;
    if (l >= kCrfMaxLabels) return;
    mmf_segmentation_model m{};
    int a2 = 0, first = -1;
    if (l < tab.L) {
        double s1 = 0.0, s2 = 0.0;
        for (int g = 0; g < nwg; ++g) s1 += slab[(size_t)g * 2 * kCrfMaxLabels + l], s2 += slab[(size_t)g * 2 * kCrfMaxLabels + kCrfMaxLabels + l];
        const unsigned long long b = best[l];
        if (b) a2 = (int)((b - 1ull) >> 32), first = (int)(unsigned)((b - 1ull) & 0xffffffffull);
        const unsigned count = (unsigned)(a2 >> 1) + ((a2 & 1) & (a2 >> 1 & 1));  // rint(area2 / 2): a half goes to the even side
        const unsigned n = g_pix[l];
        m.id = tab.id[l];
        m.super_pixel_count = (unsigned)((float)count * 16.0f);
        m.avg_confidence = avg_confidence;
        if (n) {
            const double mean = s1 / (double)n, var = s2 / (double)n - mean * mean;
            m.depth_mean = (float)mean;
            m.depth_std = (float)__builtin_sqrt(var > 0.0 ? var : 0.0);
        }
    }
    out->models[l] = m, out->area2[l] = a2, out->first_cell[l] = first;
    if (l == 0) {
        const unsigned cells = tab.allow_new ? g_pix[tab.L - 1] / 16u : 0u;
        const int has_new = tab.allow_new && (float)cells / (float)(w * h) > new_model_size ? 1 : 0;
        out->allow_new = tab.allow_new, out->has_new_label = has_new, out->new_cells = cells;
        out->n_entries = tab.L - (tab.allow_new && !has_new ? 1 : 0);
    }
}

}  // namespace mmf
