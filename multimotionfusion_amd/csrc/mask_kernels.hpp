// mask_kernels.hpp -- the segmentation from a frame's GIVEN label image: the first branch of
// Segmentation::performSegmentation (Core/Segmentation/Segmentation.cpp:89-147: `frame.mask.total() != 0`), on the device.
// Textually included from mmf_hip.hip.
//
//   mask_bins_kernel<PASS 1>   per input label (256 bins): pixels, sum of depth, smallest pixel index (:106-123, :132-136)
//   mask_decide_kernel         one workgroup, a thread per label: the raster-first unmapped label becomes the new one
//                              (:114-118), the label -> id and label -> entry lookups, counts and depth means per entry (:137)
//   mask_bins_kernel<PASS 2>   writes the id image through the lookup (:109-118) and sums |mean - depth| per label (:139-142)
//   mask_finish_kernel         depth_std per entry (:143-144), the model data (:125-129), the table; re-arms the integer bins
//
// Determinism: the float sums are float64 and no float atomic takes part.  A wave adds the values of its lanes
// that carry one label by a butterfly over all 64 lanes (the other lanes add 0.0) and ONE lane adds the result to the wave's
// own LDS bin, in program order; a workgroup's four bins are added ((w0 + w1) + w2) + w3 into its row of the slab and the
// rows are added in workgroup order by the next one-workgroup launch.  Pixel counts and first indices are integer atomics
// (LDS, then global).  The launch geometry depends on W*H only, so one input gives one bit pattern.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmf {

constexpr int kMaskThreads = 256;
constexpr int kMaskVec = 4;                                     // pixels per load
constexpr int kMaskIters = 4;                                   // loads per thread
constexpr int kMaskTile = kMaskThreads * kMaskVec * kMaskIters;  // pixels per workgroup
constexpr unsigned kMaskNoIndex = 0xffffffffu;
constexpr uint16_t kMaskNoEntryWide = 0xffffu;  // (16 bits: 255 models + the new label are the entries 0 .. 255)

struct MaskArgs {
    int n;            // W * H
    int n_models;     // M: active models in list order
    int allow_new;
    unsigned next_id;
    uint8_t ids[256];      // [M]
    uint8_t mapping[256];  // the table as the frame finds it
};

// what the decide launch leaves for pass 2 and the finish launch
struct MaskPlan {
    uint8_t mask_value[256];  // per label: the id its pixels get
    uint16_t entry[256];      // per label: index into the model data, kMaskNoEntryWide = its id is in no entry (B7, deviation 2)
    float label_mean[256];    // per label: depth_mean of its entry
    unsigned entry_n[256];    // per entry: pixels whose output id is the entry's (the depth statistics' n)
    unsigned entry_pix[256];  // per entry: outIdsArray[id] (:112, :118, :121)
    float entry_mean[256];
    uint8_t mapping[256];     // the table after this frame
    int n_entries, has_new_label, new_label;
};

// what the host reads back (one pinned copy per call)
struct MaskSummary {
    int has_new_label, new_label, n_models_out, allow_new;
    uint8_t mapping[256];
    mmf_segmentation_model models[256];
};

__device__ __forceinline__ double mask_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One wave, one pixel per lane (label < 0: no pixel): per distinct label the butterfly sum of `val` goes into bin[label];
// with COUNT the number of pixels and the smallest pixel index go into the workgroup's integer bins.
template <bool COUNT>
__device__ __forceinline__ void mask_wave_bin(int label, double val, unsigned pix, unsigned npix_each, int lane, volatile double* bin,
                                              unsigned* s_cnt, unsigned* s_min) {
    unsigned long long todo = __ballot(label >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int cur = __shfl(label, leader);
        const bool mine = label == cur;
        const unsigned long long who = __ballot(mine);
        const double s = mask_wave_sum(mine ? val : 0.0);
        if (lane == leader) {
            bin[cur] += s;
            if (COUNT) {
                atomicAdd(&s_cnt[cur], (unsigned)__popcll(who) * npix_each);
                atomicMin(&s_min[cur], pix);  // (the leader is the lowest lane: its pixel is the wave's first of this label)
            }
        }
        todo &= ~who;
    }
}

// PASS 1: bins of {pixels, sum depth, first index} per label.  PASS 2: mask_out through the plan, bins of sum |mean - d|.
// VEC: labels / mask_out are 4-byte and depth 16-byte aligned (the loads are one dword / one dwordx4 per lane); otherwise
// the same pixels in the same order by scalar loads -- same sums, bit for bit.
template <int PASS, bool VEC>
__global__ __launch_bounds__(kMaskThreads) void mask_bins_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ depth,
                                                                 int n, const MaskPlan* __restrict__ plan, uint8_t* __restrict__ mask_out,
                                                                 double* __restrict__ slab, unsigned* __restrict__ g_cnt,
                                                                 unsigned* __restrict__ g_min) {
    __shared__ double s_sum[kMaskThreads / 64][256];
    __shared__ unsigned s_cnt[256], s_min[256];
    __shared__ float s_mean[256];
    __shared__ uint8_t s_val[256];
    __shared__ uint16_t s_ent[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < kMaskThreads / 64; ++w) s_sum[w][tid] = 0.0;
    if (PASS == 1) {
        s_cnt[tid] = 0u, s_min[tid] = kMaskNoIndex;
    } else {
        s_mean[tid] = plan->label_mean[tid], s_val[tid] = plan->mask_value[tid], s_ent[tid] = plan->entry[tid];
    }
    __syncthreads();
    volatile double* bin = s_sum[wave];
    const long long tile0 = (long long)blockIdx.x * kMaskTile;
#pragma unroll 1
    for (int it = 0; it < kMaskIters; ++it) {
        const long long p0 = tile0 + (long long)it * (kMaskThreads * kMaskVec) + (long long)tid * kMaskVec;
        int lab[kMaskVec];
        float d[kMaskVec];
        if (p0 + kMaskVec <= (long long)n) {
            if (VEC) {
                const uchar4 l4 = *reinterpret_cast<const uchar4*>(labels + p0);
                const float4 d4 = *reinterpret_cast<const float4*>(depth + p0);
                lab[0] = l4.x, lab[1] = l4.y, lab[2] = l4.z, lab[3] = l4.w;
                d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
            } else {
#pragma unroll
                for (int k = 0; k < kMaskVec; ++k) lab[k] = labels[p0 + k], d[k] = depth[p0 + k];
            }
        } else {  // the ragged tail of the image
#pragma unroll
            for (int k = 0; k < kMaskVec; ++k) {
                const bool in = p0 + k < (long long)n;
                lab[k] = in ? (int)labels[p0 + k] : -1;
                d[k] = in ? depth[p0 + k] : 0.f;
            }
        }
        double v[kMaskVec];
        if (PASS == 1) {
#pragma unroll
            for (int k = 0; k < kMaskVec; ++k) v[k] = (double)d[k];
        } else {
            uint8_t o[kMaskVec];
#pragma unroll
            for (int k = 0; k < kMaskVec; ++k) {
                const int l = lab[k] < 0 ? 0 : lab[k];
                o[k] = s_val[l];
                // (:141) one float32 subtraction of the rounded mean; labels without an entry take part in no statistics
                v[k] = s_ent[l] != kMaskNoEntryWide ? (double)fabsf(s_mean[l] - d[k]) : 0.0;
            }
            if (p0 + kMaskVec <= (long long)n) {
                if (VEC) {
                    *reinterpret_cast<uchar4*>(mask_out + p0) = make_uchar4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < kMaskVec; ++k) mask_out[p0 + k] = o[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < kMaskVec; ++k)
                    if (p0 + k < (long long)n) mask_out[p0 + k] = o[k];
            }
        }
        // the usual case -- the wave's 256 pixels carry one label -- takes one butterfly instead of four
        const bool same4 = lab[0] >= 0 && lab[0] == lab[1] && lab[0] == lab[2] && lab[0] == lab[3];
        const int first = __shfl(lab[0], 0);
        if (__all(same4 && lab[0] == first)) {
            mask_wave_bin<PASS == 1>(lab[0], ((v[0] + v[1]) + v[2]) + v[3], (unsigned)p0, kMaskVec, lane, bin, s_cnt, s_min);
        } else {
#pragma unroll
            for (int k = 0; k < kMaskVec; ++k) mask_wave_bin<PASS == 1>(lab[k], v[k], (unsigned)(p0 + k), 1u, lane, bin, s_cnt, s_min);
        }
    }
    __syncthreads();
    slab[(size_t)blockIdx.x * 256 + tid] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
    if (PASS == 1 && s_cnt[tid]) {
        atomicAdd(&g_cnt[tid], s_cnt[tid]);
        atomicMin(&g_min[tid], s_min[tid]);
    }
}

// One workgroup of 256, thread = label (then thread = entry).  g_cnt / g_min: pass 1's integer bins; slab = pass 1's rows.
__global__ __launch_bounds__(256) void mask_decide_kernel(MaskArgs a, const double* __restrict__ slab, int nwg,
                                                          const unsigned* __restrict__ g_cnt, const unsigned* __restrict__ g_min,
                                                          MaskPlan* __restrict__ plan) {
    __shared__ double s_sum[256];
    __shared__ unsigned s_cnt[256];
    __shared__ uint16_t s_ent[256], s_id2e[256];
    __shared__ uint8_t s_counted[256];
    __shared__ float s_mean[256];
    __shared__ unsigned s_newmin;
    __shared__ int s_newlabel;
    const int l = threadIdx.x;
    double sum = 0.0;
    for (int w = 0; w < nwg; ++w) sum += slab[(size_t)w * 256 + l];  // workgroup order
    const unsigned cnt = g_cnt[l], first = g_min[l];
    unsigned map = a.mapping[l];
    const bool unmapped = l != 0 && map == 0u && cnt > 0u;
    if (l == 0) s_newmin = kMaskNoIndex, s_newlabel = -1;
    s_id2e[l] = kMaskNoEntryWide;
    __syncthreads();
    if (a.allow_new && unmapped) atomicMin(&s_newmin, first);  // (:114: the first unmapped pixel in raster order)
    if (l < a.n_models) s_id2e[a.ids[l]] = (uint16_t)l;       // modelIdToIndex (:98-100)
    __syncthreads();
    const bool has_new = a.allow_new && s_newmin != kMaskNoIndex;
    if (has_new && unmapped && first == s_newmin) {  // (first indices are distinct: one label)
        map = a.next_id;                             // (:116)
        s_newlabel = l;
    }
    if (l == 0 && has_new) s_id2e[a.next_id] = (uint16_t)a.n_models;  // (:101; the host refuses a next_id that is a model's)
    __syncthreads();
    const unsigned val = l == 0 ? 0u : map;  // (:108: label 0 never reads the table)
    s_ent[l] = s_id2e[val];
    s_counted[l] = (l == 0 || val != 0u) ? 1 : 0;  // (:108-119: an unmapped label that stays unmapped increments nothing)
    s_sum[l] = sum, s_cnt[l] = cnt;
    __syncthreads();
    const int entries = a.n_models + (has_new ? 1 : 0);
    float mean = 0.f;
    if (l < entries) {
        unsigned n = 0u, pix = 0u;
        double s = 0.0;
        for (int j = 0; j < 256; ++j)  // label order
            if (s_ent[j] == (uint16_t)l) {
                n += s_cnt[j];
                if (s_counted[j]) pix += s_cnt[j];
                s += s_sum[j];
            }
        mean = n ? (float)(s / (double)n) : 0.f;  // (:137)
        plan->entry_n[l] = n, plan->entry_pix[l] = pix, plan->entry_mean[l] = mean;
    }
    s_mean[l] = mean;
    __syncthreads();
    plan->mask_value[l] = (uint8_t)val;
    plan->entry[l] = s_ent[l];
    plan->label_mean[l] = s_ent[l] != kMaskNoEntryWide ? s_mean[s_ent[l]] : 0.f;
    plan->mapping[l] = (uint8_t)map;
    if (l == 0) plan->n_entries = entries, plan->has_new_label = has_new ? 1 : 0, plan->new_label = s_newlabel;
}

// One workgroup of 256.  slab = pass 2's rows.  Leaves the integer bins as pass 1 of the next call expects them.
__global__ __launch_bounds__(256) void mask_finish_kernel(MaskArgs a, const double* __restrict__ slab, int nwg,
                                                          const MaskPlan* __restrict__ plan, unsigned* __restrict__ g_cnt,
                                                          unsigned* __restrict__ g_min, MaskSummary* __restrict__ out) {
    __shared__ double s_sum[256];
    __shared__ uint16_t s_ent[256];
    const int l = threadIdx.x;
    double sum = 0.0;
    for (int w = 0; w < nwg; ++w) sum += slab[(size_t)w * 256 + l];
    s_sum[l] = sum, s_ent[l] = plan->entry[l];
    __syncthreads();
    const int entries = plan->n_entries;
    if (l < entries) {
        double s = 0.0;
        for (int j = 0; j < 256; ++j)
            if (s_ent[j] == (uint16_t)l) s += s_sum[j];
        const unsigned n = plan->entry_n[l], spc = plan->entry_pix[l] / (16u * 16u);
        mmf_segmentation_model m;
        m.id = l < a.n_models ? (unsigned)a.ids[l] : a.next_id;
        m.super_pixel_count = l < a.n_models ? spc : (spc > 1u ? spc : 1u);  // (:126, :129)
        m.avg_confidence = 0.4f;
        m.depth_mean = plan->entry_mean[l];
        m.depth_std = n ? (float)(s / (double)n) : 0.f;  // (:144)
        out->models[l] = m;
    }
    out->mapping[l] = plan->mapping[l];
    if (l == 0) {
        out->has_new_label = plan->has_new_label, out->new_label = plan->new_label;
        out->n_models_out = entries, out->allow_new = a.allow_new;
    }
    g_cnt[l] = 0u, g_min[l] = kMaskNoIndex;
}

}  // namespace mmf
