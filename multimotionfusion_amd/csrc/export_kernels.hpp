// export_kernels.hpp -- Model::exportModelPLY's loop (Core/Model/Model.cpp:1547-1594) on the device: the surfels of a store
// whose confidence is above a threshold, in ascending surfel index, as packed 31-byte PLY records
//   x y z (f32) | r g b (u8) | nx ny nz (f32) | radius (f32)
// in three launches whatever the count (export_count_kernel, scan_top_kernel of surfel_kernels.hpp over the per-workgroup
// counts, export_write_kernel).  Textually included by mmf_hip.hip behind surfel_kernels.hpp (SurfelSoA, Mat4).
//
// Arithmetic (the library is built with -ffp-contract=off, the parentheses say the order):
//   position  ((p0 x + p1 y) + p2 z) + p3 per row p of the pose
//   colour    c = (int)colour24; r = c >> 16 & 255, g = c >> 8 & 255, b = c & 255
//   normal    -((r0 nx + r1 ny) + r2 nz) per row r of the pose's upper-left 3 x 3
//   radius    copied
// A record is 31 bytes, 31 = 3 (mod 4): a workgroup's byte range in the output starts at any of the four alignments.  The
// workgroup stages its records in LDS shifted by that alignment, so that an aligned dword of the output is an aligned dword of
// LDS, and stores its range with dword stores, single bytes only at the head (up to 3) and the tail (up to 3).
#pragma once

namespace mmf {

constexpr int kExportBlock = 256;                   // surfels per workgroup = threads per workgroup (four waves of 64)
constexpr int kExportRecord = 31;                   // bytes per record
constexpr int kExportLdsWords = (3 + kExportBlock * kExportRecord + 3) / 4;  // 7 936 B of records + the shift

// strict: a NaN confidence is dropped (Model.cpp:1552)
__device__ __forceinline__ bool export_keeps(float conf, float threshold) { return conf > threshold; }

// the number of kept surfels among the lanes below this one, and -- in *total -- in the workgroup.  wave_counts: 4 words of LDS
__device__ __forceinline__ unsigned export_block_rank(bool keep, unsigned* wave_counts, unsigned* total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(keep ? 1 : 0);
    if (lane == 0) wave_counts[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < kExportBlock / 64; ++w) {
        const unsigned c = wave_counts[w];
        before += w < wave ? c : 0u;
        all += c;
    }
    *total = all;
    return before + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

// launch 1: block_counts[b] = the kept surfels among [256 b, 256 b + 256).  Reads the confidences only (16 B per surfel)
__global__ __launch_bounds__(kExportBlock) void export_count_kernel(SurfelSoA s, unsigned count, float threshold,
                                                                    unsigned* __restrict__ block_counts) {
    __shared__ unsigned wave_counts[kExportBlock / 64];
    const unsigned i = blockIdx.x * kExportBlock + threadIdx.x;
    const bool keep = i < count && export_keeps(s.pos[i].w, threshold);
    unsigned total;
    export_block_rank(keep, wave_counts, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__device__ __forceinline__ void export_put_u32(unsigned char* dst, unsigned v) {
    dst[0] = (unsigned char)(v & 255u), dst[1] = (unsigned char)(v >> 8 & 255u);
    dst[2] = (unsigned char)(v >> 16 & 255u), dst[3] = (unsigned char)(v >> 24);
}
__device__ __forceinline__ void export_put_f32(unsigned char* dst, float v) { export_put_u32(dst, __float_as_uint(v)); }

// launch 3: block_offsets = the exclusive scan of launch 1's counts (scan_top_kernel).  out: 4-byte aligned, room for every
// kept record.  The other 32 bytes of a surfel are read for the kept ones only.
__global__ __launch_bounds__(kExportBlock) void export_write_kernel(SurfelSoA s, unsigned count, float threshold, Mat4 pose,
                                                                    const unsigned* __restrict__ block_offsets,
                                                                    unsigned char* __restrict__ out) {
    __shared__ unsigned wave_counts[kExportBlock / 64];
    __shared__ unsigned lds_words[kExportLdsWords];
    unsigned char* lds = reinterpret_cast<unsigned char*>(lds_words);
    const unsigned t = threadIdx.x, i = blockIdx.x * kExportBlock + t;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep = false;
    if (i < count) {
        p = s.pos[i];
        keep = export_keeps(p.w, threshold);
    }
    unsigned kept;
    const unsigned rank = export_block_rank(keep, wave_counts, &kept);
    if (kept == 0) return;  // (uniform over the workgroup)
    const size_t g0 = (size_t)block_offsets[blockIdx.x] * kExportRecord;  // the workgroup's first byte in the output
    const unsigned shift = (unsigned)(g0 & 3u);                           // LDS byte k + shift = output byte g0 + k
    if (keep) {
        const float colour = s.col[i].x;
        const float4 n = s.nrm[i];
        const float* m = pose.m;
        unsigned char* rec = lds + shift + rank * kExportRecord;
        export_put_f32(rec + 0, ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3]);
        export_put_f32(rec + 4, ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7]);
        export_put_f32(rec + 8, ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]);
        const int c = (int)colour;
        rec[12] = (unsigned char)(c >> 16 & 255), rec[13] = (unsigned char)(c >> 8 & 255), rec[14] = (unsigned char)(c & 255);
        export_put_f32(rec + 15, -((m[0] * n.x + m[1] * n.y) + m[2] * n.z));
        export_put_f32(rec + 19, -((m[4] * n.x + m[5] * n.y) + m[6] * n.z));
        export_put_f32(rec + 23, -((m[8] * n.x + m[9] * n.y) + m[10] * n.z));
        export_put_f32(rec + 27, n.w);
    }
    __syncthreads();
    const unsigned bytes = kept * kExportRecord;
    const unsigned head = min(bytes, (4u - shift) & 3u);  // single bytes up to the first aligned dword of the output
    const unsigned words = (bytes - head) / 4u;
    const unsigned tail = bytes - head - 4u * words;      // ... and behind the last whole one
    if (t < head) out[g0 + t] = lds[shift + t];
    unsigned* out_words = reinterpret_cast<unsigned*>(out + g0 + head);  // (g0 + head) % 4 == 0 == (shift + head) % 4
    const unsigned* src_words = lds_words + (shift + head) / 4u;
    for (unsigned k = t; k < words; k += kExportBlock) out_words[k] = src_words[k];
    if (t < tail) out[g0 + head + 4u * words + t] = lds[shift + head + 4u * words + t];
}

}  // namespace mmf
