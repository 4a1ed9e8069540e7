// ferns_kernels.hpp -- the fern keyframe database (Core/Ferns.cpp:72-143, 145-203, 322-337): the encoding of a
// frame's fill-in images into fern codes, the search over the stored keyframes and the decisions of addFrame / findFrame up
// to (not including) the fern odometry.  Textually included from mmf_hip.hip.  One process call is three launches whatever
// the number of ferns, of keyframes and the image size; nothing here waits for the host, the number of keyframes lives on the
// device and the decision to append is taken there.
//
//   ferns_encode_kernel  the small images (GPUResize's nearest sample, DESIGN.md A3 / A7: pixel (i, j) of the w x h image is
//                        the source texel (texel((i + 0.5f) / w, width), texel((j + 0.5f) / h, height)), rows not flipped),
//                        then -- in workgroups of their own -- one lane per fern: the code from the same source texel, a
//                        ballot / popcount per wave of 64 gives the wave's count of good codes
//   ferns_search_kernel  one wave per stored keyframe, four keyframes per workgroup: the current codes once per workgroup in
//                        LDS, the keyframe's row as dwords; co[j] (codes equal and not 255) and both[j] (neither 255) are integer
//                        butterflies over the wave; dissim[j] = (maxCo - co[j]) / maxCo with one correctly rounded division
//   ferns_select_kernel  one workgroup: the minimum of addFrame (over every keyframe) and of findFrame (over the keyframes
//                        older than the time gap) by the order-free rule "lowest dissim, then lowest j", the similarity of
//                        findFrame's keyframe, the result record, and -- when the add rule holds and there is room -- the
//                        copy of the current frame into slot n
//
// Everything that decides is an integer or one IEEE operation: the results do not depend on the launch geometry.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmf {

constexpr int kFernsThreads = 256;
constexpr int kFernsSearchWaves = kFernsThreads / 64;  // keyframes per workgroup of the search
constexpr int kFernsSelectThreads = 1024;
constexpr int kFernsSelectWaves = kFernsSelectThreads / 64;
constexpr int kFernsMaxNum = 16384;  // the current codes of a workgroup of the search live in LDS
constexpr unsigned kFernsBadCode = 255u;

struct FernsGeom {
    int width, height;  // the frame
    int w, h;           // the small images: width / 8, height / 8
    int num;            // ferns
    int stride;         // bytes of a row of codes: num rounded up to dwords, the padding holds kFernsBadCode
    int capacity;       // keyframes
    int image_blocks;   // workgroups of the encode launch that write the small images ...
    int code_blocks;    // ... and that write the codes: code_blocks * 4 waves, each with a count of good codes
};

struct FernsFrame {  // the frame's fill-in images, full size
    const uchar4* image;
    const float4* vert;
    const float4* norm;
};
struct FernsCur {  // the current frame
    uchar4* image;
    float4* vert;
    float4* norm;
    uint8_t* codes;   // [stride]
    int* wave_good;   // [code_blocks * 4]
};
struct FernsDb {  // the stored keyframes, slot by slot
    uint8_t* codes;  // [capacity][stride]
    int* good;
    int* times;
    float* poses;    // [capacity][16]
    uchar4* image;   // [capacity][h][w]
    float4* vert;
    float4* norm;
    int* n;          // keyframes stored
    int* dropped;    // frames the add rule accepted while the database was full
};
struct FernsCall {
    float pose[16];
    int time;
    int flags;  // MMF_FERNS_FIND | MMF_FERNS_ADD
    int min_time_gap;
    float threshold;
    float min_similarity;
};

__device__ __forceinline__ int ferns_texel(float coord, int size) {
    const int t = (int)floorf(coord * (float)size);
    return t < 0 ? 0 : (t > size - 1 ? size - 1 : t);
}
// the source texel of small pixel (i, j)
__device__ __forceinline__ size_t ferns_source(const FernsGeom& g, int i, int j) {
    const float tx = (i + 0.5f) / g.w, ty = (j + 0.5f) / g.h;
    return (size_t)ferns_texel(ty, g.height) * g.width + ferns_texel(tx, g.width);
}
__device__ __forceinline__ int ferns_wave_sum(int v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(kFernsThreads) void ferns_encode_kernel(FernsGeom g, FernsFrame in, const int* __restrict__ table, FernsCur cur) {
    const int b = (int)blockIdx.x;
    if (b < g.image_blocks) {
        const int i = b * kFernsThreads + (int)threadIdx.x;
        if (i >= g.w * g.h) return;
        const size_t t = ferns_source(g, i % g.w, i / g.w);
        cur.image[i] = in.image[t];
        cur.vert[i] = in.vert[t];
        cur.norm[i] = in.norm[t];
        return;
    }
    // one lane per byte of the row of codes: ferns, then the padding
    const int i = (b - g.image_blocks) * kFernsThreads + (int)threadIdx.x;
    unsigned code = kFernsBadCode;
    if (i < g.num) {
        const int* f = table + 6 * (size_t)i;
        const size_t t = ferns_source(g, f[0], f[1]);
        const float z = in.vert[t].z;
        if (z > 0.f) {  // (a NaN compares false)
            const uchar4 p = in.image[t];
            const float mm = z * 1000.0f;
            // a product of 2^31 or more (the conversion is undefined there) counts as greater
            const bool deep = mm >= 2147483648.0f ? true : (int)mm > f[5];
            code = ((int)p.x > f[2] ? 8u : 0u) | ((int)p.y > f[3] ? 4u : 0u) | ((int)p.z > f[4] ? 2u : 0u) | (deep ? 1u : 0u);
        }
    }
    const unsigned long long good = __ballot(code != kFernsBadCode);
    if (i < g.stride) cur.codes[i] = (uint8_t)code;
    if ((threadIdx.x & 63u) == 0u) cur.wave_good[i >> 6] = (int)__popcll(good);
}

// good codes of the current frame: the sum of the encode launch's wave counts, by one wave
__device__ __forceinline__ int ferns_good_cur(const FernsGeom& g, const int* wave_good, int lane) {
    int s = 0;
    for (int k = lane; k < g.code_blocks * kFernsSearchWaves; k += 64) s += wave_good[k];
    return ferns_wave_sum(s);
}

__global__ __launch_bounds__(kFernsThreads) void ferns_search_kernel(FernsGeom g, const uint8_t* __restrict__ cur_codes,
                                                                     const int* __restrict__ wave_good, FernsDb db, int* __restrict__ co,
                                                                     int* __restrict__ both, float* __restrict__ dissim) {
    extern __shared__ uint32_t s_cur[];  // [stride / 4]
    __shared__ int s_good;
    const int n = *db.n;
    const int j0 = (int)blockIdx.x * kFernsSearchWaves;
    if (j0 >= n) return;  // (the whole workgroup: no barrier is passed)
    const int words = g.stride >> 2, lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int d = (int)threadIdx.x; d < words; d += kFernsThreads) s_cur[d] = reinterpret_cast<const uint32_t*>(cur_codes)[d];
    if (wave == 0) {
        const int s = ferns_good_cur(g, wave_good, lane);
        if (lane == 0) s_good = s;
    }
    __syncthreads();
    const int j = j0 + wave;
    if (j >= n) return;
    const uint32_t* row = reinterpret_cast<const uint32_t*>(db.codes + (size_t)j * g.stride);
    int c = 0, bo = 0;
    for (int d = lane; d < words; d += 64) {
        const uint32_t a = s_cur[d], r = row[d];
#pragma unroll
        for (int k = 0; k < 32; k += 8) {
            const unsigned ca = (a >> k) & 255u, cr = (r >> k) & 255u;
            c += (ca != kFernsBadCode && ca == cr) ? 1 : 0;
            bo += (ca != kFernsBadCode && cr != kFernsBadCode) ? 1 : 0;
        }
    }
    c = ferns_wave_sum(c), bo = ferns_wave_sum(bo);
    if (lane == 0) {
        const int gj = db.good[j];
        const float max_co = (float)(s_good < gj ? s_good : gj);
        co[j] = c, both[j] = bo;
        dissim[j] = __fdiv_rn(max_co - (float)c, max_co);  // (0 / 0: NaN, which no comparison accepts)
    }
}

// lowest dissim, then lowest j; (FLT_MAX, -1): none
__device__ __forceinline__ void ferns_take(float& d, int& j, float d2, int j2) {
    if (d2 < d || (d2 == d && j2 >= 0 && (j < 0 || j2 < j))) d = d2, j = j2;
}

__global__ __launch_bounds__(kFernsSelectThreads) void ferns_select_kernel(FernsGeom g, FernsCur cur, FernsDb db, const int* __restrict__ co,
                                                                           const int* __restrict__ both, const float* __restrict__ dissim,
                                                                           FernsCall call, mmf_ferns_result_t* __restrict__ out) {
    __shared__ float s_da[kFernsSelectWaves], s_df[kFernsSelectWaves];
    __shared__ int s_ja[kFernsSelectWaves], s_jf[kFernsSelectWaves], s_good, s_added;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = *db.n;
    if (wave == 0) {
        const int s = ferns_good_cur(g, cur.wave_good, lane);
        if (lane == 0) s_good = s;
    }
    float da = FLT_MAX, df = FLT_MAX;
    int ja = -1, jf = -1;
    for (int j = tid; j < n; j += kFernsSelectThreads) {  // (ascending j per lane: a strict < keeps the lowest)
        const float d = dissim[j];
        if (d < da) da = d, ja = j;
        if (d < df && (long long)call.time - (long long)db.times[j] > (long long)call.min_time_gap) df = d, jf = j;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        ferns_take(da, ja, __shfl_xor(da, m), __shfl_xor(ja, m));
        ferns_take(df, jf, __shfl_xor(df, m), __shfl_xor(jf, m));
    }
    if (lane == 0) s_da[wave] = da, s_ja[wave] = ja, s_df[wave] = df, s_jf[wave] = jf;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kFernsSelectWaves; ++k) ferns_take(da, ja, s_da[k], s_ja[k]), ferns_take(df, jf, s_df[k], s_jf[k]);
        const int good = s_good;
        const bool add = (call.flags & MMF_FERNS_ADD) != 0, find = (call.flags & MMF_FERNS_FIND) != 0;
        // Ferns.cpp:112-128: the minimum is only looked for when the frame has a good code
        const float add_min = (add && good > 0) ? da : FLT_MAX;
        const bool wanted = add && (add_min > call.threshold || n == 0) && good > 0;
        const bool added = wanted && n < g.capacity;
        const int dropped = (wanted && !added) ? atomicAdd(db.dropped, 1) + 1 : *db.dropped;
        const int closest = find ? jf : -1;
        const float sim = closest >= 0 ? __fdiv_rn((float)co[closest], (float)both[closest]) : 0.f;  // blockHDAware (:322-337)
        out->added = added ? 1 : 0;
        out->dropped_total = dropped;
        out->count = n + (added ? 1 : 0);
        out->good_codes = good;
        out->add_minimum = add_min;
        out->closest = closest;
        out->closest_dissim = closest >= 0 ? df : FLT_MAX;
        out->closest_similarity = sim;
        out->candidate = (closest >= 0 && sim > call.min_similarity) ? 1 : 0;
        for (int k = 0; k < 16; ++k) out->closest_pose[k] = closest >= 0 ? db.poses[16 * (size_t)closest + k] : 0.f;
        out->closest_time = closest >= 0 ? db.times[closest] : 0;
        if (added) {
            db.good[n] = good, db.times[n] = call.time;
            for (int k = 0; k < 16; ++k) db.poses[16 * (size_t)n + k] = call.pose[k];
        }
        s_added = added ? 1 : 0;
    }
    __syncthreads();
    if (!s_added) return;
    // the current frame becomes keyframe n (n < capacity)
    const int words = g.stride >> 2, px = g.w * g.h;
    uint32_t* row = reinterpret_cast<uint32_t*>(db.codes + (size_t)n * g.stride);
    for (int d = tid; d < words; d += kFernsSelectThreads) row[d] = reinterpret_cast<const uint32_t*>(cur.codes)[d];
    uchar4* image = db.image + (size_t)n * px;
    float4* vert = db.vert + (size_t)n * px;
    float4* norm = db.norm + (size_t)n * px;
    for (int i = tid; i < px; i += kFernsSelectThreads) image[i] = cur.image[i], vert[i] = cur.vert[i], norm[i] = cur.norm[i];
    if (tid == 0) atomicAdd(db.n, 1);  // (every lane read n in front of the first barrier)
}

}  // namespace mmf
