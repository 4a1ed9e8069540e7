// import_kernels.hpp -- the inverse of export_write_kernel (export_kernels.hpp): packed 31-byte PLY records
//   x y z (f32) | r g b (u8) | nx ny nz (f32) | radius (f32)
// become the surfels of a store, record i -> surfel i, in ONE launch whatever the count; and the timestamps of a store set to
// one time, in one launch.  Textually included by export_host.hpp behind export_kernels.hpp (kExportBlock, kExportRecord).
// The reference restores no surfels: the confidence and both times are the caller's.
//
// Arithmetic (the library is built with -ffp-contract=off, the parentheses say the order) -- the export's:
//   position  ((q0 x + q1 y) + q2 z) + q3 per row q of the pose
//   normal    -((r0 nx + r1 ny) + r2 nz) per row r of the pose's upper-left 3 x 3 (the export negates, so does the import)
//   colour    colour24 = (float)(r << 16 | g << 8 | b), exact (< 2^24); the colour vector's second component is 0
//   radius    copied;  confidence, initTime = timestamp = time: the launch's arguments
// Layout: a workgroup of 256 threads owns 256 records = 7 936 bytes = 1 984 dwords = 496 x 16 bytes, so with a 16-byte
// aligned base EVERY workgroup's byte range starts 16-byte aligned (the export's ranges start wherever the kept records
// before them end: there the count of records per workgroup varies, here it is 256).  Only the last range ends ragged, at
// 31 n mod 4.  The range comes into LDS with 16-byte loads, dword loads behind the last whole 16 bytes; the last dword may
// reach up to three bytes past the records into the buffer's padding, which no decoded field reads.  A thread then takes
// its record from LDS: a field at byte b is the dwords b / 4 and b / 4 + 1 shifted by b mod 4 bytes.
#pragma once

namespace mmf {

constexpr int kImportRangeWords = kExportBlock * kExportRecord / 4;  // 1 984: a workgroup's records
constexpr int kImportLdsWords = kImportRangeWords + 4;               // + the dword a field at shift 0 names but does not use
static_assert(kExportBlock * kExportRecord % 16 == 0, "a workgroup's byte range starts 16-byte aligned");

// the four bytes at byte `b` of the staged range, little endian.  b mod 4 == 0: the second dword is shifted out entirely
__device__ __forceinline__ unsigned import_get_u32(const unsigned* lds_words, unsigned b) {
    return __builtin_amdgcn_alignbyte(lds_words[(b >> 2) + 1], lds_words[b >> 2], b & 3u);
}
__device__ __forceinline__ float import_get_f32(const unsigned* lds_words, unsigned b) { return __uint_as_float(import_get_u32(lds_words, b)); }

// words: the records as dwords, 16-byte aligned, (31 n + 3) / 4 of them readable.  dst: room for n surfels
__global__ __launch_bounds__(kExportBlock) void import_unpack_kernel(const unsigned* __restrict__ words, unsigned n, Mat4 pose,
                                                                    float confidence, float time, SurfelSoA dst) {
    __shared__ __align__(16) unsigned lds_words[kImportLdsWords];
    const unsigned t = threadIdx.x, first = blockIdx.x * kExportBlock;
    if (first >= n) return;  // (uniform over the workgroup; the grid has no such workgroup)
    const unsigned here = min((unsigned)kExportBlock, n - first);
    const unsigned n_words = (here * kExportRecord + 3u) / 4u, n_quads = n_words / 4u;
    const unsigned* src = words + (size_t)blockIdx.x * kImportRangeWords;
    const uint4* src4 = reinterpret_cast<const uint4*>(src);
    uint4* lds4 = reinterpret_cast<uint4*>(lds_words);
    for (unsigned k = t; k < n_quads; k += kExportBlock) lds4[k] = src4[k];
    for (unsigned k = 4u * n_quads + t; k < n_words; k += kExportBlock) lds_words[k] = src[k];
    __syncthreads();
    if (t >= here) return;
    const unsigned b = t * kExportRecord;
    const float x = import_get_f32(lds_words, b + 0), y = import_get_f32(lds_words, b + 4), z = import_get_f32(lds_words, b + 8);
    const unsigned rgb = import_get_u32(lds_words, b + 12);  // r | g << 8 | b << 16 | the normal's first byte << 24
    const float nx = import_get_f32(lds_words, b + 15), ny = import_get_f32(lds_words, b + 19), nz = import_get_f32(lds_words, b + 23);
    const float radius = import_get_f32(lds_words, b + 27);
    const float* m = pose.m;
    const unsigned i = first + t;
    dst.pos[i] = make_float4(((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                             ((m[8] * x + m[9] * y) + m[10] * z) + m[11], confidence);
    const unsigned colour24 = (rgb & 255u) << 16 | (rgb & 0xff00u) | (rgb >> 16 & 255u);
    dst.col[i] = make_float4((float)colour24, 0.f, time, time);
    dst.nrm[i] = make_float4(-((m[0] * nx + m[1] * ny) + m[2] * nz), -((m[4] * nx + m[5] * ny) + m[6] * nz),
                             -((m[8] * nx + m[9] * ny) + m[10] * nz), radius);
}

// the timestamp (the colour vector's fourth component) of the first `count` surfels; initTime and everything else stay
__global__ __launch_bounds__(kExportBlock) void import_stamp_kernel(float4* __restrict__ col, unsigned count, float time) {
    const unsigned i = blockIdx.x * kExportBlock + threadIdx.x;
    if (i < count) col[i].w = time;
}

}  // namespace mmf
