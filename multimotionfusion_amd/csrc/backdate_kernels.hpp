// backdate_kernels.hpp -- the device side of Model::refineTrackSubset (Core/Model/Model.cpp:649-737): the back-dated pose list
// a spawned model brings, from the tracker's table and view log (tracker_kernels.hpp).  DESIGN.md B9, 4.12.
//
// The WINDOW is the last `len` logged frames, entry j = the frame with stamp s - len + 1 + j (s = the newest).  The host knows
// a bound of len (history and what the ring holds); the table's common track length, which bounds it too, is known to the
// device alone, so every kernel derives len itself from the head record and the chain kernel reports it.
//
// Three launches whatever len, the number of tracks and the slot counts are:
//   mark    workgroup j = window frame j: for every table row the index of its keypoint in that frame's slot
//   chain   one workgroup: the reference's chain rule over the counts, into one record (pinned + device)
//   gather  workgroup b = entry b + 1: the rows of its problem, in table order, behind the problems before it
// No atomics, no memset: every cell a later kernel reads has been written by an earlier one of the same call.
#pragma once
#include "tracker_kernels.hpp"

namespace mmf {

constexpr int kTrkBackdateMax = 256;  // the longest window (mmf_tracker_backdate: history above it is refused)
constexpr int kBdNull = -1;           // ent: the track has no keypoint in the frame (or is not of the segment)
constexpr int kBdNotFinite = -2;      // ent: it has one whose coordinate is not finite

struct TrkBackdate {  // what the chain kernel reports: pinned host memory and a device copy the gather kernel reads
    int len;          // entries of the window, >= 1
    int n_problems;   // entries with status 0 behind entry 0
    int rows;         // rows of all problems
    int n_tracks;     // the table's rows
    int from[kTrkBackdateMax], both[kTrkBackdateMax], nvalid[kTrkBackdateMax], status[kTrkBackdateMax];
    int offset[kTrkBackdateMax + 1];  // exclusive: the first row of entry j's problem; offset[len] = rows
};

// len of this call: the host's bound (history, the ring) cut by the table's common track length; never below 1
__device__ __forceinline__ int bd_window(const TrkTable& T, int bound) {
    const int nt = min(T.head->n_tracks, T.capacity);
    return max(1, min(min(bound, kTrkBackdateMax), nt > 0 ? T.head->length : 0));
}

// the rows of slot `slot` when it carries frame `stamp`, else 0 (a frame the ring does not hold has no keypoints)
__device__ __forceinline__ int bd_slot_count(const TrkLog& L, int slot, long long stamp) {
    return (slot >= 0 && slot < L.frames && L.stamp[slot] == stamp) ? min(max(L.count[slot], 0), L.max_kp) : 0;
}

// mark: ent[j][i] = the index, in the slot of window frame j, of the keypoint of table row i (binary search of the row's
// uid: a slot is in table order = uid ascending), kBdNotFinite when its logged coordinate has a non-finite component,
// kBdNull when the frame has none or the row does not carry `label`.  Every cell of the rows below n_tracks is written.
__global__ __launch_bounds__(kTrkBlock) void trk_backdate_mark_kernel(TrkTable T, TrkLog L, int label, int bound, long long newest,
                                                                      int* __restrict__ ent, int stride) {
    const int j = blockIdx.x;
    const int len = bd_window(T, bound);
    if (j >= len) return;
    const int nt = min(T.head->n_tracks, T.capacity);
    const long long stamp = newest - len + 1 + j;
    const int slot = stamp >= 0 ? (int)(stamp % L.frames) : -1;
    const int n = bd_slot_count(L, slot, stamp);
    const long long* uid = L.uid + (size_t)max(slot, 0) * L.max_kp;
    const float* co = L.co + (size_t)max(slot, 0) * L.max_kp * 3;
    for (int i = threadIdx.x; i < nt; i += kTrkBlock) {
        int e = kBdNull;
        if (T.label[i] == label) {
            const long long u = T.uid[i];
            int lo = 0, hi = n;  // the first entry with uid >= u
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (uid[mid] < u) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n && uid[lo] == u) e = trk_finite3(co + 3 * (size_t)lo) ? lo : kBdNotFinite;
        }
        ent[(size_t)j * stride + i] = e;
    }
}

// sum of (a, b) over the workgroup; every lane calls it and gets the totals
__device__ __forceinline__ void bd_block_sum2(int a, int b, int* ta, int* tb) {
    __shared__ int part[2][kTrkBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) a += __shfl_down(a, d, 64), b += __shfl_down(b, d, 64);
    __syncthreads();  // the previous call's totals have been read
    if (lane == 0) part[0][w] = a, part[1][w] = b;
    __syncthreads();
    int sa = 0, sb = 0;
#pragma unroll
    for (int k = 0; k < kTrkBlock / 64; ++k) sa += part[0][k], sb += part[1][k];
    *ta = sa, *tb = sb;
}

// chain (:680-725): ik = 0; for jk = 1 .. len - 1: both = rows with a keypoint at ik and at jk, nvalid = those finite at both;
// fewer than 3 valid: the entry repeats its predecessor and ik stays, else it is a problem and ik = jk.  Only the counts
// decide.  The record goes to pinned memory and to its device copy, every field of entries 0 .. len - 1 written.
__global__ __launch_bounds__(kTrkBlock) void trk_backdate_chain_kernel(TrkTable T, int bound, const int* __restrict__ ent, int stride,
                                                                       TrkBackdate* __restrict__ pinned, TrkBackdate* __restrict__ dev) {
    const int tid = threadIdx.x;
    const int len = bd_window(T, bound);
    const int nt = min(T.head->n_tracks, T.capacity);
    int ik = 0, off = 0, problems = 0;
    for (int jk = 1; jk < len; ++jk) {
        int cb = 0, cv = 0;
        for (int i = tid; i < nt; i += kTrkBlock) {
            const int a = ent[(size_t)ik * stride + i], b = ent[(size_t)jk * stride + i];
            cb += (a != kBdNull && b != kBdNull) ? 1 : 0;
            cv += (a >= 0 && b >= 0) ? 1 : 0;
        }
        int both, nvalid;
        bd_block_sum2(cb, cv, &both, &nvalid);
        const bool few = nvalid < 3;
        if (tid == 0) {
            pinned->from[jk] = ik, pinned->both[jk] = both, pinned->nvalid[jk] = nvalid, pinned->status[jk] = few ? 1 : 0;
            pinned->offset[jk] = off;
            dev->from[jk] = ik, dev->both[jk] = both, dev->nvalid[jk] = nvalid, dev->status[jk] = few ? 1 : 0;
            dev->offset[jk] = off;
        }
        if (!few) ik = jk, off += nvalid, problems += 1;
    }
    if (tid == 0) {
        pinned->from[0] = -1, pinned->both[0] = 0, pinned->nvalid[0] = 0, pinned->status[0] = 0, pinned->offset[0] = 0;
        dev->from[0] = -1, dev->both[0] = 0, dev->nvalid[0] = 0, dev->status[0] = 0, dev->offset[0] = 0;
        pinned->offset[len] = off, dev->offset[len] = off;
        pinned->len = len, pinned->n_problems = problems, pinned->rows = off, pinned->n_tracks = nt;
        dev->len = len, dev->n_problems = problems, dev->rows = off, dev->n_tracks = nt;
    }
}

// gather: workgroup b = entry jk = b + 1.  The rows valid at from[jk] and at jk, in table order (ordered compaction), to
// p0 (the coordinates at from[jk]) / p1 (those at jk) [rows][3] at the problem's offset; rows past `row_cap` are not written
__global__ __launch_bounds__(kTrkBlock) void trk_backdate_gather_kernel(TrkLog L, const TrkBackdate* __restrict__ rec,
                                                                        const int* __restrict__ ent, int stride, long long newest,
                                                                        float* __restrict__ p0, float* __restrict__ p1, int row_cap) {
    const int tid = threadIdx.x, jk = blockIdx.x + 1;
    const int len = min(max(rec->len, 1), kTrkBackdateMax);
    if (jk >= len || rec->status[jk] != 0) return;
    const int ik = min(max(rec->from[jk], 0), len - 1);
    const int nt = min(max(rec->n_tracks, 0), stride);
    const int off = rec->offset[jk];
    const long long s0 = newest - len + 1 + ik, s1 = newest - len + 1 + jk;
    if (s0 < 0 || s1 < 0) return;
    const float* c0 = L.co + (size_t)(s0 % L.frames) * L.max_kp * 3;
    const float* c1 = L.co + (size_t)(s1 % L.frames) * L.max_kp * 3;
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += kTrkBlock) {
        const int i = i0 + tid;
        int a = kBdNull, b = kBdNull;
        if (i < nt) a = ent[(size_t)ik * stride + i], b = ent[(size_t)jk * stride + i];
        const bool take = a >= 0 && b >= 0 && a < L.max_kp && b < L.max_kp;
        int tot;
        const int rank = trk_block_rank(take, &tot);
        const int d = off + base + rank;
        if (take && d >= 0 && d < row_cap) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p0[3 * (size_t)d + k] = c0[3 * (size_t)a + k], p1[3 * (size_t)d + k] = c1[3 * (size_t)b + k];
        }
        base += tot;
    }
}

}  // namespace mmf
