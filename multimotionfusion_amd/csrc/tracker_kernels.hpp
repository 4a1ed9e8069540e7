// tracker_kernels.hpp -- the keypoint track table on the device (gfx950): tracker::PointTracker
// (Core/Utils/PointTracker.cpp:27-226), the per-model track sets (Model::tracks, Model::updateTracks,
// Core/Model/Model.cpp:630-640) and the pair lists of Model::getLastTrackTransform (:739-775).
//
// The table is a structure of arrays over `capacity` tracks in the order of the reference's `tracks` vector.  It keeps
// what the reference's consumers read and not the history: the descriptor of the last non-null keypoint, the last two
// slots (end()[-1] = slot 0 `cur`, end()[-2] = slot 1 `prev`), the age (frames since the last non-null keypoint), the
// number of non-null keypoints and the stamp of the last one (prune), a 256-bit set of model ids per track (every
// Model::tracks at once) and a uid that is never reused.  A null slot holds zeros.
//
// Every operation is a fixed number of launches on the context's stream, whatever the number of keypoints and tracks,
// and none reads anything back: counts the next kernel needs stay in the table's head record on the device.  The
// bookkeeping kernels are ONE workgroup of 1024 lanes (a table is a few thousand tracks: this is latency, not
// bandwidth): ordered compactions from 64-bit ballots and a scan over the 16 wave totals.  Descriptor rows (1 KB) move
// in grid kernels, one wave of 64 lanes x 16 B per row.  The counters the host reads go to a pinned record with
// ordinary stores at the end of the kernel that changes them.
//
// The view log (off unless switched on) is the bounded history Model::store's views are built from: a ring of the visible
// sets of the last adds, and a model's views from it (the second half of this file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hpp"

namespace mmf {

constexpr int kTrkDim = 256;     // SuperPoint descriptors
constexpr int kTrkWords = 8;     // 256 model ids
constexpr int kTrkBlock = 1024;  // lanes of the bookkeeping workgroup
constexpr int kTrkMaxModels = 256;
constexpr float kTrkFiller = 1e30f;  // a padding row of the gathered train set: its distance to anything is +inf

struct TrkHead {  // on the device
    int n_tracks, length, dropped, n_active;
    long long next_uid;
    int kp_failed, pad_;  // adds whose keypoint source had failed (mmf_tracker_add_keypoints_device)
};

struct TrkRecord {  // pinned host memory the kernels write
    int n_tracks, length, dropped, dropped_last, n_visible, kp_failed;
    int pair_count[kTrkMaxModels];
};

struct TrkTable {
    int capacity;
    TrkHead* head;
    int *age, *nvalid, *label;
    long long *last_stamp, *uid;
    int* xy[2];         // [capacity][2]
    float* co[2];       // [capacity][3]
    long long* ts[2];   // [capacity]
    int* ok[2];         // [capacity] non-null flag
    unsigned* member;   // [capacity][8]
};

struct TrkModelSet {
    unsigned w[kTrkWords];
};
struct TrkModelList {
    int n;
    unsigned char id[kTrkMaxModels];
};

// exclusive rank of this lane among the lanes of the workgroup with `flag`, in lane order; *total = their number.
// Every lane of the (kTrkBlock wide) workgroup calls it.
__device__ __forceinline__ int trk_block_rank(bool flag, int* total) {
    __shared__ int wave_sum[kTrkBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();  // the previous call's totals have been read
    if (lane == 0) wave_sum[w] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kTrkBlock / 64; ++k) {
        const int s = wave_sum[k];
        base += k < w ? s : 0;
        tot += s;
    }
    *total = tot;
    return base + in_wave;
}

__device__ __forceinline__ float trk_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool trk_finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// add, step 1: the keypoints of the frame (PointTracker.cpp:35-56, float operation for float operation: the build has
// -ffp-contract=off), the ordered compaction of the active tracks (getLastActiveKeypoints, :205-224) and the shift of
// every track by one null keypoint (:71-73).  An empty table is not shifted: its length restarts at 1 (:61-66).
__device__ __forceinline__ void trk_begin_body(TrkTable T, int n, const int* __restrict__ q_xy, const float* __restrict__ depth,
                                               int width, int height, float fx, float fy, float cx, float cy, int history,
                                               float* __restrict__ q_co, int* __restrict__ active_idx) {
    const int tid = threadIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity);
    for (int q = tid; q < n; q += kTrkBlock) {
        const int x = q_xy[2 * q], y = q_xy[2 * q + 1];
        float X = trk_nan(), Y = trk_nan(), Z = trk_nan();
        if (x >= 0 && x < width && y >= 0 && y < height) {
            const float z = depth[(size_t)y * width + x];
            if (z > 0.f) {
                X = (z * ((float)x - cx)) / fx;
                Y = (z * ((float)y - cy)) / fy;
                Z = z;
            }
        }
        q_co[3 * q] = X, q_co[3 * q + 1] = Y, q_co[3 * q + 2] = Z;
    }
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += kTrkBlock) {
        const int i = i0 + tid;
        const bool in = i < nt;
        const bool active = in && (history == 0 || T.age[i] < history);
        int tot;
        const int rank = trk_block_rank(active, &tot);
        if (active) active_idx[base + rank] = i;
        base += tot;
        if (in) {
            T.xy[1][2 * i] = T.xy[0][2 * i], T.xy[1][2 * i + 1] = T.xy[0][2 * i + 1];
            T.xy[0][2 * i] = 0, T.xy[0][2 * i + 1] = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) T.co[1][3 * i + k] = T.co[0][3 * i + k], T.co[0][3 * i + k] = 0.f;
            T.ts[1][i] = T.ts[0][i], T.ts[0][i] = 0;
            T.ok[1][i] = T.ok[0][i], T.ok[0][i] = 0;
            T.age[i] += 1;
        }
    }
    if (tid == 0) {
        T.head->n_active = base;
        T.head->length = nt ? T.head->length + 1 : 1;
    }
}

__global__ __launch_bounds__(kTrkBlock) void trk_begin_kernel(TrkTable T, int n, const int* __restrict__ q_xy,
                                                              const float* __restrict__ depth, int width, int height, float fx,
                                                              float fy, float cx, float cy, int history,
                                                              float* __restrict__ q_co, int* __restrict__ active_idx) {
    trk_begin_body(T, n, q_xy, depth, width, height, fx, fy, cx, cy, history, q_co, active_idx);
}

// the same with the number of keypoints on the device (device_count, match_kernels.hpp): rows from it on are not read
__global__ __launch_bounds__(kTrkBlock) void trk_begin_counted_kernel(TrkTable T, const int* __restrict__ n_dev,
                                                                      const int* __restrict__ fail_dev, int n_max,
                                                                      const int* __restrict__ q_xy, const float* __restrict__ depth,
                                                                      int width, int height, float fx, float fy, float cx, float cy,
                                                                      int history, float* __restrict__ q_co,
                                                                      int* __restrict__ active_idx) {
    trk_begin_body(T, device_count(n_dev, fail_dev, n_max), q_xy, depth, width, height, fx, fy, cx, cy, history, q_co, active_idx);
}

// add, step 2: the descriptors of the active tracks, in order, as the train set of the search; the rows from n_active
// to nt_pad (what the host knows to be no less than the number of tracks) are padding that nothing matches
__global__ __launch_bounds__(256) void trk_gather_kernel(TrkTable T, const float* __restrict__ desc,
                                                         const int* __restrict__ active_idx, float* __restrict__ train, int nt_pad) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const int na = min(T.head->n_active, T.capacity);
    for (int r = wave; r < nt_pad; r += waves) {
        float4 v = make_float4(kTrkFiller, kTrkFiller, kTrkFiller, kTrkFiller);
        if (r < na) {
            const int i = min(max(active_idx[r], 0), T.capacity - 1);
            v = reinterpret_cast<const float4*>(desc + (size_t)i * kTrkDim)[lane];
        }
        reinterpret_cast<float4*>(train + (size_t)r * kTrkDim)[lane] = v;
    }
}

// add, step 3 (after the search): matched tracks get their keypoint (:107-112), unmatched keypoints start tracks in
// ascending query index (:116-121); appends past the capacity are dropped and counted.  dest_row[q] = the row the
// descriptor of keypoint q goes to, or -1.
__device__ __forceinline__ void trk_finish_body(TrkTable T, TrkRecord* __restrict__ rec, int n, const int* __restrict__ q_xy,
                                                const float* __restrict__ q_co, const int* __restrict__ train_idx,
                                                const int* __restrict__ active_idx, long long timestamp,
                                                int* __restrict__ dest_row) {
    const int tid = threadIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity), na = min(T.head->n_active, T.capacity);
    const long long uid0 = T.head->next_uid;
    int base = 0;
    for (int q0 = 0; q0 < n; q0 += kTrkBlock) {
        const int q = q0 + tid;
        const bool in = q < n;
        int t = in ? train_idx[q] : 0;
        if (t >= na) t = -1;  // (a padding row never matches)
        const bool fresh = in && t < 0;
        int tot;
        const int rank = trk_block_rank(fresh, &tot);
        int dst = -1;
        if (in && !fresh) {
            dst = active_idx[t];
            if (dst < 0 || dst >= nt) dst = -1;
        } else if (fresh && nt + base + rank < T.capacity) {
            dst = nt + base + rank;
        }
        if (in) dest_row[q] = dst;
        if (dst >= 0) {
            const size_t i = (size_t)dst;
            T.xy[0][2 * i] = q_xy[2 * q], T.xy[0][2 * i + 1] = q_xy[2 * q + 1];
#pragma unroll
            for (int k = 0; k < 3; ++k) T.co[0][3 * i + k] = q_co[3 * q + k];
            T.ts[0][i] = timestamp, T.ok[0][i] = 1;
            T.age[i] = 0, T.last_stamp[i] = timestamp;
            if (fresh) {
                T.nvalid[i] = 1, T.uid[i] = uid0 + base + rank, T.label[i] = -1;
                T.xy[1][2 * i] = 0, T.xy[1][2 * i + 1] = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) T.co[1][3 * i + k] = 0.f;
                T.ts[1][i] = 0, T.ok[1][i] = 0;
#pragma unroll
                for (int w = 0; w < kTrkWords; ++w) T.member[kTrkWords * i + w] = 0u;
            } else {
                T.nvalid[i] += 1;
            }
        }
        base += tot;
    }
    if (tid == 0) {
        const int appended = min(base, T.capacity - nt), lost = base - appended;
        T.head->n_tracks = nt + appended;
        T.head->next_uid = uid0 + appended;
        T.head->dropped += lost;
        if (nt + appended == 0) T.head->length = 0;
        rec->n_tracks = nt + appended, rec->length = T.head->length, rec->dropped = T.head->dropped, rec->dropped_last = lost;
    }
}

__global__ __launch_bounds__(kTrkBlock) void trk_finish_kernel(TrkTable T, TrkRecord* __restrict__ rec, int n,
                                                               const int* __restrict__ q_xy, const float* __restrict__ q_co,
                                                               const int* __restrict__ train_idx,
                                                               const int* __restrict__ active_idx, long long timestamp,
                                                               int* __restrict__ dest_row) {
    trk_finish_body(T, rec, n, q_xy, q_co, train_idx, active_idx, timestamp, dest_row);
}

// the same with the number of keypoints on the device; a source that had failed (*fail_dev set: the frame is one without
// keypoints) is counted in the head and the record
__global__ __launch_bounds__(kTrkBlock) void trk_finish_counted_kernel(TrkTable T, TrkRecord* __restrict__ rec,
                                                                       const int* __restrict__ n_dev,
                                                                       const int* __restrict__ fail_dev, int n_max,
                                                                       const int* __restrict__ q_xy, const float* __restrict__ q_co,
                                                                       const int* __restrict__ train_idx,
                                                                       const int* __restrict__ active_idx, long long timestamp,
                                                                       int* __restrict__ dest_row) {
    trk_finish_body(T, rec, device_count(n_dev, fail_dev, n_max), q_xy, q_co, train_idx, active_idx, timestamp, dest_row);
    if (threadIdx.x == 0) {
        if (fail_dev && *fail_dev) T.head->kp_failed += 1;
        rec->kp_failed = T.head->kp_failed;
    }
}

// descriptor rows of a set of keypoints to their rows of the table (dest_row < 0: nowhere)
__device__ __forceinline__ void trk_scatter_rows_body(const float* __restrict__ q_desc, int n, const int* __restrict__ dest_row,
                                                      float* __restrict__ desc, int capacity) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    for (int q = wave; q < n; q += waves) {
        const int d = dest_row[q];
        if (d < 0 || d >= capacity) continue;
        reinterpret_cast<float4*>(desc + (size_t)d * kTrkDim)[lane] = reinterpret_cast<const float4*>(q_desc + (size_t)q * kTrkDim)[lane];
    }
}

__global__ __launch_bounds__(256) void trk_scatter_rows_kernel(const float* __restrict__ q_desc, int n,
                                                               const int* __restrict__ dest_row, float* __restrict__ desc,
                                                               int capacity) {
    trk_scatter_rows_body(q_desc, n, dest_row, desc, capacity);
}

__global__ __launch_bounds__(256) void trk_scatter_rows_counted_kernel(const float* __restrict__ q_desc, const int* __restrict__ n_dev,
                                                                       const int* __restrict__ fail_dev, int n_max,
                                                                       const int* __restrict__ dest_row, float* __restrict__ desc,
                                                                       int capacity) {
    trk_scatter_rows_body(q_desc, device_count(n_dev, fail_dev, n_max), dest_row, desc, capacity);
}

// prune (:170-203): tracks with fewer than min_kps keypoints whose last keypoint is older than min_time go; the others
// close up in order.  A chunk of 1024 tracks is read into registers before any of it is written, and what it writes lies
// below the next chunk.  map[dst] = src for the descriptor rows, which move into the table's second buffer.
__global__ __launch_bounds__(kTrkBlock) void trk_prune_kernel(TrkTable T, TrkRecord* __restrict__ rec, int min_kps,
                                                              long long min_time, int* __restrict__ map) {
    const int tid = threadIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity);
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += kTrkBlock) {
        const int i = i0 + tid;
        const bool in = i < nt;
        int age = 0, nvalid = 0, label = 0, xy[2][2] = {}, ok[2] = {};
        long long last = 0, uid = 0, ts[2] = {};
        float co[2][3] = {};
        unsigned mem[kTrkWords] = {};
        if (in) {
            age = T.age[i], nvalid = T.nvalid[i], label = T.label[i], last = T.last_stamp[i], uid = T.uid[i];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                xy[s][0] = T.xy[s][2 * i], xy[s][1] = T.xy[s][2 * i + 1];
#pragma unroll
                for (int k = 0; k < 3; ++k) co[s][k] = T.co[s][3 * i + k];
                ts[s] = T.ts[s][i], ok[s] = T.ok[s][i];
            }
#pragma unroll
            for (int w = 0; w < kTrkWords; ++w) mem[w] = T.member[kTrkWords * (size_t)i + w];
        }
        const bool keep = in && !(nvalid < min_kps && last < min_time);
        int tot;
        const int rank = trk_block_rank(keep, &tot);  // (its barriers order the reads above before the writes below)
        if (keep) {
            const size_t d = (size_t)(base + rank);
            map[d] = i;
            T.age[d] = age, T.nvalid[d] = nvalid, T.label[d] = label, T.last_stamp[d] = last, T.uid[d] = uid;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                T.xy[s][2 * d] = xy[s][0], T.xy[s][2 * d + 1] = xy[s][1];
#pragma unroll
                for (int k = 0; k < 3; ++k) T.co[s][3 * d + k] = co[s][k];
                T.ts[s][d] = ts[s], T.ok[s][d] = ok[s];
            }
#pragma unroll
            for (int w = 0; w < kTrkWords; ++w) T.member[kTrkWords * d + w] = mem[w];
        }
        base += tot;
    }
    if (tid == 0) {
        T.head->n_tracks = base;
        if (base == 0) T.head->length = 0;
        rec->n_tracks = base, rec->length = T.head->length;
    }
}

// rows map[0 .. n) of `from` to rows 0 .. n of `to`; n = *count (on the device), a different buffer: no row is
// overwritten before another wave has read it
__global__ __launch_bounds__(256) void trk_gather_rows_kernel(const float* __restrict__ from, const int* __restrict__ map,
                                                              const int* __restrict__ count, float* __restrict__ to, int capacity) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const int n = min(*count, capacity);
    for (int r = wave; r < n; r += waves) {
        const int s = min(max(map[r], 0), capacity - 1);
        reinterpret_cast<float4*>(to + (size_t)r * kTrkDim)[lane] = reinterpret_cast<const float4*>(from + (size_t)s * kTrkDim)[lane];
    }
}

// associate (MultiMotionFusion.cpp:425-436, 584-604): label = the id image at the last keypoint of every visible track
// inside the image; for every listed model whose label some track carries, a labelled track belongs to it exactly when
// it carries its label (updateTracks(segm_tracks[id], all other segments' tracks)).  Unlabelled tracks keep their sets.
__global__ __launch_bounds__(kTrkBlock) void trk_associate_kernel(TrkTable T, const unsigned char* __restrict__ mask, int width,
                                                                  int height, TrkModelSet listed) {
    __shared__ unsigned present[kTrkWords];
    const int tid = threadIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity);
    if (tid < kTrkWords) present[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < nt; i += kTrkBlock) {
        int l = -1;
        if (T.ok[0][i]) {
            const int x = T.xy[0][2 * i], y = T.xy[0][2 * i + 1];
            if (x >= 0 && x < width && y >= 0 && y < height) l = mask[(size_t)y * width + x];
        }
        T.label[i] = l;
        if (l >= 0) atomicOr(&present[l >> 5], 1u << (l & 31));
    }
    __syncthreads();
    for (int i = tid; i < nt; i += kTrkBlock) {
        const int l = T.label[i];
        if (l < 0) continue;
#pragma unroll
        for (int w = 0; w < kTrkWords; ++w) {
            const unsigned upd = listed.w[w] & present[w];
            unsigned m = T.member[kTrkWords * (size_t)i + w] & ~upd;
            if ((l >> 5) == w) m |= upd & (1u << (l & 31));
            T.member[kTrkWords * (size_t)i + w] = m;
        }
    }
}

// every track joins (clear = 0: updateTracks(tracks, {}), initGlobalTracks) or leaves (clear = 1) the models of `set`
__global__ __launch_bounds__(256) void trk_member_kernel(TrkTable T, TrkModelSet set, int clear) {
    const int nt = min(T.head->n_tracks, T.capacity);
    for (int e = blockIdx.x * 256 + threadIdx.x; e < nt * kTrkWords; e += gridDim.x * 256) {
        const unsigned s = set.w[e & (kTrkWords - 1)];
        T.member[e] = clear ? (T.member[e] & ~s) : (T.member[e] | s);
    }
}

// pairs (Model::getLastTrackTransform, :747-761): workgroup j = model list.id[j]; the ordered compaction of its tracks
// whose last two keypoints exist and are finite -> p0 (prev) / p1 (cur) [j][stride][3] and the count, in pinned memory
__global__ __launch_bounds__(kTrkBlock) void trk_pairs_kernel(TrkTable T, TrkRecord* __restrict__ rec, TrkModelList list,
                                                              float* __restrict__ p0, float* __restrict__ p1, int stride) {
    const int tid = threadIdx.x, j = blockIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity);
    const int m = list.id[j];
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += kTrkBlock) {
        const int i = i0 + tid;
        bool take = false;
        float a[3] = {}, b[3] = {};
        if (i < nt && ((T.member[kTrkWords * (size_t)i + (m >> 5)] >> (m & 31)) & 1u) && T.ok[0][i] && T.ok[1][i]) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = T.co[1][3 * i + k], b[k] = T.co[0][3 * i + k];
            take = trk_finite3(a) && trk_finite3(b);
        }
        int tot;
        const int rank = trk_block_rank(take, &tot);
        if (take && base + rank < stride) {
            const size_t d = ((size_t)j * stride + base + rank) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) p0[d + k] = a[k], p1[d + k] = b[k];
        }
        base += tot;
    }
    if (tid == 0) {
        rec->pair_count[j] = min(base, stride);
        if (j == 0) rec->n_tracks = nt, rec->length = T.head->length, rec->dropped = T.head->dropped;
    }
}

// visible (track->back() of every track that has one, MultiMotionFusion.cpp:428-431): ordered compaction -> rows
__global__ __launch_bounds__(kTrkBlock) void trk_visible_kernel(TrkTable T, TrkRecord* __restrict__ rec, int* __restrict__ map,
                                                                int* __restrict__ count, int* __restrict__ xy,
                                                                float* __restrict__ co, long long* __restrict__ uid) {
    const int tid = threadIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity);
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += kTrkBlock) {
        const int i = i0 + tid;
        const bool vis = i < nt && T.ok[0][i];
        int tot;
        const int rank = trk_block_rank(vis, &tot);
        if (vis) {
            const size_t d = (size_t)(base + rank);
            map[d] = i;
            xy[2 * d] = T.xy[0][2 * i], xy[2 * d + 1] = T.xy[0][2 * i + 1];
#pragma unroll
            for (int k = 0; k < 3; ++k) co[3 * d + k] = T.co[0][3 * i + k];
            uid[d] = T.uid[i];
        }
        base += tot;
    }
    if (tid == 0) {
        *count = base;
        rec->n_visible = base, rec->n_tracks = nt, rec->length = T.head->length, rec->dropped = T.head->dropped;
    }
}

// ---- the view log: a ring of the visible sets of the last `frames` adds (Model::store's views come from it) -------------
struct TrkLog {  // slot s = stamp % frames; all null while the log is off
    int frames, max_kp;
    int* count;        // [frames]
    long long* stamp;  // [frames] the add that wrote the slot, -1: none
    long long* uid;    // [frames][max_kp]
    float* co;         // [frames][max_kp][3] camera frame
    float* desc;       // [frames][max_kp][256] the descriptor of THAT frame's keypoint
};

// add, step 5 (log on): the visible set after the add, in table order, into slot `slot`; map[d] = the table row whose
// descriptor is row d of the slot (trk_gather_rows_kernel moves it), *slot_count rows.  A visible set never exceeds the
// keypoints of the add; rows past max_kp are dropped all the same.
__global__ __launch_bounds__(kTrkBlock) void trk_log_kernel(TrkTable T, TrkLog L, int slot, long long stamp, int* __restrict__ map) {
    const int tid = threadIdx.x;
    const int nt = min(T.head->n_tracks, T.capacity);
    long long* uid = L.uid + (size_t)slot * L.max_kp;
    float* co = L.co + (size_t)slot * L.max_kp * 3;
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += kTrkBlock) {
        const int i = i0 + tid;
        const bool vis = i < nt && T.ok[0][i];
        int tot;
        const int rank = trk_block_rank(vis, &tot);
        if (vis && base + rank < L.max_kp) {
            const size_t d = (size_t)(base + rank);
            map[d] = i;
            uid[d] = T.uid[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) co[3 * d + k] = T.co[0][3 * i + k];
        }
        base += tot;
    }
    if (tid == 0) L.count[slot] = min(base, L.max_kp), L.stamp[slot] = stamp;
}

struct TrkViewRequest {  // one view of mmf_tracker_model_views, uploaded by the host
    int slot;            // the ring slot of its frame, -1: the frame is not in the ring
    int pad_;
    long long stamp;     // the frame; the slot must carry it
    float pose[16];      // row-major 4 x 4, camera frame -> model frame at that frame
};

// project_kp (Model.cpp:130-141): float -> double, ((r0 x + r1 y) + r2 z) + t with every product and sum rounded on its own,
// -> float
__device__ __forceinline__ float trk_project_row(const float* __restrict__ p, int r, double x, double y, double z) {
    const double a = __dmul_rn((double)p[4 * r], x), b = __dmul_rn((double)p[4 * r + 1], y), c = __dmul_rn((double)p[4 * r + 2], z);
    return (float)__dadd_rn(__dadd_rn(__dadd_rn(a, b), c), (double)p[4 * r + 3]);
}

// a model's views, step 1: workgroup v = view v walks its slot in chunks.  A logged keypoint is taken when its uid is in
// the table now (binary search: the table is sorted by uid -- appends take ascending uids, prune is a stable compaction),
// that track has bit `model` now, and its coordinate in the model's frame is finite.  Ordered compaction -> row[v][k] =
// the ring row of the k-th keypoint of the view, co[v][k] its coordinate; the count goes to pinned memory and to dev_count.
__global__ __launch_bounds__(kTrkBlock) void trk_views_kernel(TrkTable T, TrkLog L, const TrkViewRequest* __restrict__ req, int n_views,
                                                              int model, int* __restrict__ row, float* __restrict__ co,
                                                              int* __restrict__ pinned_count, int* __restrict__ dev_count) {
    const int tid = threadIdx.x, v = blockIdx.x;
    if (v >= n_views) return;
    const int nt = min(T.head->n_tracks, T.capacity);
    const int slot = req[v].slot;
    int n = 0;
    if (slot >= 0 && slot < L.frames && L.stamp[slot] == req[v].stamp) n = min(max(L.count[slot], 0), L.max_kp);
    const float* pose = req[v].pose;
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += kTrkBlock) {
        const int k = k0 + tid;
        bool take = false;
        float out[3] = {};
        if (k < n) {
            const size_t e = (size_t)slot * L.max_kp + k;
            const long long u = L.uid[e];
            int lo = 0, hi = nt;  // the first row with uid >= u
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (T.uid[mid] < u) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nt && T.uid[lo] == u && ((T.member[kTrkWords * (size_t)lo + (model >> 5)] >> (model & 31)) & 1u)) {
                const double x = (double)L.co[3 * e], y = (double)L.co[3 * e + 1], z = (double)L.co[3 * e + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r) out[r] = trk_project_row(pose, r, x, y, z);
                take = trk_finite3(out);
            }
        }
        int tot;
        const int rank = trk_block_rank(take, &tot);
        if (take) {
            const size_t d = (size_t)v * L.max_kp + base + rank;
            row[d] = slot * L.max_kp + k;
#pragma unroll
            for (int r = 0; r < 3; ++r) co[3 * d + r] = out[r];
        }
        base += tot;
    }
    if (tid == 0) pinned_count[v] = base, dev_count[v] = base;
}

// a model's views, step 2: the rows of view blockIdx.y, one after the other behind the rows of the views before it
// (descriptors: one wave of 64 lanes x 16 B per row)
__global__ __launch_bounds__(256) void trk_views_pack_kernel(TrkLog L, const int* __restrict__ dev_count, int n_views,
                                                             const int* __restrict__ row, const float* __restrict__ co,
                                                             float* __restrict__ out_desc, float* __restrict__ out_co) {
    __shared__ int part[256];
    const int v = blockIdx.y;
    if (v >= n_views) return;
    int s = 0;
    for (int k = threadIdx.x; k < v; k += 256) s += dev_count[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    const size_t off = (size_t)part[0];
    const int n = min(dev_count[v], L.max_kp);
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const size_t ring_rows = (size_t)L.frames * L.max_kp;
    for (int k = wave; k < n; k += waves) {
        const size_t d = (size_t)v * L.max_kp + k;
        const size_t src = min((size_t)max(row[d], 0), ring_rows - 1);
        reinterpret_cast<float4*>(out_desc + (off + k) * kTrkDim)[lane] = reinterpret_cast<const float4*>(L.desc + src * kTrkDim)[lane];
        if (lane < 3) out_co[(off + k) * 3 + lane] = co[3 * d + lane];
    }
}

}  // namespace mmf
