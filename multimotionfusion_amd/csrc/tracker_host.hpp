// tracker_host.hpp -- the C ABI of the device-resident keypoint track table (tracker_kernels.hpp).  Textually included by
// mmf_hip.hip (it uses that file's helpers, match_kernels.hpp and rigid_ransac.hpp).
//
// Everything is enqueued on the context's stream.  The host keeps only an UPPER BOUND of the number of tracks (it grows
// by the keypoints of every add -- by max_keypoints where their number is known to the device alone -- and becomes exact
// whenever a call waits: pairs, visible, status, download): the search
// of an add runs on that many gathered rows, the ones past the active tracks being padding no keypoint can match.
// The stamp of the newest frame (adds since creation / reset) is exact on the host: the view log's slots go by it.
#pragma once

#include "tracker_kernels.hpp"
#include "backdate_kernels.hpp"

struct mmf_tracker {
    mmf_ctx* ctx = nullptr;
    int width = 0, height = 0, capacity = 0, cap_pad = 0, max_keypoints = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    mmf::TrkTable T{};
    float* desc[2] = {nullptr, nullptr};  // [cap_pad][256] each; desc[cur] is live, prune moves the rows to the other
    int cur = 0;
    float* train = nullptr;  // [cap_pad][256] the gathered rows of the active tracks
    int *active_idx = nullptr, *map = nullptr, *count = nullptr;
    int *q_xy = nullptr, *dest_row = nullptr, *train_idx = nullptr;
    float *q_co = nullptr, *q_dist = nullptr, *norms = nullptr;
    unsigned long long* keys = nullptr;
    int* vis_xy = nullptr;
    float *vis_co = nullptr, *vis_desc = nullptr;
    long long* vis_uid = nullptr;
    mmf::TrkRecord* rec = nullptr;  // pinned
    float *p0 = nullptr, *p1 = nullptr;  // pinned [pair_models][capacity][3]
    int pair_models = 0;
    int bound = 0;  // no fewer than the tracks of the table
    const int* kp_status = nullptr;  // DEVICE word the device-count add reads (mmf_tracker_set_keypoint_status); null: none
    long long caller_adds = 0;       // adds through the public calls (the fusion's in-frame front end tells its own from them)
    int last_launches = 0;
    std::vector<void*> device_allocs;
    // the view log (mmf_tracker_set_view_log) and the views built from it (mmf_tracker_model_views)
    mmf::TrkLog log{};        // all null while the log is off
    long long frame = 0;      // adds since creation / reset = the stamp of the newest frame
    long long log_first = 0;  // the first stamp the ring can hold: the log was switched on, or the tracker reset, before it
    int view_cap = 0;         // views the request / row / count buffers hold
    mmf::TrkViewRequest *req_pin = nullptr, *req_dev = nullptr;
    int *view_count_pin = nullptr, *view_count_dev = nullptr, *view_row = nullptr;
    float *view_co = nullptr, *view_out_desc = nullptr, *view_out_co = nullptr;
    size_t view_out_rows = 0;
    // back-dating (mmf_tracker_backdate, backdate_host.hpp): the workspace of `bd_history` window frames, all null until reserved
    std::vector<long long> add_ts;  // the timestamp of the add that wrote slot stamp % log.frames (host side; the log's size)
    int bd_history = 0;
    int* bd_ent = nullptr;                                  // [bd_history][cap_pad]
    mmf::TrkBackdate *bd_pin = nullptr, *bd_dev = nullptr;  // the chain kernel's record
    float *bd_p0 = nullptr, *bd_p1 = nullptr;               // [bd_row_cap][3] the problems' rows
    int bd_row_cap = 0;
    mmf::TrkBackdate bd_last{};  // the record of the last call (mmf_tracker_backdate_rows)
    bool bd_valid = false;
};

template <typename P>
static int tracker_dev_alloc(mmf_tracker* t, P** p, size_t count) {
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(P)));
    t->device_allocs.push_back(*p);
    MMF_HIP_TRY(hipMemsetAsync(*p, 0, std::max<size_t>(count, 1) * sizeof(P), t->ctx->stream));
    return MMF_OK;
}

static inline unsigned tracker_row_blocks(int rows) { return (unsigned)std::min(256, std::max(1, (rows + 3) / 4)); }

static int tracker_clear(mmf_tracker* t) {
    hipStream_t st = t->ctx->stream;
    MMF_HIP_TRY(hipMemsetAsync(t->T.head, 0, sizeof(mmf::TrkHead), st));
    MMF_HIP_TRY(hipStreamSynchronize(st));
    std::memset(t->rec, 0, sizeof(mmf::TrkRecord));
    t->bound = 0, t->cur = 0, t->last_launches = 0;
    t->frame = 0, t->log_first = 1;  // (the stream has been awaited: no slot of the ring is of interest any more)
    std::fill(t->add_ts.begin(), t->add_ts.end(), 0ll);
    t->bd_valid = false;
    return MMF_OK;
}

static void tracker_free_log(mmf_tracker* t) {
    (void)hipFree(t->log.count);
    (void)hipFree(t->log.stamp);
    (void)hipFree(t->log.uid);
    (void)hipFree(t->log.co);
    (void)hipFree(t->log.desc);
    t->log = mmf::TrkLog{};
}

static void tracker_free_backdate(mmf_tracker* t) {
    if (t->bd_pin) (void)hipHostFree(t->bd_pin);
    (void)hipFree(t->bd_dev);
    (void)hipFree(t->bd_ent);
    (void)hipFree(t->bd_p0);
    (void)hipFree(t->bd_p1);
    t->bd_pin = t->bd_dev = nullptr, t->bd_ent = nullptr, t->bd_p0 = t->bd_p1 = nullptr;
    t->bd_history = 0, t->bd_row_cap = 0, t->bd_valid = false;
}

static void tracker_free_views(mmf_tracker* t) {
    if (t->req_pin) (void)hipHostFree(t->req_pin);
    if (t->view_count_pin) (void)hipHostFree(t->view_count_pin);
    (void)hipFree(t->req_dev);
    (void)hipFree(t->view_count_dev);
    (void)hipFree(t->view_row);
    (void)hipFree(t->view_co);
    t->req_pin = t->req_dev = nullptr, t->view_count_pin = t->view_count_dev = t->view_row = nullptr, t->view_co = nullptr;
    t->view_cap = 0;
}

extern "C" void mmf_tracker_destroy(mmf_tracker* t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
    for (void* p : t->device_allocs) (void)hipFree(p);
    tracker_free_log(t);
    tracker_free_views(t);
    tracker_free_backdate(t);
    (void)hipFree(t->view_out_desc);
    (void)hipFree(t->view_out_co);
    if (t->rec) (void)hipHostFree(t->rec);
    if (t->p0) (void)hipHostFree(t->p0);
    if (t->p1) (void)hipHostFree(t->p1);
    delete t;
}

static int tracker_create_impl(mmf_tracker* t) {
    const size_t C = (size_t)t->cap_pad, K = (size_t)t->max_keypoints;
    int rc = 0;
    auto A = [&](auto** p, size_t n) { if (!rc) rc = tracker_dev_alloc(t, p, n); };
    A(&t->T.head, 1);
    A(&t->T.age, C), A(&t->T.nvalid, C), A(&t->T.label, C), A(&t->T.last_stamp, C), A(&t->T.uid, C);
    for (int s = 0; s < 2; ++s) A(&t->T.xy[s], 2 * C), A(&t->T.co[s], 3 * C), A(&t->T.ts[s], C), A(&t->T.ok[s], C);
    A(&t->T.member, mmf::kTrkWords * C);
    A(&t->desc[0], C * mmf::kTrkDim), A(&t->desc[1], C * mmf::kTrkDim), A(&t->train, C * mmf::kTrkDim);
    A(&t->active_idx, C), A(&t->map, C), A(&t->count, 1);
    A(&t->q_xy, 2 * K), A(&t->dest_row, K), A(&t->train_idx, K), A(&t->q_co, 3 * K), A(&t->q_dist, K);
    A(&t->norms, K + C), A(&t->keys, K + C);
    A(&t->vis_xy, 2 * C), A(&t->vis_co, 3 * C), A(&t->vis_desc, C * mmf::kTrkDim), A(&t->vis_uid, C);
    if (rc) return rc;
    MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->rec), sizeof(mmf::TrkRecord), hipHostMallocMapped | hipHostMallocCoherent));
    t->T.capacity = t->capacity;
    return tracker_clear(t);
}

extern "C" int mmf_tracker_create(mmf_ctx* c, int width, int height, float fx, float fy, float cx, float cy, int capacity,
                                  int max_keypoints, mmf_tracker** out) {
    MMF_REQUIRE(c && out, "mmf_tracker_create: null argument");
    MMF_REQUIRE(width > 0 && height > 0 && capacity > 0 && max_keypoints > 0 && capacity <= (1 << 22) && max_keypoints <= (1 << 20),
                "mmf_tracker_create: sizes must be positive (capacity <= 2^22, max_keypoints <= 2^20)");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_tracker* t = new (std::nothrow) mmf_tracker();
    MMF_REQUIRE(t != nullptr, "mmf_tracker_create: out of host memory");
    t->ctx = c, t->width = width, t->height = height, t->capacity = capacity, t->max_keypoints = max_keypoints;
    t->cap_pad = (capacity + 63) / 64 * 64;
    t->fx = fx, t->fy = fy, t->cx = cx, t->cy = cy;
    const int rc = tracker_create_impl(t);
    if (rc) {
        const std::string msg = g_last_error;
        mmf_tracker_destroy(t);
        return fail(rc, msg);
    }
    *out = t;
    return MMF_OK;
}

extern "C" int mmf_tracker_reset(mmf_tracker* t) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_reset: null tracker");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    return tracker_clear(t);
}

extern "C" int mmf_tracker_last_launches(mmf_tracker* t) { return t ? t->last_launches : -1; }

// the host has waited for the stream: the record is what the table holds
static void tracker_refresh(mmf_tracker* t) { t->bound = std::min(t->capacity, std::max(0, t->rec->n_tracks)); }

// the end of an add: the stamp, and with the view log on the frame's visible set into its slot of the ring (two more
// launches, nothing read back); the add's timestamp stays on the host, beside the slot's stamp
static void tracker_add_tail(mmf_tracker* t, long long timestamp) {
    using namespace mmf;
    hipStream_t st = t->ctx->stream;
    t->last_launches = 7;
    t->frame += 1;
    if (t->log.frames > 0) {
        const int slot = (int)(t->frame % t->log.frames);
        t->add_ts[(size_t)slot] = timestamp;
        hipLaunchKernelGGL(trk_log_kernel, dim3(1), dim3(kTrkBlock), 0, st, t->T, t->log, slot, t->frame, t->map);
        hipLaunchKernelGGL(trk_gather_rows_kernel, dim3(tracker_row_blocks(t->max_keypoints)), dim3(256), 0, st,
                           (const float*)t->desc[t->cur], (const int*)t->map, (const int*)(t->log.count + slot),
                           t->log.desc + (size_t)slot * t->max_keypoints * kTrkDim, t->capacity);
        t->last_launches = 9;
    }
}

extern "C" int mmf_tracker_add_keypoints(mmf_tracker* t, int n, const int* xy, const float* descriptor, const float* depth,
                                         long long timestamp, float min_feature_distance, int history) {
    MMF_REQUIRE(t && n >= 0 && depth && ((xy && descriptor) || n == 0), "mmf_tracker_add_keypoints: null argument");
    MMF_REQUIRE(n <= t->max_keypoints, "mmf_tracker_add_keypoints: more keypoints than max_keypoints");
    MMF_REQUIRE(history >= 0, "mmf_tracker_add_keypoints: negative history");
    MMF_REQUIRE(((uintptr_t)descriptor & 15u) == 0, "mmf_tracker_add_keypoints: 16-byte aligned descriptor rows");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    using namespace mmf;
    const int nt_pad = std::min(t->cap_pad, std::max(64, (t->bound + 63) / 64 * 64));
    hipLaunchKernelGGL(trk_begin_kernel, dim3(1), dim3(kTrkBlock), 0, st, t->T, n, xy, depth, t->width, t->height, t->fx, t->fy, t->cx,
                       t->cy, history, t->q_co, t->active_idx);
    hipLaunchKernelGGL(trk_gather_kernel, dim3(tracker_row_blocks(nt_pad)), dim3(256), 0, st, t->T, (const float*)t->desc[t->cur],
                       (const int*)t->active_idx, t->train, nt_pad);
    // the search: the kernels of mmf_match_descriptors.  Without keypoints one padding row stands in for the query set (its
    // result is not read), so that the call is the same launches whatever n is.
    const float* q = n ? descriptor : t->train;
    const int nq = std::max(n, 1);
    unsigned long long *row_best = t->keys, *col_best = t->keys + nq;
    float *qn = t->norms, *tn = t->norms + nq;
    hipLaunchKernelGGL(row_norms_kernel, dim3((nq + 31) / 32 + (nt_pad + 31) / 32), dim3(64), 0, st, q, nq, (const float*)t->train, nt_pad,
                       kTrkDim, qn, tn, row_best, col_best, kNoMatchKey);
    hipLaunchKernelGGL(match_tile64_kernel, dim3((nt_pad + 63) / 64, (nq + 63) / 64), dim3(256), 0, st, q, (const float*)t->train,
                       (const float*)qn, (const float*)tn, nq, nt_pad, kTrkDim, row_best, col_best);
    hipLaunchKernelGGL(match_cross_check_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, row_best, (const unsigned long long*)col_best,
                       nq, min_feature_distance, t->train_idx, t->q_dist);
    hipLaunchKernelGGL(trk_finish_kernel, dim3(1), dim3(kTrkBlock), 0, st, t->T, t->rec, n, xy, (const float*)t->q_co,
                       (const int*)t->train_idx, (const int*)t->active_idx, timestamp, t->dest_row);
    hipLaunchKernelGGL(trk_scatter_rows_kernel, dim3(tracker_row_blocks(std::max(n, 1))), dim3(256), 0, st, descriptor, n,
                       (const int*)t->dest_row, t->desc[t->cur], t->capacity);
    tracker_add_tail(t, timestamp);
    MMF_HIP_TRY(hipGetLastError());
    t->bound = (int)std::min<long long>(t->capacity, (long long)t->bound + n);
    t->caller_adds += 1;
    return MMF_OK;
}

// mmf_tracker_add_keypoints with the number of keypoints in DEVICE memory: the same 7 (9) launches, the `counted` forms of
// the kernels that take n.  Their grids, and the [query ; train] layouts of keys / norms, are those of max_keypoints
// queries; rows from n on (stale keypoints of earlier frames) are read by none of them.  The host's bound grows by the
// most there can be: the padding rows that costs are fillers nothing matches.
static int tracker_add_counted(mmf_tracker* t, const int* n_dev, const int* fail_dev, const int* xy, const float* descriptor,
                               const float* depth, long long timestamp, float min_feature_distance, int history) {
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    using namespace mmf;
    const int K = t->max_keypoints;
    const int nt_pad = std::min(t->cap_pad, std::max(64, (t->bound + 63) / 64 * 64));
    hipLaunchKernelGGL(trk_begin_counted_kernel, dim3(1), dim3(kTrkBlock), 0, st, t->T, n_dev, fail_dev, K, xy, depth, t->width,
                       t->height, t->fx, t->fy, t->cx, t->cy, history, t->q_co, t->active_idx);
    hipLaunchKernelGGL(trk_gather_kernel, dim3(tracker_row_blocks(nt_pad)), dim3(256), 0, st, t->T, (const float*)t->desc[t->cur],
                       (const int*)t->active_idx, t->train, nt_pad);
    unsigned long long *row_best = t->keys, *col_best = t->keys + K;
    float *qn = t->norms, *tn = t->norms + K;
    hipLaunchKernelGGL(row_norms_counted_kernel, dim3((K + 31) / 32 + (nt_pad + 31) / 32), dim3(64), 0, st, descriptor, n_dev, fail_dev, K,
                       (const float*)t->train, nt_pad, kTrkDim, qn, tn, row_best, col_best, kNoMatchKey);
    hipLaunchKernelGGL(match_tile64_counted_kernel, dim3((nt_pad + 63) / 64, (K + 63) / 64), dim3(256), 0, st, descriptor,
                       (const float*)t->train, (const float*)qn, (const float*)tn, n_dev, fail_dev, K, nt_pad, kTrkDim, row_best, col_best);
    hipLaunchKernelGGL(match_cross_check_counted_kernel, dim3((K + 255) / 256), dim3(256), 0, st, row_best,
                       (const unsigned long long*)col_best, n_dev, fail_dev, K, min_feature_distance, t->train_idx, t->q_dist);
    hipLaunchKernelGGL(trk_finish_counted_kernel, dim3(1), dim3(kTrkBlock), 0, st, t->T, t->rec, n_dev, fail_dev, K, xy,
                       (const float*)t->q_co, (const int*)t->train_idx, (const int*)t->active_idx, timestamp, t->dest_row);
    hipLaunchKernelGGL(trk_scatter_rows_counted_kernel, dim3(tracker_row_blocks(K)), dim3(256), 0, st, descriptor, n_dev, fail_dev, K,
                       (const int*)t->dest_row, t->desc[t->cur], t->capacity);
    tracker_add_tail(t, timestamp);
    MMF_HIP_TRY(hipGetLastError());
    t->bound = (int)std::min<long long>(t->capacity, (long long)t->bound + K);
    return MMF_OK;
}

extern "C" int mmf_tracker_add_keypoints_device(mmf_tracker* t, const int* n_dev, const int* xy, const float* descriptor,
                                                const float* depth, long long timestamp, float min_feature_distance, int history) {
    MMF_REQUIRE(t && n_dev && xy && descriptor && depth, "mmf_tracker_add_keypoints_device: null argument");
    MMF_REQUIRE(history >= 0, "mmf_tracker_add_keypoints_device: negative history");
    MMF_REQUIRE(((uintptr_t)descriptor & 15u) == 0, "mmf_tracker_add_keypoints_device: 16-byte aligned descriptor rows");
    const int rc = tracker_add_counted(t, n_dev, t->kp_status, xy, descriptor, depth, timestamp, min_feature_distance, history);
    if (!rc) t->caller_adds += 1;
    return rc;
}

// the status word of whatever produces *n_dev (mmf_superpoint_device_features' neighbour, say): a DEVICE int the device-count
// adds read from now on; while it is not 0 an add is a frame without keypoints and counts as failed.  NULL: none.
extern "C" int mmf_tracker_set_keypoint_status(mmf_tracker* t, const int* status_dev) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_set_keypoint_status: null tracker");
    t->kp_status = status_dev;
    return MMF_OK;
}

// waits: the device-count adds since creation / reset whose status word was set
extern "C" int mmf_tracker_keypoint_failures(mmf_tracker* t, int* failures) {
    MMF_REQUIRE(t && failures, "mmf_tracker_keypoint_failures: null argument");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    MMF_HIP_TRY(wait_stream(t->ctx->stream));
    tracker_refresh(t);
    *failures = t->rec->kp_failed;
    return MMF_OK;
}

// the view log: frames = 0 switches it off (the default) and frees the ring; any other value allocates a ring of that many
// slots HERE, behind a wait for the stream (work in flight may still write the old ring), never in the frame path.  It starts
// empty: the first frame it can hold is the next add.
extern "C" int mmf_tracker_set_view_log(mmf_tracker* t, int frames) {
    MMF_REQUIRE(t && frames >= 0 && frames <= (1 << 16), "mmf_tracker_set_view_log: frames must be 0 .. 65536");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    if (frames == 0 && t->log.frames == 0) return MMF_OK;
    hipStream_t st = t->ctx->stream;
    MMF_HIP_TRY(hipStreamSynchronize(st));
    tracker_free_log(t);
    t->log_first = t->frame + 1;
    t->add_ts.assign((size_t)frames, 0ll);
    t->bd_valid = false;
    if (frames == 0) return MMF_OK;
    const size_t F = (size_t)frames, K = (size_t)t->max_keypoints;
    mmf::TrkLog L{};
    L.frames = frames, L.max_kp = t->max_keypoints;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&L.count), F * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&L.stamp), F * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&L.uid), F * K * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&L.co), F * K * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&L.desc), F * K * mmf::kTrkDim * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(L.count, 0, F * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(L.stamp, 0xff, F * sizeof(long long), st);  // -1: no frame
    t->log = L;
    if (e != hipSuccess) {
        tracker_free_log(t);
        MMF_HIP_TRY(e);
    }
    return MMF_OK;
}

extern "C" int mmf_tracker_frame(mmf_tracker* t) { return t ? (int)t->frame : -1; }

// the frame `stamp` is in the ring: logged since the log was switched on / the tracker reset, and not yet overwritten
static bool tracker_in_log(const mmf_tracker* t, long long stamp) {
    return t->log.frames > 0 && stamp >= t->log_first && stamp <= t->frame && stamp > t->frame - t->log.frames;
}

// Model::store's views (Model.cpp:1617-1644, computeTrackProjectionFirstFrame :508-522, project_kp :130-141, the filter of
// getBestMatch :806-811) of one model from the log: view v = the logged keypoints of frame frames[v], in log order, whose
// track is in the table and in the model NOW, in the frame poses[v] maps the camera frame to, the non-finite ones dropped.
// One launch (flags, compaction, coordinates, counts), ONE wait, one launch that packs the rows.  *counts = pinned HOST
// [n_views], *descriptor / *coordinate = DEVICE, the views' rows one after the other; valid until the tracker's next call.
// *missing = the views whose frame is not in the ring (they are empty).
extern "C" int mmf_tracker_model_views(mmf_tracker* t, int model_id, int n_views, const int* frames, const float* poses,
                                       const int** counts, const float** descriptor, const float** coordinate, int* missing) {
    MMF_REQUIRE(t && n_views >= 0 && n_views <= 65535 && ((frames && poses) || n_views == 0), "mmf_tracker_model_views: bad argument");
    MMF_REQUIRE(model_id >= 0 && model_id < mmf::kTrkMaxModels, "mmf_tracker_model_views: model ids are 0 .. 255");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    using namespace mmf;
    const size_t K = (size_t)t->max_keypoints;
    if (std::max(n_views, 1) > t->view_cap) {  // (every earlier views call has been awaited; what packed its rows may still run)
        MMF_HIP_TRY(hipStreamSynchronize(st));
        tracker_free_views(t);
        const size_t cap = (size_t)std::max(16, 2 * n_views);
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->req_pin), cap * sizeof(TrkViewRequest), hipHostMallocDefault));
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->view_count_pin), cap * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->req_dev), cap * sizeof(TrkViewRequest)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->view_count_dev), cap * sizeof(int)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->view_row), cap * K * sizeof(int)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->view_co), cap * K * 3 * sizeof(float)));
        t->view_cap = (int)cap;
    }
    int absent = 0;
    for (int v = 0; v < n_views; ++v) {
        TrkViewRequest& r = t->req_pin[v];
        const bool in = tracker_in_log(t, frames[v]);
        absent += in ? 0 : 1;
        r.slot = in ? (int)(frames[v] % t->log.frames) : -1, r.pad_ = 0, r.stamp = frames[v];
        std::memcpy(r.pose, poses + 16 * (size_t)v, sizeof(r.pose));
        t->view_count_pin[v] = 0;
    }
    if (n_views > 0)
        MMF_HIP_TRY(hipMemcpyAsync(t->req_dev, t->req_pin, (size_t)n_views * sizeof(TrkViewRequest), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(trk_views_kernel, dim3((unsigned)std::max(n_views, 1)), dim3(kTrkBlock), 0, st, t->T, t->log,
                       (const TrkViewRequest*)t->req_dev, n_views, model_id, t->view_row, t->view_co, t->view_count_pin, t->view_count_dev);
    MMF_HIP_TRY(hipGetLastError());
    MMF_HIP_TRY(wait_stream(st));
    size_t total = 0;
    int most = 0;
    for (int v = 0; v < n_views; ++v) {
        MMF_REQUIRE(t->view_count_pin[v] >= 0 && (size_t)t->view_count_pin[v] <= K, "mmf_tracker_model_views: a view's count is out of range");
        total += (size_t)t->view_count_pin[v], most = std::max(most, t->view_count_pin[v]);
    }
    if (std::max<size_t>(total, 1) > t->view_out_rows) {  // (the stream is idle: nothing reads the old buffers)
        (void)hipFree(t->view_out_desc);
        (void)hipFree(t->view_out_co);
        t->view_out_desc = t->view_out_co = nullptr, t->view_out_rows = 0;
        const size_t cap = std::max<size_t>(64, total + total / 2);
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->view_out_desc), cap * kTrkDim * sizeof(float)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->view_out_co), cap * 3 * sizeof(float)));
        t->view_out_rows = cap;
    }
    hipLaunchKernelGGL(trk_views_pack_kernel, dim3(tracker_row_blocks(std::max(most, 1)), (unsigned)std::max(n_views, 1)), dim3(256), 0, st,
                       t->log, (const int*)t->view_count_dev, n_views, (const int*)t->view_row, (const float*)t->view_co, t->view_out_desc,
                       t->view_out_co);
    MMF_HIP_TRY(hipGetLastError());
    t->last_launches = 2;
    if (counts) *counts = t->view_count_pin;
    if (descriptor) *descriptor = t->view_out_desc;
    if (coordinate) *coordinate = t->view_out_co;
    if (missing) *missing = absent;
    return MMF_OK;
}

extern "C" int mmf_tracker_prune(mmf_tracker* t, int min_kps, long long min_time) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_prune: null tracker");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    hipLaunchKernelGGL(mmf::trk_prune_kernel, dim3(1), dim3(mmf::kTrkBlock), 0, st, t->T, t->rec, min_kps, min_time, t->map);
    hipLaunchKernelGGL(mmf::trk_gather_rows_kernel, dim3(tracker_row_blocks(std::max(t->bound, 1))), dim3(256), 0, st,
                       (const float*)t->desc[t->cur], (const int*)t->map, (const int*)&t->T.head->n_tracks, t->desc[t->cur ^ 1],
                       t->capacity);
    MMF_HIP_TRY(hipGetLastError());
    t->cur ^= 1;
    t->last_launches = 2;
    return MMF_OK;
}

static int tracker_model_set(const int* model_ids, int n_models, mmf::TrkModelSet* set, const char* who) {
    std::memset(set, 0, sizeof(*set));
    if (n_models < 0 || (n_models > 0 && !model_ids)) return fail(MMF_ERR_INVALID, std::string(who) + ": bad model list");
    for (int k = 0; k < n_models; ++k) {
        if (model_ids[k] < 0 || model_ids[k] >= mmf::kTrkMaxModels) return fail(MMF_ERR_INVALID, std::string(who) + ": model ids are 0 .. 255");
        set->w[model_ids[k] >> 5] |= 1u << (model_ids[k] & 31);
    }
    return MMF_OK;
}

extern "C" int mmf_tracker_associate(mmf_tracker* t, const uint8_t* mask, const int* model_ids, int n_models) {
    MMF_REQUIRE(t && mask, "mmf_tracker_associate: null argument");
    mmf::TrkModelSet set;
    int rc = tracker_model_set(model_ids, n_models, &set, "mmf_tracker_associate");
    if (rc) return rc;
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipLaunchKernelGGL(mmf::trk_associate_kernel, dim3(1), dim3(mmf::kTrkBlock), 0, t->ctx->stream, t->T, mask, t->width, t->height, set);
    MMF_HIP_TRY(hipGetLastError());
    t->last_launches = 1;
    return MMF_OK;
}

static int tracker_member(mmf_tracker* t, const mmf::TrkModelSet& set, int clear) {
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    const unsigned blocks = (unsigned)std::min(64, std::max(1, (t->bound * mmf::kTrkWords + 255) / 256));
    hipLaunchKernelGGL(mmf::trk_member_kernel, dim3(blocks), dim3(256), 0, t->ctx->stream, t->T, set, clear);
    MMF_HIP_TRY(hipGetLastError());
    t->last_launches = 1;
    return MMF_OK;
}

extern "C" int mmf_tracker_associate_all(mmf_tracker* t, const int* model_ids, int n_models) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_associate_all: null tracker");
    mmf::TrkModelSet set;
    int rc = tracker_model_set(model_ids, n_models, &set, "mmf_tracker_associate_all");
    if (rc) return rc;
    return tracker_member(t, set, 0);
}

extern "C" int mmf_tracker_forget_model(mmf_tracker* t, int model_id) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_forget_model: null tracker");
    mmf::TrkModelSet set;
    int rc = tracker_model_set(&model_id, 1, &set, "mmf_tracker_forget_model");
    if (rc) return rc;
    return tracker_member(t, set, 1);
}

// the pair lists of n_models models in one launch and one wait.  *p0 / *p1 = pinned [n_models][*stride][3], *counts =
// pinned [n_models]; they stay valid until the next call of the tracker that writes them.
extern "C" int mmf_tracker_last_pairs(mmf_tracker* t, const int* model_ids, int n_models, const float** p0, const float** p1,
                                      const int** counts, int* stride) {
    MMF_REQUIRE(t && n_models >= 0 && n_models <= mmf::kTrkMaxModels && (model_ids || n_models == 0), "mmf_tracker_last_pairs: bad argument");
    mmf::TrkModelList list;
    std::memset(&list, 0, sizeof(list));
    list.n = n_models;
    for (int k = 0; k < n_models; ++k) {
        MMF_REQUIRE(model_ids[k] >= 0 && model_ids[k] < mmf::kTrkMaxModels, "mmf_tracker_last_pairs: model ids are 0 .. 255");
        list.id[k] = (unsigned char)model_ids[k];
    }
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    if (n_models > t->pair_models) {  // (every earlier pairs call has been awaited)
        if (t->p0) (void)hipHostFree(t->p0);
        if (t->p1) (void)hipHostFree(t->p1);
        t->p0 = t->p1 = nullptr, t->pair_models = 0;
        const int cap = std::min(mmf::kTrkMaxModels, std::max(16, 2 * n_models));
        const size_t bytes = (size_t)cap * t->capacity * 3 * sizeof(float);
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->p0), bytes, hipHostMallocMapped | hipHostMallocCoherent));
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->p1), bytes, hipHostMallocMapped | hipHostMallocCoherent));
        t->pair_models = cap;
    }
    t->last_launches = 0;
    if (n_models > 0) {
        hipLaunchKernelGGL(mmf::trk_pairs_kernel, dim3((unsigned)n_models), dim3(mmf::kTrkBlock), 0, st, t->T, t->rec, list, t->p0, t->p1,
                           t->capacity);
        MMF_HIP_TRY(hipGetLastError());
        t->last_launches = 1;
        MMF_HIP_TRY(wait_stream(st));
        tracker_refresh(t);
    }
    if (p0) *p0 = t->p0;
    if (p1) *p1 = t->p1;
    if (counts) *counts = t->rec->pair_count;
    if (stride) *stride = t->capacity;
    return MMF_OK;
}

static const mmf::RigidRANSAC::Config kTrackRansac{10, 0.03f, 0.6f};  // Model.h: getLastTrackTransform's default

// Model::getLastTrackTransform from n pairs: a fresh RigidRANSAC (:771); fewer than 3 pairs: identity, no inliers (:766-768)
static mmf::RigidRANSAC::Result tracker_transform(const float* p0, const float* p1, int n, const mmf::RigidRANSAC::Config& cfg) {
    if (n < 3) return mmf::RigidRANSAC::Result{};
    mmf::RigidRANSAC ransac(cfg);
    return ransac.estimate(p0, p1, n);
}

extern "C" int mmf_tracker_last_track_transform(mmf_tracker* t, int model_id, const mmf_ransac_config* cfg, float T[16], float* error,
                                                unsigned char* inlier, int* has_inlier) {
    MMF_REQUIRE(t && T, "mmf_tracker_last_track_transform: null argument");
    const float *p0 = nullptr, *p1 = nullptr;
    const int* counts = nullptr;
    int rc = mmf_tracker_last_pairs(t, &model_id, 1, &p0, &p1, &counts, nullptr);
    if (rc) return rc;
    const mmf::RigidRANSAC::Config c = cfg ? mmf::RigidRANSAC::Config{cfg->iterations, cfg->inlier_threshold, cfg->inlier_fraction} : kTrackRansac;
    const int n = counts[0];
    const mmf::RigidRANSAC::Result res = tracker_transform(p0, p1, n, c);
    isometry_to_4x4(res.transformation, T);
    if (error) *error = res.error;
    if (has_inlier) *has_inlier = res.inlier.empty() ? 0 : 1;
    if (inlier)
        for (int i = 0; i < n; ++i) inlier[i] = res.inlier.empty() ? 0 : res.inlier[(size_t)i];
    return MMF_OK;
}

// the visible set into the tracker's device buffers and the wait; *n rows
static int tracker_visible_device(mmf_tracker* t, int* n) {
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    hipLaunchKernelGGL(mmf::trk_visible_kernel, dim3(1), dim3(mmf::kTrkBlock), 0, st, t->T, t->rec, t->map, t->count, t->vis_xy, t->vis_co,
                       t->vis_uid);
    hipLaunchKernelGGL(mmf::trk_gather_rows_kernel, dim3(tracker_row_blocks(std::max(t->bound, 1))), dim3(256), 0, st,
                       (const float*)t->desc[t->cur], (const int*)t->map, (const int*)t->count, t->vis_desc, t->capacity);
    MMF_HIP_TRY(hipGetLastError());
    t->last_launches = 2;
    MMF_HIP_TRY(wait_stream(st));
    tracker_refresh(t);
    *n = std::min(t->capacity, std::max(0, t->rec->n_visible));
    return MMF_OK;
}

extern "C" int mmf_tracker_visible(mmf_tracker* t, int capacity, int* n, int* xy, float* coordinate, float* descriptor, long long* uid) {
    MMF_REQUIRE(t && n && capacity >= 0, "mmf_tracker_visible: bad argument");
    int rc = tracker_visible_device(t, n);
    if (rc) return rc;
    const size_t k = (size_t)*n;
    if (k == 0 || !(xy || coordinate || descriptor || uid)) return MMF_OK;
    MMF_REQUIRE(*n <= capacity, "mmf_tracker_visible: more visible tracks than the arrays hold");
    if (xy) MMF_HIP_TRY(hipMemcpy(xy, t->vis_xy, k * 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (coordinate) MMF_HIP_TRY(hipMemcpy(coordinate, t->vis_co, k * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (descriptor) MMF_HIP_TRY(hipMemcpy(descriptor, t->vis_desc, k * mmf::kTrkDim * sizeof(float), hipMemcpyDeviceToHost));
    if (uid) MMF_HIP_TRY(hipMemcpy(uid, t->vis_uid, k * sizeof(long long), hipMemcpyDeviceToHost));
    return MMF_OK;
}

extern "C" int mmf_tracker_status(mmf_tracker* t, int* n_tracks, int* length, int* dropped) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_status: null tracker");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    MMF_HIP_TRY(wait_stream(t->ctx->stream));
    tracker_refresh(t);
    if (n_tracks) *n_tracks = t->rec->n_tracks;
    if (length) *length = t->rec->length;
    if (dropped) *dropped = t->rec->dropped;
    return MMF_OK;
}

// the whole table into HOST arrays of `capacity` rows (the two-slot arrays: slot 0 = cur at row 0, slot 1 = prev at row
// `capacity`); any array may be null
extern "C" int mmf_tracker_download(mmf_tracker* t, int capacity, int* n_tracks, float* descriptor, int* age, int* nvalid,
                                    long long* last_stamp, long long* uid, int* xy, float* coordinate, long long* timestamp,
                                    int* nonnull, unsigned* member, int* label) {
    MMF_REQUIRE(t && n_tracks && capacity >= 0, "mmf_tracker_download: bad argument");
    int rc = mmf_tracker_status(t, n_tracks, nullptr, nullptr);
    if (rc) return rc;
    const size_t n = (size_t)*n_tracks, C = (size_t)capacity;
    if (n == 0) return MMF_OK;
    MMF_REQUIRE(*n_tracks <= capacity, "mmf_tracker_download: more tracks than the arrays hold");
    auto get = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    MMF_HIP_TRY(get(descriptor, t->desc[t->cur], n * mmf::kTrkDim * sizeof(float)));
    MMF_HIP_TRY(get(age, t->T.age, n * sizeof(int)));
    MMF_HIP_TRY(get(nvalid, t->T.nvalid, n * sizeof(int)));
    MMF_HIP_TRY(get(last_stamp, t->T.last_stamp, n * sizeof(long long)));
    MMF_HIP_TRY(get(uid, t->T.uid, n * sizeof(long long)));
    MMF_HIP_TRY(get(member, t->T.member, n * mmf::kTrkWords * sizeof(unsigned)));
    MMF_HIP_TRY(get(label, t->T.label, n * sizeof(int)));
    for (size_t s = 0; s < 2; ++s) {
        MMF_HIP_TRY(get(xy ? xy + s * C * 2 : nullptr, t->T.xy[s], n * 2 * sizeof(int)));
        MMF_HIP_TRY(get(coordinate ? coordinate + s * C * 3 : nullptr, t->T.co[s], n * 3 * sizeof(float)));
        MMF_HIP_TRY(get(timestamp ? timestamp + s * C : nullptr, t->T.ts[s], n * sizeof(long long)));
        MMF_HIP_TRY(get(nonnull ? nonnull + s * C : nullptr, t->T.ok[s], n * sizeof(int)));
    }
    return MMF_OK;
}

#include "backdate_host.hpp"
