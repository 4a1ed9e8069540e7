// redetect_host.hpp -- the view store and Model::getBestMatch (Core/Model/Model.cpp:781-874) on top of
// redetect_kernels.hpp.  Textually included by mmf_hip.hip (it uses that file's helpers and rigid_ransac.hpp).
//
// A view = the valid keypoints of one time index of a model's stored local tracks (tracks_local: the result of
// computeTrackProjectionFirstFrame, Model.cpp:508-522, null and non-finite keypoints dropped, :806-811): n descriptors of
// 256 floats on the device, n coordinates in the model's frame on the host (RigidRANSAC is host code).  All views of all
// models share one descriptor buffer, each padded with zero rows to a multiple of 32; the per-tile table says which view
// a 32-row tile belongs to and how many of its rows are real.
//
// Growth: the buffers double.  The old ones are copied on the context's stream and are NOT freed until the store is
// destroyed (`retired`): work already enqueued keeps reading memory that stays valid, and no hipFree -- a device-wide
// synchronisation -- happens between frames.  The doubling bounds what is retired by the size of the live buffers.
// The match workspace and the result buffers are different: every match is awaited by the host before its call returns,
// so nothing enqueued reads them when they grow.
#pragma once

#include "redetect_kernels.hpp"

constexpr int kRdDim = 256;  // SuperPoint descriptors

struct RdView {
    int model, index, rows;  // model id, time index inside the model's stored tracks, valid keypoints
    size_t row0, coord0;     // first row in the descriptor buffer (a multiple of 32); first point in `coords`
};

struct RdSet {  // one query set of a batch of matches
    const float* q;  // DEVICE [nq][256]
    int nq;
    size_t q0;  // offset of the set in the query-row dimension of the workspace and of the results
};

struct mmf_viewstore {
    mmf_ctx* ctx = nullptr;
    std::vector<RdView> views;  // store order = model by model as stored, a model's views ascending
    std::vector<float> coords;
    std::vector<mmf::RdTile> tiles_host;
    float *desc = nullptr, *tn = nullptr;
    mmf::RdTile* tiles = nullptr;
    size_t cap_rows = 0, n_rows = 0;  // rows = 32 * tiles
    std::vector<void*> retired;
    void* ws = nullptr;  // qn | row_best | col_best
    size_t ws_bytes = 0;
    int* out_row = nullptr;  // host memory the device writes: [view][query row] store row or -1
    float* out_dist = nullptr;
    size_t out_cap = 0;
    float *q_pin = nullptr, *q_dev = nullptr;  // queries handed in on the host (the fusion's keypoints)
    size_t q_cap = 0;
    int last_launches = 0;
    // mmf_viewstore_store_device: per-tile first packed row (device) and the coordinates on their way to `coords` (pinned)
    int* src0_dev = nullptr;
    size_t src0_cap = 0;
    float* co_pin = nullptr;
    size_t co_cap = 0;
    // the device verifier (mmf_viewstore_set_verifier; nothing below is allocated, written or launched without one): the
    // books again on the device, the match rows, the per-view estimates and the records the host reads
    mmf_ransac_batch* verifier = nullptr;
    float* coords_dev = nullptr;  // `coords`
    size_t coords_cap = 0;        // points
    mmf::RdViewDev* views_dev = nullptr;
    size_t views_cap = 0;
    int* rows_dev = nullptr;  // rd_cross_kernel's rows, laid out as out_row
    size_t rows_cap = 0;
    mmf::RdViewResult* per_view = nullptr;
    size_t per_view_cap = 0;
    unsigned char* per_view_inlier = nullptr;
    size_t per_view_inlier_cap = 0;
    unsigned char *arg_pin = nullptr, *arg_dev = nullptr;  // the sets and the asked models on their way to the device
    size_t arg_cap = 0;
    mmf::RdRecord* rec_pin = nullptr;  // host memory the device writes: [set][asked model]
    size_t rec_cap = 0;
    unsigned char* rec_inlier_pin = nullptr;
    size_t rec_inlier_cap = 0;
    float *qc_pin = nullptr, *qc_dev = nullptr;  // query coordinates handed in on the host (the fusion's keypoints)
    size_t qc_cap = 0;
    int rec_stride = 0, rec_asked = 0;  // layout of the last verification's records
};

extern "C" int mmf_viewstore_create(mmf_ctx* c, mmf_viewstore** out) {
    MMF_REQUIRE(c && out, "mmf_viewstore_create: null argument");
    *out = new (std::nothrow) mmf_viewstore();
    MMF_REQUIRE(*out != nullptr, "mmf_viewstore_create: out of host memory");
    (*out)->ctx = c;
    return MMF_OK;
}

extern "C" void mmf_viewstore_destroy(mmf_viewstore* vs) {
    if (!vs) return;
    (void)hipSetDevice(vs->ctx->device);
    (void)hipStreamSynchronize(vs->ctx->stream);
    for (void* p : vs->retired) (void)hipFree(p);
    (void)hipFree(vs->desc);
    (void)hipFree(vs->tn);
    (void)hipFree(vs->tiles);
    (void)hipFree(vs->ws);
    (void)hipFree(vs->q_dev);
    if (vs->out_row) (void)hipHostFree(vs->out_row);
    if (vs->out_dist) (void)hipHostFree(vs->out_dist);
    if (vs->q_pin) (void)hipHostFree(vs->q_pin);
    (void)hipFree(vs->src0_dev);
    if (vs->co_pin) (void)hipHostFree(vs->co_pin);
    (void)hipFree(vs->coords_dev);
    (void)hipFree(vs->views_dev);
    (void)hipFree(vs->rows_dev);
    (void)hipFree(vs->per_view);
    (void)hipFree(vs->per_view_inlier);
    (void)hipFree(vs->arg_dev);
    (void)hipFree(vs->qc_dev);
    if (vs->arg_pin) (void)hipHostFree(vs->arg_pin);
    if (vs->rec_pin) (void)hipHostFree(vs->rec_pin);
    if (vs->rec_inlier_pin) (void)hipHostFree(vs->rec_inlier_pin);
    if (vs->qc_pin) (void)hipHostFree(vs->qc_pin);
    delete vs;
}

static bool viewstore_has_model(const mmf_viewstore* vs, int model) {
    for (const RdView& v : vs->views)
        if (v.model == model) return true;
    return false;
}

// room for `rows` more rows (a multiple of 32): new buffers of twice the size, the old contents copied on the stream
static int viewstore_reserve(mmf_viewstore* vs, size_t rows) {
    if (vs->n_rows + rows <= vs->cap_rows) return MMF_OK;
    size_t cap = vs->cap_rows ? vs->cap_rows * 2 : 4096;
    while (cap < vs->n_rows + rows) cap *= 2;
    hipStream_t st = vs->ctx->stream;
    float *desc = nullptr, *tn = nullptr;
    mmf::RdTile* tiles = nullptr;
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&desc), cap * kRdDim * sizeof(float)));
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&tn), cap * sizeof(float)));
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&tiles), cap / 32 * sizeof(mmf::RdTile)));
    if (vs->n_rows) {
        MMF_HIP_TRY(hipMemcpyAsync(desc, vs->desc, vs->n_rows * kRdDim * sizeof(float), hipMemcpyDeviceToDevice, st));
        MMF_HIP_TRY(hipMemcpyAsync(tn, vs->tn, vs->n_rows * sizeof(float), hipMemcpyDeviceToDevice, st));
        MMF_HIP_TRY(hipMemcpyAsync(tiles, vs->tiles, vs->n_rows / 32 * sizeof(mmf::RdTile), hipMemcpyDeviceToDevice, st));
    }
    for (void* p : {(void*)vs->desc, (void*)vs->tn, (void*)vs->tiles})
        if (p) vs->retired.push_back(p);  // (enqueued work may still read them: freed with the store)
    vs->desc = desc, vs->tn = tn, vs->tiles = tiles, vs->cap_rows = cap;
    return MMF_OK;
}

// With a verifier attached the store keeps its coordinates and its view table on the device as well: the points from
// `first_point` on are uploaded (growth copies the earlier ones like the descriptors and retires the old buffer), the view
// table -- small -- whole.  Waits for the stream: the sources are pageable.  Without a verifier: nothing.
static int viewstore_device_books(mmf_viewstore* vs, size_t first_point) {
    if (!vs->verifier) return MMF_OK;
    hipStream_t st = vs->ctx->stream;
    const size_t P = vs->coords.size() / 3, V = vs->views.size();
    if (P > vs->coords_cap) {
        size_t cap = vs->coords_cap ? vs->coords_cap * 2 : 4096;
        while (cap < P) cap *= 2;
        float* fresh = nullptr;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&fresh), cap * 3 * sizeof(float)));
        if (vs->coords_dev && first_point)
            MMF_HIP_TRY(hipMemcpyAsync(fresh, vs->coords_dev, first_point * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (vs->coords_dev) vs->retired.push_back(vs->coords_dev);
        vs->coords_dev = fresh, vs->coords_cap = cap;
    }
    if (P > first_point)
        MMF_HIP_TRY(hipMemcpyAsync(vs->coords_dev + 3 * first_point, vs->coords.data() + 3 * first_point, (P - first_point) * 3 * sizeof(float),
                                   hipMemcpyHostToDevice, st));
    if (V > vs->views_cap) {
        size_t cap = vs->views_cap ? vs->views_cap * 2 : 256;
        while (cap < V) cap *= 2;
        mmf::RdViewDev* fresh = nullptr;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&fresh), cap * sizeof(mmf::RdViewDev)));
        if (vs->views_dev) vs->retired.push_back(vs->views_dev);
        vs->views_dev = fresh, vs->views_cap = cap;
    }
    std::vector<mmf::RdViewDev> table(V);
    for (size_t v = 0; v < V; ++v)
        table[v] = mmf::RdViewDev{vs->views[v].model, vs->views[v].index, vs->views[v].rows, (int)vs->views[v].row0, (int)vs->views[v].coord0};
    if (V) MMF_HIP_TRY(hipMemcpyAsync(vs->views_dev, table.data(), V * sizeof(mmf::RdViewDev), hipMemcpyHostToDevice, st));
    MMF_HIP_TRY(hipStreamSynchronize(st));
    return MMF_OK;
}

// Model::store (Model.cpp:1617-1632): the views of one model.  counts[n_views] valid keypoints per view (0 allowed);
// descriptor / coordinate = the views' rows one after the other.  *stored = 0: the model has stored views already and
// this call changed nothing (:1618-1621).
extern "C" int mmf_viewstore_store(mmf_viewstore* vs, int model_id, int n_views, const int* counts, const float* descriptor,
                                   const float* coordinate, int* stored) {
    MMF_REQUIRE(vs && n_views >= 0 && (counts || n_views == 0), "mmf_viewstore_store: bad argument");
    if (stored) *stored = 0;
    if (viewstore_has_model(vs, model_id)) return MMF_OK;
    size_t total = 0, padded = 0;
    for (int v = 0; v < n_views; ++v) {
        MMF_REQUIRE(counts[v] >= 0, "mmf_viewstore_store: negative view size");
        total += (size_t)counts[v], padded += ((size_t)counts[v] + 31) / 32 * 32;
    }
    MMF_REQUIRE(total == 0 || (descriptor && coordinate), "mmf_viewstore_store: null descriptors or coordinates");
    MMF_REQUIRE(vs->n_rows + padded < (size_t)1 << 31, "mmf_viewstore_store: more than 2^31 rows");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    hipStream_t st = vs->ctx->stream;
    if (padded) {
        int rc = viewstore_reserve(vs, padded);
        if (rc) return rc;
    }
    std::vector<float> block(padded * kRdDim, 0.f);  // the views' rows with their zero padding
    const size_t first_tile = vs->tiles_host.size(), first_point = vs->coords.size() / 3;
    size_t src = 0, dst = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)counts[v];
        vs->views.push_back(RdView{model_id, v, counts[v], vs->n_rows + dst, vs->coords.size() / 3});
        if (n) {
            std::memcpy(block.data() + dst * kRdDim, descriptor + src * kRdDim, n * kRdDim * sizeof(float));
            vs->coords.insert(vs->coords.end(), coordinate + src * 3, coordinate + (src + n) * 3);
        }
        for (size_t r = 0; r < n; r += 32)
            vs->tiles_host.push_back(mmf::RdTile{(int)vs->views.size() - 1, (int)std::min<size_t>(32, n - r)});
        src += n, dst += (n + 31) / 32 * 32;
    }
    if (padded) {
        MMF_HIP_TRY(hipMemcpyAsync(vs->desc + vs->n_rows * kRdDim, block.data(), padded * kRdDim * sizeof(float), hipMemcpyHostToDevice, st));
        MMF_HIP_TRY(hipMemcpyAsync(vs->tiles + first_tile, vs->tiles_host.data() + first_tile, padded / 32 * sizeof(mmf::RdTile),
                                   hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mmf::rd_train_norms_kernel, dim3((unsigned)(padded / 32)), dim3(64), 0, st, vs->desc + vs->n_rows * kRdDim,
                           (int)padded, kRdDim, vs->tn + vs->n_rows);
        MMF_HIP_TRY(hipGetLastError());
        MMF_HIP_TRY(hipStreamSynchronize(st));  // `block` leaves scope
        vs->n_rows += padded;
    }
    int rc = viewstore_device_books(vs, first_point);
    if (rc) return rc;
    if (stored) *stored = 1;
    return MMF_OK;
}

// mmf_viewstore_store with the views' rows on the DEVICE (mmf_tracker_model_views): counts = HOST, descriptor / coordinate =
// DEVICE, packed.  A kernel scatters the rows to their 32-row-padded places and writes the padding; tiles and norms as above;
// the coordinates reach `coords` through pinned memory.  One wait at the end.  The store is then what mmf_viewstore_store
// leaves with the same views downloaded.
extern "C" int mmf_viewstore_store_device(mmf_viewstore* vs, int model_id, int n_views, const int* counts, const float* descriptor,
                                          const float* coordinate, int* stored) {
    MMF_REQUIRE(vs && n_views >= 0 && (counts || n_views == 0), "mmf_viewstore_store_device: bad argument");
    if (stored) *stored = 0;
    if (viewstore_has_model(vs, model_id)) return MMF_OK;
    size_t total = 0, padded = 0;
    for (int v = 0; v < n_views; ++v) {
        MMF_REQUIRE(counts[v] >= 0, "mmf_viewstore_store_device: negative view size");
        total += (size_t)counts[v], padded += ((size_t)counts[v] + 31) / 32 * 32;
    }
    MMF_REQUIRE(total == 0 || (descriptor && coordinate), "mmf_viewstore_store_device: null descriptors or coordinates");
    MMF_REQUIRE(((uintptr_t)descriptor & 15u) == 0, "mmf_viewstore_store_device: 16-byte aligned rows");
    MMF_REQUIRE(vs->n_rows + padded < (size_t)1 << 31, "mmf_viewstore_store_device: more than 2^31 rows");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    hipStream_t st = vs->ctx->stream;
    if (padded) {
        int rc = viewstore_reserve(vs, padded);
        if (rc) return rc;
        if (padded / 32 > vs->src0_cap) {  // (every earlier store has been awaited)
            (void)hipFree(vs->src0_dev);
            vs->src0_dev = nullptr, vs->src0_cap = 0;
            MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&vs->src0_dev), padded / 32 * 2 * sizeof(int)));
            vs->src0_cap = padded / 32 * 2;
        }
        if (total * 3 > vs->co_cap) {
            if (vs->co_pin) (void)hipHostFree(vs->co_pin);
            vs->co_pin = nullptr, vs->co_cap = 0;
            MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&vs->co_pin), total * 6 * sizeof(float), hipHostMallocDefault));
            vs->co_cap = total * 6;
        }
    }
    const size_t first_tile = vs->tiles_host.size(), first_view = vs->views.size(), first_point = vs->coords.size() / 3;
    std::vector<int> src0;
    size_t src = 0, dst = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)counts[v];
        vs->views.push_back(RdView{model_id, v, counts[v], vs->n_rows + dst, vs->coords.size() / 3 + src});
        for (size_t r = 0; r < n; r += 32) {
            vs->tiles_host.push_back(mmf::RdTile{(int)vs->views.size() - 1, (int)std::min<size_t>(32, n - r)});
            src0.push_back((int)(src + r));
        }
        src += n, dst += (n + 31) / 32 * 32;
    }
    if (padded) {
        hipError_t e = hipMemcpyAsync(vs->tiles + first_tile, vs->tiles_host.data() + first_tile, padded / 32 * sizeof(mmf::RdTile), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(vs->src0_dev, src0.data(), src0.size() * sizeof(int), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(mmf::rd_scatter_views_kernel, dim3((unsigned)(padded / 32)), dim3(256), 0, st, descriptor,
                               (const mmf::RdTile*)(vs->tiles + first_tile), (const int*)vs->src0_dev, vs->desc + vs->n_rows * kRdDim);
            hipLaunchKernelGGL(mmf::rd_train_norms_kernel, dim3((unsigned)(padded / 32)), dim3(64), 0, st, vs->desc + vs->n_rows * kRdDim,
                               (int)padded, kRdDim, vs->tn + vs->n_rows);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(vs->co_pin, coordinate, total * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // `src0` leaves scope; the coordinates have arrived
        if (e != hipSuccess) {  // nothing of the model stays in the books
            vs->views.resize(first_view), vs->tiles_host.resize(first_tile);
            MMF_HIP_TRY(e);
        }
        vs->coords.insert(vs->coords.end(), vs->co_pin, vs->co_pin + total * 3);
        vs->n_rows += padded;
    }
    int rc = viewstore_device_books(vs, first_point);
    if (rc) return rc;
    if (stored) *stored = 1;
    return MMF_OK;
}

// a model that no longer exists: its views stay where they are (nothing moves) but belong to nobody
extern "C" int mmf_viewstore_forget(mmf_viewstore* vs, int model_id) {
    MMF_REQUIRE(vs != nullptr, "mmf_viewstore_forget: null store");
    bool changed = false;
    for (RdView& v : vs->views)
        if (v.model == model_id) v.model = -1, changed = true;
    if (changed && vs->verifier) {
        MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
        return viewstore_device_books(vs, vs->coords.size() / 3);
    }
    return MMF_OK;
}

// attaches the device verifier (NULL detaches it): views stored before the call are uploaded here.  The batch object belongs
// to the caller and outlives its attachment.
extern "C" int mmf_viewstore_set_verifier(mmf_viewstore* vs, mmf_ransac_batch* b) {
    MMF_REQUIRE(vs != nullptr, "mmf_viewstore_set_verifier: null store");
    MMF_REQUIRE(!b || b->ctx == vs->ctx, "mmf_viewstore_set_verifier: the batch object belongs to another context");
    vs->verifier = b;
    if (!b) return MMF_OK;
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    return viewstore_device_books(vs, 0);
}

extern "C" int mmf_viewstore_num_views(mmf_viewstore* vs) { return vs ? (int)vs->views.size() : -1; }
extern "C" int mmf_viewstore_view(mmf_viewstore* vs, int view, int* model_id, int* index, int* rows) {
    MMF_REQUIRE(vs && view >= 0 && view < (int)vs->views.size(), "mmf_viewstore_view: bad argument");
    if (model_id) *model_id = vs->views[(size_t)view].model;
    if (index) *index = vs->views[(size_t)view].index;
    if (rows) *rows = vs->views[(size_t)view].rows;
    return MMF_OK;
}
// a view's rows back on the HOST, [rows][256] and [rows][3], without the zero rows that pad it to a tile (either destination
// may be NULL).  Synchronous.
extern "C" int mmf_viewstore_download_view(mmf_viewstore* vs, int view, int capacity_rows, float* descriptor, float* coordinate) {
    MMF_REQUIRE(vs && view >= 0 && view < (int)vs->views.size(), "mmf_viewstore_download_view: bad argument");
    const RdView& v = vs->views[(size_t)view];
    MMF_REQUIRE(capacity_rows >= v.rows, "mmf_viewstore_download_view: capacity_rows below the view's rows");
    if (v.rows == 0) return MMF_OK;
    const size_t n = (size_t)v.rows;
    if (coordinate) std::memcpy(coordinate, vs->coords.data() + 3 * v.coord0, n * 3 * sizeof(float));
    if (descriptor) {
        MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
        MMF_HIP_TRY(hipMemcpyAsync(descriptor, vs->desc + v.row0 * kRdDim, n * kRdDim * sizeof(float), hipMemcpyDeviceToHost, vs->ctx->stream));
        MMF_HIP_TRY(hipStreamSynchronize(vs->ctx->stream));
    }
    return MMF_OK;
}
extern "C" int mmf_viewstore_last_launches(mmf_viewstore* vs) { return vs ? vs->last_launches : -1; }

// the three launches of every set, on `st`; results in out_row / out_dist at [view * nq + i] + V * q0 of the set.
// Nothing is enqueued when the store has no rows.  The caller waits for `st` before it reads.
static int viewstore_enqueue(mmf_viewstore* vs, hipStream_t st, const RdSet* sets, int n_sets) {
    vs->last_launches = 0;
    const size_t V = vs->views.size(), R = vs->n_rows;
    size_t total_q = 0;
    for (int s = 0; s < n_sets; ++s) total_q += (size_t)sets[s].nq;
    if (V == 0 || total_q == 0) return MMF_OK;
    const size_t n_out = V * total_q;
    if (n_out > vs->out_cap) {  // (every earlier match has been awaited)
        if (vs->out_row) (void)hipHostFree(vs->out_row);
        if (vs->out_dist) (void)hipHostFree(vs->out_dist);
        vs->out_row = nullptr, vs->out_dist = nullptr, vs->out_cap = 0;
        const size_t cap = n_out + n_out / 2;
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&vs->out_row), cap * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&vs->out_dist), cap * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
        vs->out_cap = cap;
    }
    if (R == 0) {  // views, all of them empty: no query row has a match
        for (size_t e = 0; e < n_out; ++e) vs->out_row[e] = -1, vs->out_dist[e] = 0.f;
        return MMF_OK;
    }
    if (vs->verifier && n_out > vs->rows_cap) {  // (every earlier verification has been awaited)
        (void)hipFree(vs->rows_dev);
        vs->rows_dev = nullptr, vs->rows_cap = 0;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&vs->rows_dev), (n_out + n_out / 2) * sizeof(int)));
        vs->rows_cap = n_out + n_out / 2;
    }
    int* rows_dev = vs->verifier ? vs->rows_dev : nullptr;
    const size_t need = 8 * (n_out + (size_t)n_sets * R) + 4 * total_q;
    if (need > vs->ws_bytes) {
        (void)hipFree(vs->ws);
        vs->ws = nullptr, vs->ws_bytes = 0;
        MMF_HIP_TRY(hipMalloc(&vs->ws, need + need / 2));
        vs->ws_bytes = need + need / 2;
    }
    unsigned long long* row_keys = static_cast<unsigned long long*>(vs->ws);
    unsigned long long* col_keys = row_keys + n_out;
    float* qn_all = reinterpret_cast<float*>(col_keys + (size_t)n_sets * R);
    const unsigned tiles = (unsigned)(R / 32);
    for (int s = 0; s < n_sets; ++s) {
        const int nq = sets[s].nq;
        if (nq == 0) continue;
        const size_t nk = V * (size_t)nq;
        unsigned long long *row_best = row_keys + V * sets[s].q0, *col_best = col_keys + (size_t)s * R;
        float* qn = qn_all + sets[s].q0;
        const unsigned qblocks = (unsigned)((nq + 31) / 32);
        const unsigned rblocks = (unsigned)std::min<size_t>(2048, (nk + R + 255) / 256);
        hipLaunchKernelGGL(mmf::rd_begin_kernel, dim3(qblocks + rblocks), dim3(64), 0, st, sets[s].q, nq, kRdDim, qn, row_best, nk,
                           col_best, R);
        hipLaunchKernelGGL(mmf::rd_tile_kernel, dim3(tiles, qblocks), dim3(64), 0, st, sets[s].q, (const float*)vs->desc,
                           (const float*)qn, (const float*)vs->tn, (const mmf::RdTile*)vs->tiles, nq, kRdDim, row_best, col_best);
        hipLaunchKernelGGL(mmf::rd_cross_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st,
                           (const unsigned long long*)row_best, (const unsigned long long*)col_best, nq, nk,
                           vs->out_row + V * sets[s].q0, vs->out_dist + V * sets[s].q0, rows_dev ? rows_dev + V * sets[s].q0 : (int*)nullptr);
        vs->last_launches += 3;
    }
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// one query set (DEVICE [nq][256], 16-byte aligned) against every view: HOST train_idx / distance [views][nq], the row of
// the view or -1 -- what cv::BFMatcher(NORM_L2, true).match(query, view) returns per view (Model.cpp:836-838).  Synchronous.
extern "C" int mmf_viewstore_match(mmf_viewstore* vs, const float* query, int nq, int* train_idx, float* distance) {
    MMF_REQUIRE(vs && nq >= 0 && (query || nq == 0), "mmf_viewstore_match: bad argument");
    MMF_REQUIRE(((uintptr_t)query & 15u) == 0, "mmf_viewstore_match: 16-byte aligned rows");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    const RdSet set{query, nq, 0};
    int rc = viewstore_enqueue(vs, vs->ctx->stream, &set, 1);
    if (rc) return rc;
    MMF_HIP_TRY(wait_stream(vs->ctx->stream));
    const size_t V = vs->views.size();
    for (size_t v = 0; v < V && nq > 0; ++v)
        for (int i = 0; i < nq; ++i) {
            const size_t e = v * (size_t)nq + (size_t)i;
            const int row = vs->out_row[e];
            if (train_idx) train_idx[e] = row < 0 ? -1 : row - (int)vs->views[v].row0;
            if (distance) distance[e] = row < 0 ? 0.f : vs->out_dist[e];
        }
    return MMF_OK;
}

struct RdBest {
    mmf::Isometry3f transformation;
    float error = std::numeric_limits<float>::infinity();
    int inliers = 0, view = -1, n_matches = 0;
    std::vector<unsigned char> inlier;
    bool found = false;
};

// Model::getBestMatch (:832-873) of `model` from the results of a set that has been matched and awaited: views in ascending
// index, at least 3 matches (:839), ONE RigidRANSAC for the call (:847), estimates without inliers dropped
// (:859), the smallest error wins, the first of equals (:870-873).  coordinate = HOST [nq][3] of the query keypoints.
static RdBest viewstore_best(const mmf_viewstore* vs, int model, const RdSet& set, const float* coordinate,
                             const mmf::RigidRANSAC::Config& cfg) {
    RdBest best;
    mmf::RigidRANSAC ransac(cfg);
    const size_t V = vs->views.size();
    std::vector<float> query, train;
    for (size_t v = 0; v < V; ++v) {
        const RdView& view = vs->views[v];
        if (view.model != model || view.rows == 0) continue;  // (:823-830: time indices without data are skipped)
        const int* rows = vs->out_row + V * set.q0 + v * (size_t)set.nq;
        query.clear(), train.clear();
        for (int i = 0; i < set.nq; ++i) {
            if (rows[i] < 0) continue;
            const float* p = vs->coords.data() + 3 * (view.coord0 + (size_t)rows[i] - view.row0);
            query.insert(query.end(), coordinate + 3 * i, coordinate + 3 * i + 3);
            train.insert(train.end(), p, p + 3);
        }
        const int n = (int)(query.size() / 3);
        if (n < 3) continue;
        mmf::RigidRANSAC::Result est = ransac.estimate(query.data(), train.data(), n);
        int count = 0;
        for (unsigned char b : est.inlier) count += b ? 1 : 0;
        if (count == 0) continue;
        if (!best.found || est.error < best.error) {
            best.found = true;
            best.transformation = est.transformation, best.error = est.error, best.inliers = count;
            best.view = view.index, best.n_matches = n;
            best.inlier.swap(est.inlier);
        }
    }
    return best;
}

static const mmf::RigidRANSAC::Config kRedetectRansac{10, 0.03f, 0.8f};  // MultiMotionFusion.cpp:513

// Model::getBestMatch(keypoints, {10, 0.03, 0.8}) for the model `model_id`: query = DEVICE descriptors [nq][256],
// coordinate = HOST [nq][3].  *found = 0: no view gave an estimate (the reference returns a default Result: identity,
// error +inf).  T = RigidRANSAC::Result::transformation (query ~ T train), *view = the winning view's index in the model,
// *n_matches its matches, inlier (optional, capacity nq) = Result::inlier over the hash-sorted matches.  Synchronous.
extern "C" int mmf_viewstore_best_match(mmf_viewstore* vs, int model_id, const float* query, const float* coordinate, int nq,
                                        float T[16], float* error, int* inliers, int* view, int* n_matches, unsigned char* inlier,
                                        int* found) {
    MMF_REQUIRE(vs && T && error && nq >= 0 && ((query && coordinate) || nq == 0), "mmf_viewstore_best_match: bad argument");
    MMF_REQUIRE(((uintptr_t)query & 15u) == 0, "mmf_viewstore_best_match: 16-byte aligned rows");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    RdBest best;
    if (viewstore_has_model(vs, model_id) && model_id >= 0) {
        const RdSet set{query, nq, 0};
        int rc = viewstore_enqueue(vs, vs->ctx->stream, &set, 1);
        if (rc) return rc;
        MMF_HIP_TRY(wait_stream(vs->ctx->stream));
        if (nq > 0) best = viewstore_best(vs, model_id, set, coordinate, kRedetectRansac);
    }
    isometry_to_4x4(best.transformation, T);
    *error = best.error;
    if (inliers) *inliers = best.inliers;
    if (view) *view = best.view;
    if (n_matches) *n_matches = best.n_matches;
    if (inlier)
        for (int i = 0; i < best.n_matches && i < nq; ++i) inlier[i] = best.inlier[(size_t)i];
    if (found) *found = best.found ? 1 : 0;
    return MMF_OK;
}

// ---- the device verifier (ransac_kernels.hpp) -------------------------------------------------------------
template <class T>
static int viewstore_grow_dev(T** p, size_t* cap, size_t need) {  // (every earlier verification has been awaited)
    if (need <= *cap) return MMF_OK;
    (void)hipFree(*p);
    *p = nullptr, *cap = 0;
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), (need + need / 2) * sizeof(T)));
    *cap = need + need / 2;
    return MMF_OK;
}
template <class T>
static int viewstore_grow_pin(T** p, size_t* cap, size_t need, unsigned flags) {
    if (need <= *cap) return MMF_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr, *cap = 0;
    MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(p), (need + need / 2) * sizeof(T), flags));
    *cap = need + need / 2;
    return MMF_OK;
}

// Behind viewstore_enqueue of the same sets (same order, same q0) on `st`: the verify launch, grid = views x sets, and the
// launch that picks per (set, asked model).  sets[s].coordinate = DEVICE; every nq <= the verifier's max_points (a larger
// set's blocks return at once and its records say "not found").  Records: rec_pin[s * n_asked + a], the winner's inlier
// flags at rec_inlier_pin[(s * n_asked + a) * rec_stride].  Needs views with rows (viewstore_enqueue launched something).
static int viewstore_enqueue_verify(mmf_viewstore* vs, hipStream_t st, const mmf::RdVerifySet* sets, int n_sets, const int* asked, int n_asked) {
    const size_t V = vs->views.size();
    int stride = 1;
    for (int s = 0; s < n_sets; ++s) stride = std::max(stride, sets[s].nq);
    const size_t pairs = (size_t)n_sets * V, recs = (size_t)n_sets * (size_t)n_asked;
    const size_t arg_bytes = (size_t)n_sets * sizeof(mmf::RdVerifySet) + (size_t)n_asked * sizeof(int);
    int rc = viewstore_grow_dev(&vs->per_view, &vs->per_view_cap, pairs);
    if (!rc) rc = viewstore_grow_dev(&vs->per_view_inlier, &vs->per_view_inlier_cap, pairs * (size_t)stride);
    if (rc) return rc;
    if (arg_bytes > vs->arg_cap) {
        (void)hipFree(vs->arg_dev);
        if (vs->arg_pin) (void)hipHostFree(vs->arg_pin);
        vs->arg_dev = vs->arg_pin = nullptr, vs->arg_cap = 0;
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&vs->arg_pin), arg_bytes * 2, hipHostMallocDefault));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&vs->arg_dev), arg_bytes * 2));
        vs->arg_cap = arg_bytes * 2;
    }
    if (!rc) rc = viewstore_grow_pin(&vs->rec_pin, &vs->rec_cap, recs, hipHostMallocMapped | hipHostMallocCoherent);
    if (!rc) rc = viewstore_grow_pin(&vs->rec_inlier_pin, &vs->rec_inlier_cap, recs * (size_t)stride, hipHostMallocMapped | hipHostMallocCoherent);
    if (rc) return rc;
    std::memcpy(vs->arg_pin, sets, (size_t)n_sets * sizeof(mmf::RdVerifySet));
    std::memcpy(vs->arg_pin + (size_t)n_sets * sizeof(mmf::RdVerifySet), asked, (size_t)n_asked * sizeof(int));
    MMF_HIP_TRY(hipMemcpyAsync(vs->arg_dev, vs->arg_pin, arg_bytes, hipMemcpyHostToDevice, st));
    const mmf::RdVerifySet* sets_dev = reinterpret_cast<const mmf::RdVerifySet*>(vs->arg_dev);
    const int* asked_dev = reinterpret_cast<const int*>(vs->arg_dev + (size_t)n_sets * sizeof(mmf::RdVerifySet));
    const mmf::RansacDeviceConfig dc = vs->verifier->device_config();
    hipLaunchKernelGGL(mmf::rd_verify_kernel, dim3((unsigned)V, (unsigned)n_sets), dim3(64), mmf::ransac_lds_bytes(dc.cap, true), st,
                       (const mmf::RdViewDev*)vs->views_dev, (int)V, sets_dev, asked_dev, n_asked, (const int*)vs->rows_dev,
                       (const float*)vs->coords_dev, dc, vs->per_view, vs->per_view_inlier, stride);
    hipLaunchKernelGGL(mmf::rd_pick_kernel, dim3((unsigned)n_asked, (unsigned)n_sets), dim3(64), 0, st, (const mmf::RdViewDev*)vs->views_dev,
                       (int)V, asked_dev, n_asked, (const mmf::RdViewResult*)vs->per_view, (const unsigned char*)vs->per_view_inlier, stride,
                       vs->rec_pin, vs->rec_inlier_pin);
    MMF_HIP_TRY(hipGetLastError());
    vs->last_launches += 2;
    vs->rec_stride = stride, vs->rec_asked = n_asked;
    return MMF_OK;
}

// mmf_viewstore_best_match with the geometric verification on the device, under the per-view rule (a fresh RigidRANSAC per
// view): query = DEVICE [nq][256], coordinate = DEVICE [nq][3], nq <= the verifier's max_points.  The three
// match launches and two more whatever the store holds, one record through pinned memory, one wait.
extern "C" int mmf_viewstore_best_match_device(mmf_viewstore* vs, int model_id, const float* query, const float* coordinate, int nq,
                                               float T[16], float* error, int* inliers, int* view, int* n_matches,
                                               unsigned char* inlier, int* found) {
    MMF_REQUIRE(vs && T && error && nq >= 0 && ((query && coordinate) || nq == 0), "mmf_viewstore_best_match_device: bad argument");
    MMF_REQUIRE(((uintptr_t)query & 15u) == 0, "mmf_viewstore_best_match_device: 16-byte aligned rows");
    if (!vs->verifier) return fail(MMF_ERR_STATE, "mmf_viewstore_best_match_device: no verifier attached (mmf_viewstore_set_verifier)");
    MMF_REQUIRE(nq <= vs->verifier->max_points, "mmf_viewstore_best_match_device: more query rows than the verifier's max_points");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    mmf::RdRecord rec;
    std::memset(&rec, 0, sizeof(rec));
    for (int k = 0; k < 16; k += 5) rec.T[k] = 1.f;
    rec.error = std::numeric_limits<float>::infinity(), rec.view = -1;
    vs->last_launches = 0;
    if (viewstore_has_model(vs, model_id) && model_id >= 0 && nq > 0) {
        const RdSet set{query, nq, 0};
        int rc = viewstore_enqueue(vs, vs->ctx->stream, &set, 1);
        if (rc) return rc;
        if (vs->last_launches) {  // (a store of empty views: nothing was launched, nothing can match)
            const mmf::RdVerifySet vset{coordinate, nq, 0};
            rc = viewstore_enqueue_verify(vs, vs->ctx->stream, &vset, 1, &model_id, 1);
            if (rc) return rc;
            MMF_HIP_TRY(wait_stream(vs->ctx->stream));
            rec = vs->rec_pin[0];
            if (inlier && rec.found)
                for (int i = 0; i < rec.n_matches && i < nq; ++i) inlier[i] = vs->rec_inlier_pin[i];
        }
    }
    std::memcpy(T, rec.T, sizeof(rec.T));
    *error = rec.error;
    if (inliers) *inliers = rec.inliers;
    if (view) *view = rec.view;
    if (n_matches) *n_matches = rec.n_matches;
    if (found) *found = rec.found;
    return MMF_OK;
}

// Model::getBestMatch of `model` on the HOST under the per-view rule: what the device verifier computes, for a set that
// does not fit it (more rows than max_points).  From the results of a set that has been matched and awaited.
static RdBest viewstore_best_fresh(const mmf_viewstore* vs, int model, const RdSet& set, const float* coordinate,
                                   const mmf::RigidRANSAC::Config& cfg) {
    RdBest best;
    const size_t V = vs->views.size();
    std::vector<float> query, train;
    std::vector<unsigned short> triples(3 * (size_t)cfg.iterations);
    for (size_t v = 0; v < V; ++v) {
        const RdView& view = vs->views[v];
        if (view.model != model || view.rows == 0) continue;
        const int* rows = vs->out_row + V * set.q0 + v * (size_t)set.nq;
        query.clear(), train.clear();
        for (int i = 0; i < set.nq; ++i) {
            if (rows[i] < 0) continue;
            const float* p = vs->coords.data() + 3 * (view.coord0 + (size_t)rows[i] - view.row0);
            query.insert(query.end(), coordinate + 3 * i, coordinate + 3 * i + 3);
            train.insert(train.end(), p, p + 3);
        }
        const int n = (int)(query.size() / 3);
        if (n < 3 || n > 65535) continue;
        mmf::ransac_triples(cfg.iterations, n, triples.data());
        mmf::Isometry3f T;
        float error;
        std::vector<unsigned char> inl((size_t)n);
        const int count = mmf::ransac_core_host(cfg, triples.data(), query.data(), train.data(), n, &T, &error, inl.data());
        if (count == 0) continue;
        if (!best.found || error < best.error) {
            best.found = true;
            best.transformation = T, best.error = error, best.inliers = count;
            best.view = view.index, best.n_matches = n;
            best.inlier.swap(inl);
        }
    }
    return best;
}

// pinned + device staging for `rows` query rows handed in on the host (every earlier match has been awaited)
static int viewstore_stage(mmf_viewstore* vs, size_t rows) {
    if (rows <= vs->q_cap) return MMF_OK;
    if (vs->q_pin) (void)hipHostFree(vs->q_pin);
    (void)hipFree(vs->q_dev);
    vs->q_pin = nullptr, vs->q_dev = nullptr, vs->q_cap = 0;
    const size_t cap = rows + rows / 2 + 64;
    MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&vs->q_pin), cap * kRdDim * sizeof(float), hipHostMallocDefault));
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&vs->q_dev), cap * kRdDim * sizeof(float)));
    vs->q_cap = cap;
    return MMF_OK;
}
