// redetect_host.hpp -- the view store and Model::getBestMatch (Core/Model/Model.cpp:781-874) on top of
// redetect_kernels.hpp.  Textually included by mmf_hip.hip behind stream_lane.hpp (it uses that file's owners, mmf_hip.hip's
// helpers and rigid_ransac.hpp).
//
// A view = the valid keypoints of one time index of a model's stored local tracks (tracks_local: the result of
// computeTrackProjectionFirstFrame, Model.cpp:508-522, null and non-finite keypoints dropped, :806-811): n descriptors of
// 256 floats on the device, n coordinates in the model's frame on the host (RigidRANSAC is host code).  All views of all
// models share one descriptor buffer, each padded with zero rows to a multiple of 32; the per-tile table says which view
// a 32-row tile belongs to and how many of its rows are real.
//
// Memory: every buffer lives in an owner (DeviceBuf / PinnedBuf), so destroying the store is `delete`, and is reached
// through one of three helpers.  RdStoreBuf, the store's own buffers: they double, the old contents are copied on the
// context's stream and the old buffer is NOT freed until the store is destroyed (`retired`) -- work already enqueued keeps
// reading memory that stays valid, and no device memory is released (a device-wide synchronisation) between frames; the
// doubling bounds what is retired by the size of the live buffers.  RdScratch, everything else: released and allocated
// anew, half as large again as asked, when it is too small.  RdStaged: pinned and device scratch of one size with the copy
// between.
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

// ---- the three shapes of the store's memory ----------------------------------------------------------------------------------
constexpr unsigned kRdOnDevice = ~0u;  // RdScratch's `Where`: device memory; any other value = pinned, hipHostMalloc's flags
constexpr unsigned kRdDeviceWrites = hipHostMallocMapped | hipHostMallocCoherent;  // pinned memory the device writes
constexpr unsigned kRdForCopies = hipHostMallocDefault;                           // pinned memory a copy reads or writes

// Memory that only the store's own calls touch.  Every earlier store, match and verification has been awaited by the host
// before its call returned, so nothing enqueued reads the buffer when it is released.
template <class T, unsigned Where = kRdOnDevice>
struct RdScratch {
    std::conditional_t<Where == kRdOnDevice, DeviceBuf<T>, PinnedBuf<T>> buf;
    size_t cap = 0;  // elements
    hipError_t reserve(size_t need) {
        if (need <= cap) return hipSuccess;
        buf.reset(), cap = 0;
        const size_t fresh = need + need / 2;
        hipError_t e;
        if constexpr (Where == kRdOnDevice) e = buf.create(fresh);
        else e = buf.create(fresh, Where);
        if (e == hipSuccess) cap = fresh;
        return e;
    }
    T* get() const { return buf.get(); }
};

// what the host hands to the device: filled at pin.get(), read by the kernels at dev.get()
template <class T>
struct RdStaged {
    RdScratch<T, kRdForCopies> pin;
    RdScratch<T> dev;
    hipError_t reserve(size_t need) {
        const hipError_t e = pin.reserve(need);
        return e != hipSuccess ? e : dev.reserve(need);
    }
    hipError_t upload(size_t count, hipStream_t st) const {
        return hipMemcpyAsync(dev.get(), pin.get(), count * sizeof(T), hipMemcpyHostToDevice, st);
    }
};

using RdRetired = std::vector<DeviceMem>;  // (enqueued work may still read them: freed with the store)

// A buffer of the store itself, which enqueued work may read: `fresh` allocates the larger one and copies the first `keep`
// elements on the stream, `adopt` makes it the live one and retires the old one; `grow` is the two for a buffer that grows
// alone.
template <class T>
struct RdStoreBuf {
    DeviceBuf<T> buf;
    size_t cap = 0;  // elements
    hipError_t fresh(size_t new_cap, size_t keep, hipStream_t st, DeviceBuf<T>* out) const {
        const hipError_t e = out->create(new_cap);
        if (e != hipSuccess || !buf || !keep) return e;
        return hipMemcpyAsync(out->get(), buf.get(), keep * sizeof(T), hipMemcpyDeviceToDevice, st);
    }
    void adopt(DeviceBuf<T>&& f, size_t new_cap, RdRetired& retired) {
        if (buf) retired.push_back(std::move(buf));
        buf = std::move(f), cap = new_cap;
    }
    hipError_t grow(size_t new_cap, size_t keep, hipStream_t st, RdRetired& retired) {
        DeviceBuf<T> f;
        const hipError_t e = fresh(new_cap, keep, st, &f);
        if (e == hipSuccess) adopt(std::move(f), new_cap, retired);
        return e;
    }
    T* get() const { return buf.get(); }
};

// the doubling of the store's own buffers: from `first` elements on, until `need` fit
static size_t viewstore_doubled(size_t cap, size_t first, size_t need) {
    cap = cap ? cap * 2 : first;
    while (cap < need) cap *= 2;
    return cap;
}

// ---- the store's state, by the calls that own it ----------------------------------------------------------------------------
struct RdBooks {  // what is stored: appended to by the store calls, disowned by forget; every other call reads it
    std::vector<RdView> views;  // store order = model by model as stored, a model's views ascending
    std::vector<float> coords;
    std::vector<mmf::RdTile> tiles_host;
    RdStoreBuf<float> desc, tn;
    RdStoreBuf<mmf::RdTile> tiles;
    size_t cap_rows = 0, n_rows = 0;  // rows = 32 * tiles
    RdRetired retired;
};
struct RdMatchScratch {  // viewstore_enqueue writes it; lives until the call that enqueued has waited and read its results
    RdScratch<unsigned char> ws;  // qn | row_best | col_best
    RdScratch<int, kRdDeviceWrites> out_row;  // [view][query row] store row or -1
    RdScratch<float, kRdDeviceWrites> out_dist;
    int last_launches = 0;
};
struct RdQueryStaging {  // viewstore_stage .. the wait behind the match: queries handed in on the host (the fusion's keypoints)
    RdStaged<float> q, qc;  // descriptors [rows][256], coordinates [rows][3]
};
struct RdDeviceStoreStaging {  // inside one mmf_viewstore_store_device
    RdScratch<int> src0;                 // per tile its first packed row
    RdScratch<float, kRdForCopies> co;  // the coordinates on their way to `coords`
};
// mmf_viewstore_set_verifier attaches it; nothing here is allocated, written or launched without one.  The books again on
// the device (viewstore_device_books), then per verification (viewstore_enqueue_verify .. the wait and the reading of the
// records) the match rows, the per-view estimates and the records the host reads.
struct RdVerifier {
    mmf_ransac_batch* verifier = nullptr;
    RdStoreBuf<float> coords_dev;  // `coords`
    RdStoreBuf<mmf::RdViewDev> views_dev;
    RdScratch<int> rows_dev;  // rd_cross_kernel's rows, laid out as out_row
    RdScratch<mmf::RdViewResult> per_view;
    RdScratch<unsigned char> per_view_inlier;
    RdStaged<unsigned char> arg;  // the sets and the asked models on their way to the device
    RdScratch<mmf::RdRecord, kRdDeviceWrites> rec;  // [set][asked model]
    RdScratch<unsigned char, kRdDeviceWrites> rec_inlier;
    int rec_stride = 0, rec_asked = 0;  // layout of the last verification's records
};

struct mmf_viewstore {
    mmf_ctx* ctx = nullptr;
    RdBooks books;
    RdMatchScratch match;
    RdQueryStaging query;
    RdDeviceStoreStaging dstore;
    RdVerifier ver;
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
    delete vs;
}

static bool viewstore_has_model(const mmf_viewstore* vs, int model) {
    for (const RdView& v : vs->books.views)
        if (v.model == model) return true;
    return false;
}

// room for `rows` more rows (a multiple of 32): new buffers of twice the size, the old contents copied on the stream.
// All three exist before one is adopted: a failure leaves the store as it was and frees the fresh ones.
static int viewstore_reserve(mmf_viewstore* vs, size_t rows) {
    RdBooks& b = vs->books;
    if (b.n_rows + rows <= b.cap_rows) return MMF_OK;
    const size_t cap = viewstore_doubled(b.cap_rows, 4096, b.n_rows + rows);
    hipStream_t st = vs->ctx->stream;
    DeviceBuf<float> desc, tn;
    DeviceBuf<mmf::RdTile> tiles;
    MMF_HIP_TRY(b.desc.fresh(cap * kRdDim, b.n_rows * kRdDim, st, &desc));
    MMF_HIP_TRY(b.tn.fresh(cap, b.n_rows, st, &tn));
    MMF_HIP_TRY(b.tiles.fresh(cap / 32, b.n_rows / 32, st, &tiles));
    b.desc.adopt(std::move(desc), cap * kRdDim, b.retired);
    b.tn.adopt(std::move(tn), cap, b.retired);
    b.tiles.adopt(std::move(tiles), cap / 32, b.retired);
    b.cap_rows = cap;
    return MMF_OK;
}

// With a verifier attached the store keeps its coordinates and its view table on the device as well: the points from
// `first_point` on are uploaded (growth copies the earlier ones like the descriptors and retires the old buffer), the view
// table -- small -- whole.  Waits for the stream: the sources are pageable.  Without a verifier: nothing.
static int viewstore_device_books(mmf_viewstore* vs, size_t first_point) {
    RdVerifier& d = vs->ver;
    if (!d.verifier) return MMF_OK;
    const RdBooks& b = vs->books;
    hipStream_t st = vs->ctx->stream;
    const size_t P = b.coords.size() / 3, V = b.views.size();
    if (3 * P > d.coords_dev.cap)
        MMF_HIP_TRY(d.coords_dev.grow(3 * viewstore_doubled(d.coords_dev.cap / 3, 4096, P), 3 * first_point, st, vs->books.retired));
    if (P > first_point)
        MMF_HIP_TRY(hipMemcpyAsync(d.coords_dev.get() + 3 * first_point, b.coords.data() + 3 * first_point, (P - first_point) * 3 * sizeof(float),
                                   hipMemcpyHostToDevice, st));
    if (V > d.views_dev.cap) MMF_HIP_TRY(d.views_dev.grow(viewstore_doubled(d.views_dev.cap, 256, V), 0, st, vs->books.retired));
    std::vector<mmf::RdViewDev> table(V);
    for (size_t v = 0; v < V; ++v)
        table[v] = mmf::RdViewDev{b.views[v].model, b.views[v].index, b.views[v].rows, (int)b.views[v].row0, (int)b.views[v].coord0};
    if (V) MMF_HIP_TRY(hipMemcpyAsync(d.views_dev.get(), table.data(), V * sizeof(mmf::RdViewDev), hipMemcpyHostToDevice, st));
    MMF_HIP_TRY(hipStreamSynchronize(st));
    return MMF_OK;
}

struct RdStoreCall {  // what the shared part of a store call tells the entry point's upload
    size_t total = 0, padded = 0;  // the model's rows: as handed in, and with every view padded to a multiple of 32
    size_t first_tile = 0;         // the model's first tile in tiles_host / tiles
    std::vector<int> src0;         // per tile of the model its first row in the rows handed in
};

// Model::store (Model.cpp:1617-1632), the part that does not depend on where the rows are: `who` = the entry point, for the
// messages.  The views and tiles enter the books, `upload(call, &coords)` brings the padded rows, the tiles and the norms to
// the device at row n_rows, waits for the stream, and says where on the HOST the total x 3 coordinates are.  If it fails,
// nothing of the model stays in the books; if not, the coordinates and the rows are committed.
template <class Upload>
static int viewstore_store_model(mmf_viewstore* vs, const std::string& who, int model_id, int n_views, const int* counts,
                                 const float* descriptor, const float* coordinate, int* stored, Upload upload) {
    MMF_REQUIRE(vs && n_views >= 0 && (counts || n_views == 0), who + ": bad argument");
    if (stored) *stored = 0;
    if (viewstore_has_model(vs, model_id)) return MMF_OK;
    RdBooks& b = vs->books;
    RdStoreCall call;
    for (int v = 0; v < n_views; ++v) {
        MMF_REQUIRE(counts[v] >= 0, who + ": negative view size");
        call.total += (size_t)counts[v], call.padded += ((size_t)counts[v] + 31) / 32 * 32;
    }
    MMF_REQUIRE(call.total == 0 || (descriptor && coordinate), who + ": null descriptors or coordinates");
    MMF_REQUIRE(b.n_rows + call.padded < (size_t)1 << 31, who + ": more than 2^31 rows");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    if (call.padded) {
        int rc = viewstore_reserve(vs, call.padded);
        if (rc) return rc;
    }
    const size_t first_view = b.views.size(), first_point = b.coords.size() / 3;
    call.first_tile = b.tiles_host.size();
    size_t src = 0, dst = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)counts[v];
        b.views.push_back(RdView{model_id, v, counts[v], b.n_rows + dst, first_point + src});
        for (size_t r = 0; r < n; r += 32) {
            b.tiles_host.push_back(mmf::RdTile{(int)b.views.size() - 1, (int)std::min<size_t>(32, n - r)});
            call.src0.push_back((int)(src + r));
        }
        src += n, dst += (n + 31) / 32 * 32;
    }
    const float* coords = nullptr;
    int rc = upload(call, &coords);
    if (rc) {  // nothing of the model stays in the books
        b.views.resize(first_view), b.tiles_host.resize(call.first_tile);
        return rc;
    }
    if (call.total) b.coords.insert(b.coords.end(), coords, coords + call.total * 3);
    b.n_rows += call.padded;
    rc = viewstore_device_books(vs, first_point);
    if (rc) return rc;
    if (stored) *stored = 1;
    return MMF_OK;
}

// Model::store (Model.cpp:1617-1632): the views of one model.  counts[n_views] valid keypoints per view (0 allowed);
// descriptor / coordinate = the views' rows one after the other.  *stored = 0: the model has stored views already and
// this call changed nothing (:1618-1621).
extern "C" int mmf_viewstore_store(mmf_viewstore* vs, int model_id, int n_views, const int* counts, const float* descriptor,
                                   const float* coordinate, int* stored) {
    return viewstore_store_model(vs, "mmf_viewstore_store", model_id, n_views, counts, descriptor, coordinate, stored,
                                 [&](const RdStoreCall& c, const float** coords) -> int {
        *coords = coordinate;
        if (!c.padded) return MMF_OK;
        const RdBooks& b = vs->books;
        hipStream_t st = vs->ctx->stream;
        std::vector<float> block(c.padded * kRdDim, 0.f);  // the views' rows with their zero padding
        for (size_t t = 0; t < c.src0.size(); ++t)
            std::memcpy(block.data() + t * 32 * kRdDim, descriptor + (size_t)c.src0[t] * kRdDim,
                        (size_t)b.tiles_host[c.first_tile + t].valid * kRdDim * sizeof(float));
        float* desc = b.desc.get() + b.n_rows * kRdDim;
        MMF_HIP_TRY(hipMemcpyAsync(desc, block.data(), c.padded * kRdDim * sizeof(float), hipMemcpyHostToDevice, st));
        MMF_HIP_TRY(hipMemcpyAsync(b.tiles.get() + c.first_tile, b.tiles_host.data() + c.first_tile, c.padded / 32 * sizeof(mmf::RdTile),
                                   hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mmf::rd_train_norms_kernel, dim3((unsigned)(c.padded / 32)), dim3(64), 0, st, desc, (int)c.padded, kRdDim,
                           b.tn.get() + b.n_rows);
        MMF_HIP_TRY(hipGetLastError());
        MMF_HIP_TRY(hipStreamSynchronize(st));  // `block` leaves scope
        return MMF_OK;
    });
}

// mmf_viewstore_store with the views' rows on the DEVICE (mmf_tracker_model_views): counts = HOST, descriptor / coordinate =
// DEVICE, packed.  A kernel scatters the rows to their 32-row-padded places and writes the padding; tiles and norms as above;
// the coordinates reach `coords` through pinned memory.  One wait at the end.  The store is then what mmf_viewstore_store
// leaves with the same views downloaded.
extern "C" int mmf_viewstore_store_device(mmf_viewstore* vs, int model_id, int n_views, const int* counts, const float* descriptor,
                                          const float* coordinate, int* stored) {
    return viewstore_store_model(vs, "mmf_viewstore_store_device", model_id, n_views, counts, descriptor, coordinate, stored,
                                 [&](const RdStoreCall& c, const float** coords) -> int {
        MMF_REQUIRE(((uintptr_t)descriptor & 15u) == 0, "mmf_viewstore_store_device: 16-byte aligned rows");
        if (!c.padded) return MMF_OK;
        const RdBooks& b = vs->books;
        RdDeviceStoreStaging& s = vs->dstore;
        hipStream_t st = vs->ctx->stream;
        MMF_HIP_TRY(s.src0.reserve(c.padded / 32));
        MMF_HIP_TRY(s.co.reserve(c.total * 3));
        float* desc = b.desc.get() + b.n_rows * kRdDim;
        MMF_HIP_TRY(hipMemcpyAsync(b.tiles.get() + c.first_tile, b.tiles_host.data() + c.first_tile, c.padded / 32 * sizeof(mmf::RdTile),
                                   hipMemcpyHostToDevice, st));
        MMF_HIP_TRY(hipMemcpyAsync(s.src0.get(), c.src0.data(), c.src0.size() * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mmf::rd_scatter_views_kernel, dim3((unsigned)(c.padded / 32)), dim3(256), 0, st, descriptor,
                           (const mmf::RdTile*)(b.tiles.get() + c.first_tile), (const int*)s.src0.get(), desc);
        hipLaunchKernelGGL(mmf::rd_train_norms_kernel, dim3((unsigned)(c.padded / 32)), dim3(64), 0, st, desc, (int)c.padded, kRdDim,
                           b.tn.get() + b.n_rows);
        MMF_HIP_TRY(hipGetLastError());
        MMF_HIP_TRY(hipMemcpyAsync(s.co.get(), coordinate, c.total * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
        MMF_HIP_TRY(hipStreamSynchronize(st));  // `c.src0` may go; the coordinates have arrived
        *coords = s.co.get();
        return MMF_OK;
    });
}

// a model that no longer exists: its views stay where they are (nothing moves) but belong to nobody
extern "C" int mmf_viewstore_forget(mmf_viewstore* vs, int model_id) {
    MMF_REQUIRE(vs != nullptr, "mmf_viewstore_forget: null store");
    bool changed = false;
    for (RdView& v : vs->books.views)
        if (v.model == model_id) v.model = -1, changed = true;
    if (changed && vs->ver.verifier) {
        MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
        return viewstore_device_books(vs, vs->books.coords.size() / 3);
    }
    return MMF_OK;
}

// attaches the device verifier (NULL detaches it): views stored before the call are uploaded here.  The batch object belongs
// to the caller and outlives its attachment.
extern "C" int mmf_viewstore_set_verifier(mmf_viewstore* vs, mmf_ransac_batch* b) {
    MMF_REQUIRE(vs != nullptr, "mmf_viewstore_set_verifier: null store");
    MMF_REQUIRE(!b || b->ctx == vs->ctx, "mmf_viewstore_set_verifier: the batch object belongs to another context");
    vs->ver.verifier = b;
    if (!b) return MMF_OK;
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    return viewstore_device_books(vs, 0);
}

extern "C" int mmf_viewstore_num_views(mmf_viewstore* vs) { return vs ? (int)vs->books.views.size() : -1; }
extern "C" int mmf_viewstore_view(mmf_viewstore* vs, int view, int* model_id, int* index, int* rows) {
    MMF_REQUIRE(vs && view >= 0 && view < (int)vs->books.views.size(), "mmf_viewstore_view: bad argument");
    const RdView& v = vs->books.views[(size_t)view];
    if (model_id) *model_id = v.model;
    if (index) *index = v.index;
    if (rows) *rows = v.rows;
    return MMF_OK;
}
// a view's rows back on the HOST, [rows][256] and [rows][3], without the zero rows that pad it to a tile (either destination
// may be NULL).  Synchronous.
extern "C" int mmf_viewstore_download_view(mmf_viewstore* vs, int view, int capacity_rows, float* descriptor, float* coordinate) {
    MMF_REQUIRE(vs && view >= 0 && view < (int)vs->books.views.size(), "mmf_viewstore_download_view: bad argument");
    const RdView& v = vs->books.views[(size_t)view];
    MMF_REQUIRE(capacity_rows >= v.rows, "mmf_viewstore_download_view: capacity_rows below the view's rows");
    if (v.rows == 0) return MMF_OK;
    const size_t n = (size_t)v.rows;
    if (coordinate) std::memcpy(coordinate, vs->books.coords.data() + 3 * v.coord0, n * 3 * sizeof(float));
    if (descriptor) {
        MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
        MMF_HIP_TRY(hipMemcpyAsync(descriptor, vs->books.desc.get() + v.row0 * kRdDim, n * kRdDim * sizeof(float), hipMemcpyDeviceToHost,
                                   vs->ctx->stream));
        MMF_HIP_TRY(hipStreamSynchronize(vs->ctx->stream));
    }
    return MMF_OK;
}
extern "C" int mmf_viewstore_last_launches(mmf_viewstore* vs) { return vs ? vs->match.last_launches : -1; }

// the three launches of every set, on `st`; results in out_row / out_dist at [view * nq + i] + V * q0 of the set.
// Nothing is enqueued when the store has no rows.  The caller waits for `st` before it reads.
static int viewstore_enqueue(mmf_viewstore* vs, hipStream_t st, const RdSet* sets, int n_sets) {
    const RdBooks& b = vs->books;
    RdMatchScratch& m = vs->match;
    m.last_launches = 0;
    const size_t V = b.views.size(), R = b.n_rows;
    size_t total_q = 0;
    for (int s = 0; s < n_sets; ++s) total_q += (size_t)sets[s].nq;
    if (V == 0 || total_q == 0) return MMF_OK;
    const size_t n_out = V * total_q;
    MMF_HIP_TRY(m.out_row.reserve(n_out));
    MMF_HIP_TRY(m.out_dist.reserve(n_out));
    if (R == 0) {  // views, all of them empty: no query row has a match
        for (size_t e = 0; e < n_out; ++e) m.out_row.get()[e] = -1, m.out_dist.get()[e] = 0.f;
        return MMF_OK;
    }
    if (vs->ver.verifier) MMF_HIP_TRY(vs->ver.rows_dev.reserve(n_out));
    int* rows_dev = vs->ver.verifier ? vs->ver.rows_dev.get() : nullptr;
    MMF_HIP_TRY(m.ws.reserve(8 * (n_out + (size_t)n_sets * R) + 4 * total_q));
    unsigned long long* row_keys = reinterpret_cast<unsigned long long*>(m.ws.get());
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
        hipLaunchKernelGGL(mmf::rd_tile_kernel, dim3(tiles, qblocks), dim3(64), 0, st, sets[s].q, (const float*)b.desc.get(),
                           (const float*)qn, (const float*)b.tn.get(), (const mmf::RdTile*)b.tiles.get(), nq, kRdDim, row_best, col_best);
        hipLaunchKernelGGL(mmf::rd_cross_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st,
                           (const unsigned long long*)row_best, (const unsigned long long*)col_best, nq, nk,
                           m.out_row.get() + V * sets[s].q0, m.out_dist.get() + V * sets[s].q0,
                           rows_dev ? rows_dev + V * sets[s].q0 : (int*)nullptr);
        m.last_launches += 3;
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
    const size_t V = vs->books.views.size();
    for (size_t v = 0; v < V && nq > 0; ++v)
        for (int i = 0; i < nq; ++i) {
            const size_t e = v * (size_t)nq + (size_t)i;
            const int row = vs->match.out_row.get()[e];
            if (train_idx) train_idx[e] = row < 0 ? -1 : row - (int)vs->books.views[v].row0;
            if (distance) distance[e] = row < 0 ? 0.f : vs->match.out_dist.get()[e];
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

// Model::getBestMatch (:832-873) of `model` from the results of a set that has been matched and awaited: the model's views in
// store order, i.e. ascending index (:823-830: time indices without data are skipped), at least 3 matches
// (:839), estimates without inliers dropped (:859), the smallest error wins, the first of equals (:870-873).
// coordinate = HOST [nq][3] of the query keypoints.  estimate(query, train, n, &est) fills transformation, error, inliers and
// inlier of `est` from n >= 3 pairs, or returns false: it does not take the view.
template <class Estimate>
static RdBest viewstore_best_of_views(const mmf_viewstore* vs, int model, const RdSet& set, const float* coordinate, Estimate estimate) {
    RdBest best;
    const RdBooks& b = vs->books;
    const size_t V = b.views.size();
    std::vector<float> query, train;
    for (size_t v = 0; v < V; ++v) {
        const RdView& view = b.views[v];
        if (view.model != model || view.rows == 0) continue;
        const int* rows = vs->match.out_row.get() + V * set.q0 + v * (size_t)set.nq;
        query.clear(), train.clear();
        for (int i = 0; i < set.nq; ++i) {
            if (rows[i] < 0) continue;
            const float* p = b.coords.data() + 3 * (view.coord0 + (size_t)rows[i] - view.row0);
            query.insert(query.end(), coordinate + 3 * i, coordinate + 3 * i + 3);
            train.insert(train.end(), p, p + 3);
        }
        const int n = (int)(query.size() / 3);
        if (n < 3) continue;
        RdBest est;
        if (!estimate(query.data(), train.data(), n, &est) || est.inliers == 0) continue;
        if (!best.found || est.error < best.error) {
            est.found = true, est.view = view.index, est.n_matches = n;
            best = std::move(est);
        }
    }
    return best;
}

// the reference's rule: ONE RigidRANSAC for the call, its state carries from view to view (:847)
static RdBest viewstore_best(const mmf_viewstore* vs, int model, const RdSet& set, const float* coordinate,
                             const mmf::RigidRANSAC::Config& cfg) {
    mmf::RigidRANSAC ransac(cfg);
    return viewstore_best_of_views(vs, model, set, coordinate, [&](const float* query, const float* train, int n, RdBest* est) {
        mmf::RigidRANSAC::Result r = ransac.estimate(query, train, n);
        est->transformation = r.transformation, est->error = r.error;
        for (unsigned char flag : r.inlier) est->inliers += flag ? 1 : 0;
        est->inlier.swap(r.inlier);
        return true;
    });
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
// Behind viewstore_enqueue of the same sets (same order, same q0) on `st`: the verify launch, grid = views x sets, and the
// launch that picks per (set, asked model).  sets[s].coordinate = DEVICE; every nq <= the verifier's max_points (a larger
// set's blocks return at once and its records say "not found").  Records: rec[s * n_asked + a], the winner's inlier
// flags at rec_inlier[(s * n_asked + a) * rec_stride].  Needs views with rows (viewstore_enqueue launched something).
static int viewstore_enqueue_verify(mmf_viewstore* vs, hipStream_t st, const mmf::RdVerifySet* sets, int n_sets, const int* asked, int n_asked) {
    RdVerifier& d = vs->ver;
    const size_t V = vs->books.views.size();
    int stride = 1;
    for (int s = 0; s < n_sets; ++s) stride = std::max(stride, sets[s].nq);
    const size_t pairs = (size_t)n_sets * V, recs = (size_t)n_sets * (size_t)n_asked;
    const size_t set_bytes = (size_t)n_sets * sizeof(mmf::RdVerifySet), arg_bytes = set_bytes + (size_t)n_asked * sizeof(int);
    MMF_HIP_TRY(d.per_view.reserve(pairs));
    MMF_HIP_TRY(d.per_view_inlier.reserve(pairs * (size_t)stride));
    MMF_HIP_TRY(d.arg.reserve(arg_bytes));
    MMF_HIP_TRY(d.rec.reserve(recs));
    MMF_HIP_TRY(d.rec_inlier.reserve(recs * (size_t)stride));
    std::memcpy(d.arg.pin.get(), sets, set_bytes);
    std::memcpy(d.arg.pin.get() + set_bytes, asked, (size_t)n_asked * sizeof(int));
    MMF_HIP_TRY(d.arg.upload(arg_bytes, st));
    const mmf::RdVerifySet* sets_dev = reinterpret_cast<const mmf::RdVerifySet*>(d.arg.dev.get());
    const int* asked_dev = reinterpret_cast<const int*>(d.arg.dev.get() + set_bytes);
    const mmf::RansacDeviceConfig dc = d.verifier->device_config();
    hipLaunchKernelGGL(mmf::rd_verify_kernel, dim3((unsigned)V, (unsigned)n_sets), dim3(64), mmf::ransac_lds_bytes(dc.cap, true), st,
                       (const mmf::RdViewDev*)d.views_dev.get(), (int)V, sets_dev, asked_dev, n_asked, (const int*)d.rows_dev.get(),
                       (const float*)d.coords_dev.get(), dc, d.per_view.get(), d.per_view_inlier.get(), stride);
    hipLaunchKernelGGL(mmf::rd_pick_kernel, dim3((unsigned)n_asked, (unsigned)n_sets), dim3(64), 0, st, (const mmf::RdViewDev*)d.views_dev.get(),
                       (int)V, asked_dev, n_asked, (const mmf::RdViewResult*)d.per_view.get(), (const unsigned char*)d.per_view_inlier.get(),
                       stride, d.rec.get(), d.rec_inlier.get());
    MMF_HIP_TRY(hipGetLastError());
    vs->match.last_launches += 2;
    d.rec_stride = stride, d.rec_asked = n_asked;
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
    if (!vs->ver.verifier) return fail(MMF_ERR_STATE, "mmf_viewstore_best_match_device: no verifier attached (mmf_viewstore_set_verifier)");
    MMF_REQUIRE(nq <= vs->ver.verifier->max_points, "mmf_viewstore_best_match_device: more query rows than the verifier's max_points");
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    mmf::RdRecord rec;
    std::memset(&rec, 0, sizeof(rec));
    for (int k = 0; k < 16; k += 5) rec.T[k] = 1.f;
    rec.error = std::numeric_limits<float>::infinity(), rec.view = -1;
    vs->match.last_launches = 0;
    if (viewstore_has_model(vs, model_id) && model_id >= 0 && nq > 0) {
        const RdSet set{query, nq, 0};
        int rc = viewstore_enqueue(vs, vs->ctx->stream, &set, 1);
        if (rc) return rc;
        if (vs->match.last_launches) {  // (a store of empty views: nothing was launched, nothing can match)
            const mmf::RdVerifySet vset{coordinate, nq, 0};
            rc = viewstore_enqueue_verify(vs, vs->ctx->stream, &vset, 1, &model_id, 1);
            if (rc) return rc;
            MMF_HIP_TRY(wait_stream(vs->ctx->stream));
            rec = vs->ver.rec.get()[0];
            if (inlier && rec.found)
                for (int i = 0; i < rec.n_matches && i < nq; ++i) inlier[i] = vs->ver.rec_inlier.get()[i];
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
// does not fit it (more rows than max_points) -- the triples drawn anew per view, no view of more than 65535 pairs.  From
// the results of a set that has been matched and awaited.
static RdBest viewstore_best_fresh(const mmf_viewstore* vs, int model, const RdSet& set, const float* coordinate,
                                   const mmf::RigidRANSAC::Config& cfg) {
    std::vector<unsigned short> triples(3 * (size_t)cfg.iterations);
    return viewstore_best_of_views(vs, model, set, coordinate, [&](const float* query, const float* train, int n, RdBest* est) {
        if (n > 65535) return false;
        mmf::ransac_triples(cfg.iterations, n, triples.data());
        est->inlier.resize((size_t)n);
        est->inliers = mmf::ransac_core_host(cfg, triples.data(), query, train, n, &est->transformation, &est->error, est->inlier.data());
        return true;
    });
}

// the record of a verification as the estimate the host rules return (without the inlier flags, which stay in rec_inlier)
static RdBest viewstore_best_of_record(const mmf::RdRecord& rec) {
    RdBest best;
    best.found = rec.found != 0, best.error = rec.error, best.inliers = rec.inliers, best.view = rec.view, best.n_matches = rec.n_matches;
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) best.transformation.R[r * 3 + q] = rec.T[r * 4 + q];
        best.transformation.t[r] = rec.T[r * 4 + 3];
    }
    return best;
}

// Queries handed in on the host: room for `rows` query rows, and for their coordinates if they travel too (the device
// verifier's).  *desc [rows][256] / *coord [rows][3] = the pinned memory the caller fills before viewstore_upload_staged,
// which enqueues the copies on `st`; the kernels read vs->query.q.dev / qc.dev.
static int viewstore_stage(mmf_viewstore* vs, size_t rows, bool with_coords, float** desc, float** coord) {
    MMF_HIP_TRY(vs->query.q.reserve(rows * kRdDim));
    if (with_coords) MMF_HIP_TRY(vs->query.qc.reserve(rows * 3));
    *desc = vs->query.q.pin.get(), *coord = with_coords ? vs->query.qc.pin.get() : nullptr;
    return MMF_OK;
}
static int viewstore_upload_staged(mmf_viewstore* vs, size_t rows, bool with_coords, hipStream_t st) {
    MMF_HIP_TRY(vs->query.q.upload(rows * kRdDim, st));
    if (with_coords) MMF_HIP_TRY(vs->query.qc.upload(rows * 3, st));
    return MMF_OK;
}

// ---- a frame's batch: several query sets handed in on the host against several models (frame_redetect) --------
struct RdBatch {
    std::vector<RdSet> sets;    // the caller gives nq and q0 (the rows of the sets before it); viewstore_batch_run gives q
    std::vector<int> asked;     // the models the device verifier picks for, in the caller's order
    std::vector<float> coords;  // HOST [rows][3], the sets behind one another
    bool on_device = false;     // the device rule: the coordinates travel too, a set beyond max_points goes to the host core
    bool verified = false;      // the two verification launches were enqueued: the records are this batch's
};

// Stages the sets, has fill(desc HOST [rows][256], coord HOST [rows][3]) write their rows, uploads, enqueues the three match
// launches per set and -- on_device (needs a verifier attached) with models asked for and a match launched -- the two
// verification launches for all (set, asked model) pairs, and waits for `st`: the one wait of the batch.
template <class Fill>
static int viewstore_batch_run(mmf_viewstore* vs, hipStream_t st, RdBatch* b, bool on_device, Fill fill) {
    size_t rows = 0;
    for (const RdSet& s : b->sets) rows += (size_t)s.nq;
    b->on_device = on_device, b->verified = false;
    b->coords.assign(rows * 3, 0.f);
    float *q_fill = nullptr, *qc_fill = nullptr;
    int rc = viewstore_stage(vs, rows, on_device, &q_fill, &qc_fill);
    if (rc) return rc;
    for (RdSet& s : b->sets) s.q = vs->query.q.dev.get() + s.q0 * kRdDim;
    if (rows) {
        fill(q_fill, b->coords.data());
        if (on_device) std::memcpy(qc_fill, b->coords.data(), rows * 3 * sizeof(float));
        rc = viewstore_upload_staged(vs, rows, on_device, st);
        if (rc) return rc;
    }
    rc = viewstore_enqueue(vs, st, b->sets.data(), (int)b->sets.size());
    if (rc) return rc;
    // (no match launched -- a store without rows: nothing can be found)
    if (on_device && vs->match.last_launches > 0 && !b->asked.empty()) {
        std::vector<mmf::RdVerifySet> vsets(b->sets.size());
        for (size_t s = 0; s < vsets.size(); ++s)
            vsets[s] = mmf::RdVerifySet{vs->query.qc.dev.get() + b->sets[s].q0 * 3, b->sets[s].nq, (int)b->sets[s].q0};
        rc = viewstore_enqueue_verify(vs, st, vsets.data(), (int)vsets.size(), b->asked.data(), (int)b->asked.size());
        if (rc) return rc;
        b->verified = true;
    }
    MMF_HIP_TRY(wait_stream(st));
    return MMF_OK;
}

// set s is verified on the host under the verifier's rule: it has more rows than the verifier takes
static bool viewstore_batch_too_large(const mmf_viewstore* vs, const RdBatch& b, size_t s) {
    return b.on_device && b.sets[s].nq > vs->ver.verifier->max_points;
}

// Model::getBestMatch of `model` for set s of a batch that has run.  The host rule: one engine for the pair.  The device rule:
// the record of (s, model) -- looked up by the model's id among `asked`, wherever the caller's own list has it by now -- or,
// for a set too large, the host core per view.  with_flags: the inlier flags of a record too (the host rules always give them).
static RdBest viewstore_batch_best(const mmf_viewstore* vs, const RdBatch& b, size_t s, int model, bool with_flags) {
    const float* coordinate = b.coords.data() + b.sets[s].q0 * 3;
    if (model < 0) return RdBest();  // (forgotten views carry -1: they belong to nobody)
    if (!b.on_device) return viewstore_best(vs, model, b.sets[s], coordinate, kRedetectRansac);
    if (viewstore_batch_too_large(vs, b, s)) return viewstore_best_fresh(vs, model, b.sets[s], coordinate, vs->ver.verifier->cfg);
    const size_t a = (size_t)(std::find(b.asked.begin(), b.asked.end(), model) - b.asked.begin());
    if (!b.verified || a == b.asked.size()) return RdBest();
    const size_t r = s * b.asked.size() + a;
    RdBest best = viewstore_best_of_record(vs->ver.rec.get()[r]);
    if (with_flags && best.found) {
        const unsigned char* flags = vs->ver.rec_inlier.get() + r * (size_t)vs->ver.rec_stride;
        best.inlier.assign(flags, flags + best.n_matches);
    }
    return best;
}

// The batch above through the C ABI, for the tests: every (set, asked model) pair's estimate.  descriptor / coordinate = HOST,
// the sets behind one another.  rule 0 = the host rule, 1 = the device verifier's (MMF_ERR_STATE without one attached; sets
// beyond its max_points are verified by the host core and counted in *host_verified).  records [n_sets * n_asked], model_id =
// the asked id; inlier (optional) [n_sets * n_asked][inlier_stride], inlier_stride >= the largest set.  Synchronous.
extern "C" int mmf_debug_viewstore_best_match_batch(mmf_viewstore* vs, int n_sets, const int* nq, const float* descriptor,
                                                    const float* coordinate, int n_asked, const int* asked, int rule,
                                                    mmf_debug_redetect_record* records, unsigned char* inlier, int inlier_stride,
                                                    int* host_verified) {
    MMF_REQUIRE(vs && n_sets >= 0 && n_asked >= 0 && (rule == 0 || rule == 1), "mmf_debug_viewstore_best_match_batch: bad argument");
    MMF_REQUIRE((nq || n_sets == 0) && (asked || n_asked == 0), "mmf_debug_viewstore_best_match_batch: null table");
    MMF_REQUIRE(records || n_sets == 0 || n_asked == 0, "mmf_debug_viewstore_best_match_batch: null records");
    if (rule == 1 && !vs->ver.verifier)
        return fail(MMF_ERR_STATE, "mmf_debug_viewstore_best_match_batch: no verifier attached (mmf_viewstore_set_verifier)");
    RdBatch b;
    size_t rows = 0;
    int largest = 0;
    for (int s = 0; s < n_sets; ++s) {
        MMF_REQUIRE(nq[s] >= 0, "mmf_debug_viewstore_best_match_batch: negative set size");
        b.sets.push_back(RdSet{nullptr, nq[s], rows});
        rows += (size_t)nq[s], largest = std::max(largest, nq[s]);
    }
    MMF_REQUIRE(rows == 0 || (descriptor && coordinate), "mmf_debug_viewstore_best_match_batch: null descriptors or coordinates");
    MMF_REQUIRE(!inlier || inlier_stride >= largest, "mmf_debug_viewstore_best_match_batch: inlier_stride below the largest set");
    b.asked.assign(asked, asked + n_asked);
    MMF_HIP_TRY(hipSetDevice(vs->ctx->device));
    int rc = viewstore_batch_run(vs, vs->ctx->stream, &b, rule == 1, [&](float* desc, float* coord) {
        std::memcpy(desc, descriptor, rows * kRdDim * sizeof(float));
        std::memcpy(coord, coordinate, rows * 3 * sizeof(float));
    });
    if (rc) return rc;
    if (host_verified) *host_verified = 0;
    for (size_t s = 0; s < b.sets.size(); ++s) {
        if (host_verified && viewstore_batch_too_large(vs, b, s)) ++*host_verified;
        for (size_t a = 0; a < b.asked.size(); ++a) {
            const RdBest best = viewstore_batch_best(vs, b, s, b.asked[a], true);
            const size_t r = s * b.asked.size() + a;
            mmf_debug_redetect_record& rec = records[r];
            isometry_to_4x4(best.transformation, rec.T);
            rec.error = best.error, rec.inliers = best.inliers, rec.view = best.view, rec.n_matches = best.n_matches;
            rec.found = best.found ? 1 : 0, rec.model_id = b.asked[a];
            if (!inlier) continue;
            unsigned char* flags = inlier + r * (size_t)inlier_stride;
            std::memset(flags, 0, (size_t)inlier_stride);
            for (size_t i = 0; i < best.inlier.size() && (int)i < best.n_matches; ++i) flags[i] = best.inlier[i];
        }
    }
    return MMF_OK;
}
