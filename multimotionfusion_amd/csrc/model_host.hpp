// model_host.hpp -- the surfel model on the host.  Restates Core/Model/Model.{h,cpp}, Core/Model/ModelProjection.{h,cpp} and
// Shaders/{FeedbackBuffer,FillIn}.cpp.  Textually included by mmf_hip.hip right behind surfel_kernels.hpp and pass_rect.hpp (it
// uses that file's helpers: the error macros, Enqueuer, tunables(), mmf_ctx).  What it holds, in this order:
//   * the words of totals[] (ModelTotalsWord) and `struct mmf_model`, its state grouped by protocol: the surfel count's
//     hand-over from a clean pass to the host (ModelCount), the inputs the orchestrator sets around passes it enqueues ahead
//     of the pose (ModelDeviceInputs), the generations and known-box flags of the restricted passes (ModelGenerations);
//   * kModelBuffers, the ONE list of the slab's buffers: the slab's size, every pointer and mmf_model_texture's answers;
//   * mmf_model_create / model_create_bookkeeping / mmf_model_destroy, model_resolve_count, model_reset_store;
//   * the mmf_model_* C ABI and the enqueuers of the map passes (predictIndices, combinedPredict, synthesizeDepth, fuse,
//     clean, fill-in);
//   * what the orchestrator may ask about a model without knowing its members: model_is_bookkeeping, model_pred_box,
//     model_latest_thumb_count, model_predict_batchable.
//
// A pass is enqueued in two ways: model by model (model_predict_indices, model_combined_predict,
// mmf_model_synthesize_depth, model_fuse, mmf_model_clean) and for all object models in one launch per pass
// (models_fuse_clean_rect, models_combined_predict_rect).  Both must hand the kernels the same arguments, so how a model's
// state becomes a pass's arguments is written ONCE per pass: model_index_args, model_splat_args, model_fuse_args,
// model_clean_args.  Likewise the splat launch plan (model_splat_plan: launch count, deep store or not, the plausible grid)
// and the host's bookkeeping behind a clean pass (model_clean_enqueued).
#pragma once

// The words of mmf_model::totals (device) and of mmf_model::count.host_totals (pinned host memory, device visible).
enum ModelTotalsWord : int {
    kScanTotalA = 0,     // grand total of the scan over flags_a: the surfel count behind initialise / clean
    kScanTotalB = 1,     // grand total of the scan over flags_b (initialise)
    kFillInThumb = 2,    // the thumbnail count of mmf_model_requires_fill_in
    kThumbCount0 = 4,    // thumbnail_count_px's two counters: a resolve pass counts into [kThumbCount0 + (gen.thumb & 1)]
    kThumbCount1 = 5,
    kCountWord = 8,      // host_totals only: the count the last clean pass published ...
    kCountSeqWord = 9,   // ... and that pass's sequence number, stored after it
    kTotalsWords = 16    // the size of either array
};
// model_read_totals copies the words below kThumbCount0 to host_totals, and a store reset zeroes them
constexpr size_t kTotalsReadBackBytes = kThumbCount0 * sizeof(unsigned);

// The surfel count's hand-over from a clean pass to the host.  After clean() the new count is on its way to host_totals (the
// scatter's last workgroup stores it there); until a host decision needs it, launches are sized by `bound` and read the exact
// value from totals[kScanTotalA] on the device.
struct ModelCount {
    unsigned value = 0;    // host copy of the number of surfels in set[cur]; exact unless `pending`
    bool pending = false;
    unsigned bound = 0;
    unsigned seq = 0;      // the sequence number of the last clean pass
    hipStream_t stream = nullptr;         // the stream that pass ran on when it is not the context's (a batched pass)
    unsigned* host_totals = nullptr;      // pinned, device visible (ModelTotalsWord)
    unsigned* host_totals_dev = nullptr;  // ... as the device addresses it
    // the number of surfels a launch is sized for
    unsigned launch_size() const { return pending ? bound : value; }
    // the device word a kernel reads the exact count from; null: the launch size is exact
    const unsigned* exact_dev(const unsigned* totals) const { return pending ? totals + kScanTotalA : nullptr; }
    // an empty store (the caller has let an in-flight count land: model_resolve_count)
    void clear() { value = 0, pending = false, bound = 0; }
};

// What the orchestrator sets around passes it enqueues before the tracked pose has reached the host (frame_enqueue_ahead):
// device copies of what the pass arguments otherwise carry by value.
struct ModelDeviceInputs {
    const float* pose = nullptr;    // the pose itself and computeFusionWeight(1) (OdomState::pose_out, fusion_weight) for a
    const float* weight = nullptr;  // fuse pass; `weighting` is then the multiplier
    const int* abort = nullptr;     // the word that tells such a pass that the result it would read is void (MMF_SPECULATION_GUARD)
    const float* t_inv = nullptr;   // inverse(pose) for the projections (OdomState::pose_inv)
    FrameRider rider;               // for the predict() right behind a chain: carried by its resolve launch (frame_rider.hpp)
    // back to none.  (Not the rider: the launch that carries it takes it, model_predict_indices.)
    void reset() { pose = weight = t_inv = nullptr, abort = nullptr; }
    // none pending: what a batched fuse + clean needs (its items have no room for any of them)
    bool none() const { return none_for_predict() && !pose && !weight; }
    // a prediction's arguments carry neither pose nor weight (SplatArgs), so its batch does not ask about them
    bool none_for_predict() const { return rider.st == nullptr && !t_inv && !abort; }
    // choosing that batch's members also asks about the pose (the orchestrator sets it only while t_inv is set: no more models left out)
    bool none_for_predict_batch() const { return none_for_predict() && !pose; }
};

// pass_rect.hpp: the numbers of a model's projection / index-resolve / prediction-resolve launches, and whether the non-zero
// boxes (PassBoxes) describe the images -- a full-frame pass leaves them unknown: the next restricted resolve then covers the
// whole image once.
struct ModelGenerations {
    unsigned key = 0, idx = 0, spl = 0;  // the kernels' kgen / igen / sgen
    bool idx_nz_known = false, spl_nz_known = false;
    unsigned long long tex = 0;  // bumped by every pass that rewrites the prediction / fill-in images
    // generation of the thumbnail counters (thumbnail_count_px): bumped only by the resolve passes that count into them, so that
    // a stand-alone performFillIn (which rewrites images but counts nothing) cannot flip the slot a reader looks at
    unsigned long long thumb = 0;
};

struct mmf_model {
    mmf_ctx* ctx = nullptr;
    int width = 0, height = 0;
    float cx = 0, cy = 0, fx = 0, fy = 0;
    unsigned char id = 0;
    float conf_threshold = 10.f;
    float max_depth = FLT_MAX;  // Model::maxDepth (Model.h:129, set per object from the segmentation: MultiMotionFusion.cpp:486,586)
    int capacity = 0;
    float pose[16];
    ModelCount count;
    ModelDeviceInputs dev;
    ModelGenerations gen;

    // one slab of HBM; every buffer below points into it (kModelBuffers: the one list of them).  Null: a bookkeeping model
    void* slab = nullptr;
    size_t slab_bytes = 0;
    SurfelSoA set[2];  // ping-pong surfel stores (Model.cpp:174-188: two VBOs)
    int cur = 0;
    SurfelSoA meas;    // per-pixel measurement of the data pass (the "update map" + newUnstableBuffer)
    SurfelSoA cand2;   // second per-pixel candidate set (first frame: filtered-depth pass)
    unsigned* flags_a = nullptr;   // count + npix
    unsigned* flags_b = nullptr;   // npix
    unsigned* prefix_a = nullptr;  // count + npix
    unsigned* prefix_b = nullptr;  // npix
    unsigned* block_sums = nullptr;
    unsigned* totals = nullptr;    // ModelTotalsWord
    unsigned* winner = nullptr;    // capacity
    float2* conf_time = nullptr;   // capacity + npix
    unsigned long long* keys = nullptr;  // npix
    float4* rays = nullptr;              // npix: the pixels' normalised viewing rays (splat_ray_kernel), transposed
    // sparse index map (ModelProjection.cpp:28-41)
    unsigned* index = nullptr;
    float4 *vertConf = nullptr, *colorTime = nullptr, *normRad = nullptr;
    // splat prediction (ModelProjection.cpp:47-55)
    uchar4* image = nullptr;
    float4 *vertexConf = nullptr, *normalRadius = nullptr;
    unsigned short* time_tex = nullptr;
    float* synth_depth = nullptr;  // ModelProjection::synthesizeDepth target (depthTexture, R32F)
    void* export_rm = nullptr;     // row-major copies of the (transposed) index-map images for mmf_model_texture
    // fill-in (Shaders/FillIn.cpp)
    float4 *fill_vertex = nullptr, *fill_normal = nullptr;
    uchar4* fill_image = nullptr;
    // pass_rect.hpp: where this model's key image was written and where its images are non-zero (device; ModelGenerations)
    PassBoxes* boxes = nullptr;
    // export_host.hpp: the workspace of mmf_model_export_cloud (an allocation of its own, made by the first export) and the
    // launches of the last one
    void* export_ws = nullptr;
    size_t export_ws_bytes = 0;
    int export_launches = 0;
    int import_launches = 0;  // import_host.hpp: the launches of the last mmf_model_import_cloud
};

// Every buffer of the slab, ONCE, in the order it is carved.  The slab's size, the pointers and mmf_model_texture's answers
// all come from this list; the order, the sizes and the 256-byte rounding of every entry are pinned by
// tests/test_gpu_model_buffers.py.
struct ModelBuffer {
    const char* name;  // what mmf_model_texture knows it by (null: not exposed)
    size_t member;     // where its pointer lives in mmf_model
    size_t per_surfel, per_pixel, per_scan_block, fixed;  // its bytes: per surfel of capacity, per pixel, per 256 of both, plus
    bool exported;     // an index-map image: lives transposed, mmf_model_texture hands out a row-major copy in export_rm
    constexpr size_t bytes(size_t cap, size_t npix) const {
        return per_surfel * cap + per_pixel * npix + per_scan_block * ((cap + npix) / 256) + fixed;
    }
};
constexpr size_t kExportPerPixel = 4 + 3 * 16;  // the four exported images, one behind the other
#define MMF_MODEL_BUF(name, m, per_surfel, per_pixel) {name, offsetof(mmf_model, m), per_surfel, per_pixel, 0, 0, false}
#define MMF_MODEL_SOA(m, per_surfel, per_pixel) \
    MMF_MODEL_BUF(nullptr, m.pos, per_surfel, per_pixel), MMF_MODEL_BUF(nullptr, m.col, per_surfel, per_pixel), MMF_MODEL_BUF(nullptr, m.nrm, per_surfel, per_pixel)
constexpr ModelBuffer kModelBuffers[] = {
    MMF_MODEL_SOA(set[0], 16, 0),
    MMF_MODEL_SOA(set[1], 16, 0),
    MMF_MODEL_SOA(meas, 0, 16),
    MMF_MODEL_SOA(cand2, 0, 16),
    MMF_MODEL_BUF(nullptr, flags_a, 4, 4),
    MMF_MODEL_BUF(nullptr, flags_b, 0, 4),
    MMF_MODEL_BUF(nullptr, prefix_a, 4, 4),
    MMF_MODEL_BUF(nullptr, prefix_b, 0, 4),
    {nullptr, offsetof(mmf_model, block_sums), 0, 0, 4, 2 * 4, false},  // ((cap + npix) / 256 + 2) words
    {nullptr, offsetof(mmf_model, totals), 0, 0, 0, kTotalsWords * sizeof(unsigned), false},
    MMF_MODEL_BUF(nullptr, winner, 4, 0),
    MMF_MODEL_BUF(nullptr, conf_time, 8, 8),
    MMF_MODEL_BUF(nullptr, keys, 0, 8),
    MMF_MODEL_BUF(nullptr, rays, 0, 16),
    {"index", offsetof(mmf_model, index), 0, 4, 0, 0, true},
    {"vertConf", offsetof(mmf_model, vertConf), 0, 16, 0, 0, true},
    {"colorTime", offsetof(mmf_model, colorTime), 0, 16, 0, 0, true},
    {"normRad", offsetof(mmf_model, normRad), 0, 16, 0, 0, true},
    MMF_MODEL_BUF("image", image, 0, 4),
    MMF_MODEL_BUF("vertexConf", vertexConf, 0, 16),
    MMF_MODEL_BUF("normalRadius", normalRadius, 0, 16),
    MMF_MODEL_BUF("time", time_tex, 0, 2),
    MMF_MODEL_BUF("depth", synth_depth, 0, 4),
    MMF_MODEL_BUF(nullptr, export_rm, 0, kExportPerPixel),
    MMF_MODEL_BUF("fillVertex", fill_vertex, 0, 16),
    MMF_MODEL_BUF("fillNormal", fill_normal, 0, 16),
    MMF_MODEL_BUF("fillImage", fill_image, 0, 4),
};
#undef MMF_MODEL_SOA
#undef MMF_MODEL_BUF
constexpr size_t model_exported_per_pixel() {
    size_t sum = 0;
    for (const ModelBuffer& b : kModelBuffers) sum += b.exported ? b.per_pixel : 0;
    return sum;
}
static_assert(model_exported_per_pixel() == kExportPerPixel, "export_rm holds exactly the exported images");

// calls place(entry, offset in the slab) for every buffer in carve order; returns the slab's size
template <typename F>
static size_t model_walk_slab(size_t cap, size_t npix, F&& place) {
    size_t off = 0;
    for (const ModelBuffer& b : kModelBuffers) {
        place(b, off);
        off = align_up(off + b.bytes(cap, npix), 256);
    }
    return off;
}

static Cam make_cam(const mmf_model* m, bool double_reciprocal) {
    Cam c;
    c.cx = m->cx, c.cy = m->cy, c.fx = m->fx, c.fy = m->fy;
    if (double_reciprocal) {  // Model.cpp:920-921: 1.0 / fx in double, then to float
        c.ifx = (float)(1.0 / m->fx), c.ify = (float)(1.0 / m->fy);
    } else {  // FeedbackBuffer.cpp:86-87, FillIn.cpp:93-94: 1.0f / fx
        c.ifx = 1.0f / m->fx, c.ify = 1.0f / m->fy;
    }
    return c;
}

static void inverse4f_host(const float* m, float* inv) { inverse4f(m, inv); }  // Eigen `pose.inverse()` (ModelProjection.cpp:108)

static inline dim3 grid1d(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// exclusive scan of n flags -> prefix, grand total -> *total_dev
static int device_scan(mmf_ctx* c, const unsigned* flags, unsigned n, unsigned* prefix, unsigned* block_sums,
                       unsigned* total_dev) {
    const unsigned nblocks = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nblocks), dim3(kScanBlock), 0, c->stream, flags, n, block_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kScanBlock), 0, c->stream, block_sums, nblocks, total_dev);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nblocks), dim3(kScanBlock), 0, c->stream, flags, n, block_sums, prefix);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

static void identity16(float* m) {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
}

// a model's header: what it is and where it stands (identity pose), no store and no images yet; nullptr: out of host memory
static mmf_model* model_alloc(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy, unsigned char id,
                              float conf_threshold, int capacity) {
    mmf_model* m = new (std::nothrow) mmf_model();
    if (!m) return nullptr;
    m->ctx = c;
    m->width = width, m->height = height;
    m->cx = cx, m->cy = cy, m->fx = fx, m->fy = fy;
    m->id = id;
    m->conf_threshold = conf_threshold;
    m->capacity = capacity;
    identity16(m->pose);
    return m;
}

extern "C" int mmf_model_create(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy,
                                unsigned char id, float conf_threshold, int max_surfels, mmf_model** out) {
    MMF_REQUIRE(c && out, "mmf_model_create: null argument");
    MMF_REQUIRE(width >= 32 && height >= 32 && width % 4 == 0 && height % 4 == 0, "mmf_model_create: bad size");
    MMF_HIP_TRY(hipSetDevice(c->device));
    // Model::MAX_VERTICES (Model.cpp:119-126)
    mmf_model* m = model_alloc(c, width, height, cx, cy, fx, fy, id, conf_threshold, max_surfels > 0 ? max_surfels : 1024 * 1024);
    MMF_REQUIRE(m != nullptr, "mmf_model_create: out of host memory");
    const size_t npix = (size_t)width * height, cap = (size_t)m->capacity;
    // every buffer out of one allocation, each 256-byte aligned (kModelBuffers); from here on a failure unmakes what is there
    m->slab_bytes = model_walk_slab(cap, npix, [](const ModelBuffer&, size_t) {});
    hipError_t e = hipMalloc(&m->slab, m->slab_bytes);
    if (e != hipSuccess) {
        mmf_model_destroy(m);
        return fail(MMF_ERR_HIP, std::string("mmf_model_create: hipMalloc: ") + hipGetErrorString(e));
    }
    MMF_HIP_TRY(hipMemsetAsync(m->slab, 0, m->slab_bytes, c->stream), mmf_model_destroy(m));
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->boxes), sizeof(PassBoxes)), mmf_model_destroy(m));
    MMF_HIP_TRY(hipMemsetAsync(m->boxes, 0, sizeof(PassBoxes), c->stream), mmf_model_destroy(m));
    model_walk_slab(cap, npix, [m](const ModelBuffer& b, size_t at) {
        const void* p = static_cast<char*>(m->slab) + at;
        std::memcpy(reinterpret_cast<char*>(m) + b.member, &p, sizeof(p));
    });
    hipLaunchKernelGGL(fill_u32_kernel, grid1d(cap), dim3(256), 0, c->stream, m->winner, cap, kNoWinner);
    // the key image starts empty and every resolve kernel hands it back empty
    hipLaunchKernelGGL(fill_u64_kernel, grid1d(npix), dim3(256), 0, c->stream, m->keys, npix, kEmptyKey);
    hipLaunchKernelGGL(splat_ray_kernel, grid1d(npix), dim3(256), 0, c->stream, make_cam(m, false), width, height, m->rays);
    MMF_HIP_TRY(hipGetLastError(), mmf_model_destroy(m));
    const size_t totals_bytes = kTotalsWords * sizeof(unsigned);
    MMF_HIP_TRY(hipHostMalloc(&m->count.host_totals, totals_bytes, hipHostMallocMapped | hipHostMallocCoherent), mmf_model_destroy(m));
    std::memset(m->count.host_totals, 0, totals_bytes);
    MMF_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&m->count.host_totals_dev), m->count.host_totals, 0), mmf_model_destroy(m));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream), mmf_model_destroy(m));
    *out = m;
    return MMF_OK;
}

// The model of a rigid body ANOTHER rank owns (mmf_fusion_set_shard; fusion_state.hpp: a shard rank's bookkeeping copies): the
// host struct only -- id, thresholds and pose -- no slab, no boxes, no pinned words, nothing a pass could be enqueued on
// (every rank used to allocate every model's stores).  model_is_bookkeeping tells it apart.
static int model_create_bookkeeping(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy, unsigned char id,
                                    float conf_threshold, mmf_model** out) {
    mmf_model* m = model_alloc(c, width, height, cx, cy, fx, fy, id, conf_threshold, 0);
    MMF_REQUIRE(m != nullptr, "mmf_model_create: out of host memory");
    *out = m;
    return MMF_OK;
}

static inline bool model_is_bookkeeping(const mmf_model* m) { return m->slab == nullptr; }

// Safe on a half-built model (mmf_model_create's failure paths: whatever is there is freed behind the stream's work, e.g. the
// slab's memset) and on a bookkeeping one: model_alloc leaves every pointer null, and a null pointer frees nothing.
extern "C" void mmf_model_destroy(mmf_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->slab);
    (void)hipFree(m->boxes);
    (void)hipFree(m->export_ws);
    (void)hipHostFree(m->count.host_totals);
    delete m;
}

extern "C" int mmf_model_set_pose(mmf_model* m, const float pose[16]) {
    MMF_REQUIRE(m && pose, "mmf_model_set_pose: null argument");
    std::memcpy(m->pose, pose, sizeof(m->pose));
    return MMF_OK;
}
extern "C" int mmf_model_get_pose(mmf_model* m, float pose[16]) {
    MMF_REQUIRE(m && pose, "mmf_model_get_pose: null argument");
    std::memcpy(pose, m->pose, sizeof(m->pose));
    return MMF_OK;
}
// Model::setMaxDepth / setConfidenceThreshold (Model.h:224-230)
extern "C" int mmf_model_set_max_depth(mmf_model* m, float max_depth) {
    MMF_REQUIRE(m != nullptr, "mmf_model_set_max_depth: null model");
    m->max_depth = max_depth;
    return MMF_OK;
}
extern "C" int mmf_model_set_confidence_threshold(mmf_model* m, float conf_threshold) {
    MMF_REQUIRE(m != nullptr, "mmf_model_set_confidence_threshold: null model");
    m->conf_threshold = conf_threshold;
    return MMF_OK;
}
extern "C" float mmf_model_confidence_threshold(mmf_model* m) { return m ? m->conf_threshold : 0.f; }
extern "C" int mmf_model_id(mmf_model* m) { return m ? (int)m->id : -1; }
// makes m->count.value exact again (after the stream has passed the clean pass that produced it)
static int model_resolve_count(mmf_model* m) {
    ModelCount& n = m->count;
    if (!n.pending) return MMF_OK;
    // only the copy that follows the clean pass is awaited, not whatever has been enqueued since (a stream
    // synchronisation here idled the GPU for ~45 us per frame: the splat of the frame was already in the queue)
    // (it arrives without a runtime copy: the clean pass stores it into pinned memory, then the sequence number)
    const volatile unsigned* flag = &n.host_totals[kCountSeqWord];
    bool seen = false;
    const auto t_poll = std::chrono::steady_clock::now();
    while (!seen) {
        for (int i = 0; i < 4096 && !seen; ++i) seen = *flag == n.seq;
        if (seen || std::chrono::steady_clock::now() - t_poll > std::chrono::seconds(5)) break;
    }
    if (!seen) {
        MMF_HIP_TRY(hipStreamSynchronize(n.stream ? n.stream : m->ctx->stream));
        MMF_REQUIRE(*flag == n.seq, "model: the surfel count did not reach the host");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const unsigned total = n.host_totals[kCountWord];
    n.value = total < (unsigned)m->capacity ? total : (unsigned)m->capacity;
    n.pending = false;
    return MMF_OK;
}

// an empty store at the identity pose (mmf_fusion_reset); a bookkeeping model has no device words to zero
static int model_reset_store(mmf_model* m) {
    if (int rc = model_resolve_count(m)) return rc;  // lets an in-flight count land before it is dropped
    m->count.clear();
    if (!model_is_bookkeeping(m)) MMF_HIP_TRY(hipMemsetAsync(m->totals, 0, kTotalsReadBackBytes, m->ctx->stream));
    identity16(m->pose);
    m->max_depth = FLT_MAX;
    return MMF_OK;
}

extern "C" int mmf_model_count(mmf_model* m, unsigned* count) {
    MMF_REQUIRE(m && count, "mmf_model_count: null argument");
    const int rc_count = model_resolve_count(m);
    if (rc_count) return rc_count;
    *count = m->count.value;
    return MMF_OK;
}

// MultiMotionFusion::filterDepth (MultiMotionFusion.cpp:897-904)
static int filter_depth_on(mmf_ctx* c, Enqueuer& q, const float* depth, int cols, int rows, float max_depth, float* out) {
    MMF_REQUIRE(c && depth && out && cols > 0 && rows > 0, "mmf_filter_depth: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (cols % 2 == 0 && ((uintptr_t)depth & 7u) == 0 && ((uintptr_t)out & 7u) == 0)  // two pixels per lane
        q.launch(bilateral_filter2_kernel, tile_grid(cols / 2, rows), tile_block(), depth, cols, rows, max_depth, out);
    else
        q.launch(bilateral_filter_kernel, tile_grid(cols, rows), tile_block(), depth, cols, rows, max_depth, out);
    return MMF_OK;
}
static int filter_depth_on(mmf_ctx* c, hipStream_t stream, const float* depth, int cols, int rows, float max_depth,
                           float* out) {
    Enqueuer q(stream);
    if (int rc = filter_depth_on(c, q, depth, cols, rows, max_depth, out)) return rc;
    MMF_HIP_TRY(q.flush());
    return MMF_OK;
}

extern "C" int mmf_filter_depth(mmf_ctx* c, const float* depth, int cols, int rows, float max_depth, float* out) {
    MMF_REQUIRE(c != nullptr, "mmf_filter_depth: bad argument");
    return filter_depth_on(c, c->stream, depth, cols, rows, max_depth, out);
}

static int model_read_totals(mmf_model* m) {
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipMemcpyAsync(m->count.host_totals, m->totals, kTotalsReadBackBytes, hipMemcpyDeviceToHost, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    return MMF_OK;
}

// Model::initialise (Model.cpp:267-312) with the two FeedbackBuffer::compute passes it consumes
extern "C" int mmf_model_initialise(mmf_model* m, const uint8_t* rgb, const float* depth_raw,
                                    const float* depth_filtered, int time, float max_depth) {
    MMF_REQUIRE(m && rgb && depth_raw && depth_filtered, "mmf_model_initialise: null argument");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int npix = m->width * m->height;
    const Cam cam = make_cam(m, false);
    hipLaunchKernelGGL(feedback_kernel, grid1d(npix), dim3(256), 0, c->stream, rgb, depth_raw, m->width, m->height, cam,
                       time, max_depth, m->meas, m->flags_a);
    hipLaunchKernelGGL(feedback_kernel, grid1d(npix), dim3(256), 0, c->stream, rgb, depth_filtered, m->width, m->height,
                       cam, time, max_depth, m->cand2, m->flags_b);
    MMF_HIP_TRY(hipGetLastError());
    int rc = device_scan(c, m->flags_a, npix, m->prefix_a, m->block_sums, &m->totals[kScanTotalA]);
    if (rc) return rc;
    rc = device_scan(c, m->flags_b, npix, m->prefix_b, m->block_sums, &m->totals[kScanTotalB]);
    if (rc) return rc;
    hipLaunchKernelGGL(init_scatter_kernel, grid1d(npix), dim3(256), 0, c->stream, npix, m->meas, m->flags_a,
                       m->prefix_a, m->cand2, m->flags_b, m->prefix_b, m->set[m->cur], (unsigned)m->capacity);
    MMF_HIP_TRY(hipGetLastError());
    rc = model_read_totals(m);
    if (rc) return rc;
    // "both raw and filtered have the same amount of vertices" (Model.cpp:292); capped by the buffer
    const unsigned total = m->count.host_totals[kScanTotalA];
    m->count.value = total < (unsigned)m->capacity ? total : (unsigned)m->capacity;
    m->count.pending = false;
    return MMF_OK;
}

static IndexArgs model_index_args(mmf_model* m, int time, float depth_cutoff, int time_delta) {
    IndexArgs a;
    inverse4f_host(m->pose, a.t_inv.m);
    a.t_inv_dev = m->dev.t_inv;
    a.abort_dev = m->dev.abort;
    a.c = make_cam(m, false);
    a.cols = m->width, a.rows = m->height;
    a.maxDepth = depth_cutoff;
    a.time = time, a.timeDelta = time_delta;
    return a;
}

// ModelProjection::predictIndices (ModelProjection.cpp:94-143)
// projected: the surfels are in the key image already (model_fuse with then_index); only the resolve is left
static int model_predict_indices(mmf_model* m, int time, float depth_cutoff, int time_delta, bool projected) {
    MMF_REQUIRE(m != nullptr, "mmf_model_predict_indices: null model");
    if (int rc0 = model_resolve_count(m)) return rc0;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const size_t npix = (size_t)m->width * m->height;
    const IndexArgs a = model_index_args(m, time, depth_cutoff, time_delta);
    m->gen.idx_nz_known = false;  // (pass_rect.hpp: a full-frame resolve; the non-zero box is not kept)
    // frame_rider.hpp: when this is the frame's first projection, its first launch carries the tracking result's hand-over
    // to the host and its second the fusion weight (each a few microseconds on one extra workgroup, shorter than its carrier)
    FrameRider publish = m->dev.rider, weight = m->dev.rider;
    publish.what = 1u, weight.what = 2u;
    m->dev.rider = FrameRider();
    MMF_REQUIRE(!(projected && publish.st), "mmf_model_predict_indices: a tracking result to hand over, but no projection launch to carry it");
    if (!projected && (m->count.value || publish.st))
        hipLaunchKernelGGL(index_map_kernel, dim3((unsigned)((m->count.value + 255) / 256) + (publish.st ? 1u : 0u)), dim3(256), 0, c->stream,
                           m->set[m->cur], (int)m->count.value, a, m->keys, publish);
    hipLaunchKernelGGL(index_resolve_kernel, dim3((unsigned)((npix + 255) / 256) + (weight.st ? 1u : 0u)), dim3(256), 0, c->stream,
                       m->set[m->cur], a, m->keys, m->index, m->vertConf, m->colorTime, m->normRad, weight);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}
extern "C" int mmf_model_predict_indices(mmf_model* m, int time, float depth_cutoff, int time_delta) {
    return model_predict_indices(m, time, depth_cutoff, time_delta, false);
}

// the two thumbnail counters of thumbnail_count_px (surfel_kernels.hpp) ...
static unsigned* model_thumb_counts(mmf_model* m) { return &m->totals[kThumbCount0]; }
// ... and the one the latest prediction counted into: its covered thumbnail samples (device)
static const unsigned* model_latest_thumb_count(const mmf_model* m) { return &m->totals[kThumbCount0 + (m->gen.thumb & 1)]; }
// where the latest prediction is non-zero (device, PassBoxes::spl_nz of its last resolve); null: unknown
static const int* model_pred_box(const mmf_model* m) {
    return m->boxes && m->gen.spl_nz_known ? m->boxes->spl_nz[m->gen.spl & 1u] : nullptr;
}
// splat_kernel's launch: a fixed number of workgroups that deal the surfels out among their waves (surfel_kernels.hpp)
// 512 workgroups = two waves per SIMD for a small store (an object model); a store of half a surfel per pixel and more
// needs the latency of its LDS searches and ray look-ups hidden: 2048 workgroups (combinedPredict 55 -> 52 us on the
// headline loop's 246 k surfels, 124 -> 107 us on 740 k; 1024 / 1280 / 4096: within 1 us of 2048)
static dim3 splat_grid(size_t bound, bool deep = false) {
    const unsigned wgs = tunables().splat_wgs > 0 ? (unsigned)tunables().splat_wgs : (deep ? 2048u : 512u);
    const size_t one_per_thread = (bound + 255) / 256;
    return dim3((unsigned)std::max<size_t>(1, std::min<size_t>(one_per_thread, wgs)));
}
#ifdef MMF_SPLAT_COUNT
extern "C" int mmf_debug_splat_counts(unsigned long long out[4], int reset) {
    MMF_HIP_TRY(hipDeviceSynchronize());
    MMF_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_splat_dbg), 32));
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_splat_dbg), z, 32));
    }
    return MMF_OK;
}
#endif
extern "C" int mmf_debug_depth_keys(mmf_ctx* c, const float* z_dev, int n, float max_depth, unsigned* fast_dev, unsigned* divided_dev) {
    MMF_REQUIRE(c && z_dev && fast_dev && divided_dev && n > 0, "mmf_debug_depth_keys: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(depth_key_probe_kernel, grid1d((size_t)n), dim3(256), 0, c->stream, z_dev, n, max_depth, fast_dev, divided_dev);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}
static Override g_splat_bound;  // the early depth test of a deep store; unset: what the environment says (MMF_SPLAT_BOUND), else by the surfel count; -1 / 0 / 1: mmf_debug_set_splat_bound
extern "C" int mmf_debug_set_splat_bound(int mode) {
    g_splat_bound.set(mode < 0 ? -1 : (mode ? 1 : 0));
    return MMF_OK;
}
// the arguments of the rasterising and resolving passes of combinedPredict / synthesizeDepth; early_z = 0 until the caller of a deep store sets it
static SplatArgs model_splat_args(const mmf_model* m, float depth_cutoff, float conf_threshold, int time, int max_time, int time_delta) {
    SplatArgs a;
    inverse4f_host(m->pose, a.t_inv.m);
    a.t_inv_dev = m->dev.t_inv;
    a.abort_dev = m->dev.abort;
    a.c = make_cam(m, false);
    a.cols = m->width, a.rows = m->height;
    a.maxDepth = depth_cutoff;
    a.confThreshold = conf_threshold;
    a.time = time, a.maxTime = max_time, a.timeDelta = time_delta;
    a.early_z = 0;
    a.rays = m->rays;
    return a;
}
// how a model's combinedPredict is launched
struct SplatPlan {
    unsigned launch_count;  // surfels the rasterising launch is sized for (0: none)
    bool deep;              // splat_kernel<true>, SplatArgs::early_z
    unsigned box_grid;      // workgroups of the box-noting rasteriser (splat_box_kernel and its batched form); 0: no launch
};
static SplatPlan model_splat_plan(const mmf_model* m) {
    SplatPlan p;
    // right after clean() the exact count may still be in flight to the host: size the launch by the bound
    // and let the kernel read the count on the device instead of waiting for it
    p.launch_count = m->count.launch_size();
    // a DEEP store (two surfels per pixel and more: occluded layers) looks at the key image before it evaluates a fragment
    // (surfel_kernels.hpp, splat_kernel<true>): a fraction of the fragments and of their atomics.  Same images either way.
    const int bound_mode = (int)g_splat_bound.get(tunables().splat_bound);
    const size_t npix =(size_t)m->width * m->height;
    p.deep = bound_mode < 0 ? (size_t)p.launch_count >= 2 * npix : bound_mode != 0;
    // The bound right after clean() is count + every pixel; the waves deal the surfels out whatever the grid is, and every
    // wave with a surfel notes its sprites' box: size the grid by what the store can plausibly hold (the count before the
    // clean pass, doubled, + 8192) -- 4 000 one-surfel waves noting into four words took 180 us
    const size_t plausible = std::min<size_t>(p.launch_count, (size_t)m->count.value * 2 + 8192);
    p.box_grid = p.launch_count ? splat_grid(plausible, plausible >= npix / 2).x : 0u;
    return p;
}
// ModelProjection::combinedPredict(ACTIVE) (ModelProjection.cpp:187-269); Model.h:210-214
// fill_rgb / fill_depth != nullptr: Model::performFillIn in the same pass as the resolve (the orchestrator's predict)
static int model_combined_predict(mmf_model* m, float depth_cutoff, int time, int max_time, int time_delta,
                                  const uint8_t* fill_rgb, const float* fill_depth, int frame_to_frame_rgb, int lost) {
    MMF_REQUIRE(m != nullptr, "mmf_model_combined_predict: null model");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    ++m->gen.tex;
    ++m->gen.thumb;
    m->gen.spl_nz_known = false;  // (pass_rect.hpp)
    SplatArgs a = model_splat_args(m, depth_cutoff, m->conf_threshold, time, max_time, time_delta);
    const SplatPlan plan = model_splat_plan(m);
    const unsigned launch_count = plan.launch_count;
    const bool deep = plan.deep;
    a.early_z = deep ? 1 : 0;
    // An OBJECT model (no fill-in, no deep store): the rasterising pass also notes the box of its sprites and the resolve keeps it
    // as the box the prediction is non-zero in (PassBoxes::spl_nz) -- the model-side preparation that follows walks that box
    // instead of the frame.  The grid is the plan's plausible one rather than the bound's.
    const bool keep_box = m->boxes != nullptr && !(fill_rgb && fill_depth) && !deep && m->id != 0;
    if (keep_box) {
        ++m->gen.key, ++m->gen.spl;
        if (launch_count)
            hipLaunchKernelGGL(splat_box_kernel, dim3(plan.box_grid), dim3(256), 0, c->stream, m->set[m->cur],
                               (int)launch_count, a, m->keys, m->count.exact_dev(m->totals), m->boxes, m->gen.key);
        hipLaunchKernelGGL(splat_resolve_keep_box_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0, c->stream, m->set[m->cur], a, m->keys,
                           m->image, m->vertexConf, m->normalRadius, m->time_tex, model_thumb_counts(m), (int)(m->gen.thumb & 1), m->boxes, m->gen.key,
                           m->gen.spl);
        m->gen.spl_nz_known = true;
        MMF_HIP_TRY(hipGetLastError());
        return MMF_OK;
    }
    if (launch_count)
        hipLaunchKernelGGL(deep ? splat_kernel<true> : splat_kernel<false>, splat_grid(launch_count, (size_t)launch_count >= (size_t)m->width * m->height / 2), dim3(256), 0, c->stream,
                           m->set[m->cur], (int)launch_count, a, m->keys, m->count.exact_dev(m->totals));
    if (fill_rgb && fill_depth) {  // (a pending frame rider stays for the predictIndices that follows: frame_rider.hpp)
        hipLaunchKernelGGL(splat_resolve_fill_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0,
                           c->stream, m->set[m->cur], a, m->keys, m->image, m->vertexConf, m->normalRadius, m->time_tex, fill_depth,
                           fill_rgb, lost ? 1 : 0, (lost || frame_to_frame_rgb) ? 1 : 0, m->fill_vertex, m->fill_normal,
                           m->fill_image, model_thumb_counts(m), (int)(m->gen.thumb & 1));
    } else
        hipLaunchKernelGGL(splat_resolve_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0, c->stream, m->set[m->cur], a, m->keys, m->image,
                           m->vertexConf, m->normalRadius, m->time_tex, model_thumb_counts(m), (int)(m->gen.thumb & 1));
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_model_combined_predict(mmf_model* m, float depth_cutoff, int time, int max_time, int time_delta) {
    return model_combined_predict(m, depth_cutoff, time, max_time, time_delta, nullptr, nullptr, 0, 0);
}

// ModelProjection::synthesizeDepth (ModelProjection.cpp:275-335): same sprites and depth test as
// combinedPredict, only corrected_pos.z is kept
extern "C" int mmf_model_synthesize_depth(mmf_model* m, float depth_cutoff, float conf_threshold, int time, int max_time,
                                          int time_delta) {
    MMF_REQUIRE(m != nullptr, "mmf_model_synthesize_depth: null model");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const SplatArgs a = model_splat_args(m, depth_cutoff, conf_threshold, time, max_time, time_delta);  // (early_z stays 0)
    if (int rc0 = model_resolve_count(m)) return rc0;
    if (m->count.value)
        hipLaunchKernelGGL(splat_kernel<false>, splat_grid(m->count.value), dim3(256), 0, c->stream, m->set[m->cur], (int)m->count.value, a,
                           m->keys, nullptr);
    hipLaunchKernelGGL(splat_depth_resolve_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0, c->stream, m->set[m->cur], a, m->keys,
                       m->synth_depth);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// the arguments of fuse's data-association pass
static FuseArgs model_fuse_args(const mmf_model* m, int time, float depth_cutoff, float weighting) {
    FuseArgs a;
    std::memcpy(a.pose.m, m->pose, sizeof(m->pose));
    a.c = make_cam(m, true);
    a.cols = m->width, a.rows = m->height;
    a.time = time;
    a.weighting = weighting;
    a.pose_dev = m->dev.pose, a.weight_dev = m->dev.weight, a.weight_mult = weighting;
    a.abort_dev = m->dev.abort;
    a.maskID = m->id;
    a.maxDepth = depth_cutoff < m->max_depth ? depth_cutoff : m->max_depth;  // std::min(depthCutoff, maxDepth) (Model.cpp:928)
    a.count = (int)m->count.value;
    return a;
}

// Model::fuse (Model.cpp:893-1048): data association + update; `weighting` = computeFusionWeight()
// then_index: the update pass also projects every surfel into the key image with these arguments -- the first half of
// the predictIndices that follows a fuse (fuse_update_index_kernel); the caller continues with model_predict_indices(projected)
static int model_fuse(mmf_model* m, int time, const uint8_t* rgb, const uint8_t* mask, const float* depth_raw,
                      const float* depth_filtered, float depth_cutoff, float weighting, const IndexArgs* then_index) {
    MMF_REQUIRE(m && rgb && mask && depth_raw && depth_filtered, "mmf_model_fuse: null argument");
    if (int rc0 = model_resolve_count(m)) return rc0;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const FuseArgs a = model_fuse_args(m, time, depth_cutoff, weighting);
    hipLaunchKernelGGL(fuse_data_kernel, grid1d((size_t)((m->width + 1) / 2) * ((m->height + 1) / 2)), dim3(256), 0, c->stream, rgb, depth_raw, depth_filtered, mask,
                       m->index, m->vertConf, m->normRad, a, m->meas, m->flags_b, m->winner);
    if (m->count.value && then_index)
        hipLaunchKernelGGL(fuse_update_index_kernel, grid1d(m->count.value), dim3(256), 0, c->stream, m->set[m->cur], (int)m->count.value,
                           m->meas, time, m->winner, *then_index, m->keys);
    else if (m->count.value)
        hipLaunchKernelGGL(fuse_update_kernel, grid1d(m->count.value), dim3(256), 0, c->stream, m->set[m->cur], (int)m->count.value,
                           m->meas, time, m->winner);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}
extern "C" int mmf_model_fuse(mmf_model* m, int time, const uint8_t* rgb, const uint8_t* mask, const float* depth_raw,
                              const float* depth_filtered, float depth_cutoff, float weighting) {
    return model_fuse(m, time, rgb, mask, depth_raw, depth_filtered, depth_cutoff, weighting, nullptr);
}

// the arguments of clean's flag pass
static CleanArgs model_clean_args(const mmf_model* m, int time, int time_delta, float outlier_coeff) {
    CleanArgs a;
    inverse4f_host(m->pose, a.t_inv.m);
    a.t_inv_dev = m->dev.t_inv;
    a.abort_dev = m->dev.abort;
    a.c = make_cam(m, false);
    a.cols = m->width, a.rows = m->height;
    a.time = time, a.timeDelta = time_delta;
    a.confThreshold = m->conf_threshold;
    a.outlierCoeff = outlier_coeff;
    a.maskID = m->id;
    a.count = (int)m->count.value;
    a.npix = m->width * m->height;
    return a;
}
// The host's bookkeeping behind an enqueued clean pass; st: the stream it went to when that is not the context's (a batch).
// glGetQueryObjectuiv(countQuery) in the reference (Model.cpp:1166) stalls for the count; here the scatter's last
// workgroup stores it into the host's pinned words, where the next call that needs it on the host picks it up
static void model_clean_enqueued(mmf_model* m, hipStream_t st) {
    const unsigned n = m->count.value + (unsigned)(m->width * m->height);  // the count's bound: every pixel could still be a candidate
    m->count.bound = n < (unsigned)m->capacity ? n : (unsigned)m->capacity;
    m->count.pending = true;
    m->count.stream = st;
    m->cur = 1 - m->cur;
}

// Model::clean (Model.cpp:1050-1182); must follow mmf_model_fuse + mmf_model_predict_indices of the same frame
extern "C" int mmf_model_clean(mmf_model* m, int time, int time_delta, float depth_cutoff, const float* depth_filtered,
                               const uint8_t* mask, float outlier_coeff) {
    (void)depth_cutoff;  // only consumed by the deformation part, which never runs (nodes == 0)
    MMF_REQUIRE(m && depth_filtered && mask, "mmf_model_clean: null argument");
    if (int rc0 = model_resolve_count(m)) return rc0;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int npix = m->width * m->height;
    const CleanArgs a = model_clean_args(m, time, time_delta, outlier_coeff);
    const unsigned n = m->count.value + npix;
    hipLaunchKernelGGL(clean_flag_kernel, grid1d(n), dim3(256), 0, c->stream, m->set[m->cur], m->meas, m->flags_b, a,
                       m->index, m->vertConf, m->colorTime, depth_filtered, mask, m->flags_a, m->conf_time, m->block_sums);
    hipLaunchKernelGGL(clean_scatter_kernel, grid1d(n), dim3(256), 0, c->stream, m->set[m->cur], m->meas, (int)m->count.value,
                       npix, m->flags_a, m->block_sums, m->conf_time, m->set[1 - m->cur], m->capacity, &m->totals[kScanTotalA],
                       m->count.host_totals_dev + kCountWord, ++m->count.seq, m->dev.abort);
    MMF_HIP_TRY(hipGetLastError());
    model_clean_enqueued(m, nullptr);
    return MMF_OK;
}

// ---- the same passes RESTRICTED to where the models are (pass_rect.hpp): nine launches for all of them ----
// mask_boxes: the id image's boxes of this frame (mask_boxes_kernel, generation mask_gen), device
static int models_fuse_clean_rect(mmf_model* const* ms, int n, hipStream_t st, int time, int time_delta, float depth_cutoff,
                                  const uint8_t* rgb, const uint8_t* mask, const float* depth_raw, const float* depth_filtered,
                                  float outlier_coeff, const float* weighting, const unsigned long long* mask_boxes, unsigned mask_gen) {
    MMF_REQUIRE(ms && n >= 1 && n <= kMaxPassBatch && rgb && mask && depth_raw && depth_filtered && weighting && mask_boxes,
                "models_fuse_clean_rect: bad argument");
    MMF_HIP_TRY(hipSetDevice(ms[0]->ctx->device));
    PassBatch<index_map_box_item> b_map;
    PassBatch<index_resolve_rect_item> b_res1, b_res2;
    PassBatch<fuse_data_rect_item> b_fuse;
    PassBatch<fuse_update_index_box_item> b_upd;
    PassBatch<clean_rect_item> b_clean;
    unsigned g_map = 0, g_upd = 0;
    for (int k = 0; k < n; ++k) {
        mmf_model* m = ms[k];
        // (the builders hand the device-side inputs on as the per-model passes need them: a batch has none)
        MMF_REQUIRE(m && m->boxes && m->dev.none(),
                    "models_fuse_clean_rect: a model with a pending hand-over or a device-side pose");
        if (int rc0 = model_resolve_count(m)) return rc0;
        const IndexArgs ia = model_index_args(m, time, depth_cutoff, time_delta);
        // predictIndices: projection (generation kgen + 1) and its resolve
        index_map_box_item& im = b_map.m[k];
        im.s = m->set[m->cur], im.count = (int)m->count.value, im.a = ia, im.keys = m->keys, im.boxes = m->boxes, im.kgen = ++m->gen.key;
        im.grid = (m->count.value + 255u) / 256u;
        index_resolve_rect_item& r1 = b_res1.m[k];
        r1.s = m->set[m->cur], r1.a = ia, r1.keys = m->keys, r1.index = m->index, r1.vertConf = m->vertConf, r1.colorTime = m->colorTime,
        r1.normRad = m->normRad, r1.boxes = m->boxes, r1.kgen = m->gen.key, r1.igen = ++m->gen.idx, r1.prev_whole = m->gen.idx_nz_known ? 0 : 1;
        m->gen.idx_nz_known = true;
        // fuse: data association over the id's box, then the update pass with the next projection (generation kgen + 1)
        fuse_data_rect_item& fd = b_fuse.m[k];
        fd.rgb = rgb, fd.depth_raw = depth_raw, fd.depth_fil = depth_filtered, fd.mask = mask, fd.index = m->index, fd.vertConf = m->vertConf,
        fd.normRad = m->normRad, fd.a = model_fuse_args(m, time, depth_cutoff, weighting[k]), fd.meas = m->meas, fd.new_flags = m->flags_b, fd.winner = m->winner;
        fd.mask_box = mask_boxes + 4 * (size_t)m->id, fd.mask_gen = mask_gen;
        fuse_update_index_box_item& fu = b_upd.m[k];
        fu.s = m->set[m->cur], fu.count = (int)m->count.value, fu.meas = m->meas, fu.time = time, fu.winner = m->winner, fu.a = ia, fu.keys = m->keys,
        fu.boxes = m->boxes, fu.kgen = ++m->gen.key;
        fu.grid = (m->count.value + 255u) / 256u;
        index_resolve_rect_item& r2 = b_res2.m[k];
        r2 = r1;
        r2.kgen = m->gen.key, r2.igen = ++m->gen.idx, r2.prev_whole = 0;
        // clean
        clean_rect_item& cl = b_clean.m[k];
        cl.s = m->set[m->cur], cl.meas = m->meas, cl.new_flags = m->flags_b, cl.a = model_clean_args(m, time, time_delta, outlier_coeff), cl.index = m->index, cl.vertConf = m->vertConf,
        cl.colorTime = m->colorTime, cl.depth_in = depth_filtered, cl.mask = mask, cl.keep = m->flags_a, cl.conf_time = m->conf_time,
        cl.block_sums = m->block_sums, cl.dst = m->set[1 - m->cur], cl.capacity = m->capacity, cl.total_out = &m->totals[kScanTotalA],
        cl.total_host = m->count.host_totals_dev + kCountWord, cl.seq = ++m->count.seq, cl.mask_box = fd.mask_box, cl.mask_gen = mask_gen;
        g_map = std::max(g_map, im.grid), g_upd = std::max(g_upd, fu.grid);
        model_clean_enqueued(m, st);
    }
    const dim3 blk(256), rect(kRectGroups, n);
    if (g_map) hipLaunchKernelGGL(index_map_box_batched_kernel, dim3(g_map, n), blk, 0, st, b_map);
    hipLaunchKernelGGL(index_resolve_rect_batched_kernel, rect, blk, 0, st, b_res1);
    hipLaunchKernelGGL(fuse_data_rect_batched_kernel, rect, blk, 0, st, b_fuse);
    if (g_upd) hipLaunchKernelGGL(fuse_update_index_box_batched_kernel, dim3(g_upd, n), blk, 0, st, b_upd);
    hipLaunchKernelGGL(index_resolve_rect_batched_kernel, rect, blk, 0, st, b_res2);
    hipLaunchKernelGGL(clean_flag_rect_batched_kernel, rect, blk, 0, st, b_clean);
    hipLaunchKernelGGL(clean_scatter_rect_batched_kernel, rect, blk, 0, st, b_clean);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

static int models_combined_predict_rect(mmf_model* const* ms, int n, hipStream_t st, float depth_cutoff, int time, int max_time,
                                        int time_delta) {
    MMF_REQUIRE(ms && n >= 1 && n <= kMaxPassBatch, "models_combined_predict_rect: bad argument");
    MMF_HIP_TRY(hipSetDevice(ms[0]->ctx->device));
    PassBatch<splat_box_item> b_splat;
    PassBatch<splat_resolve_rect_item> b_res;
    unsigned g_splat = 0;
    for (int k = 0; k < n; ++k) {
        mmf_model* m = ms[k];
        MMF_REQUIRE(m && m->boxes && m->dev.none_for_predict(), "models_combined_predict_rect: a model with a device-side pose");
        ++m->gen.tex;
        ++m->gen.thumb;
        // early_z stays 0: the caller batches no deep store (model_predict_batchable)
        const SplatArgs a = model_splat_args(m, depth_cutoff, m->conf_threshold, time, max_time, time_delta);
        const SplatPlan plan = model_splat_plan(m);
        splat_box_item& sp = b_splat.m[k];
        sp.s = m->set[m->cur], sp.count = (int)plan.launch_count, sp.a = a, sp.keys = m->keys, sp.count_dev = m->count.exact_dev(m->totals);
        sp.boxes = m->boxes, sp.kgen = ++m->gen.key;
        sp.grid = plan.box_grid;
        splat_resolve_rect_item& sr = b_res.m[k];
        sr.s = m->set[m->cur], sr.a = a, sr.keys = m->keys, sr.image = m->image, sr.vertexConf = m->vertexConf, sr.normalRadius = m->normalRadius,
        sr.time_out = m->time_tex, sr.thumb = model_thumb_counts(m), sr.gen = (int)(m->gen.thumb & 1);
        sr.boxes = m->boxes, sr.kgen = m->gen.key, sr.sgen = ++m->gen.spl, sr.prev_whole = m->gen.spl_nz_known ? 0 : 1;
        m->gen.spl_nz_known = true;
        g_splat = std::max(g_splat, sp.grid);
    }
    if (g_splat) hipLaunchKernelGGL(splat_box_batched_kernel, dim3(g_splat, n), dim3(256), 0, st, b_splat);
    hipLaunchKernelGGL(splat_resolve_rect_batched_kernel, dim3(kRectGroups, n), dim3(256), 0, st, b_res);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}
// can a model's combinedPredict go into a batch (models_combined_predict_rect)?  Not a deep store (its rasterising pass is
// another kernel), not one with pending device-side inputs
static bool model_predict_batchable(const mmf_model* m) {
    return !model_splat_plan(m).deep && m->dev.none_for_predict_batch();
}

// Model::performFillIn (Model.cpp:1607-1616)
extern "C" int mmf_model_perform_fill_in(mmf_model* m, const uint8_t* rgb, const float* depth_filtered,
                                         int frame_to_frame_rgb, int lost) {
    MMF_REQUIRE(m && rgb && depth_filtered, "mmf_model_perform_fill_in: null argument");
    ++m->gen.tex;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int npix = m->width * m->height;
    hipLaunchKernelGGL(fill_in_kernel, grid1d(npix), dim3(256), 0, c->stream, m->vertexConf, m->normalRadius, m->image,
                       depth_filtered, rgb, m->width, m->height, make_cam(m, false), lost ? 1 : 0,
                       (lost || frame_to_frame_rgb) ? 1 : 0, m->fill_vertex, m->fill_normal, m->fill_image);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// MultiMotionFusion::requiresFillIn (MultiMotionFusion.cpp:877-895)
extern "C" int mmf_model_requires_fill_in(mmf_model* m, float ratio, int* result) {
    MMF_REQUIRE(m && result, "mmf_model_requires_fill_in: null argument");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int dc = m->width / 20, dr = m->height / 20;
    MMF_HIP_TRY(hipMemsetAsync(&m->totals[kFillInThumb], 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(thumbnail_count_kernel, grid1d(dc * dr), dim3(256), 0, c->stream, m->image, m->width, m->height,
                       &m->totals[kFillInThumb]);
    MMF_HIP_TRY(hipGetLastError());
    int rc = model_read_totals(m);
    if (rc) return rc;
    *result = ((float)m->count.host_totals[kFillInThumb] / (float)(dr * dc) < ratio) ? 1 : 0;
    return MMF_OK;
}

// Model::getModel() (Model.h:297, Model.cpp:357: the vertex buffer the last fuse / clean left = vbos[target]) as a view of the
// surfel store in HBM: three float4 arrays and the number of surfels in them.  The pointers stay valid until
// the next fuse / clean / initialise of this model (the two stores ping-pong).
extern "C" int mmf_model_surfel_arrays(mmf_model* m, const float** pos_conf, const float** colour_time, const float** normal_radius,
                                       unsigned* count) {
    MMF_REQUIRE(m && pos_conf && colour_time && normal_radius && count, "mmf_model_surfel_arrays: null argument");
    if (int rc0 = model_resolve_count(m)) return rc0;
    *pos_conf = reinterpret_cast<const float*>(m->set[m->cur].pos);
    *colour_time = reinterpret_cast<const float*>(m->set[m->cur].col);
    *normal_radius = reinterpret_cast<const float*>(m->set[m->cur].nrm);
    *count = m->count.value;
    return MMF_OK;
}

// Model::downloadMap (Model.cpp:1353-1384): 48-byte AoS surfels {pos+conf, colour/time, normal+radius}
extern "C" int mmf_model_download_map(mmf_model* m, float* host_aos, unsigned max_surfels, unsigned* count_out) {
    MMF_REQUIRE(m && host_aos && count_out, "mmf_model_download_map: null argument");
    if (int rc0 = model_resolve_count(m)) return rc0;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const unsigned n = m->count.value < max_surfels ? m->count.value : max_surfels;
    *count_out = n;
    if (!n) return MMF_OK;
    float4* stage = nullptr;
    MMF_HIP_TRY(hipMalloc(&stage, (size_t)n * 48));
    hipLaunchKernelGGL(soa_to_aos_kernel, grid1d(n), dim3(256), 0, c->stream, m->set[m->cur], (int)n, stage);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_aos, stage, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(stage);
    if (e != hipSuccess) return fail(MMF_ERR_HIP, std::string("mmf_model_download_map: ") + hipGetErrorString(e));
    return MMF_OK;
}

// test / restore hook: replace the store's content with host AoS surfels
extern "C" int mmf_model_upload_map(mmf_model* m, const float* host_aos, unsigned count) {
    MMF_REQUIRE(m && (host_aos || count == 0) && count <= (unsigned)m->capacity, "mmf_model_upload_map: bad argument");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (int rc0 = model_resolve_count(m)) return rc0;  // lets an in-flight count land before it is replaced
    m->count.value = count;
    if (!count) return MMF_OK;
    float4* stage = nullptr;
    MMF_HIP_TRY(hipMalloc(&stage, (size_t)count * 48));
    hipError_t e = hipMemcpyAsync(stage, host_aos, (size_t)count * 48, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(aos_to_soa_kernel, grid1d(count), dim3(256), 0, c->stream, stage, (int)count, m->set[m->cur]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(stage);
    if (e != hipSuccess) return fail(MMF_ERR_HIP, std::string("mmf_model_upload_map: ") + hipGetErrorString(e));
    return MMF_OK;
}

// device images of the projections (the reference's GPUTexture getters, ModelProjection.h:52-77,
// Model.h:232-244).  names: index vertConf colorTime normRad | image vertexConf normalRadius time |
// depth (synthesizeDepth) | fillVertex fillNormal fillImage
// (not on the frame's path: the passes read the struct's pointers)
template <typename T>
static void* model_export_row_major(mmf_model* m, const void* src, size_t off, size_t npix) {
    T* dst = reinterpret_cast<T*>(reinterpret_cast<char*>(m->export_rm) + off);
    hipLaunchKernelGGL((untranspose_kernel<T>), grid1d(npix), dim3(256), 0, m->ctx->stream, static_cast<const T*>(src), m->width, m->height, dst);
    return dst;
}
extern "C" int mmf_model_texture(mmf_model* m, const char* name, void** dev_ptr, size_t* bytes) {
    MMF_REQUIRE(m && name && dev_ptr && bytes, "mmf_model_texture: null argument");
    const size_t npix = (size_t)m->width * m->height;
    size_t export_off = 0;  // the exported images lie in export_rm one behind the other, in the table's order
    for (const ModelBuffer& b : kModelBuffers) {
        const size_t n = b.bytes((size_t)m->capacity, npix);
        if (b.name && std::strcmp(b.name, name) == 0) {
            void* p;
            std::memcpy(&p, reinterpret_cast<const char*>(m) + b.member, sizeof(p));
            // the index map lives transposed in HBM (index_map_kernel); the getters hand out a row-major copy
            // made on the model's stream: the index image of 4-byte words, the other three of float4
            if (b.exported)
                p = b.per_pixel == sizeof(unsigned) ? model_export_row_major<unsigned>(m, p, export_off, npix)
                                                    : model_export_row_major<float4>(m, p, export_off, npix);
            *dev_ptr = p;
            *bytes = n;
            return MMF_OK;
        }
        if (b.exported) export_off += n;
    }
    return fail(MMF_ERR_INVALID, "mmf_model_texture: unknown name '" + std::string(name) + "'");
}
