// model_host.hpp -- the surfel model on the host: struct mmf_model, the mmf_model_* C ABI and the enqueuers of the map passes
// (predictIndices, combinedPredict, synthesizeDepth, fuse, clean, fill-in) over surfel_kernels.hpp and pass_rect.hpp.
// Restates Core/Model/Model.{h,cpp}, Core/Model/ModelProjection.{h,cpp} and Shaders/{FeedbackBuffer,FillIn}.cpp.
// Textually included by mmf_hip.hip right behind those two kernel files (it uses that file's helpers: the error macros,
// Enqueuer, tunables(), mmf_ctx).
//
// A pass is enqueued in two ways: model by model (model_predict_indices, model_combined_predict,
// mmf_model_synthesize_depth, model_fuse, mmf_model_clean) and for all object models in one launch per pass
// (models_fuse_clean_rect, models_combined_predict_rect).  Both must hand the kernels the same arguments, so how a model's
// state becomes a pass's arguments is written ONCE per pass: model_index_args, model_splat_args, model_fuse_args,
// model_clean_args.  Likewise the splat launch plan (model_splat_plan: launch count, deep store or not, the plausible grid)
// and the host's bookkeeping behind a clean pass (model_clean_enqueued).
#pragma once

constexpr int kCountWord = 8, kCountSeqWord = 9;  // in mmf_model::host_totals

struct mmf_model {
    mmf_ctx* ctx = nullptr;
    int width = 0, height = 0;
    float cx = 0, cy = 0, fx = 0, fy = 0;
    unsigned char id = 0;
    float conf_threshold = 10.f;
    float max_depth = FLT_MAX;  // Model::maxDepth (Model.h:129, set per object from the segmentation: MultiMotionFusion.cpp:486,586)
    int capacity = 0;
    unsigned long long tex_gen = 0;    // bumped by every pass that rewrites the prediction / fill-in images
    // generation of the thumbnail counters (thumbnail_count_px): bumped only by the resolve passes that count into them, so that
    // a stand-alone performFillIn (which rewrites images but counts nothing) cannot flip the slot a reader looks at
    unsigned long long thumb_gen = 0;
    const float* pose_dev = nullptr;    // likewise the pose itself and computeFusionWeight(1) (OdomState::pose_out,
    const float* weight_dev = nullptr;  // fusion_weight) for a fuse pass; `weighting` is then the multiplier
    const int* abort_dev = nullptr;    // ... and the word that tells such a pass that the result it would read is void (MMF_SPECULATION_GUARD)
    const float* t_inv_dev = nullptr;  // set by the orchestrator around projections it enqueues before the tracked pose has
                                       // reached the host: the device copy of inverse(pose) (OdomState::pose_inv)
    FrameRider rider;  // set by the orchestrator for the predict() right behind a chain: carried by its resolve launch
    float pose[16];
    unsigned count = 0;  // host copy of the number of surfels in set[cur]
    // After clean() the new count is on its way to host_totals (asynchronous copy on the stream); until a host
    // decision needs it, launches are sized by count_bound and read the exact value from totals[0] on the device.
    bool count_pending = false;
    unsigned count_bound = 0;

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
    unsigned* totals = nullptr;    // [0] scan total a, [1] scan total b, [2] thumbnail count
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
    unsigned* host_totals = nullptr;      // pinned, device visible: words 0..3 = copies of totals[], kCountWord / kCountSeqWord =
    unsigned* host_totals_dev = nullptr;  // the count the last clean pass published and its sequence number
    unsigned count_seq = 0;
    hipStream_t count_stream = nullptr;  // the stream the last clean pass ran on when it is not the context's (a batched pass)
    // pass_rect.hpp: where this model's key image was written and where its images are non-zero (device), the numbers of its
    // projection / index-resolve / prediction-resolve launches, and whether the non-zero boxes describe the images (a
    // full-frame pass leaves them unknown: the next restricted resolve then covers the whole image once)
    PassBoxes* boxes = nullptr;
    unsigned kgen = 0, igen = 0, sgen = 0;
    bool idx_nz_known = false, spl_nz_known = false;
};

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
    for (int i = 0; i < 16; ++i) m->pose[i] = (i % 5 == 0) ? 1.f : 0.f;
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
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    size_t o_set[2][3], o_meas[3], o_cand[3];
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 3; ++k) o_set[s][k] = carve(cap * 16);
    for (int k = 0; k < 3; ++k) o_meas[k] = carve(npix * 16);
    for (int k = 0; k < 3; ++k) o_cand[k] = carve(npix * 16);
    const size_t o_fa = carve((cap + npix) * 4), o_fb = carve(npix * 4), o_pa = carve((cap + npix) * 4),
                 o_pb = carve(npix * 4), o_bs = carve(((cap + npix) / 256 + 2) * 4), o_tot = carve(64),
                 o_win = carve(cap * 4), o_ct = carve((cap + npix) * 8), o_keys = carve(npix * 8), o_rays = carve(npix * 16),
                 o_idx = carve(npix * 4), o_vc = carve(npix * 16), o_ctm = carve(npix * 16), o_nr = carve(npix * 16),
                 o_img = carve(npix * 4), o_vxc = carve(npix * 16), o_nrr = carve(npix * 16), o_tt = carve(npix * 2), o_sd = carve(npix * 4), o_ex = carve(npix * 52),
                 o_fv = carve(npix * 16), o_fn = carve(npix * 16), o_fi = carve(npix * 4);
    m->slab_bytes = off;
    hipError_t e = hipMalloc(&m->slab, m->slab_bytes);
    if (e != hipSuccess) {
        delete m;
        return fail(MMF_ERR_HIP, std::string("mmf_model_create: hipMalloc: ") + hipGetErrorString(e));
    }
    MMF_HIP_TRY(hipMemsetAsync(m->slab, 0, m->slab_bytes, c->stream));
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->boxes), sizeof(PassBoxes)));
    MMF_HIP_TRY(hipMemsetAsync(m->boxes, 0, sizeof(PassBoxes), c->stream));
    char* b = static_cast<char*>(m->slab);
    for (int s = 0; s < 2; ++s)
        m->set[s] = SurfelSoA{(float4*)(b + o_set[s][0]), (float4*)(b + o_set[s][1]), (float4*)(b + o_set[s][2])};
    m->meas = SurfelSoA{(float4*)(b + o_meas[0]), (float4*)(b + o_meas[1]), (float4*)(b + o_meas[2])};
    m->cand2 = SurfelSoA{(float4*)(b + o_cand[0]), (float4*)(b + o_cand[1]), (float4*)(b + o_cand[2])};
    m->flags_a = (unsigned*)(b + o_fa), m->flags_b = (unsigned*)(b + o_fb);
    m->prefix_a = (unsigned*)(b + o_pa), m->prefix_b = (unsigned*)(b + o_pb);
    m->block_sums = (unsigned*)(b + o_bs), m->totals = (unsigned*)(b + o_tot);
    m->winner = (unsigned*)(b + o_win), m->conf_time = (float2*)(b + o_ct);
    m->keys = (unsigned long long*)(b + o_keys);
    m->rays = (float4*)(b + o_rays);
    m->index = (unsigned*)(b + o_idx);
    m->vertConf = (float4*)(b + o_vc), m->colorTime = (float4*)(b + o_ctm), m->normRad = (float4*)(b + o_nr);
    m->image = (uchar4*)(b + o_img), m->vertexConf = (float4*)(b + o_vxc), m->normalRadius = (float4*)(b + o_nrr);
    m->time_tex = (unsigned short*)(b + o_tt);
    m->synth_depth = (float*)(b + o_sd);
    m->export_rm = (void*)(b + o_ex);
    m->fill_vertex = (float4*)(b + o_fv), m->fill_normal = (float4*)(b + o_fn), m->fill_image = (uchar4*)(b + o_fi);
    hipLaunchKernelGGL(fill_u32_kernel, grid1d(cap), dim3(256), 0, c->stream, m->winner, cap, kNoWinner);
    // the key image starts empty and every resolve kernel hands it back empty
    hipLaunchKernelGGL(fill_u64_kernel, grid1d(npix), dim3(256), 0, c->stream, m->keys, npix, kEmptyKey);
    hipLaunchKernelGGL(splat_ray_kernel, grid1d(npix), dim3(256), 0, c->stream, make_cam(m, false), width, height, m->rays);
    MMF_HIP_TRY(hipGetLastError());
    MMF_HIP_TRY(hipHostMalloc(&m->host_totals, 64, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(m->host_totals, 0, 64);
    MMF_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&m->host_totals_dev), m->host_totals, 0));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    *out = m;
    return MMF_OK;
}

// The model of a rigid body another rank owns: id, thresholds and pose on the host, no surfel store, no images
// (mmf_fusion_set_shard; the round-2 advisor's finding: every rank allocated every model's stores)
static int model_create_bookkeeping(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy, unsigned char id,
                                    float conf_threshold, mmf_model** out) {
    mmf_model* m = model_alloc(c, width, height, cx, cy, fx, fy, id, conf_threshold, 0);
    MMF_REQUIRE(m != nullptr, "mmf_model_create: out of host memory");
    *out = m;
    return MMF_OK;
}

extern "C" void mmf_model_destroy(mmf_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->slab);
    (void)hipFree(m->boxes);
    (void)hipHostFree(m->host_totals);
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
// makes m->count exact again (after the stream has passed the clean pass that produced it)
static int model_resolve_count(mmf_model* m) {
    if (!m->count_pending) return MMF_OK;
    // only the copy that follows the clean pass is awaited, not whatever has been enqueued since (a stream
    // synchronisation here idled the GPU for ~45 us per frame: the splat of the frame was already in the queue)
    // (it arrives without a runtime copy: the clean pass stores it into pinned memory, then the sequence number)
    const volatile unsigned* flag = &m->host_totals[kCountSeqWord];
    bool seen = false;
    const auto t_poll = std::chrono::steady_clock::now();
    while (!seen) {
        for (int i = 0; i < 4096 && !seen; ++i) seen = *flag == m->count_seq;
        if (seen || std::chrono::steady_clock::now() - t_poll > std::chrono::seconds(5)) break;
    }
    if (!seen) {
        MMF_HIP_TRY(hipStreamSynchronize(m->count_stream ? m->count_stream : m->ctx->stream));
        MMF_REQUIRE(*flag == m->count_seq, "model: the surfel count did not reach the host");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const unsigned total = m->host_totals[kCountWord];
    m->count = total < (unsigned)m->capacity ? total : (unsigned)m->capacity;
    m->count_pending = false;
    return MMF_OK;
}

extern "C" int mmf_model_count(mmf_model* m, unsigned* count) {
    MMF_REQUIRE(m && count, "mmf_model_count: null argument");
    const int rc_count = model_resolve_count(m);
    if (rc_count) return rc_count;
    *count = m->count;
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
    MMF_HIP_TRY(hipMemcpyAsync(m->host_totals, m->totals, 16, hipMemcpyDeviceToHost, c->stream));
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
    int rc = device_scan(c, m->flags_a, npix, m->prefix_a, m->block_sums, &m->totals[0]);
    if (rc) return rc;
    rc = device_scan(c, m->flags_b, npix, m->prefix_b, m->block_sums, &m->totals[1]);
    if (rc) return rc;
    hipLaunchKernelGGL(init_scatter_kernel, grid1d(npix), dim3(256), 0, c->stream, npix, m->meas, m->flags_a,
                       m->prefix_a, m->cand2, m->flags_b, m->prefix_b, m->set[m->cur], (unsigned)m->capacity);
    MMF_HIP_TRY(hipGetLastError());
    rc = model_read_totals(m);
    if (rc) return rc;
    // "both raw and filtered have the same amount of vertices" (Model.cpp:292); capped by the buffer
    m->count = m->host_totals[0] < (unsigned)m->capacity ? m->host_totals[0] : (unsigned)m->capacity;
    m->count_pending = false;
    return MMF_OK;
}

static IndexArgs model_index_args(mmf_model* m, int time, float depth_cutoff, int time_delta) {
    IndexArgs a;
    inverse4f_host(m->pose, a.t_inv.m);
    a.t_inv_dev = m->t_inv_dev;
    a.abort_dev = m->abort_dev;
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
    m->idx_nz_known = false;  // (pass_rect.hpp: a full-frame resolve; the non-zero box is not kept)
    // frame_rider.hpp: when this is the frame's first projection, its first launch carries the tracking result's hand-over
    // to the host and its second the fusion weight (each a few microseconds on one extra workgroup, shorter than its carrier)
    FrameRider publish = m->rider, weight = m->rider;
    publish.what = 1u, weight.what = 2u;
    m->rider = FrameRider();
    MMF_REQUIRE(!(projected && publish.st), "mmf_model_predict_indices: a tracking result to hand over, but no projection launch to carry it");
    if (!projected && (m->count || publish.st))
        hipLaunchKernelGGL(index_map_kernel, dim3((unsigned)((m->count + 255) / 256) + (publish.st ? 1u : 0u)), dim3(256), 0, c->stream,
                           m->set[m->cur], (int)m->count, a, m->keys, publish);
    hipLaunchKernelGGL(index_resolve_kernel, dim3((unsigned)((npix + 255) / 256) + (weight.st ? 1u : 0u)), dim3(256), 0, c->stream,
                       m->set[m->cur], a, m->keys, m->index, m->vertConf, m->colorTime, m->normRad, weight);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}
extern "C" int mmf_model_predict_indices(mmf_model* m, int time, float depth_cutoff, int time_delta) {
    return model_predict_indices(m, time, depth_cutoff, time_delta, false);
}

// the two thumbnail counters of thumbnail_count_px (surfel_kernels.hpp): the count of the latest prediction is [thumb_gen & 1]
static unsigned* model_thumb_counts(mmf_model* m) { return &m->totals[4]; }
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
    a.t_inv_dev = m->t_inv_dev;
    a.abort_dev = m->abort_dev;
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
    p.launch_count = m->count_pending ? m->count_bound : m->count;
    // a DEEP store (two surfels per pixel and more: occluded layers) looks at the key image before it evaluates a fragment
    // (surfel_kernels.hpp, splat_kernel<true>): a fraction of the fragments and of their atomics.  Same images either way.
    const int bound_mode = (int)g_splat_bound.get(tunables().splat_bound);
    const size_t npix =(size_t)m->width * m->height;
    p.deep = bound_mode < 0 ? (size_t)p.launch_count >= 2 * npix : bound_mode != 0;
    // The bound right after clean() is count + every pixel; the waves deal the surfels out whatever the grid is, and every
    // wave with a surfel notes its sprites' box: size the grid by what the store can plausibly hold (the count before the
    // clean pass, doubled, + 8192) -- 4 000 one-surfel waves noting into four words took 180 us
    const size_t plausible = std::min<size_t>(p.launch_count, (size_t)m->count * 2 + 8192);
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
    ++m->tex_gen;
    ++m->thumb_gen;
    m->spl_nz_known = false;  // (pass_rect.hpp)
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
        ++m->kgen, ++m->sgen;
        if (launch_count)
            hipLaunchKernelGGL(splat_box_kernel, dim3(plan.box_grid), dim3(256), 0, c->stream, m->set[m->cur],
                               (int)launch_count, a, m->keys, m->count_pending ? m->totals : nullptr, m->boxes, m->kgen);
        hipLaunchKernelGGL(splat_resolve_keep_box_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0, c->stream, m->set[m->cur], a, m->keys,
                           m->image, m->vertexConf, m->normalRadius, m->time_tex, model_thumb_counts(m), (int)(m->thumb_gen & 1), m->boxes, m->kgen,
                           m->sgen);
        m->spl_nz_known = true;
        MMF_HIP_TRY(hipGetLastError());
        return MMF_OK;
    }
    if (launch_count)
        hipLaunchKernelGGL(deep ? splat_kernel<true> : splat_kernel<false>, splat_grid(launch_count, (size_t)launch_count >= (size_t)m->width * m->height / 2), dim3(256), 0, c->stream,
                           m->set[m->cur], (int)launch_count, a, m->keys, m->count_pending ? m->totals : nullptr);
    if (fill_rgb && fill_depth) {  // (a pending frame rider stays for the predictIndices that follows: frame_rider.hpp)
        hipLaunchKernelGGL(splat_resolve_fill_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0,
                           c->stream, m->set[m->cur], a, m->keys, m->image, m->vertexConf, m->normalRadius, m->time_tex, fill_depth,
                           fill_rgb, lost ? 1 : 0, (lost || frame_to_frame_rgb) ? 1 : 0, m->fill_vertex, m->fill_normal,
                           m->fill_image, model_thumb_counts(m), (int)(m->thumb_gen & 1));
    } else
        hipLaunchKernelGGL(splat_resolve_kernel, dim3(splat_tile_grid(m->width, m->height)), dim3(256), 0, c->stream, m->set[m->cur], a, m->keys, m->image,
                           m->vertexConf, m->normalRadius, m->time_tex, model_thumb_counts(m), (int)(m->thumb_gen & 1));
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
    if (m->count)
        hipLaunchKernelGGL(splat_kernel<false>, splat_grid(m->count), dim3(256), 0, c->stream, m->set[m->cur], (int)m->count, a,
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
    a.pose_dev = m->pose_dev, a.weight_dev = m->weight_dev, a.weight_mult = weighting;
    a.abort_dev = m->abort_dev;
    a.maskID = m->id;
    a.maxDepth = depth_cutoff < m->max_depth ? depth_cutoff : m->max_depth;  // std::min(depthCutoff, maxDepth) (Model.cpp:928)
    a.count = (int)m->count;
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
    if (m->count && then_index)
        hipLaunchKernelGGL(fuse_update_index_kernel, grid1d(m->count), dim3(256), 0, c->stream, m->set[m->cur], (int)m->count,
                           m->meas, time, m->winner, *then_index, m->keys);
    else if (m->count)
        hipLaunchKernelGGL(fuse_update_kernel, grid1d(m->count), dim3(256), 0, c->stream, m->set[m->cur], (int)m->count,
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
    a.t_inv_dev = m->t_inv_dev;
    a.abort_dev = m->abort_dev;
    a.c = make_cam(m, false);
    a.cols = m->width, a.rows = m->height;
    a.time = time, a.timeDelta = time_delta;
    a.confThreshold = m->conf_threshold;
    a.outlierCoeff = outlier_coeff;
    a.maskID = m->id;
    a.count = (int)m->count;
    a.npix = m->width * m->height;
    return a;
}
// The host's bookkeeping behind an enqueued clean pass; st: the stream it went to when that is not the context's (a batch).
// glGetQueryObjectuiv(countQuery) in the reference (Model.cpp:1166) stalls for the count; here the scatter's last
// workgroup stores it into the host's pinned words, where the next call that needs it on the host picks it up
static void model_clean_enqueued(mmf_model* m, hipStream_t st) {
    const unsigned n = m->count + (unsigned)(m->width * m->height);  // the count's bound: every pixel could still be a candidate
    m->count_bound = n < (unsigned)m->capacity ? n : (unsigned)m->capacity;
    m->count_pending = true;
    m->count_stream = st;
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
    const unsigned n = m->count + npix;
    hipLaunchKernelGGL(clean_flag_kernel, grid1d(n), dim3(256), 0, c->stream, m->set[m->cur], m->meas, m->flags_b, a,
                       m->index, m->vertConf, m->colorTime, depth_filtered, mask, m->flags_a, m->conf_time, m->block_sums);
    hipLaunchKernelGGL(clean_scatter_kernel, grid1d(n), dim3(256), 0, c->stream, m->set[m->cur], m->meas, (int)m->count,
                       npix, m->flags_a, m->block_sums, m->conf_time, m->set[1 - m->cur], m->capacity, &m->totals[0],
                       m->host_totals_dev + kCountWord, ++m->count_seq, m->abort_dev);
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
        MMF_REQUIRE(m && m->boxes && m->rider.st == nullptr && !m->t_inv_dev && !m->pose_dev && !m->weight_dev && !m->abort_dev,
                    "models_fuse_clean_rect: a model with a pending hand-over or a device-side pose");
        if (int rc0 = model_resolve_count(m)) return rc0;
        const IndexArgs ia = model_index_args(m, time, depth_cutoff, time_delta);
        // predictIndices: projection (generation kgen + 1) and its resolve
        index_map_box_item& im = b_map.m[k];
        im.s = m->set[m->cur], im.count = (int)m->count, im.a = ia, im.keys = m->keys, im.boxes = m->boxes, im.kgen = ++m->kgen;
        im.grid = (m->count + 255u) / 256u;
        index_resolve_rect_item& r1 = b_res1.m[k];
        r1.s = m->set[m->cur], r1.a = ia, r1.keys = m->keys, r1.index = m->index, r1.vertConf = m->vertConf, r1.colorTime = m->colorTime,
        r1.normRad = m->normRad, r1.boxes = m->boxes, r1.kgen = m->kgen, r1.igen = ++m->igen, r1.prev_whole = m->idx_nz_known ? 0 : 1;
        m->idx_nz_known = true;
        // fuse: data association over the id's box, then the update pass with the next projection (generation kgen + 1)
        fuse_data_rect_item& fd = b_fuse.m[k];
        fd.rgb = rgb, fd.depth_raw = depth_raw, fd.depth_fil = depth_filtered, fd.mask = mask, fd.index = m->index, fd.vertConf = m->vertConf,
        fd.normRad = m->normRad, fd.a = model_fuse_args(m, time, depth_cutoff, weighting[k]), fd.meas = m->meas, fd.new_flags = m->flags_b, fd.winner = m->winner;
        fd.mask_box = mask_boxes + 4 * (size_t)m->id, fd.mask_gen = mask_gen;
        fuse_update_index_box_item& fu = b_upd.m[k];
        fu.s = m->set[m->cur], fu.count = (int)m->count, fu.meas = m->meas, fu.time = time, fu.winner = m->winner, fu.a = ia, fu.keys = m->keys,
        fu.boxes = m->boxes, fu.kgen = ++m->kgen;
        fu.grid = (m->count + 255u) / 256u;
        index_resolve_rect_item& r2 = b_res2.m[k];
        r2 = r1;
        r2.kgen = m->kgen, r2.igen = ++m->igen, r2.prev_whole = 0;
        // clean
        clean_rect_item& cl = b_clean.m[k];
        cl.s = m->set[m->cur], cl.meas = m->meas, cl.new_flags = m->flags_b, cl.a = model_clean_args(m, time, time_delta, outlier_coeff), cl.index = m->index, cl.vertConf = m->vertConf,
        cl.colorTime = m->colorTime, cl.depth_in = depth_filtered, cl.mask = mask, cl.keep = m->flags_a, cl.conf_time = m->conf_time,
        cl.block_sums = m->block_sums, cl.dst = m->set[1 - m->cur], cl.capacity = m->capacity, cl.total_out = &m->totals[0],
        cl.total_host = m->host_totals_dev + kCountWord, cl.seq = ++m->count_seq, cl.mask_box = fd.mask_box, cl.mask_gen = mask_gen;
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
        MMF_REQUIRE(m && m->boxes && m->rider.st == nullptr && !m->t_inv_dev && !m->abort_dev, "models_combined_predict_rect: a model with a device-side pose");
        ++m->tex_gen;
        ++m->thumb_gen;
        // early_z stays 0: the caller batches no deep store (model_predict_batchable)
        const SplatArgs a = model_splat_args(m, depth_cutoff, m->conf_threshold, time, max_time, time_delta);
        const SplatPlan plan = model_splat_plan(m);
        splat_box_item& sp = b_splat.m[k];
        sp.s = m->set[m->cur], sp.count = (int)plan.launch_count, sp.a = a, sp.keys = m->keys, sp.count_dev = m->count_pending ? m->totals : nullptr;
        sp.boxes = m->boxes, sp.kgen = ++m->kgen;
        sp.grid = plan.box_grid;
        splat_resolve_rect_item& sr = b_res.m[k];
        sr.s = m->set[m->cur], sr.a = a, sr.keys = m->keys, sr.image = m->image, sr.vertexConf = m->vertexConf, sr.normalRadius = m->normalRadius,
        sr.time_out = m->time_tex, sr.thumb = model_thumb_counts(m), sr.gen = (int)(m->thumb_gen & 1);
        sr.boxes = m->boxes, sr.kgen = m->kgen, sr.sgen = ++m->sgen, sr.prev_whole = m->spl_nz_known ? 0 : 1;
        m->spl_nz_known = true;
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
    return !model_splat_plan(m).deep && m->rider.st == nullptr && !m->t_inv_dev && !m->abort_dev && !m->pose_dev;
}

// Model::performFillIn (Model.cpp:1607-1616)
extern "C" int mmf_model_perform_fill_in(mmf_model* m, const uint8_t* rgb, const float* depth_filtered,
                                         int frame_to_frame_rgb, int lost) {
    MMF_REQUIRE(m && rgb && depth_filtered, "mmf_model_perform_fill_in: null argument");
    ++m->tex_gen;
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
    MMF_HIP_TRY(hipMemsetAsync(&m->totals[2], 0, 4, c->stream));
    hipLaunchKernelGGL(thumbnail_count_kernel, grid1d(dc * dr), dim3(256), 0, c->stream, m->image, m->width, m->height,
                       &m->totals[2]);
    MMF_HIP_TRY(hipGetLastError());
    int rc = model_read_totals(m);
    if (rc) return rc;
    *result = ((float)m->host_totals[2] / (float)(dr * dc) < ratio) ? 1 : 0;
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
    *count = m->count;
    return MMF_OK;
}

// Model::downloadMap (Model.cpp:1353-1384): 48-byte AoS surfels {pos+conf, colour/time, normal+radius}
extern "C" int mmf_model_download_map(mmf_model* m, float* host_aos, unsigned max_surfels, unsigned* count_out) {
    MMF_REQUIRE(m && host_aos && count_out, "mmf_model_download_map: null argument");
    if (int rc0 = model_resolve_count(m)) return rc0;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const unsigned n = m->count < max_surfels ? m->count : max_surfels;
    *count_out = n;
    if (!n) return MMF_OK;
    // stage through the (free) other surfel set as an AoS image
    float4* aos = m->set[1 - m->cur].pos;  // 3 * 16 B * capacity contiguous? no: use its three arrays in turn
    (void)aos;
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
    m->count = count;
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
extern "C" int mmf_model_texture(mmf_model* m, const char* name, void** dev_ptr, size_t* bytes) {
    MMF_REQUIRE(m && name && dev_ptr && bytes, "mmf_model_texture: null argument");
    const size_t npix = (size_t)m->width * m->height;
    const std::string s(name);
    void* p = nullptr;
    size_t b = 0;
    // the index map lives transposed in HBM (index_map_kernel); the getters hand out a row-major copy
    // made on the model's stream
    auto exported = [&](auto* src, size_t off) {
        using T = typename std::remove_pointer<decltype(src)>::type;
        T* dst = reinterpret_cast<T*>(reinterpret_cast<char*>(m->export_rm) + off);
        hipLaunchKernelGGL((untranspose_kernel<T>), grid1d(npix), dim3(256), 0, m->ctx->stream, src, m->width, m->height, dst);
        return (void*)dst;
    };
    if (s == "index") p = exported(m->index, 0), b = npix * 4;
    else if (s == "vertConf") p = exported(m->vertConf, npix * 4), b = npix * 16;
    else if (s == "colorTime") p = exported(m->colorTime, npix * 20), b = npix * 16;
    else if (s == "normRad") p = exported(m->normRad, npix * 36), b = npix * 16;
    else if (s == "image") p = m->image, b = npix * 4;
    else if (s == "vertexConf") p = m->vertexConf, b = npix * 16;
    else if (s == "normalRadius") p = m->normalRadius, b = npix * 16;
    else if (s == "time") p = m->time_tex, b = npix * 2;
    else if (s == "depth") p = m->synth_depth, b = npix * 4;
    else if (s == "fillVertex") p = m->fill_vertex, b = npix * 16;
    else if (s == "fillNormal") p = m->fill_normal, b = npix * 16;
    else if (s == "fillImage") p = m->fill_image, b = npix * 4;
    else return fail(MMF_ERR_INVALID, "mmf_model_texture: unknown name '" + s + "'");
    *dev_ptr = p;
    *bytes = b;
    return MMF_OK;
}
