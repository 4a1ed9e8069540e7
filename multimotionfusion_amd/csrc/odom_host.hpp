// odom_host.hpp -- RGBDOdometry on the host: struct mmf_odom (its state by protocol, the one table of its slab's buffers),
// create / destroy, the init* and pyramid entry points of the reference's call order, statistics, covariance, timing and the
// test accessors of the buffers.  Restates Core/Utils/RGBDOdometry.{h,cpp} outside getIncrementalTransformation.
// The batched preparation is prep_host.hpp, the Gauss-Newton chain chain_host.hpp.  Textually included by mmf_hip.hip behind
// its stand-alone kernel entry points (it uses that file's helpers: the error macros, Enqueuer, mmf_ctx, the launch_* helpers).
#pragma once

// ---------------------------------------------------------------------------------------------
// RGBDOdometry object
// ---------------------------------------------------------------------------------------------
constexpr int kMaxTimedLaunches = 48;  // 19 iterations x (producer + step)

// The host state of an odometry is six small protocols, each between a few functions; a struct each, named for the code that
// writes it (prep_host.hpp, chain_host.hpp, and the orchestrator through them).  Plain data: no invariant is kept here.

// Input aliasing (odom_take_prediction, prep_model_done, mmf_odom_build_depth_pyramid):
// The reference COPIES its inputs at each init* call (RGBDOdometry.cpp:125,130; Model.cpp:359-388).
// An owner that guarantees the images stay untouched until getIncrementalTransformation returns
// (the native orchestrator: they live in its model / frame slabs) sets alias_inputs, and the three
// device-to-device copies per frame (2 x 4.9 MB + 1.2 MB at 640x480) become pointer assignments.
struct OdomInputs {
    bool alias_inputs = false;
    const float *vtmp = nullptr, *ntmp = nullptr;  // what populateRGBDData / copyMaps read: own copy or alias
    const float* depth_l0 = nullptr;               // level 0 of the depth pyramid: own copy or alias
    bool have_tmp = false;  // vmaps_tmp filled by an initICP* call (ordering contract)
    // set by the batched model-side preparation (prep_collect_model): gradients and point clouds are already built, and next_depth is
    // last_depth (both come from the same prediction, RGBDOdometry.cpp:179 -- see odom_populate_rgbd)
    bool prep_batched = false;
};
// What the batched preparation leaves for the next one and for the chain (prep_host.hpp: prep_depth_jobs, prep_image_jobs,
// prep_model_done, odom_adopt_gradients):
// extent.hpp: three boxes of four words (extent_of_level), noted by the model-side preparation's depth jobs when the owner asks for it (extent_gen != 0:
// the number of the frame they were noted for), read by the two-launch chain's passes
struct OdomPrepNotes {
    unsigned extent_gen = 0;
    // prep_batch.hpp (PrepJob::rect_*): the box an object model's model-side preparation last found its prediction non-zero
    // in (device: two slots of four ints, the preparation's number & 1; inside the slab, behind the extent words), and whether
    // it describes the buffers (any preparation of the whole frame leaves it unknown)
    int* box = nullptr;
    unsigned gen = 0;
    bool box_known = false;
    unsigned sensor_gen = 0;     // number of the last sensor-side depth preparation (its smallest depth: extent words 18 / 19)
    float sensor_cutoff = 0.f;   // ... and the depth cut-off its vertex maps were made with
    bool grad_pending = false;   // grad_w_* hold a prepared frame's gradients
};
// The SO3 pre-alignment run ahead of the tracking (set by the orchestrator around odom_prefetch_so3, consumed by odom_chain_begin):
struct OdomSo3Prefetch {
    bool prefetched = false;  // this frame's SO3 pre-alignment already ran (odom_prefetch_so3)
    const OdomState* stage = nullptr;  // ... in this state (nullptr: in this odometry's own)
    bool retry_prefetched = false;  // what the last odom_enqueue_tracking consumed (a chain that gives up is enqueued again)
    const OdomState* retry_stage = nullptr;
};
// Begin speculation (odom_begin_rider writes, odom_chain_begin consumes):
// the beginning of the next tracking already ran, with these arguments, on the last launch of the preparation enqueued ahead
// of it (track_kernels.hpp: prep_batch_begin_kernel); ok: the caller vouches that nothing touched the state since
struct OdomBeginSpec {
    bool valid = false, ok = false;
    BeginArgs args;
};
// The tracking call in flight (odom_chain_call, odom_enqueue_tracking, odom_chain_publish -> odom_finish_tracking, odom_retrack_prepare):
struct OdomCall {
    bool pending_icp = false, pending_so3 = false;  // mode of the tracking call that is in flight (enqueue -> finish)
    hipStream_t track_stream = nullptr;             // the stream that call's chain runs on (the batch leader's)
    mmf_odom* result_of = nullptr;                  // the odometry (batch leader) whose chain publishes this one's result
    unsigned publish_seq = 0;          // sequence number of the last chain enqueued
    bool walked_by_extent = false;  // the last chain enqueued walked this model by its extents (gn_iter_mixed_kernel)
    bool two_launch_once = false;  // the next chain this odometry leads is the two-launch chain (a frame tracked again)
    int last_gn_fault = 0;          // OdomState::gn_fault of the last result picked up (odom_finish_tracking)
};
// Measurement (mmf_odom_enable_timing, odom_timed_slot, odom_finish_tracking):
// measurement mode: every producer / rgb_step launch of a tracking call carries its own
// start / stop events (hipExtLaunchKernelGGL: the dispatch's own begin / end timestamps), the whole chain two more
struct OdomTiming {
    int mode = 0;  // 1: chain events only; 2: also every kernel of the chain
    hipEvent_t ev_kernel[2 * kMaxTimedLaunches] = {};
    int kind[kMaxTimedLaunches] = {};  // level * 2 + (0 producer | 1 rgb_step)
    int n = 0;
    hipEvent_t ev_chain[2] = {};
    mmf_odom_timing acc;
};

struct mmf_odom {
    mmf_ctx* ctx = nullptr;
    int width = 0, height = 0;
    float cx = 0, cy = 0, fx = 0, fy = 0;
    float dist_thres = 0, angle_thres = 0;
    float sobel_scale = 0.125f;         // RGBDOdometry.cpp:31-32
    float max_depth_delta_rgb = 0.07f;  // :33
    float max_depth_rgb = 6.0f;         // :34
    float min_grad[MMF_NUM_PYRS] = {5, 3, 1};  // :103-105

    // one slab of HBM; every buffer below points into it (kOdomBuffers: the one list of them)
    void* slab = nullptr;
    size_t slab_bytes = 0;
    float *vmaps_tmp = nullptr, *nmaps_tmp = nullptr;
    float *vmaps_g_prev[MMF_NUM_PYRS], *nmaps_g_prev[MMF_NUM_PYRS];
    float *vmaps_curr[MMF_NUM_PYRS], *nmaps_curr[MMF_NUM_PYRS];
    float *last_depth[MMF_NUM_PYRS], *next_depth[MMF_NUM_PYRS], *depth_pyr[MMF_NUM_PYRS];
    uint8_t *last_image[MMF_NUM_PYRS], *next_image[MMF_NUM_PYRS], *last_next_image[MMF_NUM_PYRS];
    int16_t *dIdx[MMF_NUM_PYRS], *dIdy[MMF_NUM_PYRS];
    // The gradient images are double buffered: the batched image-side preparation writes grad_w_*, the chain reads dIdx /
    // dIdy, and odom_adopt_gradients swaps the two when a prepared frame becomes the frame that is tracked -- so that the
    // NEXT frame's image side can be prepared while this frame's chain still reads its gradients.
    int16_t *grad_w_dx[MMF_NUM_PYRS], *grad_w_dy[MMF_NUM_PYRS];
    float* cloud[MMF_NUM_PYRS];
    float* cloud4[MMF_NUM_PYRS];  // the same points as {X, Y, Z, 1/Z} (16-byte records: what gn_iter_kernel gathers)
    mmf_dataterm* corres[MMF_NUM_PYRS];
    float* prev_packed[MMF_NUM_PYRS];  // model vertex + normal, pixel interleaved 24-byte records (the ICP gather side)
    OdomState* state = nullptr;  // device
    // reduction scratch of the Gauss-Newton loop and the two error images, inside the slab: every odometry object has
    // its own (concurrent chains on different streams, or one batched chain addressing model m at slab(m) - slab(0))
    float* gn_partials_f = nullptr;
    float* gn_partials_icp = nullptr;
    int2* gn_partials_res = nullptr;
    unsigned* gn_ticket = nullptr;
    float *icp_err = nullptr, *rgb_err = nullptr;  // Model::icpError / rgbError (R32F), written on the last level-0 iteration
    unsigned long long* extent = nullptr;  // extent.hpp's words (OdomPrepNotes::extent_gen)

    OdomInputs in;
    OdomPrepNotes prep;
    OdomSo3Prefetch so3;
    OdomBeginSpec spec;
    OdomCall call;
    OdomTiming timing;

    // an OBJECT model (set by the orchestrator): the two-launch chain walks its images with a quarter of the workgroups
    // (track_kernels.hpp: ChainGeom), batched or alone
    bool sparse = false;
    // ... and the one-launch chain by its extents with a fraction of the workgroups (gn_fused.hpp: gn_iter_mixed_kernel), as
    // many as the box of its own depth needed in its LAST chain plus a quarter (OdomState::gn_need; 0: no chain yet)
    int gn_need[MMF_NUM_PYRS] = {0, 0, 0};
    GnTruncated* gn_truncated = nullptr;  // test hook (mmf_debug_gn_truncate): made by the first truncated chain
    OdomState* host_result = nullptr;  // pinned, device visible: odom_publish_kernel writes it, the host polls publish_seq
    OdomState* host_result_dev = nullptr;
    bool defer_publish = false;        // set by the orchestrator: the hand-over to the host + the fusion weight ride on the
    FrameRider rider;                  // frame's next resolve launch (frame_rider.hpp) instead of ending the chain
    // The one-launch-per-iteration chain has a barrier inside every launch: its workgroups must all become resident.  Two
    // such launches from different streams can each hold part of the GPU and wait for the rest forever, so an owner that
    // keeps several chains in flight at once (the orchestrator without batching) clears this and gets the two-launch chain.
    bool exclusive_chain = true;
    mmf_odom_stats stats;
};

// a pyramid level's size and intrinsics
struct OdomLevel {
    int cols, rows;
    LevelIntr in;
};
static inline OdomLevel odom_level(const mmf_odom* o, int level) {
    return OdomLevel{o->width >> level, o->height >> level, level_intr(o->fx, o->fy, o->cx, o->cy, level)};
}

// Every buffer of the slab, ONCE, in the order it is carved.  The slab's size, the pointers and mmf_odom_buffer's answers
// all come from this list.  The order, the sizes and the 256-byte rounding of every entry are part of what the library
// computes: a batched chain addresses model m at slab(m) - slab(0) (BatchDelta), and several launch paths are chosen by a
// pointer's alignment (residual_vec4_ok, aligned16).  A run of per-level entries is carved level by level.
struct OdomBuffer {
    const char* name;   // what mmf_odom_buffer knows it by (null: not exposed)
    size_t member;      // where its pointer lives in mmf_odom (per level: the first of MMF_NUM_PYRS)
    bool per_level;     // one per pyramid level, sized by the level's pixels; else one, sized by the full image's
    size_t per_pixel;   // its bytes: this many per pixel ...
    size_t fixed;       // ... plus this many
    size_t reserve;     // bytes carved for it when that is more than it shows (0: its bytes)
    bool joined;        // placed right behind the entry before it, inside that entry's 256-byte rounding
    size_t bytes(int width, int height, int level) const {
        return per_pixel * ((size_t)(width >> (per_level ? level : 0)) * (height >> (per_level ? level : 0))) + fixed;
    }
};
#define MMF_ODOM_LEVELS(name, member, per_pixel) {name, offsetof(mmf_odom, member), true, per_pixel, 0, 0, false}
#define MMF_ODOM_SINGLE(name, member, per_pixel, fixed) {name, offsetof(mmf_odom, member), false, per_pixel, fixed, 0, false}
static const OdomBuffer kOdomBuffers[] = {
    // the two staging images (RGBA32F)
    MMF_ODOM_SINGLE(nullptr, vmaps_tmp, 4 * 4, 0),
    MMF_ODOM_SINGLE(nullptr, nmaps_tmp, 4 * 4, 0),
    MMF_ODOM_LEVELS("vmaps_g_prev", vmaps_g_prev, 3 * 4),
    MMF_ODOM_LEVELS("nmaps_g_prev", nmaps_g_prev, 3 * 4),
    MMF_ODOM_LEVELS("vmaps_curr", vmaps_curr, 3 * 4),
    MMF_ODOM_LEVELS("nmaps_curr", nmaps_curr, 3 * 4),
    MMF_ODOM_LEVELS("last_depth", last_depth, 4),
    MMF_ODOM_LEVELS("next_depth", next_depth, 4),
    MMF_ODOM_LEVELS("depth_pyr", depth_pyr, 4),
    MMF_ODOM_LEVELS("last_image", last_image, 1),
    MMF_ODOM_LEVELS("next_image", next_image, 1),
    MMF_ODOM_LEVELS("last_next_image", last_next_image, 1),
    MMF_ODOM_LEVELS("dIdx", dIdx, 2),
    MMF_ODOM_LEVELS("dIdy", dIdy, 2),
    MMF_ODOM_LEVELS(nullptr, grad_w_dx, 2),
    MMF_ODOM_LEVELS(nullptr, grad_w_dy, 2),
    MMF_ODOM_LEVELS("cloud", cloud, 3 * 4),
    MMF_ODOM_LEVELS("cloud4", cloud4, 4 * 4),  // {X, Y, Z, 1/Z} per pixel
    MMF_ODOM_LEVELS("corres", corres, sizeof(mmf_dataterm)),
    MMF_ODOM_LEVELS("prev_packed", prev_packed, 6 * 4),  // {vertex, normal} per pixel
    MMF_ODOM_SINGLE(nullptr, state, 0, sizeof(OdomState)),
    MMF_ODOM_SINGLE(nullptr, gn_partials_f, 0, sizeof(float) * kMaxGrid * kPartialStride),
    MMF_ODOM_SINGLE(nullptr, gn_partials_icp, 0, sizeof(float) * kMaxIcpGrid * kPartialStride),
    MMF_ODOM_SINGLE(nullptr, gn_partials_res, 0, sizeof(int2) * kMaxGrid),
    MMF_ODOM_SINGLE(nullptr, gn_ticket, 0, sizeof(unsigned) * kTicketWords),
    MMF_ODOM_SINGLE("icp_error", icp_err, 4, 0),  // Model::icpError / rgbError (R32F, full size; mmf_odom_buffer
    MMF_ODOM_SINGLE("rgb_error", rgb_err, 4, 0),  // ignores `level` for these and the two below)
    MMF_ODOM_SINGLE("extent", extent, 0, kExtentWords * sizeof(unsigned long long)),  // extent.hpp's words
    // PrepJob::rect_store's two slots, in the 64 bytes behind the extent words
    {"prep_box", offsetof(mmf_odom, prep.box), false, 0, 8 * sizeof(int), 64, true},
};
#undef MMF_ODOM_LEVELS
#undef MMF_ODOM_SINGLE

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// calls place(entry, level, offset in the slab) for every buffer in carve order; returns the slab's size
template <typename F>
static size_t odom_walk_slab(int width, int height, F&& place) {
    const OdomBuffer* const end = std::end(kOdomBuffers);
    size_t off = 0, tail = 0;  // the next 256-byte aligned place, and where the last entry ended
    auto put = [&](const OdomBuffer& b, int level) {
        const size_t at = b.joined ? tail : off;
        place(b, level, at);
        tail = at + std::max(b.reserve, b.bytes(width, height, level));
        off = align_up(tail, 256);
    };
    for (const OdomBuffer* b = std::begin(kOdomBuffers); b != end;) {
        const OdomBuffer* run = b + 1;  // a single entry, or every per-level entry that follows a per-level one
        while (b->per_level && run != end && run->per_level) ++run;
        for (int level = 0; level < (b->per_level ? MMF_NUM_PYRS : 1); ++level)
            for (const OdomBuffer* k = b; k != run; ++k) put(*k, level);
        b = run;
    }
    return off;
}
// the pointer of an entry at a level, as it is NOW (the image ring and the gradients swap theirs)
static void* odom_buffer_ptr(const mmf_odom* o, const OdomBuffer& b, int level) {
    void* p;
    std::memcpy(&p, reinterpret_cast<const char*>(o) + b.member + (b.per_level ? level : 0) * sizeof(void*), sizeof(p));
    return p;
}

// where a batched chain finds odometry o's buffers from the lead's: slab(o) - slab(lead) in bytes (BatchDelta)
static inline long long odom_slab_delta(const mmf_odom* o, const mmf_odom* lead) {
    return (long long)(static_cast<const char*>(o->slab) - static_cast<const char*>(lead->slab));
}

// The host side of an odometry, whole: what mmf_odom_create and odom_create_bookkeeping share.  Null: out of host memory.
static mmf_odom* odom_new_host(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy) {
    mmf_odom* o = new (std::nothrow) mmf_odom();
    if (!o) return nullptr;
    o->ctx = c;
    o->width = width, o->height = height;
    o->cx = cx, o->cy = cy, o->fx = fx, o->fy = fy;
    std::memset(&o->stats, 0, sizeof(o->stats));
    std::memset(&o->timing.acc, 0, sizeof(o->timing.acc));
    o->stats.lastICPCount = o->stats.lastRGBCount = o->stats.lastSO3Count = (float)(width * height);  // :24-28
    return o;
}

extern "C" int mmf_odom_create(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy,
                               float dist_thresh, float angle_thresh, mmf_odom** out) {
    MMF_REQUIRE(c && out, "mmf_odom_create: null argument");
    MMF_REQUIRE(width >= 32 && height >= 32 && width % 4 == 0 && height % 4 == 0 && width < 32768 && height < 32768,
                "mmf_odom_create: width/height must be multiples of 4, >= 32");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_odom* o = odom_new_host(c, width, height, cx, cy, fx, fy);
    MMF_REQUIRE(o != nullptr, "mmf_odom_create: out of host memory");
    o->dist_thres = dist_thresh;
    o->angle_thres = angle_thresh;
    // every buffer out of one allocation, each 256-byte aligned (kOdomBuffers); from here on a failure unmakes what is there
    o->slab_bytes = odom_walk_slab(width, height, [](const OdomBuffer&, int, size_t) {});
    hipError_t e = hipMalloc(&o->slab, o->slab_bytes);
    if (e != hipSuccess) {
        mmf_odom_destroy(o);
        return fail(MMF_ERR_HIP, std::string("mmf_odom_create: hipMalloc: ") + hipGetErrorString(e));
    }
    MMF_HIP_TRY(hipMemsetAsync(o->slab, 0, o->slab_bytes, c->stream), mmf_odom_destroy(o));
    odom_walk_slab(width, height, [o](const OdomBuffer& b, int level, size_t at) {
        const void* p = static_cast<char*>(o->slab) + at;
        std::memcpy(reinterpret_cast<char*>(o) + b.member + (b.per_level ? level : 0) * sizeof(void*), &p, sizeof(p));
    });
    MMF_HIP_TRY(hipHostMalloc(&o->host_result, sizeof(OdomState), hipHostMallocMapped | hipHostMallocCoherent), mmf_odom_destroy(o));
    std::memset(o->host_result, 0, sizeof(OdomState));
    MMF_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&o->host_result_dev), o->host_result, 0), mmf_odom_destroy(o));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream), mmf_odom_destroy(o));
    *out = o;
    return MMF_OK;
}

// The odometry of a model ANOTHER rank tracks (fusion_state.hpp: a shard rank's bookkeeping copies): the host
// struct only -- statistics as they arrive with the pose exchange -- no slab, no events, nothing a kernel could be given.
static int odom_create_bookkeeping(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy, mmf_odom** out) {
    mmf_odom* o = odom_new_host(c, width, height, cx, cy, fx, fy);
    MMF_REQUIRE(o != nullptr, "mmf_odom_create: out of host memory");
    *out = o;
    return MMF_OK;
}

// Safe on a half-built odometry (mmf_odom_create's failure paths) and on a bookkeeping one: a null pointer frees nothing.
extern "C" void mmf_odom_destroy(mmf_odom* o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    (void)hipStreamSynchronize(o->ctx->stream);
    (void)hipFree(o->slab);
    (void)hipFree(o->gn_truncated);
    (void)hipHostFree(o->host_result);
    for (hipEvent_t e : o->timing.ev_kernel)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : o->timing.ev_chain)
        if (e) (void)hipEventDestroy(e);
    delete o;
}

extern "C" int mmf_odom_build_depth_pyramid(mmf_odom* o, const float* depth_l0, size_t step) {
    MMF_REQUIRE(o && depth_l0, "mmf_odom_build_depth_pyramid: null argument");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const size_t s = step ? step : (size_t)o->width * 4;
    if (o->in.alias_inputs && s == (size_t)o->width * 4) {
        o->in.depth_l0 = depth_l0;
    } else {
        MMF_HIP_TRY(hipMemcpy2DAsync(o->depth_pyr[0], (size_t)o->width * 4, depth_l0, s, (size_t)o->width * 4, o->height,
                                     hipMemcpyDeviceToDevice, c->stream));
        o->in.depth_l0 = o->depth_pyr[0];
    }
    for (int i = 1; i < MMF_NUM_PYRS; ++i) {  // Model.cpp:378-382
        int rc = launch_pyrdown_f(c, i == 1 ? o->in.depth_l0 : o->depth_pyr[i - 1], o->width >> (i - 1), o->width >> (i - 1),
                                  o->height >> (i - 1), o->depth_pyr[i], o->width >> i);
        if (rc) return rc;
    }
    return MMF_OK;
}

extern "C" int mmf_odom_init_icp(mmf_odom* o, const float* const depth_pyr[MMF_NUM_PYRS],
                                 const size_t steps[MMF_NUM_PYRS], float depth_cutoff) {
    MMF_REQUIRE(o != nullptr, "mmf_odom_init_icp: null odometry");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {  // RGBDOdometry.cpp:112-115
        const auto [cols, rows, in] = odom_level(o, i);
        const float* d = depth_pyr ? depth_pyr[i] : (i == 0 && o->in.depth_l0 ? o->in.depth_l0 : o->depth_pyr[i]);
        MMF_REQUIRE(d != nullptr, "mmf_odom_init_icp: null pyramid level");
        const int ds = (depth_pyr && steps && steps[i]) ? (int)(steps[i] / 4) : cols;
        int rc = launch_create_vmap(c, in, d, ds, cols, rows, o->vmaps_curr[i],
                                    cols, depth_cutoff);
        if (rc) return rc;
        rc = launch_create_nmap(c, o->vmaps_curr[i], cols, cols, rows, o->nmaps_curr[i], cols);
        if (rc) return rc;
    }
    return MMF_OK;
}

static int odom_take_prediction(mmf_odom* o, const float* vert_rgba, const float* norm_rgba, float** vdst,
                                float** ndst) {
    mmf_ctx* c = o->ctx;
    o->in.prep_batched = false;
    const size_t bytes = (size_t)4 * o->width * o->height * sizeof(float);
    // the reference copies both textures into vmaps_tmp / nmaps_tmp (RGBDOdometry.cpp:125,130);
    // vmaps_tmp is read again by initRGB*/populateRGBDData (:179)
    if (o->in.alias_inputs) {
        o->in.vtmp = vert_rgba, o->in.ntmp = norm_rgba;
    } else {
        MMF_HIP_TRY(hipMemcpyAsync(o->vmaps_tmp, vert_rgba, bytes, hipMemcpyDeviceToDevice, c->stream));
        MMF_HIP_TRY(hipMemcpyAsync(o->nmaps_tmp, norm_rgba, bytes, hipMemcpyDeviceToDevice, c->stream));
        o->in.vtmp = o->vmaps_tmp, o->in.ntmp = o->nmaps_tmp;
    }
    o->in.have_tmp = true;
    int rc = launch_copy_maps(c, o->in.vtmp, o->in.ntmp, o->width, o->height, vdst[0], ndst[0], o->width);
    if (rc) return rc;
    for (int i = 1; i < MMF_NUM_PYRS; ++i) {
        rc = launch_resize<false>(c, vdst[i - 1], o->width >> (i - 1), o->width >> (i - 1), o->height >> (i - 1),
                                  vdst[i], o->width >> i);
        if (rc) return rc;
        rc = launch_resize<true>(c, ndst[i - 1], o->width >> (i - 1), o->width >> (i - 1), o->height >> (i - 1),
                                 ndst[i], o->width >> i);
        if (rc) return rc;
    }
    return MMF_OK;
}

extern "C" int mmf_odom_init_icp_from_prediction(mmf_odom* o, const float* vert_rgba, const float* norm_rgba,
                                                 float depth_cutoff) {
    (void)depth_cutoff;  // unused by the reference as well (RGBDOdometry.cpp:120-141)
    MMF_REQUIRE(o && vert_rgba && norm_rgba, "mmf_odom_init_icp_from_prediction: null argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    return odom_take_prediction(o, vert_rgba, norm_rgba, o->vmaps_curr, o->nmaps_curr);
}

extern "C" int mmf_odom_init_icp_model(mmf_odom* o, const float* vert_rgba, const float* norm_rgba,
                                       float depth_cutoff, const float pose[16]) {
    (void)depth_cutoff;  // unused by the reference as well (RGBDOdometry.cpp:143-175)
    MMF_REQUIRE(o && vert_rgba && norm_rgba && pose, "mmf_odom_init_icp_model: null argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    int rc = odom_take_prediction(o, vert_rgba, norm_rgba, o->vmaps_g_prev, o->nmaps_g_prev);
    if (rc) return rc;
    const float R[9] = {pose[0], pose[1], pose[2], pose[4], pose[5], pose[6], pose[8], pose[9], pose[10]};
    const float t[3] = {pose[3], pose[7], pose[11]};
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {
        const int cols = o->width >> i, rows = o->height >> i;
        rc = launch_transform(o->ctx, o->vmaps_g_prev[i], o->nmaps_g_prev[i], cols, cols, rows, R, t,
                              o->vmaps_g_prev[i], o->nmaps_g_prev[i], cols);
        if (rc) return rc;
        const int n = cols * rows;
        hipLaunchKernelGGL(pack_prev_kernel, dim3((n + 255) / 256), dim3(256), 0, o->ctx->stream, o->vmaps_g_prev[i],
                           o->nmaps_g_prev[i], n, o->prev_packed[i]);
        MMF_HIP_TRY(hipGetLastError());
    }
    return MMF_OK;
}

// RGBDOdometry.cpp:177-194 (populateRGBDData); mask pyramids are never read and are omitted
static int odom_populate_rgbd(mmf_odom* o, const uint8_t* rgb, size_t step, int channels, float** depths,
                              uint8_t** images) {
    mmf_ctx* c = o->ctx;
    o->in.prep_batched = false;
    if (!o->in.have_tmp)
        return fail(MMF_ERR_STATE, "initRGB*/initRGBModel needs a preceding initICPModel / initICP(prediction): "
                                   "it reads vmaps_tmp (RGBDOdometry.cpp:197,202)");
    int rc = launch_vertices_to_depth(c, o->in.vtmp, o->width, o->height, o->max_depth_rgb, depths[0], o->width);
    if (rc) return rc;
    for (int i = 0; i + 1 < MMF_NUM_PYRS; ++i) {
        rc = launch_pyrdown_f(c, depths[i], o->width >> i, o->width >> i, o->height >> i, depths[i + 1],
                              o->width >> (i + 1));
        if (rc) return rc;
    }
    rc = launch_intensity(c, rgb, step ? (int)step : o->width * channels, channels, o->width, o->height, images[0],
                          o->width);
    if (rc) return rc;
    for (int i = 0; i + 1 < MMF_NUM_PYRS; ++i) {
        rc = launch_pyrdown_u8(c, images[i], o->width >> i, o->width >> i, o->height >> i, images[i + 1],
                               o->width >> (i + 1));
        if (rc) return rc;
    }
    return MMF_OK;
}

extern "C" int mmf_odom_init_rgb(mmf_odom* o, const uint8_t* rgb, size_t step, int channels) {
    MMF_REQUIRE(o && rgb && (channels == 3 || channels == 4), "mmf_odom_init_rgb: bad argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    return odom_populate_rgbd(o, rgb, step, channels, o->next_depth, o->next_image);
}

extern "C" int mmf_odom_init_rgb_model(mmf_odom* o, const uint8_t* rgb, size_t step, int channels) {
    MMF_REQUIRE(o && rgb && (channels == 3 || channels == 4), "mmf_odom_init_rgb_model: bad argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    return odom_populate_rgbd(o, rgb, step, channels, o->last_depth, o->last_image);
}

extern "C" int mmf_odom_init_first_rgb(mmf_odom* o, const uint8_t* rgb, size_t step, int channels) {
    MMF_REQUIRE(o && rgb && (channels == 3 || channels == 4), "mmf_odom_init_first_rgb: bad argument");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    int rc = launch_intensity(c, rgb, step ? (int)step : o->width * channels, channels, o->width, o->height,
                              o->last_next_image[0], o->width);
    if (rc) return rc;
    for (int i = 0; i + 1 < MMF_NUM_PYRS; ++i) {  // RGBDOdometry.cpp:212-214
        rc = launch_pyrdown_u8(c, o->last_next_image[i], o->width >> i, o->width >> i, o->height >> i,
                               o->last_next_image[i + 1], o->width >> (i + 1));
        if (rc) return rc;
    }
    return MMF_OK;
}

static IcpArgs odom_icp_args(mmf_odom* o, int level, float* err_map) {
    const auto [cols, rows, in] = odom_level(o, level);
    IcpArgs a;
    a.vmap_curr = MapView{o->vmaps_curr[level], cols};
    a.nmap_curr = MapView{o->nmaps_curr[level], cols};
    a.vmap_g_prev = MapView{o->vmaps_g_prev[level], cols};
    a.nmap_g_prev = MapView{o->nmaps_g_prev[level], cols};
    a.intr = in;
    a.dist_thres = o->dist_thres;
    a.angle_thres = o->angle_thres;
    a.cols = cols;
    a.rows = rows;
    a.prev_packed = o->prev_packed[level];
    a.err_map = err_map;
    a.err_stride = cols;
    icp_args_derive(a);
    return a;
}

// measurement mode: per-launch durations of the Gauss-Newton kernels from the dispatches' own timestamps
extern "C" int mmf_odom_enable_timing(mmf_odom* o, int on) {
    MMF_REQUIRE(o != nullptr, "mmf_odom_enable_timing: null odometry");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    if (on && !o->timing.ev_chain[0]) {
        for (hipEvent_t& e : o->timing.ev_kernel) MMF_HIP_TRY(hipEventCreate(&e));
        for (hipEvent_t& e : o->timing.ev_chain) MMF_HIP_TRY(hipEventCreate(&e));
    }
    o->timing.mode = on < 0 ? 0 : (on > 2 ? 2 : on);
    std::memset(&o->timing.acc, 0, sizeof(o->timing.acc));
    return MMF_OK;
}
extern "C" int mmf_odom_get_timing(mmf_odom* o, mmf_odom_timing* out) {
    MMF_REQUIRE(o && out, "mmf_odom_get_timing: null argument");
    *out = o->timing.acc;
    return MMF_OK;
}

extern "C" int mmf_odom_get_stats(mmf_odom* o, mmf_odom_stats* out) {
    MMF_REQUIRE(o && out, "mmf_odom_get_stats: null argument");
    *out = o->stats;
    return MMF_OK;
}

// RGBDOdometry.cpp:479 -- lastA.lu().inverse(); Gauss-Jordan with partial pivoting on the host
extern "C" int mmf_odom_get_covariance(mmf_odom* o, double cov[36]) {
    MMF_REQUIRE(o && cov, "mmf_odom_get_covariance: null argument");
    double a[6][12];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            a[i][j] = o->stats.lastA[i * 6 + j];
            a[i][6 + j] = (i == j) ? 1.0 : 0.0;
        }
    for (int col = 0; col < 6; ++col) {
        int piv = col;
        for (int r = col + 1; r < 6; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (piv != col)
            for (int k = 0; k < 12; ++k) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 12; ++k) a[col][k] /= d;
        for (int r = 0; r < 6; ++r)
            if (r != col) {
                const double f = a[r][col];
                for (int k = 0; k < 12; ++k) a[r][k] -= f * a[col][k];
            }
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) cov[i * 6 + j] = a[i][6 + j];
    return MMF_OK;
}

// Test-only: a buffer of the slab by its name in kOdomBuffers (nothing on the per-frame path comes here).
extern "C" int mmf_odom_buffer(mmf_odom* o, const char* name, int level, void** dev_ptr, size_t* bytes) {
    MMF_REQUIRE(o && name && dev_ptr && bytes && level >= 0 && level < MMF_NUM_PYRS, "mmf_odom_buffer: bad argument");
    for (const OdomBuffer& b : kOdomBuffers)
        if (b.name && std::strcmp(b.name, name) == 0) {
            *dev_ptr = odom_buffer_ptr(o, b, level);
            *bytes = b.bytes(o->width, o->height, level);
            return MMF_OK;
        }
    return fail(MMF_ERR_INVALID, "mmf_odom_buffer: unknown buffer name '" + std::string(name) + "'");
}

extern "C" int mmf_odom_download(mmf_odom* o, const char* name, int level, void* host_dst, size_t host_bytes) {
    MMF_REQUIRE(host_dst != nullptr, "mmf_odom_download: null destination");
    void* p = nullptr;
    size_t b = 0;
    int rc = mmf_odom_buffer(o, name, level, &p, &b);
    if (rc) return rc;
    MMF_REQUIRE(b == host_bytes, "mmf_odom_download: size mismatch");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(host_dst, p, b, hipMemcpyDeviceToHost, o->ctx->stream));
    MMF_HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    return MMF_OK;
}

extern "C" int mmf_odom_time_icp_kernel(mmf_odom* o, int level, int reps, int variant, float* mean_us_out) {
    MMF_REQUIRE(o && mean_us_out && level >= 0 && level < MMF_NUM_PYRS && reps > 0, "mmf_odom_time_icp_kernel: bad argument");
    MMF_REQUIRE(variant == 0, "mmf_odom_time_icp_kernel: variant must be 0 (the shipped launch geometry)");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const IcpArgs a = odom_icp_args(o, level, nullptr);
    Enqueuer q(c->stream);
    // the state's pose fields are whatever the last getIncrementalTransformation left (or zero);
    // FINISH_RAW only writes out_f
    for (int w = 0; w < 3; ++w) launch_icp<FINISH_RAW>(q, o->state, a, c->partials_icp);
    MMF_HIP_TRY(q.flush());
    MMF_HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; ++r) launch_icp<FINISH_RAW>(q, o->state, a, c->partials_icp);
    MMF_HIP_TRY(q.flush());
    MMF_HIP_TRY(hipEventRecord(c->ev1, c->stream));
    MMF_HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    MMF_HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_us_out = ms * 1000.0f / reps;
    return MMF_OK;
}
