// chain_host.hpp -- getIncrementalTransformation on the host: the SO3 pre-alignment, the tracking mode, the chain's plan
// (one launch per iteration or two), the two chains, publish / finish / retrack and their test hooks, over track_kernels.hpp
// and gn_fused.hpp.  Textually included by mmf_hip.hip behind prep_host.hpp.
#pragma once

// the ten launches of the SO3 pre-alignment (RGBDOdometry.cpp:239-310): last frame's image against this frame's
// at level 2 -- no model, no pose
static int odom_enqueue_so3(mmf_odom* o, Enqueuer& q, float* partials = nullptr, unsigned* ticket = nullptr, OdomState* state = nullptr) {
    if (!partials) partials = o->gn_partials_f, ticket = o->gn_ticket;
    if (!state) state = o->state;
    const int lvl = 2;
    const auto [cols, rows, in] = odom_level(o, lvl);
    So3Args a;
    a.last_image = o->last_next_image[lvl];
    a.next_image = o->next_image[lvl];
    a.l_stride = a.n_stride = cols;
    a.cols = cols;
    a.rows = rows;
    a.intr = in;
    a.cols_magic = (unsigned)((1ull << 32) / (unsigned)cols) + 1u;
    const int grid = reduce_grid(cols * rows, kBlock);
    for (int i = 0; i < 10; ++i) q.launch((so3_kernel<FINISH_GN>), dim3(grid), dim3(kBlock), state, a, partials, ticket);
    return MMF_OK;
}

// the SO3 pre-alignment of the NEXT frame ahead of its tracking, on `stream` (after that frame's intensity
// pyramid): its begin part, then the ten launches; getIncrementalTransformation then skips both
// `stage`: the state the pre-alignment runs in (its images are o's); the caller tells the consumer (mmf_odom::so3_stage)
static int odom_prefetch_so3(mmf_odom* o, Enqueuer& q, float* partials, unsigned* ticket, OdomState* stage) {
    q.launch(so3_begin_kernel, dim3(1), dim3(64), stage, odom_level(o, 2).in);
    return odom_enqueue_so3(o, q, partials, ticket, stage);
}

// RGBDOdometry::getIncrementalTransformation (RGBDOdometry.cpp:217-477), device resident:
// every kernel below is enqueued back to back on the context's stream; the data-dependent
// `break`s of the reference (:285-292, :376-378) become flags in the device state that make the
// remaining launches of that loop return immediately.
// first half: everything up to and including the copy of the result towards the host is enqueued on the
// context's stream, nothing waits.  The orchestrator enqueues the chains of all its models (one stream each)
// before it waits for the first result.
// The models one chain of launches tracks: o[0] leads (its stream, its launch arguments), the others ride at their
// slab offsets (BatchDelta).  All share the sensor-side images (fusion_orchestrator.hpp) and the configuration.
struct TrackBatch {
    int n = 1;
    mmf_odom* o[kMaxBatch];
    BatchDelta bd;
    BeginPoses poses;
};

// The tracking mode of one call, worked out once from the reference's five settings.
struct TrackMode {
    bool icp, rgb, rgb_only, so3;
    float icp_weight;
    int iterations[MMF_NUM_PYRS];  // Gauss-Newton iterations per level
    int first_iter_level;          // the coarsest level that runs iterations (the ones below it all do)
};
static TrackMode track_mode(int rgb_only, float icp_weight, int pyramid, int fast_odom, int so3) {
    TrackMode m;
    m.icp = !rgb_only && icp_weight > 0;  // :221-222
    m.rgb = rgb_only || icp_weight < 100;
    m.rgb_only = rgb_only != 0;
    m.so3 = so3 != 0;
    m.icp_weight = icp_weight;
    const int iterations[MMF_NUM_PYRS] = {fast_odom ? 3 : 10, pyramid ? 5 : 0, pyramid ? 4 : 0};  // :312-314
    std::copy(iterations, iterations + MMF_NUM_PYRS, m.iterations);
    m.first_iter_level = MMF_NUM_PYRS - 1;
    while (m.first_iter_level > 0 && !m.iterations[m.first_iter_level]) --m.first_iter_level;
    return m;
}

// The launch arguments of one pyramid level: the correspondence pass's and the ICP reduction's.  The error images are the
// caller's (the chains write them in the last level-0 iteration only, the planner checks the odometry's own).
struct LevelArgs {
    int cols, rows;
    LevelIntr in;
    RgbResidualArgs ra;
    IcpArgs ia;
};
static LevelArgs odom_level_args(mmf_odom* o, int i, float* rgb_err, float* icp_err) {
    LevelArgs l;
    const OdomLevel lv = odom_level(o, i);
    l.cols = lv.cols, l.rows = lv.rows, l.in = lv.in;
    const float min_scale = (float)(std::pow((double)o->min_grad[i], 2.0) / std::pow((double)o->sobel_scale, 2.0));
    l.ra = make_residual_args(min_scale, o->dIdx[i], 0, o->dIdy[i], 0, o->last_depth[i], 0,
                              o->in.prep_batched ? o->last_depth[i] : o->next_depth[i], 0, o->last_image[i], 0, o->next_image[i],
                              0, o->corres[i], o->max_depth_delta_rgb, l.cols, l.rows, rgb_err, 0);
    l.ra.intr = l.in;
    l.ia = odom_icp_args(o, i, icp_err);
    return l;
}

// Launch geometry of gn_iter_kernel at a level of cols x rows pixels: a workgroup = the solver wave + the pixel waves.  The
// launch is a chain of latencies -- records, solve, two memory round trips, the count barrier -- and every workgroup waits at
// that barrier for the slowest one, so (measured on MI355X, tools/ab_libs.sh): at most one workgroup per CU (two on a CU
// reach the barrier 1.6 us after the others); exactly four pixel waves, one per SIMD, where that fits (a fifth doubles up on
// one SIMD and is the long pole of every arithmetic phase: what 640x480 suffered with four pixels per lane, 300 lanes in 256
// workgroups); as few pixels per lane as those two allow (a lane's serial arithmetic is on the critical path).  Five pixels
// per lane exist for 640x480: 240 workgroups x 256 lanes x 5.
// MMF_GN_PX="p0,p1,p2" forces the pixels per lane of a level, MMF_GN_GROUPS the workgroup limit (tuning aids).
struct GnGeometry {
    int px, lanes, threads, groups;
};
// mixed: a launch that also carries object models walked by their extents (gn_iter_mixed_kernel).  Its register count allows
// three waves per SIMD, and the GPU places a second 5-wave workgroup on a CU only with four (measured: tools/gn_mixed_probe.py
// -- the object models' workgroups started when the camera model's had finished); workgroups of FOUR waves (the solver wave
// + three pixel waves, 192 pixel lanes) take one wave slot per SIMD and three of them share a CU.  (256 lanes measured slower
// at 2, 4 and 8 models: LABNOTES.md.)
constexpr int kGnMixedLanes = 192;
static_assert(kGnMixedLanes % 64 == 0 && kGnMixedLanes <= kGnSparseLanes,
              "the sparse walk keeps a workgroup's correspondences in LDS, sized for kGnSparseLanes lanes");
static Override g_gn_px[MMF_NUM_PYRS];  // unset: MMF_GN_PX decides (default: by geometry); else mmf_debug_set_gn_px
extern "C" int mmf_debug_set_gn_px(int p0, int p1, int p2) {
    const int p[MMF_NUM_PYRS] = {p0, p1, p2};
    const bool clear = p0 < 0 || p1 < 0 || p2 < 0;
    for (int i = 0; i < MMF_NUM_PYRS; ++i) clear ? g_gn_px[i].clear() : g_gn_px[i].set(p[i]);
    return MMF_OK;
}
static bool gn_geometry(int level, int cols, int rows, GnGeometry* out, bool mixed = false) {
    if (mixed) {
        GnGeometry base;
        if (!gn_geometry(level, cols, rows, &base, false) || base.lanes != kBlock) return false;
        const int groups = (cols * rows / base.px + kGnMixedLanes - 1) / kGnMixedLanes;
        if (groups > kGnMaxGroups) return false;
        *out = GnGeometry{base.px, kGnMixedLanes, kGnMixedLanes + 64, groups};
        return true;
    }
    const int* forced = tunables().gn_px;
    const int max_groups = tunables().gn_groups;
    const int n = cols * rows;
    const int want = (level >= 0 && level < 3) ? (int)g_gn_px[level].get(forced[level]) : 0;
    // a lane's pixels lie in one row; the window words are 4-byte aligned columns
    auto allowed = [&](int px) { return cols % px == 0 && cols % 4 == 0 && (!(want == 1 || want == 2 || want == 4 || want == 5) || px == want); };
    static const int kPx[4] = {1, 2, 4, 5};
    for (int k = 0; k < 4; ++k) {  // four pixel waves per workgroup (three, 192 lanes: no different, tools/ab_env.sh)
        const int px = kPx[k];
        const int groups = (n / px + kBlock - 1) / kBlock;
        if (!allowed(px) || groups > max_groups || groups > kGnMaxGroups) continue;
        *out = GnGeometry{px, kBlock, kBlock + 64, groups};
        return true;
    }
    for (int k = 3; k >= 0; --k) {  // larger workgroups, as few of them as the limit asks for
        const int px = kPx[k];
        if (!allowed(px)) continue;
        const int total = n / px;
        const int lanes = std::max(kBlock, (total + max_groups - 1) / max_groups);
        const int groups = (total + lanes - 1) / lanes;
        if (lanes > 64 * (kGnMaxWaves - 1) || groups > kGnMaxGroups) continue;
        *out = GnGeometry{px, lanes, (lanes + 63) / 64 * 64 + 64, groups};
        return true;
    }
    return false;
}
// calls f(std::integral_constant<int, PX>) for the pixels per lane of a Gauss-Newton launch (1, 2, 4 or 5: gn_geometry)
template <typename F>
static auto with_gn_px(int px, F&& f) {
    switch (px) {
        case 5: return f(std::integral_constant<int, 5>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 1>{});
    }
}
// How the chain of one call runs: one launch per iteration (gn_iter_kernel) or two (producer + rgb_step), and how the one-launch
// chain walks the models of a batch (gn_fused.hpp: GnBatchGeom).  Made by odom_plan_chain, the only place that decides it.
struct GnChainPlan {
    bool one_launch = false;
    bool mixed = false;  // object models walked by their extents ride the launch (gn_iter_mixed_kernel)
    unsigned sparse_mask = 0, ext_gen = 0;
    GnGeometry geo[MMF_NUM_PYRS] = {};
    int groups[MMF_NUM_PYRS][kMaxBatch] = {};  // workgroups of model m at level l
};
// workgroups of an OBJECT model per launch of the one-launch chain at pyramid level l (a property of the model, batched or
// alone: its float sums keep their order): its photometric box must fit them in ONE pass (32 x 1280 pixels at 640x480 level 0,
// a box of 200 x 200), its ICP rectangle takes as many passes as it needs
static std::atomic<int> g_sparse_groups{0};  // test hook (mmf_debug_set_sparse_groups): that many at every level instead
// need: the lanes the model's box took in its last chain (0: unknown -- 32 / 24 / 16 workgroups, a box of 200 x 200 at 640x480);
// lanes: pixel lanes of a workgroup.  Returns dense_groups when the model is better walked like the camera model.
static int gn_sparse_groups(int level, int dense_groups, int need, int lanes) {
    static const int k[MMF_NUM_PYRS] = {32, 24, 16};
    const int forced = g_sparse_groups.load();
    if (forced > 0) return std::min(dense_groups, forced);
    int want = k[level < MMF_NUM_PYRS ? level : MMF_NUM_PYRS - 1];
    if (need > 0) want = std::max(8, (need + need / 4 + lanes - 1) / lanes + 1);
    return want * 4 >= dense_groups * 3 ? dense_groups : want;
}
extern "C" int mmf_debug_set_sparse_groups(int n) {
    g_sparse_groups.store(n > 0 ? n : 0);
    return MMF_OK;
}
static std::atomic<bool> g_gn_latched_off{false};
static Override g_track_cull;  // unset: MMF_TRACK_CULL decides; 0 / 1: mmf_debug_set_track_cull
extern "C" int mmf_debug_set_track_cull(int mode) {
    override_flag(g_track_cull, mode);
    return MMF_OK;
}
static std::atomic<int> g_gn_force_fault{0};
static std::atomic<int> g_sparse_check{0};
// test hooks of the object models' walk in the one-launch chain (gn_fused.hpp: gn_sparse_icp_box): checking mode on / off, and the
// number of correspondences the last chain of an odometry accepted outside the rectangle it would have walked (must be 0)
extern "C" int mmf_debug_set_sparse_check(int on) {
    g_sparse_check.store(on ? 1 : 0);
    return MMF_OK;
}
extern "C" int mmf_debug_odom_sparse_outside(mmf_odom* o, unsigned* outside, int* walked_by_extent, int rect[9]) {
    if (!o || !o->host_result) return fail(MMF_ERR_INVALID, "mmf_debug_odom_sparse_outside: null argument");
    if (outside) *outside = o->host_result->gn_dbg_outside;
    if (walked_by_extent) *walked_by_extent = o->call.walked_by_extent ? 1 : 0;
    if (rect) {
        std::memcpy(rect, o->host_result->gn_dbg_rect, sizeof(int) * 6);
        std::memcpy(rect + 6, o->gn_need, sizeof(int) * 3);
    }
    return MMF_OK;
}
static std::atomic<int> g_gn_recoveries{0};
// odom_finish_tracking: the one-launch chain gave up; track again (odom_retrack_prepare).  A private sentinel, outside the
// public mmf_status range (include/mmf_hip.h: 0 and small negatives): it never leaves the library (gn_retry_twice).
constexpr int kGnRetry = 0x6e726574;
static int gn_retry_twice() { return fail(MMF_ERR_STATE, "odometry: tracking gave up twice (the two-launch chain reported a fault)"); }

static bool odom_sparse_on() { return g_track_cull.get(tunables().track_cull) != 0; }
static void odom_begin_rider_used();
// what odom_begin_kernel is told (RGBDOdometry.cpp:221-228, 237, 252-255, 316-328); every byte defined (the blocks are compared)
static BeginArgs odom_begin_args(const mmf_odom* o, const float trans[3], const float rot[9], const TrackMode& tm,
                                 bool so3_prefetched, const OdomState* so3_stage, bool one_launch) {
    BeginArgs b;
    std::memset(&b, 0, sizeof(b));
    std::memcpy(b.trans, trans, sizeof(b.trans));
    std::memcpy(b.rot, rot, sizeof(b.rot));
    b.rgb_only = tm.rgb_only ? 1 : 0;
    b.icp = tm.icp ? 1 : 0;
    b.rgb = tm.rgb ? 1 : 0;
    b.so3 = tm.so3 ? 1 : 0;
    b.icp_weight = tm.icp_weight;
    b.so3_intr = odom_level(o, 2).in;
    b.so3_prefetched = (tm.so3 && so3_prefetched) ? 1 : 0;
    b.so3_stage = b.so3_prefetched ? so3_stage : nullptr;
    // nothing runs between the beginning and the first level's begin unless the SO3 loop does: one launch
    b.fold_level_begin = (!tm.so3 || so3_prefetched) ? 1 : 0;
    // the one-launch chain has no per-level begin: its first launch reads what this one prepares
    b.first_intr = odom_level(o, one_launch ? tm.first_iter_level : MMF_NUM_PYRS - 1).in;
    return b;
}

// can several models ride one chain (every level on the fused producer path)?  Same tests as the two-launch chain.
static bool odom_batchable(mmf_odom* o, const TrackMode& tm) {
    if (!tm.icp || !tm.rgb || tm.rgb_only || !o->in.prep_batched) return false;
    for (int i = 0; i <= tm.first_iter_level; ++i) {
        const LevelArgs l = odom_level_args(o, i, nullptr, nullptr);
        if (!residual_vec4_ok(l.ra) || !icp2_fits(l.ia, kBlock, std::min(2, icp_max_px(l.ia, 2)))) return false;
    }
    return true;
}

// can the chain run as one launch per iteration (gn_iter_kernel)?  Both terms on, four pixels per lane at every level,
// every level's grid small enough to be resident at once (the count barrier inside the launch).  MMF_GN_FUSED=0 keeps the
// two-launch chain (A/B runs, and the test that compares the two).
static Override g_gn_fused;  // unset: MMF_GN_FUSED decides (default on); 0 / 1: mmf_debug_set_gn_fused
extern "C" int mmf_debug_set_gn_fused(int on) {
    override_flag(g_gn_fused, on);
    if (on) g_gn_latched_off.store(false);  // (a test that asks for the one-launch chain again gets it)
    return MMF_OK;
}
// test hook: the next n one-launch chains of this process give up at their third launch (the count barrier of that launch
// polls zero times), as if a workgroup had never arrived: exercises the recovery below without another process on the GPU
extern "C" int mmf_debug_force_gn_fault(int n) {
    g_gn_force_fault.store(n < 0 ? 0 : n);
    return MMF_OK;
}
// test hook: the next one-launch chain of this process runs n launches of gn_iter_kernel at pyramid level first_level and
// nothing else, then ends (gn_truncated_final_kernel) and leaves its last launch's sums and the pose its last solve made in
// a buffer of the odometry's (GnTruncated; read by mmf_debug_gn_truncated).  A call that cannot take the one-launch chain while this is armed fails.
static std::atomic<int> g_gn_truncate{0};  // n << 8 | first_level
extern "C" int mmf_debug_gn_truncate(int n, int first_level) {
    if (n < 0 || n > 64 || first_level < 0 || first_level >= MMF_NUM_PYRS) return fail(MMF_ERR_INVALID, "mmf_debug_gn_truncate: bad argument");
    g_gn_truncate.store(n ? (n << 8 | first_level) : 0);
    return MMF_OK;
}
extern "C" int mmf_debug_gn_truncated(mmf_odom* o, double totals[58], unsigned count_sumsq[2], double rt[12], float pose[24]) {
    MMF_REQUIRE(o && o->gn_truncated && totals && count_sumsq && rt && pose, "mmf_debug_gn_truncated: null argument, or no truncated chain ran");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    MMF_HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    GnTruncated h;
    MMF_HIP_TRY(hipMemcpy(&h, o->gn_truncated, sizeof(h), hipMemcpyDeviceToHost));
    std::memcpy(totals, h.tot, sizeof(h.tot));
    std::memcpy(count_sumsq, h.cnt, sizeof(h.cnt));
    std::memcpy(rt, h.rt, sizeof(h.rt));
    std::memcpy(pose, h.pose, sizeof(h.pose));
    return MMF_OK;
}
// how often a one-launch chain gave up and its frame was tracked again on the two-launch chain, and whether the one-launch
// chain is still in use (it is latched off by the first such event: whatever kept its workgroups from being resident
// together -- another process on this GPU -- is likely still there)
extern "C" int mmf_gn_chain_status(int* recoveries, int* one_launch_chain_in_use) {
    if (recoveries) *recoveries = g_gn_recoveries.load();
    if (one_launch_chain_in_use) *one_launch_chain_in_use = g_gn_latched_off.load() ? 0 : 1;
    return MMF_OK;
}
// the smaller occupancy of a launch shape's two variants (with and without the error images) bounds the chain
template <typename K>
static int gn_occupancy(K with_err, K without_err, int threads) {
    int nb = 0, nb2 = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, with_err, threads, 0);
    const hipError_t e2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb2, without_err, threads, 0);
    if (e != hipSuccess || e2 != hipSuccess) return (void)hipGetLastError(), 0;
    return std::min(nb, nb2);
}
// How many workgroups of gn_iter_kernel<px, .> (mixed: gn_iter_mixed_kernel) with `threads` threads the device holds at once:
// the occupancy the runtime reports for the kernel (registers, LDS) x the compute units.  The launch spins on its own
// workgroups (count barrier), so a grid beyond this could only time out; such sizes, partitioned or smaller devices take the
// two-launch chain.
static long long gn_resident_groups(mmf_ctx* c, int px, bool mixed, int threads) {
    static std::mutex mu;
    static std::map<std::tuple<int, bool, int>, int> per_cu;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(px, mixed, threads);
    auto it = per_cu.find(key);
    if (it == per_cu.end()) {
        const int nb = with_gn_px(px, [&](auto PX) {
            constexpr int P = decltype(PX)::value;
            return mixed ? gn_occupancy(gn_iter_mixed_kernel<P, true>, gn_iter_mixed_kernel<P, false>, threads)
                         : gn_occupancy(gn_iter_kernel<P, true>, gn_iter_kernel<P, false>, threads);
        });
        it = per_cu.emplace(key, nb).first;
    }
    return (long long)it->second * c->cu_count;
}
// The chain's plan for o (batch: the models riding with it, o first).  sparse_on: object models may be walked by their extents.
static GnChainPlan odom_plan_chain(mmf_odom* o, const TrackMode& tm, const TrackBatch* batch, bool sparse_on) {
    const int models = batch ? batch->n : 1;
    const bool enabled = g_gn_fused.get(tunables().gn_fused) != 0 && o->exclusive_chain && !g_gn_latched_off.load();
    // (more than MMF_GN_FUSED_MAX models: the batched two-launch chain)
    if (!enabled || !tm.icp || !tm.rgb || tm.rgb_only || models > tunables().gn_fused_max) return GnChainPlan();
    // the models walked by their extents: object models whose preparation noted extents for THIS frame (one number for all)
    GnChainPlan pl;
    for (int m = 0; m < models && sparse_on; ++m) {
        const mmf_odom* om = batch ? batch->o[m] : o;
        if (!om->sparse || om->prep.extent_gen == 0) continue;
        if (pl.ext_gen == 0) pl.ext_gen = om->prep.extent_gen;
        if (om->prep.extent_gen == pl.ext_gen) pl.sparse_mask |= 1u << m;
    }
    pl.mixed = pl.sparse_mask != 0;
    for (int i = 0; i <= tm.first_iter_level; ++i) {
        const LevelArgs l = odom_level_args(o, i, o->rgb_err, o->icp_err);
        if (!residual_vec4_ok(l.ra) || icp_max_px(l.ia, 4) != 4 || !l.ia.prev_packed) return GnChainPlan();
        GnGeometry& geo = pl.geo[i];
        if (!gn_geometry(i, l.cols, l.rows, &geo, pl.mixed)) return GnChainPlan();
        // the count barrier inside the launch needs every workgroup of it resident at once
        long long total = 0;
        for (int m = 0; m < models; ++m) {
            const mmf_odom* om = batch ? batch->o[m] : o;
            pl.groups[i][m] = ((pl.sparse_mask >> m) & 1u) ? gn_sparse_groups(i, geo.groups, om->gn_need[i], geo.lanes) : geo.groups;
            total += pl.groups[i][m];
        }
        if (total > gn_resident_groups(o->ctx, geo.px, pl.mixed, geo.threads)) return GnChainPlan();
    }
    pl.one_launch = true;
    return pl;
}

// The models one call tracks and what both forms of the chain need to know about them, worked out once.
// Object models (extent.hpp): in the two-launch chain (track_kernels.hpp: ChainGeom) their passes skip what lies outside
// the model's own depth when the preparation noted its extents for this frame, and they walk their images with a
// quarter of the workgroups; in the one-launch chain (gn_fused.hpp: gn_iter_mixed_kernel) they walk their extents with a
// fraction of the workgroups, which is what lets ALL models of a frame be resident in one launch.
// MMF_TRACK_CULL=0 / mmf_debug_set_track_cull(0): every model like the first.
struct ChainCall {
    mmf_odom* o;  // the leader
    const TrackBatch* batch;
    TrackMode tm;
    unsigned ny;  // models
    BatchDelta bd;
    BeginPoses poses;
    float *icp_err, *rgb_err;  // the error images the last level-0 iteration writes (null: none)
    bool sparse_on, lead_sparse, foll_sparse;
    unsigned cull_gen;     // the extents the two-launch chain's passes skip by (0: none)
    bool two_launch_once;  // (odom_retrack_prepare: this frame is being tracked again)
    bool so3_ran_here;     // the SO3 loop runs in the chain, in the leader's state: shared with the others at the first level begin

    mmf_odom* model(unsigned m) const { return batch ? batch->o[m] : o; }
};
static ChainCall odom_chain_call(mmf_odom* o, const TrackMode& tm, const TrackBatch* batch, float* icp_err, float* rgb_err) {
    ChainCall x;
    x.o = o, x.batch = batch, x.tm = tm;
    x.ny = batch ? (unsigned)batch->n : 1u;
    std::memset(&x.bd, 0, sizeof(x.bd));
    std::memset(&x.poses, 0, sizeof(x.poses));
    if (batch) x.bd = batch->bd, x.poses = batch->poses;
    x.icp_err = icp_err, x.rgb_err = rgb_err;
    x.two_launch_once = false;
    for (unsigned m = 0; m < x.ny; ++m) {
        x.two_launch_once = x.two_launch_once || x.model(m)->call.two_launch_once;
        x.model(m)->call.two_launch_once = false;
    }
    x.sparse_on = odom_sparse_on();
    x.lead_sparse = x.sparse_on && o->sparse;
    x.foll_sparse = x.sparse_on && batch && x.ny > 1;
    unsigned foll_gen = x.foll_sparse ? batch->o[1]->prep.extent_gen : 0u;
    for (unsigned m = 1; m < x.ny && x.foll_sparse; ++m) {
        x.foll_sparse = batch->o[m]->sparse;
        if (batch->o[m]->prep.extent_gen != foll_gen) foll_gen = 0u;
    }
    if (!x.foll_sparse) foll_gen = 0u;
    // (the kernels drop the first model's extent in a batch; a sparse model tracked alone keeps its own)
    x.cull_gen = x.ny > 1 ? foll_gen : (x.lead_sparse ? o->prep.extent_gen : 0u);
    x.so3_ran_here = tm.so3 && !o->so3.prefetched;
    return x;
}

// measurement mode 2: the next event pair of o's chain for a launch of `kind` (level * 2 + 0 producer | 1 rgb_step)
static TimedSlot odom_timed_slot(mmf_odom* o, int kind) {
    if (o->timing.mode < 2 || o->timing.n >= kMaxTimedLaunches) return TimedSlot{};
    const int k = o->timing.n++;
    o->timing.kind[k] = kind;
    return TimedSlot{o->timing.ev_kernel[2 * k], o->timing.ev_kernel[2 * k + 1]};
}

// What a chain leaves to odom_chain_publish.
struct ChainTail {
    bool end_folded = false;     // odom_end ran in the finishing lane of the frame's last rgb_step (or in gn_final_kernel)
    bool final_pending = false;  // the one-launch chain's last solve (final_args) shares a launch with the hand-over
    GnIterArgs final_args;
};

// begin: the derivatives (unless the batched preparation wrote them), odom_begin_kernel (unless it rode the preparation:
// odom_begin_rider), the SO3 loop (:239-310)
static int odom_chain_begin(const ChainCall& x, const float trans[3], const float rot[9], bool one_launch, Enqueuer& q) {
    mmf_odom* o = x.o;
    mmf_ctx* c = o->ctx;
    if (x.tm.rgb && !o->in.prep_batched)
        for (int i = 0; i < MMF_NUM_PYRS; ++i) {  // :230-235
            int rc = launch_derivative(c, o->next_image[i], o->width >> i, o->width >> i, o->height >> i, o->dIdx[i],
                                       o->width >> i, o->dIdy[i], o->width >> i);
            if (rc) return rc;
        }
    const BeginArgs b = odom_begin_args(o, trans, rot, x.tm, o->so3.prefetched, o->so3.stage, one_launch);
    o->timing.n = 0;
    if (o->timing.mode) MMF_HIP_TRY(hipEventRecord(o->timing.ev_chain[0], c->stream));
    // from here to the last step: kernels only, enqueued one by one in call order (Enqueuer keeps the first error)
    // (the beginning may have run already, on the last launch of the preparation enqueued ahead of this frame: odom_begin_rider)
    const bool begun = o->spec.valid && o->spec.ok && !x.batch && std::memcmp(&b, &o->spec.args, sizeof(b)) == 0;
    o->spec.valid = o->spec.ok = false;
    if (!begun)
        q.launch(odom_begin_kernel, dim3(x.ny), dim3(64), o->state, b, x.bd, x.poses);
    else
        odom_begin_rider_used();
    o->so3.retry_prefetched = o->so3.prefetched, o->so3.retry_stage = o->so3.stage;  // (odom_retrack_prepare)
    if (x.so3_ran_here) {
        int rc = odom_enqueue_so3(o, q);
        if (rc) return rc;
    }
    o->so3.prefetched = false;
    o->so3.stage = nullptr;
    return MMF_OK;
}

// both terms on and every level fits: ONE launch per iteration (gn_fused.hpp) instead of producer + step, at the plan's
// geometry.  (More than three models: the batched two-launch chain is as fast (four) or faster -- 8 models 1.40 ms against
// 1.60 -- because a model's workgroups hold their CUs at the count barrier while the next models' wait for a place.)
static int odom_one_launch_chain(const ChainCall& x, const GnChainPlan& plan, Enqueuer& q, ChainTail* tail, bool truncated = false) {
    mmf_odom* o = x.o;
    GnIterArgs a;
    std::memset(&a, 0, sizeof(a));
    a.poll_sleep = tunables().gn_sleep;
    a.max_polls = kGnMaxPolls;
    a.check_sparse = g_sparse_check.load();
    bool force_fault = false;
    for (int n = g_gn_force_fault.load(); n > 0 && !force_fault;) force_fault = g_gn_force_fault.compare_exchange_weak(n, n - 1);
    int it = 0;
    for (int i = x.tm.first_iter_level; i >= 0; --i) {
        const LevelArgs l = odom_level_args(o, i, nullptr, nullptr);
        LevelArgs last = l;  // the last level-0 iteration also writes the error images
        last.ra.err_map = x.rgb_err, last.ia.err_map = x.icp_err;
        if (!o->in.prep_batched) {  // :332-334
            MMF_HIP_TRY(q.flush());
            int rc = launch_project(o->ctx, o->last_depth[i], l.cols, l.cols, l.rows, l.in, o->cloud[i], o->cloud4[i]);
            if (rc) return rc;
        }
        if (i == x.tm.first_iter_level && x.so3_ran_here)  // the SO3 loop ran in between: seed resultRt from its result now
            q.launch(gn_level_begin_kernel, dim3(x.ny), dim3(64), o->state, 1, l.in, x.bd, 1);
        const GnGeometry& geo = plan.geo[i];
        a.lanes = geo.lanes;
        a.cloud4 = reinterpret_cast<const float4*>(o->cloud4[i]);
        a.fx = l.in.fx, a.fy = l.in.fy, a.sobel_scale = o->sobel_scale;
        a.intr = l.in;
        a.ifx = 1.0 / (double)l.in.fx, a.ify = 1.0 / (double)l.in.fy;
        // object models walked by their extents: one one-dimensional grid, a geometry per model (GnBatchGeom)
        GnBatchGeom gg;
        std::memset(&gg, 0, sizeof(gg));
        if (plan.mixed) {
            for (unsigned m = 0; m < (unsigned)kMaxBatch; ++m) gg.start[m + 1] = gg.start[m] + (m < x.ny ? plan.groups[i][m] : 0);
            gg.sparse_mask = plan.sparse_mask, gg.ext_gen = plan.ext_gen, gg.level = i, gg.extent = o->extent;
            gg.sensor = o->extent, gg.sensor_gen = o->prep.sensor_gen, gg.sensor_cutoff = o->prep.sensor_cutoff;
            gg.rotate = gg.start[1];  // the object models' workgroups first (the first model of a batch is the camera model)
        }
        for (int j = 0; j < x.tm.iterations[i]; ++j) {
            const bool last_l0 = (i == 0 && j == x.tm.iterations[i] - 1);
            a.ra = last_l0 ? last.ra : l.ra;
            a.ia = last_l0 ? last.ia : l.ia;
            a.it = it;
            a.max_polls = (it == 2 && force_fault) ? 0 : kGnMaxPolls;
            const bool err = last_l0 && (x.icp_err || x.rgb_err);
            const TimedSlot slot = odom_timed_slot(o, i * 2);
            with_gn_px(geo.px, [&](auto PX) {
                constexpr int P = decltype(PX)::value;
                if (plan.mixed)
                    q.launch(slot, err ? gn_iter_mixed_kernel<P, true> : gn_iter_mixed_kernel<P, false>, dim3(gg.start[kMaxBatch]),
                             dim3(geo.threads), o->state, a, x.bd, gg);
                else
                    q.launch(slot, err ? gn_iter_kernel<P, true> : gn_iter_kernel<P, false>, dim3(geo.groups, x.ny), dim3(geo.threads),
                             o->state, a, x.bd);
            });
            ++it;
        }
    }
    if (truncated) {  // (mmf_debug_gn_truncate) no solve behind the last launch: its sums and the pose it ran with, then the frame's end
        tail->end_folded = true;
        a.it = it;
        a.intr = odom_level(o, x.tm.first_iter_level).in;  // the level the launches ran at (the loop went on to level 0)
        a.ifx = 1.0 / (double)a.intr.fx, a.ify = 1.0 / (double)a.intr.fy;
        q.launch(gn_truncated_final_kernel, dim3(1), dim3(64), o->state, a, o->gn_truncated);
        return MMF_OK;
    }
    // the last solve + RGBDOdometry.cpp:464-467: one workgroup per model
    a.it = it;
    a.intr = odom_level(o, 0).in;
    a.ifx = 1.0 / (double)a.intr.fx, a.ify = 1.0 / (double)a.intr.fy;
    tail->end_folded = true;
    // the chain's last solve shares a launch with the hand-over of the result to the host (odom_chain_publish), unless the
    // chain is being timed as such (its closing event lies between the two)
    if (o->timing.mode)
        q.launch(gn_final_kernel, dim3(x.ny), dim3(kBlock), o->state, a, x.bd);
    else
        tail->final_pending = true, tail->final_args = a;
    return MMF_OK;
}

// producer (ICP reduction + correspondence pass, or the two apart) + rgb_step per iteration
static int odom_two_launch_chain(const ChainCall& x, Enqueuer& q, ChainTail* tail) {
    mmf_odom* o = x.o;
    const TrackMode& tm = x.tm;
    auto quarter = [](int full) { return std::max(std::min(full, 32), (full + 3) / 4); };
    bool begin_folded = !x.so3_ran_here;  // this level's gn_level_begin already ran (in odom_begin_kernel, or in the
                                          // last rgb_step of the level before)
    for (int i = MMF_NUM_PYRS - 1; i >= 0; --i) {
        const bool first_level = i == MMF_NUM_PYRS - 1;
        const auto [cols, rows, in] = odom_level(o, i);
        if (tm.rgb && !o->in.prep_batched) {  // :332-334
            MMF_HIP_TRY(q.flush());
            int rc = launch_project(o->ctx, o->last_depth[i], cols, cols, rows, in, o->cloud[i], o->cloud4[i]);
            if (rc) return rc;
        }
        if (!begin_folded)
            q.launch(gn_level_begin_kernel, dim3(x.ny), dim3(64), o->state, first_level ? 1 : 0, in, x.bd,
                     (first_level && x.so3_ran_here) ? 1 : 0);
        begin_folded = false;
        if (!tm.iterations[i]) continue;

        LevelArgs l = odom_level_args(o, i, nullptr, nullptr);
        l.ra.extent = x.cull_gen ? o->extent : nullptr, l.ra.extent_gen = x.cull_gen, l.ra.extent_level = i;
        LevelArgs last = l;  // the last level-0 iteration also writes the error images
        last.ra.err_map = x.rgb_err, last.ia.err_map = x.icp_err;
        RgbStepArgs step;  // :418-423, then :425-460 in the finishing workgroup
        step.residual_partials = o->gn_partials_res;
        step.icp_partials = o->gn_partials_icp;
        step.corres = o->corres[i];
        step.cloud = nullptr, step.cloud4 = reinterpret_cast<const float4*>(o->cloud4[i]);
        step.fx = in.fx;
        step.fy = in.fy;
        step.dIdx = o->dIdx[i];
        step.dIdy = o->dIdy[i];
        step.d_stride = cols;
        step.sobel_scale = o->sobel_scale;
        step.cols = cols;
        step.rows = rows;
        step.cols_magic = l.ra.cols_magic;
        step.extent = l.ra.extent, step.extent_gen = l.ra.extent_gen, step.extent_level = l.ra.extent_level;

        for (int j = 0; j < tm.iterations[i]; ++j) {
            const bool last_l0 = (i == 0 && j == tm.iterations[i] - 1);
            const RgbResidualArgs& ra = last_l0 ? last.ra : l.ra;
            const IcpArgs& ia = last_l0 ? last.ia : l.ia;
            const bool res_vec4 = tm.rgb && residual_vec4_ok(ra);
            int res_records = tm.rgb ? reduce_grid(cols * rows, res_vec4 ? kBlock * 4 : kBlock) : 0, icp_records = 0;
            const int ipx = tm.icp ? std::min(2, icp_max_px(ia, 2)) : 1;
            ChainGeom geom;
            std::memset(&geom, 0, sizeof(geom));
            const bool fuse_producers = tm.rgb && tm.icp && res_vec4 && icp2_fits(ia, kBlock, ipx);
            if (fuse_producers) {  // ICP reduction + correspondence pass side by side in one launch
                icp_records = (cols * rows + kBlock * ipx - 1) / (kBlock * ipx);
                if (x.lead_sparse)  // (every model of this launch, then)
                    res_records = quarter(res_records);
                else if (x.foll_sparse)
                    geom.res_f = (unsigned)quarter(res_records);
                q.launch(odom_timed_slot(o, i * 2), ipx == 2 ? track_producer_kernel<2, true> : track_producer_kernel<1, true>,
                         dim3(icp_records + res_records, x.ny), dim3(kBlock), o->state, ia, (unsigned)icp_records, ra,
                         o->gn_partials_icp, o->gn_partials_res, x.bd, geom);
            } else {
                MMF_REQUIRE(x.ny == 1, "odom_enqueue_tracking: this level cannot be batched");
                if (tm.rgb)
                    q.launch(res_vec4 ? rgb_residual_kernel<FINISH_GN, 4> : rgb_residual_kernel<FINISH_GN, 1>, dim3(res_records),
                             dim3(kBlock), o->state, ra, o->gn_partials_res);
                if (tm.icp) {  // :403-410
                    icp_records = launch_icp<FINISH_GN>(q, o->state, ia, o->gn_partials_icp);
                    if (!tm.rgb)  // ICP-only tracking: one workgroup sums the records, solves, updates the pose
                        q.launch(icp_finish_kernel<FINISH_GN>, dim3(1), dim3(256), o->state, o->gn_partials_icp,
                                 (unsigned)icp_records, in);
                }
            }
            if (!tm.rgb) continue;
            RgbStepArgs a = step;
            a.residual_records = (unsigned)res_records;
            a.icp_records = (unsigned)icp_records;
            a.intr = in;
            // the last step of a level also does the next level's gn_level_begin (one launch less per
            // level).  Not with rgbOnly: its divergence `break` skips the finishing lane.
            a.next_level = 0;
            a.final_step = (last_l0 && !tm.rgb_only) ? 1 : 0;  // odom_end in the finishing lane (which rgbOnly's `break` skips)
            tail->end_folded = a.final_step != 0;
            if (j == tm.iterations[i] - 1 && i > 0 && tm.iterations[i - 1] > 0 && !tm.rgb_only) {
                a.next_level = 1;
                a.intr = odom_level(o, i - 1).in;  // only read by the finishing lane's rgb_prepare
                begin_folded = true;
            }
            int grid = reduce_grid(cols * rows, kBlock * 4);  // width, height are multiples of 4
            if (fuse_producers && x.lead_sparse)
                grid = quarter(grid);
            else if (fuse_producers && x.foll_sparse)
                geom.step_f = (unsigned)quarter(grid);
            // (the 4-pixel correspondence pass wrote compact records)
            q.launch(odom_timed_slot(o, i * 2 + 1), res_vec4 ? rgb_step_kernel<FINISH_GN, 4, true> : rgb_step_kernel<FINISH_GN, 4, false>,
                     dim3(grid, x.ny), dim3(kBlock), o->state, a, o->gn_partials_f, o->gn_ticket, x.bd, geom);
        }
    }
    return MMF_OK;
}

// publish: the end kernel, every model's result towards the host on the chain's stream, the image ring
static int odom_chain_publish(const ChainCall& x, Enqueuer& q, const ChainTail& tail) {
    mmf_odom* o = x.o;
    if (!tail.end_folded) q.launch(odom_end_kernel, dim3(x.ny), dim3(64), o->state, x.bd);
    MMF_HIP_TRY(q.flush());
    if (o->timing.mode) MMF_HIP_TRY(hipEventRecord(o->timing.ev_chain[1], o->ctx->stream));
    PublishTargets to;
    std::memset(&to, 0, sizeof(to));
    const unsigned seq = ++o->call.publish_seq;
    for (unsigned m = 0; m < x.ny; ++m) {
        mmf_odom* om = x.model(m);
        to.host[m] = om->host_result_dev;
        om->call.publish_seq = seq;
        // a follower of a batch takes the LEADER's counter: whatever its own earlier chains left in the pinned flag, it is not
        // this chain's number before this chain has written it
        om->host_result->publish_seq = ~seq;
        om->call.pending_icp = x.tm.icp, om->call.pending_so3 = x.tm.so3;
        om->call.track_stream = o->ctx->stream;
        om->call.result_of = o;
        if (om != o) om->so3.prefetched = false;
        // the image ring (:469-473).  Host bookkeeping only -- the launches above hold their pointers by value -- and
        // done here rather than when the result is picked up, so that the next frame's sensor-side preparation can be
        // enqueued while this chain runs
        if (x.tm.so3)
            for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(om->last_next_image[i], om->next_image[i]);
    }
    o->rider = FrameRider();
    if (tail.final_pending && o->defer_publish && x.ny == 1) {
        q.launch(gn_final_kernel, dim3(x.ny), dim3(kBlock), o->state, tail.final_args, x.bd);
        o->rider.st = o->state, o->rider.host = o->host_result_dev, o->rider.seq = seq;
    } else if (tail.final_pending) {
        q.launch(gn_final_publish_kernel, dim3(x.ny), dim3(kBlock), o->state, tail.final_args, x.bd, to, seq);
    } else {
        q.launch(odom_publish_kernel, dim3(x.ny), dim3(128), o->state, to, seq, x.bd);
    }
    MMF_HIP_TRY(q.flush());
    return MMF_OK;
}

static int odom_enqueue_tracking(mmf_odom* o, const float trans[3], const float rot[9], const TrackMode& tm, float* icp_err_dev,
                                 float* rgb_err_dev, const TrackBatch* batch = nullptr) {
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
#ifdef MMF_STAMPS  // (diagnostic builds: MMF_DBG_NO_ERR=1 leaves the error images out, so that a chain's last launch is an ordinary one)
    if (std::getenv("MMF_DBG_NO_ERR")) icp_err_dev = rgb_err_dev = nullptr;
#endif
    MMF_REQUIRE(!batch || batch->n == 1 || odom_batchable(o, tm), "odom_enqueue_tracking: not batchable");
    TrackMode tmx = tm;
    const int truncate = g_gn_truncate.exchange(0);
    if (truncate) {  // (mmf_debug_gn_truncate) n launches at one level
        for (int i = 0; i < MMF_NUM_PYRS; ++i) tmx.iterations[i] = 0;
        tmx.first_iter_level = truncate & 0xFF;
        tmx.iterations[tmx.first_iter_level] = truncate >> 8;
    }
    const ChainCall x = odom_chain_call(o, tmx, batch, icp_err_dev, rgb_err_dev);
    const GnChainPlan plan = x.two_launch_once ? GnChainPlan() : odom_plan_chain(o, tmx, batch, x.sparse_on);
    MMF_REQUIRE(!truncate || (plan.one_launch && x.ny == 1), "odom_enqueue_tracking: a truncated chain needs the one-launch chain of one model");
    if (truncate && !o->gn_truncated) {
        MMF_HIP_TRY(hipMalloc(&o->gn_truncated, sizeof(GnTruncated)));
        MMF_HIP_TRY(hipMemset(o->gn_truncated, 0, sizeof(GnTruncated)));
    }
    for (unsigned m = 0; m < x.ny; ++m) x.model(m)->call.walked_by_extent = plan.one_launch && ((plan.sparse_mask >> m) & 1u) != 0;
    Enqueuer q(o->ctx->stream);
    ChainTail tail;
    int rc = odom_chain_begin(x, trans, rot, plan.one_launch, q);
    if (rc == MMF_OK) rc = plan.one_launch ? odom_one_launch_chain(x, plan, q, &tail, truncate != 0) : odom_two_launch_chain(x, q, &tail);
    return rc == MMF_OK ? odom_chain_publish(x, q, tail) : rc;
}

// The beginning of the NEXT tracking of one model, to ride the last launch of the preparation that is being enqueued ahead of
// it (track_kernels.hpp: prep_batch_begin_kernel): `pose` = where that tracking will start (the model's pose now), so3_stage =
// the staged pre-alignment of that frame (null: none, the tracking runs it itself).  odom_enqueue_tracking skips its own
// odom_begin_kernel when it is about to pass these very arguments and the caller says the state was left alone (begin_spec_ok).
static Override g_begin_rider;                   // unset: MMF_BEGIN_RIDER decides (default on); 0 / 1: mmf_debug_set_begin_rider
static std::atomic<int> g_begin_riders_used{0};  // chains that found their beginning done (mmf_debug_begin_rider_count)
extern "C" int mmf_debug_set_begin_rider(int on) {
    override_flag(g_begin_rider, on);
    return MMF_OK;
}
extern "C" int mmf_debug_begin_rider_count(void) { return g_begin_riders_used.load(); }
static void odom_begin_rider_used() { g_begin_riders_used.fetch_add(1); }
static bool odom_begin_rider(mmf_odom* o, const float pose[16], const TrackMode& tm, const OdomState* so3_stage, BeginRider* out) {
    o->spec.valid = o->spec.ok = false;
    if (!g_begin_rider.get(tunables().begin_rider) || o->call.two_launch_once) return false;
    const bool one_launch = odom_plan_chain(o, tm, nullptr, odom_sparse_on()).one_launch;
    const float trans[3] = {pose[3], pose[7], pose[11]};
    const float rot[9] = {pose[0], pose[1], pose[2], pose[4], pose[5], pose[6], pose[8], pose[9], pose[10]};
    std::memset(out, 0, sizeof(*out));
    out->st = o->state;
    out->a = odom_begin_args(o, trans, rot, tm, so3_stage != nullptr, so3_stage, one_launch);
    o->spec.args = out->a;
    o->spec.valid = true;
    return true;
}

// second half: wait for the stream, hand the result out
static int odom_finish_tracking(mmf_odom* o, float trans[3], float rot[9]) {
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    // the chain it rode on publishes into this odometry's pinned state and then stores the sequence number
    if (o->call.result_of) {
        const volatile unsigned* flag = &o->host_result->publish_seq;
        bool seen = false;
        const auto t_poll = std::chrono::steady_clock::now();
        while (!seen) {  // a few seconds of polling at most, then the stream says why
            for (int i = 0; i < 4096 && !seen; ++i) seen = *flag == o->call.publish_seq;
            if (seen || std::chrono::steady_clock::now() - t_poll > std::chrono::seconds(5)) break;
        }
        if (!seen) {
            MMF_HIP_TRY(hipStreamSynchronize(o->call.track_stream));
            MMF_REQUIRE(*flag == o->call.publish_seq, "odometry: the tracking result did not reach the host");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        MMF_HIP_TRY(wait_stream(c->stream));
    }
    o->call.track_stream = nullptr, o->call.result_of = nullptr;
    const bool icp = o->call.pending_icp, so3 = o->call.pending_so3;
    if (o->timing.mode) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, o->timing.ev_chain[0], o->timing.ev_chain[1]) == hipSuccess) {
            o->timing.acc.chain_us_sum += ms * 1e3;
            o->timing.acc.chains += 1;
        }
        for (int k = 0; k < o->timing.n; ++k)
            if (hipEventElapsedTime(&ms, o->timing.ev_kernel[2 * k], o->timing.ev_kernel[2 * k + 1]) == hipSuccess) {
                const int lvl = o->timing.kind[k] >> 1, step = o->timing.kind[k] & 1;
                double* sum = step ? o->timing.acc.rgb_step_us_sum : o->timing.acc.producer_us_sum;
                double* mn = step ? o->timing.acc.rgb_step_us_min : o->timing.acc.producer_us_min;
                int* n = step ? o->timing.acc.rgb_step_launches : o->timing.acc.producer_launches;
                sum[lvl] += ms * 1e3;
                if (n[lvl] == 0 || ms * 1e3 < mn[lvl]) mn[lvl] = ms * 1e3;
                n[lvl] += 1;
            }
        o->timing.n = 0;
    }

    const OdomState* r = o->host_result;
    if (o->call.walked_by_extent) std::memcpy(o->gn_need, r->gn_need, sizeof(o->gn_need));  // (valid also when the chain gave up)
    if (r->gn_fault) {  // the one-launch chain gave up: nothing of its result is valid
        o->call.last_gn_fault = r->gn_fault;
        return kGnRetry;
    }
    o->call.last_gn_fault = 0;
    std::memcpy(trans, r->trans_out, sizeof(float) * 3);
    std::memcpy(rot, r->rot_out, sizeof(float) * 9);
    // members the reference leaves untouched in a given mode keep their previous values
    if (icp) {
        o->stats.lastICPError = r->st.lastICPError;
        o->stats.lastICPCount = r->st.lastICPCount;
    }
    o->stats.lastRGBError = r->st.lastRGBError;
    o->stats.lastRGBCount = r->st.lastRGBCount;
    if (so3) {
        o->stats.lastSO3Error = r->st.lastSO3Error;
        o->stats.lastSO3Count = r->st.lastSO3Count;
    }
    if (r->st.iterations_run > 0) {
        std::memcpy(o->stats.lastA, r->st.lastA, sizeof(double) * 36);
        std::memcpy(o->stats.lastb, r->st.lastb, sizeof(double) * 6);
    }
    o->stats.iterations_run = r->st.iterations_run;
    o->stats.so3_iterations_run = r->st.so3_iterations_run;
    return MMF_OK;
}

// A one-launch chain gave up (odom_finish_tracking returned kGnRetry for a model it tracked): the process stops using that
// chain, and every odometry the chain drove is put back to where odom_enqueue_tracking found it -- the image ring (:469-473)
// and the prefetched SO3 pre-alignment it consumed -- so that the same call can be enqueued again and take the two-launch
// chain from the pose the frame started with.  RGBDOdometry.cpp:464-467: the call returns a pose or reverts, it never aborts.
static void odom_retrack_prepare(mmf_odom* const* odoms, int n, int so3) {
    // An object model whose extent did not fit its workgroups (kGnFaultExtent) says nothing about the GPU: this frame is tracked
    // again on the two-launch chain, the model's next chain is sized by what the box needed (odom_finish_tracking has taken
    // OdomState::gn_need over), and the one-launch chain stays in use.
    bool extent_only = true;
    for (int k = 0; k < n; ++k) {
        const int fault = odoms[k]->host_result ? odoms[k]->host_result->gn_fault : 0;
        if (fault != 0 && fault != kGnFaultExtent) extent_only = false;
    }
    if (!extent_only) g_gn_latched_off.store(true);
    g_gn_recoveries.fetch_add(1);
    for (int k = 0; k < n; ++k) {
        mmf_odom* o = odoms[k];
        o->call.two_launch_once = true;
        if (so3)
            for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(o->last_next_image[i], o->next_image[i]);
        o->so3.prefetched = odoms[0]->so3.retry_prefetched, o->so3.stage = odoms[0]->so3.retry_stage;
        o->call.track_stream = nullptr, o->call.result_of = nullptr;
    }
}

extern "C" int mmf_odom_get_incremental_transformation(mmf_odom* o, float trans[3], float rot[9], int rgb_only,
                                                       float icp_weight, int pyramid, int fast_odom, int so3,
                                                       float* icp_err_dev, float* rgb_err_dev) {
    MMF_REQUIRE(o && trans && rot, "mmf_odom_get_incremental_transformation: null argument");
    const float trans0[3] = {trans[0], trans[1], trans[2]};
    float rot0[9];
    std::memcpy(rot0, rot, sizeof(rot0));
    const TrackMode tm = track_mode(rgb_only, icp_weight, pyramid, fast_odom, so3);
    int rc = odom_enqueue_tracking(o, trans, rot, tm, icp_err_dev, rgb_err_dev);
    if (rc) return rc;
    rc = odom_finish_tracking(o, trans, rot);
    if (rc != kGnRetry) return rc;
    odom_retrack_prepare(&o, 1, so3);
    rc = odom_enqueue_tracking(o, trans0, rot0, tm, icp_err_dev, rgb_err_dev);
    if (rc) return rc;
    rc = odom_finish_tracking(o, trans, rot);
    return rc == kGnRetry ? gn_retry_twice() : rc;
}
