// prep_host.hpp -- the host side of the batched frame preparation (prep_batch.hpp): the builder of a stage's jobs, the four
// stages, the collectors of the sensor side and of a model's side, and the test entry that fills them the way the
// orchestrator does.  Textually included by mmf_hip.hip behind odom_host.hpp.
#pragma once

// ---- the whole per-frame preparation in four launches (prep_batch.hpp) -------------------------
static Override g_prep_big;  // unset: MMF_PREP_BIG decides; 0: never; n > 0: that many pixels (mmf_debug_set_prep_big)
extern "C" int mmf_debug_set_prep_big(int n) {
    n < 0 ? g_prep_big.clear() : g_prep_big.set(n);
    return MMF_OK;
}
static size_t prep_big_job() {  // pixels from which a job's workgroups take four tiles each; MMF_PREP_BIG=0: never
    const long n = g_prep_big.get(tunables().prep_big);
    return n < 0 ? (size_t)200000 : (n > 0 ? (size_t)n : ~(size_t)0);
}
struct PrepBuilder {  // the jobs of one stage (possibly of several models); launched kMaxPrepJobs at a time
    std::vector<PrepJob> jobs;
    bool critical = false;  // PrepBatch::critical
    PrepJob& add(int op, int cols, int rows) {
        if (jobs.capacity() < 96) jobs.reserve(96);  // references handed out stay valid while a stage is being filled
        jobs.emplace_back();
        PrepJob& j = jobs.back();
        std::memset(&j, 0, sizeof(j));
        j.op = op;
        j.cols = cols, j.rows = rows;
        j.gx = (cols + kTileX - 1) / kTileX;
        j.reps = (size_t)cols * rows >= prep_big_job() ? 4 : 1;  // (PrepJob::reps)
        return j;
    }
    // rider: the beginning of the tracking these jobs prepare, on one more workgroup of the stage's LAST launch (BeginRider)
    template <int CAP>
    static int fill(PrepBatchT<CAP>& b, const std::vector<PrepJob>& jobs, size_t first, bool critical) {
        b.njobs = 0;
        b.critical = critical ? 1 : 0;
        int blocks = 0;
        for (size_t k = first; k < jobs.size() && b.njobs < CAP; ++k) {
            PrepJob& j = b.job[b.njobs++];
            j = jobs[k];
            j.first_block = blocks;
            blocks += j.rect_now ? j.rect_groups : j.gx * ((j.rows + kTileY * j.reps - 1) / (kTileY * j.reps));
        }
        return blocks;
    }
    int launch(Enqueuer& q, const BeginRider* rider = nullptr) {
        if (jobs.size() > (size_t)kMaxPrepJobs && !rider) {  // several models' jobs: the wide table (prep_batch.hpp)
            for (size_t first = 0; first < jobs.size(); first += kMaxPrepJobsWide) {
                PrepBatchWide b;
                const int blocks = fill(b, jobs, first, critical);
                q.launch(prep_batch_wide_kernel, dim3(blocks), tile_block(), b);
            }
            jobs.clear();
            return MMF_OK;
        }
        for (size_t first = 0; first < jobs.size(); first += kMaxPrepJobs) {
            PrepBatch b;
            const int blocks = fill(b, jobs, first, critical);
            if (rider && first + kMaxPrepJobs >= jobs.size()) {
                BeginRider r = *rider;
                r.prep_blocks = blocks;
                q.launch(prep_batch_begin_kernel, dim3(blocks + 1), tile_block(), b, r);
            } else {
                q.launch(prep_batch_kernel, dim3(blocks), tile_block(), b);
            }
        }
        jobs.clear();
        return MMF_OK;
    }
};
struct PrepStages {  // the four dependent launches of a frame's preparation
    PrepBuilder stage[4];
    void set_critical(bool on) {
        for (PrepBuilder& pb : stage) pb.critical = on;
    }
    int launch(Enqueuer& q, const BeginRider* rider = nullptr) {  // recorded; the caller flushes.  rider: on the last launch
        int last = -1;
        for (int k = 0; k < 4; ++k)
            if (!stage[k].jobs.empty()) last = k;
        for (int k = 0; k < 4; ++k)
            if (int rc = stage[k].launch(q, k == last ? rider : nullptr)) return rc;
        return MMF_OK;
    }
    int launch(hipStream_t stream, const BeginRider* rider = nullptr) {
        Enqueuer q(stream);
        if (int rc = launch(q, rider)) return rc;
        MMF_HIP_TRY(q.flush());
        return MMF_OK;
    }
    bool empty() const {
        for (const PrepBuilder& pb : stage)
            if (!pb.jobs.empty()) return false;
        return true;
    }
};

// Everything initICPModel + initRGBModel + generateCUDATextures/initICP + initRGB + the gradient and
// point-cloud passes of getIncrementalTransformation compute (RGBDOdometry.cpp:108-235, 332-334;
// Model.cpp:359-407), for inputs that stay untouched until tracking returns (the native orchestrator).
// The jobs split into those that depend only on the NEW sensor frame (filtered depth, RGB: vertex / normal maps, depth
// and intensity pyramids, gradients: prep_collect_sensor) and those that depend on the model's prediction and pose
// (prep_collect_model).  The orchestrator can run the first group for frame t+1 on a second stream while frame t is still
// being fused (mmf_fusion_prefetch_frame); PREP_ALL is both groups in the same four launches (prep_collect_all).
// Which stage a job goes to, and where in it, is fixed (prep_batch.hpp: the one arrangement): a stage's list of jobs decides
// which workgroup of the launch does what.
enum PrepSide { PREP_INPUT_IMAGE = 1, PREP_INPUT_DEPTH = 2, PREP_MODEL_SIDE = 4, PREP_ALL = 7 };

struct PrepSensorFrame {  // what the sensor side reads
    const float* depth_filtered = nullptr;  // the depth side's input
    float depth_cutoff = 0.f;
    const uint8_t* rgb = nullptr;  // the image side's input: interleaved, `channels` bytes per pixel
    int channels = 3;
};
struct PrepPrediction {  // what the model side reads: a model's prediction and the pose it is tracked from
    const float *vertex = nullptr, *normal = nullptr;  // RGBA32F
    const uint8_t* image = nullptr;
    int channels = 4;
    const float* pose = nullptr;      // row-major 4 x 4
    const float* depth_l0 = nullptr;  // the frame's filtered depth, which the model's chain reads as level 0 of the depth pyramid
    // optional device-side choice of the sources (PrepJob::sel): the alt_* images instead when *sel != 0 or, with sel_total
    // != 0, when fewer than sel_ratio of the sel_total thumbnail samples are covered
    const int* sel = nullptr;
    const float *alt_vertex = nullptr, *alt_normal = nullptr;
    const uint8_t* alt_image = nullptr;
    int sel_total = 0;
    float sel_ratio = 0.f;
    unsigned ext_gen = 0;  // != 0: the jobs that write the model's depth and vertex pyramids note the extent of what is valid (extent.hpp)
    // (device, level-0 pixels {x0, y0, x1, y1}; an OBJECT model prepared on its own only): where the prediction's images are
    // non-zero -- the jobs then cover the hull of that box and of the one the previous preparation saw (PrepJob::rect_*)
    const int* pred_box = nullptr;
};

static Override g_prep_rect;  // unset: MMF_PREP_RECT decides (default on); 0 / 1: mmf_debug_set_prep_rect
extern "C" int mmf_debug_set_prep_rect(int on) {
    override_flag(g_prep_rect, on);
    return MMF_OK;
}

static void prep_intr_f(PrepJob& j, const mmf_odom* o, int lvl) {  // f = {1/fx, 1/fy, cx, cy} of a level
    const LevelIntr in = odom_level(o, lvl).in;
    j.f[0] = 1.f / in.fx, j.f[1] = 1.f / in.fy, j.f[2] = in.cx, j.f[3] = in.cy;
}
static void prep_pose_f(PrepJob& j, const float pose[16]) {  // f = {R[9], t[3]}
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) j.f[3 * r + q] = pose[4 * r + q];
        j.f[9 + r] = pose[4 * r + 3];
    }
}
static PrepJob& prep_pyr_step(PrepBuilder& pb, const mmf_odom* o, int op, const void* src, void* dst, int lvl) {  // level lvl-1 -> lvl
    PrepJob& j = pb.add(op, o->width >> lvl, o->height >> lvl);
    j.src0 = src, j.dst0 = dst;
    j.scols = o->width >> (lvl - 1), j.srows = o->height >> (lvl - 1);
    return j;
}
// the fill-in images a model-side job reads instead of the prediction's when the device says so (PrepPrediction::sel)
static void prep_alt(PrepJob& j, const PrepPrediction& p, const void* alt0, const void* alt1 = nullptr) {
    j.sel = p.sel, j.alt0 = alt0, j.alt1 = alt1;
    if (p.sel && p.sel_total) j.sel_total = p.sel_total, j.sel_ratio = p.sel_ratio;  // *sel is a count (PrepJob::sel_total)
}

// depth side: stage k makes level k's vertex and normal maps and level k+1 of the depth pyramid -- three dependent launches
static void prep_depth_jobs(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr) {
    const float* depth[MMF_NUM_PYRS] = {fr.depth_filtered, o->depth_pyr[1], o->depth_pyr[2]};
    for (int lvl = 0; lvl < MMF_NUM_PYRS; ++lvl) {
        PrepBuilder& pb = stages.stage[lvl];
        if (lvl + 1 < MMF_NUM_PYRS) prep_pyr_step(pb, o, PREP_PYRDOWN_F, depth[lvl], o->depth_pyr[lvl + 1], lvl + 1);
        PrepJob& j = pb.add(PREP_VMAP_NMAP, o->width >> lvl, o->height >> lvl);
        j.src0 = depth[lvl], j.dst0 = o->vmaps_curr[lvl], j.dst1 = o->nmaps_curr[lvl];
        prep_intr_f(j, o, lvl);
        j.f[4] = fr.depth_cutoff;
        if (lvl == 0) {  // (extent.hpp: the sensor frame's smallest valid depth, for the object models' error-image launches)
            j.zmin = o->extent, j.zmin_gen = ++o->prep.sensor_gen;
            o->prep.sensor_cutoff = fr.depth_cutoff;
        }
    }
}
// image side: the intensity image in stage 0, then stage k+1 makes level k's gradients and level k+1 of the pyramid -- four
static void prep_image_jobs(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr) {
    PrepJob& in = stages.stage[0].add(PREP_INTENSITY, o->width, o->height);
    in.src0 = fr.rgb, in.dst0 = o->next_image[0], in.scols = o->width * fr.channels, in.channels = fr.channels;
    for (int lvl = 0; lvl < MMF_NUM_PYRS; ++lvl) {
        PrepBuilder& pb = stages.stage[lvl + 1];
        PrepJob& d = pb.add(PREP_DERIV, o->width >> lvl, o->height >> lvl);
        d.src0 = o->next_image[lvl], d.dst0 = o->grad_w_dx[lvl], d.dst1 = o->grad_w_dy[lvl];  // (odom_adopt_gradients)
        if (lvl + 1 < MMF_NUM_PYRS) prep_pyr_step(pb, o, PREP_PYRDOWN_U8, o->next_image[lvl], o->next_image[lvl + 1], lvl + 1);
    }
    o->prep.grad_pending = true;
}
static void prep_collect_sensor(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr, int sides) {
    if (sides & PREP_INPUT_DEPTH) prep_depth_jobs(stages, o, fr);
    if (sides & PREP_INPUT_IMAGE) prep_image_jobs(stages, o, fr);
}

// Model side, two dependent launches (stages 1 and 2).  Level 1 of the camera-frame model maps (before the transform into
// the global frame) is the one thing a job stores for another: it lives behind level 0's place in the two 4*N-float staging
// images, which this path does not need as copies.
static float* prep_level1_of(float* staging, const mmf_odom* o) { return staging + 3 * (size_t)o->width * o->height; }
// ... what is made from a level's images: the packed records and the point records of levels 0 and 1, level 0's depth and
// intensity.  Nothing of the preparation reads level 0's, which come straight from the prediction: l0_stage is 2, beside the
// small jobs of levels 1 and 2, so that the first launch is the three quarter-size pyramid jobs alone (1: with a sensor side
// in the same launches)
static void prep_model_level_jobs(PrepStages& stages, mmf_odom* o, const PrepPrediction& p, int l0_stage) {
    const int W = o->width, H = o->height;
    {
        PrepBuilder& pb = stages.stage[l0_stage];
        PrepJob& t = pb.add(PREP_TEX_TP, W, H);
        t.src0 = p.vertex, t.src1 = p.normal, t.dst2 = o->prev_packed[0];
        prep_alt(t, p, p.alt_vertex, p.alt_normal);
        prep_pose_f(t, p.pose);
        if (p.ext_gen) t.aabb = o->extent, t.ext_gen = p.ext_gen;  // (extent.hpp: the pixel box and depth range of the valid vertices)
        PrepJob& c = pb.add(PREP_TEX_PROJECT, W, H);
        c.src0 = p.vertex, c.dst1 = o->cloud4[0], c.dst2 = o->last_depth[0];
        prep_alt(c, p, p.alt_vertex);
        prep_intr_f(c, o, 0);
        c.f[4] = o->max_depth_rgb;
        if (p.ext_gen) c.ext = o->extent, c.ext_gen = p.ext_gen;  // (the depth jobs: extent.hpp, extent_of_level)
        PrepJob& il = pb.add(PREP_INTENSITY, W, H);
        il.src0 = p.image, il.dst0 = o->last_image[0], il.scols = W * p.channels, il.channels = p.channels;
        prep_alt(il, p, p.alt_image);
    }
    {
        PrepBuilder& pb = stages.stage[2];
        PrepJob& t = pb.add(PREP_TRANSFORM_PACK, W >> 1, H >> 1);
        t.src0 = prep_level1_of(o->vmaps_tmp, o), t.src1 = prep_level1_of(o->nmaps_tmp, o), t.dst2 = o->prev_packed[1];
        prep_pose_f(t, p.pose);
        PrepJob& c = pb.add(PREP_PROJECT, W >> 1, H >> 1);
        c.src0 = o->last_depth[1], c.dst1 = o->cloud4[1];
        prep_intr_f(c, o, 1);
    }
}
// ... and the pyramid steps: level 1 from the prediction's images, level 2 -- with its records, in the same job -- from level 1
static void prep_model_pyramid_jobs(PrepStages& stages, mmf_odom* o, const PrepPrediction& p) {
    const int W = o->width, H = o->height;
    {
        PrepBuilder& pb = stages.stage[1];
        PrepJob& d = pb.add(PREP_TEX_PYR_F, W >> 1, H >> 1);
        d.src0 = p.vertex, d.scols = W, d.srows = H, d.dst0 = o->last_depth[1], d.f[0] = o->max_depth_rgb;
        prep_alt(d, p, p.alt_vertex);
        if (p.ext_gen) d.ext = o->extent + 4, d.ext_gen = p.ext_gen;
        PrepJob& u = pb.add(PREP_TEX_PYR_U8, W >> 1, H >> 1);
        u.src0 = p.image, u.scols = W, u.srows = H, u.channels = p.channels, u.dst0 = o->last_image[1];
        prep_alt(u, p, p.alt_image);
        PrepJob& r = pb.add(PREP_TEX_RESIZE, W >> 1, H >> 1);
        r.src0 = p.vertex, r.src1 = p.normal, r.scols = W, r.srows = H;
        r.dst0 = prep_level1_of(o->vmaps_tmp, o), r.dst1 = prep_level1_of(o->nmaps_tmp, o);
        prep_alt(r, p, p.alt_vertex, p.alt_normal);
    }
    {
        PrepBuilder& pb = stages.stage[2];
        prep_pyr_step(pb, o, PREP_PYRDOWN_U8, o->last_image[1], o->last_image[2], 2);
        PrepJob& t = prep_pyr_step(pb, o, PREP_RESIZE_TP, prep_level1_of(o->vmaps_tmp, o), nullptr, 2);
        t.src1 = prep_level1_of(o->nmaps_tmp, o), t.dst2 = o->prev_packed[2];
        prep_pose_f(t, p.pose);
        PrepJob& c = prep_pyr_step(pb, o, PREP_PYR_PROJECT, o->last_depth[1], nullptr, 2);
        c.dst1 = o->cloud4[2], c.dst2 = o->last_depth[2];
        prep_intr_f(c, o, 2);
        if (p.ext_gen) c.ext = o->extent + 8, c.ext_gen = p.ext_gen;
    }
}
// what the odometry remembers of a model-side preparation.  from (null: not boxed): the jobs of `stages` from these counts
// on are this preparation's, and they cover the prediction's box only (PrepPrediction::pred_box)
static void prep_model_done(PrepStages& stages, mmf_odom* o, const PrepPrediction& p, const size_t* from) {
    o->in.depth_l0 = p.depth_l0;
    o->in.vtmp = p.vertex, o->in.ntmp = p.normal;
    o->in.have_tmp = true;
    o->prep.extent_gen = p.ext_gen;
    if (from) {
        const unsigned g = ++o->prep.gen;
        const int* prev = o->prep.box_known ? o->prep.box + 4 * ((g + 1u) & 1u) : nullptr;
        bool first = true;
        for (int k = 0; k < 4; ++k)
            for (size_t q = from[k]; q < stages.stage[k].jobs.size(); ++q) {
                PrepJob& j = stages.stage[k].jobs[q];
                int lvl = 0;
                while ((o->width >> lvl) > j.cols && lvl < MMF_NUM_PYRS - 1) ++lvl;
                j.rect_now = p.pred_box, j.rect_prev = prev;
                j.rect_level = lvl;
                j.rect_groups = lvl == 0 ? 48 : (lvl == 1 ? 32 : 16);
                j.rect_store = first ? o->prep.box + 4 * (g & 1u) : nullptr;
                first = false;
            }
    }
    o->prep.box_known = from != nullptr;
    o->in.prep_batched = true;
}
static void prep_collect_model(PrepStages& stages, mmf_odom* o, const PrepPrediction& p) {
    const bool rect_on = g_prep_rect.get(tunables().prep_rect) != 0;
    const bool boxed = p.pred_box != nullptr && p.sel == nullptr && rect_on && o->prep.box != nullptr;
    size_t from[4];
    for (int k = 0; k < 4; ++k) from[k] = stages.stage[k].jobs.size();
    prep_model_level_jobs(stages, o, p, 2);
    prep_model_pyramid_jobs(stages, o, p);
    prep_model_done(stages, o, p, boxed ? from : nullptr);
}
// One model and a sensor side not prepared ahead: both in the same four launches.  Within a stage: the depth side's jobs, what
// the model makes from a level's images, the image side's jobs, the model's pyramid steps.
static void prep_collect_all(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr, const PrepPrediction& p) {
    prep_depth_jobs(stages, o, fr);
    prep_model_level_jobs(stages, o, p, 1);
    prep_image_jobs(stages, o, fr);
    prep_model_pyramid_jobs(stages, o, p);
    prep_model_done(stages, o, p, nullptr);
}
// the gradients the batched preparation wrote last become the ones the chain reads
static void odom_adopt_gradients(mmf_odom* o) {
    if (!o->prep.grad_pending) return;
    o->prep.grad_pending = false;
    for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(o->dIdx[i], o->grad_w_dx[i]), std::swap(o->dIdy[i], o->grad_w_dy[i]);
}

// one or both halves of a sensor frame's side, as launches of their own: recorded in q (the caller flushes) or on the context's stream
static int odom_prepare_sensor(mmf_odom* o, const PrepSensorFrame& fr, int sides, Enqueuer* q = nullptr) {
    PrepStages stages;
    prep_collect_sensor(stages, o, fr, sides);
    return q ? stages.launch(*q) : stages.launch(o->ctx->stream);
}

// Test entry: the batched preparation of n stand-alone odometries as ONE set of stages, filled the way the orchestrator fills
// them (fusion_orchestrator.hpp: fusion_collect_prep) -- host plumbing around the collectors above, no kernel of its own.
extern "C" int mmf_debug_odom_prepare(mmf_odom* const* odoms, const mmf_debug_prep_prediction* preds, int n, const float* depth_filtered,
                                      float depth_cutoff, const unsigned char* rgb, int rgb_channels, int sides) {
    MMF_REQUIRE(odoms && preds && n >= 1, "mmf_debug_odom_prepare: null argument, or no odometry");
    const bool sensor = depth_filtered != nullptr || rgb != nullptr;
    MMF_REQUIRE(!sensor || (sides & ~(PREP_INPUT_IMAGE | PREP_INPUT_DEPTH)) == 0, "mmf_debug_odom_prepare: sides is a mask of 1 (image) and 2 (depth)");
    MMF_REQUIRE(!sensor || (((sides & PREP_INPUT_DEPTH) == 0 || depth_filtered) && ((sides & PREP_INPUT_IMAGE) == 0 || rgb)),
                "mmf_debug_odom_prepare: a side is asked for without its input");
    MMF_REQUIRE(!sensor || (sides & PREP_INPUT_IMAGE) == 0 || rgb_channels == 3 || rgb_channels == 4, "mmf_debug_odom_prepare: rgb_channels must be 3 or 4");
    for (int k = 0; k < n; ++k) {
        const mmf_debug_prep_prediction& d = preds[k];
        MMF_REQUIRE(odoms[k] && odoms[k]->slab && odoms[k]->ctx == odoms[0]->ctx, "mmf_debug_odom_prepare: odometries of one context");
        MMF_REQUIRE(odoms[k]->width == odoms[0]->width && odoms[k]->height == odoms[0]->height, "mmf_debug_odom_prepare: odometries of one size");
        MMF_REQUIRE(d.vertex && d.normal && d.image && d.pose && (d.channels == 3 || d.channels == 4), "mmf_debug_odom_prepare: incomplete prediction");
        MMF_REQUIRE(!d.sel || (d.alt_vertex && d.alt_normal && d.alt_image && d.sel_total >= 0), "mmf_debug_odom_prepare: sel without the alt images");
    }
    mmf_ctx* c = odoms[0]->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    auto prediction = [&](int k) {
        const mmf_debug_prep_prediction& d = preds[k];
        PrepPrediction p;
        p.vertex = d.vertex, p.normal = d.normal, p.image = d.image, p.channels = d.channels, p.pose = d.pose;
        p.depth_l0 = depth_filtered;
        p.sel = d.sel, p.alt_vertex = d.alt_vertex, p.alt_normal = d.alt_normal, p.alt_image = d.alt_image;
        p.sel_total = d.sel_total, p.sel_ratio = d.sel_ratio;
        p.ext_gen = d.ext_gen, p.pred_box = d.pred_box;
        return p;
    };
    PrepSensorFrame fr;
    fr.depth_filtered = depth_filtered, fr.depth_cutoff = depth_cutoff, fr.rgb = rgb, fr.channels = rgb_channels;
    PrepStages stages;
    if (sensor && n == 1 && sides == (PREP_INPUT_IMAGE | PREP_INPUT_DEPTH)) {
        prep_collect_all(stages, odoms[0], fr, prediction(0));
    } else {
        if (sensor) prep_collect_sensor(stages, odoms[0], fr, sides);
        for (int k = 0; k < n; ++k) prep_collect_model(stages, odoms[k], prediction(k));
    }
    if (int rc = stages.launch(c->stream)) return rc;
    for (int k = 0; k < n; ++k) odom_adopt_gradients(odoms[k]);
    return MMF_OK;
}
