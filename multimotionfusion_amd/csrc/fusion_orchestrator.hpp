// fusion_orchestrator.hpp -- MultiMotionFusion::processFrame / predict (Core/MultiMotionFusion.cpp:207-854,
// 863-875) for a list of rigid-body models: the global (camera) model plus the object models the segmentation
// spawns.  Textually included at the end of mmf_hip.hip (it uses that file's static helpers and
// model_host.hpp's enqueuers of the surfel passes), behind the files that hold what a frame works on: the fusion object
// (fusion_state.hpp, over the owners of stream_lane.hpp), the segmentation sources and side engines (fusion_hooks.hpp), the
// keypoint side (fusion_keypoints.hpp), the host-frame ring and the prefetch (fusion_ingest.hpp).  Here: FrameRun, the
// frame_* stages, processFrame and predict.
//
// The segmentation is handed in per frame (mmf_segmentation: the reference's gSLICr + dense CRF), pulled through a
// callback at the point where the reference calls performSegmentation (:412), computed from the frame's raw label image
// (mask_kernels.hpp, mmf_fusion_set_mask_segmentation: the `frame.mask` branch of Segmentation.cpp:89-147, which comes
// first as it does there) or by the built-in dense CRF (crf_kernels.hpp, mmf_fusion_set_crf_segmentation).  Of relocalisation
// the fern keyframe database runs here, off by default and observational (frame_ferns, mmf_fusion_set_fern_database); what
// stays with the caller: pose recovery from a keyframe, loss detection, deformation (closeLoops / reloc off).
//
// MI355X mapping: every model owns a LANE (a child context: its own stream + reduction scratch), so the
// latency-bound Gauss-Newton chains of different models (19 x two small launches each) overlap on the device;
// the chains of all models are enqueued before the first result is awaited.  What depends on the sensor frame
// only (bilateral filter, depth / intensity pyramids, vertex / normal maps, gradients) is computed ONCE on the
// fusion's own stream and aliased by every model's odometry -- the reference shares just the depth pyramid
// (Model::GPUSetup::depth_tmp, Model.h:103) and recomputes the rest per model.
#pragma once

// Model::computeFusionWeight (Model.cpp:876-891)
static float fusion_weight(const float* pose, const float* last_pose, float multiplier) {
    float inv[16];
    inverse4f_host(pose, inv);  // getLastTransform() = getPose().inverse() * lastPose (Model.h:305)
    return mmf::host::compute_fusion_weight(inv, last_pose, multiplier);
}
extern "C" int mmf_compute_fusion_weight(const float pose[16], const float last_pose[16], float multiplier, float* out) {
    MMF_REQUIRE(pose && last_pose && out, "mmf_compute_fusion_weight: null argument");
    *out = fusion_weight(pose, last_pose, multiplier);
    return MMF_OK;
}

// Eigen::Quaternionf(rotation).coeffs() = (x, y, z, w), float32 (Eigen/src/Geometry/Quaternion.h,
// quaternionbase_assign_impl: branch on the trace, else on the largest diagonal element)
static void pose_to_log7(const float* T, float p[7]) {
    p[0] = T[3], p[1] = T[7], p[2] = T[11];
    const float R[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
    float q[4];  // x y z w
    float t = (R[0][0] + R[1][1]) + R[2][2];
    if (t > 0.f) {
        t = std::sqrt(t + 1.0f);
        q[3] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (R[2][1] - R[1][2]) * t;
        q[1] = (R[0][2] - R[2][0]) * t;
        q[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        q[3] = (R[k][j] - R[j][k]) * t;
        q[j] = (R[j][i] + R[i][j]) * t;
        q[k] = (R[k][i] + R[i][k]) * t;
    }
    p[3] = q[0], p[4] = q[1], p[5] = q[2], p[6] = q[3];
}

// every model's odometry reads the sensor-side images of the frame from the primary (global) odometry's buffers
static void odom_alias_sensor_side(mmf_odom* o, const mmf_odom* primary) {
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {
        o->vmaps_curr[i] = primary->vmaps_curr[i], o->nmaps_curr[i] = primary->nmaps_curr[i];
        o->next_image[i] = primary->next_image[i], o->last_next_image[i] = primary->last_next_image[i];
        o->dIdx[i] = primary->dIdx[i], o->dIdy[i] = primary->dIdy[i];
        o->depth_pyr[i] = primary->depth_pyr[i];
    }
    o->in.depth_l0 = primary->in.depth_l0;
}

// where an OBJECT model's latest prediction is non-zero (model_pred_box), for a model-side preparation that may then leave
// the rest of the frame alone; null: unknown, or not such a model
static const int* fusion_pred_box(const FusionModel* fm) {
    return fm->fill_in || !fm->odom->sparse ? nullptr : model_pred_box(fm->model);
}

// Model::combinedPredict(ACTIVE) + Model::performFillIn of one model (the body of predict(), :863-875)
static int fusion_predict_model(mmf_fusion* f, FusionModel* fm) {
    const mmf_fusion_config& g = f->cfg;
    if (fm->fill_in)  // combinedPredict + performFillIn in one pass
        return model_combined_predict(fm->model, g.max_depth_processed, f->tick, f->tick, g.time_delta, f->frame_rgb,
                                      f->depth_filtered, g.frame_to_frame_rgb, /*lost*/ 0);
    return mmf_model_combined_predict(fm->model, g.max_depth_processed, f->tick, f->tick, g.time_delta);
}

// The reference predicts twice per frame: behind the tracking (:675) and at the end (:821).  The first prediction's images
// feed loop closure (closeLoops: ferns, :682, and the model-to-model odometry, :714-760), which does not run inside this
// library; the segmentation (:412) comes before it and reads the previous frame's prediction (as a segmentation callback
// does here), a caller sees the images only between calls, and the fuse / clean passes read their own index maps.  Its images are overwritten by the second prediction before
// anything can read them, so it is not enqueued (bit-identical poses, maps and images: every oracle parity test runs this
// way, and tests/test_gpu_fusion.py compares the two).  mmf_debug_set_mid_predict(1) runs it as the reference does.
static Override g_mid_predict;  // a hook only, no environment switch: unset = off; 0 / 1: mmf_debug_set_mid_predict
extern "C" int mmf_debug_set_mid_predict(int on) {
    override_flag(g_mid_predict, on);
    return MMF_OK;
}
static bool fusion_mid_predict() {
    return g_mid_predict.get(0) != 0;
}

// predictIndices -> fuse -> predictIndices -> clean of one model (:791-816 per model; models never read each
// other's surfels, so running the four passes model by model on the model's own stream gives the same maps as
// the reference's pass-by-pass loops over the list)
static int fusion_fuse_clean_model(mmf_fusion* f, FusionModel* fm, float weighting, bool indices_done = false) {
    const mmf_fusion_config& g = f->cfg;
    int rc = indices_done ? MMF_OK : mmf_model_predict_indices(fm->model, f->tick, g.max_depth_processed, g.time_delta);
    if (rc) return rc;
    // (the fuse's update pass projects the surfels for the predictIndices behind it: MMF_FUSE_INDEX=0 keeps the two apart)
    const bool merged = tunables().fuse_index;
    const IndexArgs ia = model_index_args(fm->model, f->tick, g.max_depth_processed, g.time_delta);
    rc = model_fuse(fm->model, f->tick, f->frame_rgb, f->mask.get(), f->frame_depth, f->depth_filtered, g.max_depth_processed, weighting,
                    merged ? &ia : nullptr);
    if (rc) return rc;
    rc = model_predict_indices(fm->model, f->tick, g.max_depth_processed, g.time_delta, merged);
    if (rc) return rc;
    return mmf_model_clean(fm->model, f->tick, g.time_delta, g.max_depth_processed, f->depth_filtered, f->mask.get(), g.outlier_coeff);
}

// getMaxDepth (:408): float operands, double arithmetic (1.2 is a double literal), returned as float
static float seg_max_depth(const mmf_segmentation_model& d) { return (float)((double)d.depth_mean + (double)d.depth_std * 1.2); }

// test / A-B hook: how the object models' passes go out (fusion_batch_mode)
static Override g_batch_passes;  // unset: MMF_PASS_BATCH / the number of object models decide
extern "C" int mmf_debug_set_pass_batch(int mode) {
    MMF_REQUIRE(mode == -1 || mode == 0 || mode == 2, "mmf_debug_set_pass_batch: mode must be -1, 0 or 2");
    mode < 0 ? g_batch_passes.clear() : g_batch_passes.set(mode);
    return MMF_OK;
}
// 0: model by model; 2: one launch per pass, restricted to where the models are (pass_rect.hpp).  Neither the hook nor
// MMF_PASS_BATCH says: by the number of object models this GPU runs -- model by model on the models' own streams up to three
// of them, restricted launches from four on
// (measured, LABNOTES r5: 8 models 0.69-0.70 against 0.76-0.78 ms, 5 models 0.60-0.62 against 0.65-0.67, 4 models 0.575-0.58
// against 0.55-0.59)
constexpr int kRectPassObjects = 4;
static int fusion_batch_mode(const mmf_fusion* f) {
    const int v = (int)g_batch_passes.get(tunables().pass_batch);
    if (v >= 0) return v;
    int objects = 0;
    for (size_t k = 1; k < f->models.size(); ++k) objects += fusion_owns(f, k) ? 1 : 0;
    return objects >= kRectPassObjects ? 2 : 0;
}
// the boxes of the ids of the frame's id image (pass_rect.hpp: mask_boxes_kernel), on `st`
static int fusion_note_mask_boxes(mmf_fusion* f, hipStream_t st) {
    if (!f->mask_boxes) {
        MMF_HIP_TRY(f->mask_boxes.create(256 * 4));
        MMF_HIP_TRY(hipMemsetAsync(f->mask_boxes.get(), 0, 256 * 4 * sizeof(unsigned long long), st));
    }
    ++f->mask_gen;
    const int tiles = ((f->width + 63) / 64) * ((f->height + 15) / 16);
    hipLaunchKernelGGL(mask_boxes_kernel, dim3(tiles), dim3(256), 0, st, f->mask.get(), f->width, f->height, f->mask_boxes.get(), f->mask_gen);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}
// `st` (the stream a batch of passes goes out on: objs[0]'s) waits for whatever the other models' own streams still hold
// (a stream that has drained holds nothing: no wait is enqueued)
static int fusion_lanes_join(const std::vector<FusionModel*>& objs, hipStream_t st) {
    for (size_t k = 1; k < objs.size(); ++k) {
        hipStream_t ls = objs[k]->lane->stream;
        if (ls == st) continue;
        if (hipStreamQuery(ls) == hipSuccess) continue;
        (void)hipGetLastError();
        MMF_HIP_TRY(order(ls, objs[k]->ev_done.get(), st));
    }
    return MMF_OK;
}

// inactivateModel (:962-981) without the on-disk model database: the model stores its keypoint views (when a view log is
// kept), leaves the active list and keeps its map
static int fusion_inactivate(mmf_fusion* f, FusionModel* fm) {
    int rc = fusion_store_views(f, fm);
    if (rc) return rc;
    f->models.erase(std::find(f->models.begin(), f->models.end(), fm));
    f->inactive.push_back(fm);
    return MMF_OK;
}

// spawnObjectModel (:938-947)
static int fusion_spawn(mmf_fusion* f, FusionModel** out) {
    FusionModel* fm = nullptr;
    if (!f->preallocated.empty()) {
        fm = f->preallocated.front();
        f->preallocated.erase(f->preallocated.begin());
    } else {
        int rc = fusion_model_create(f, fusion_next_model_id(f, true), f->cfg.conf_object_init, 0, true, &fm);
        if (rc) return rc;
    }
    // frameToModel.initFirstRGB(textures[RGB]) (:946): with the shared sensor-side images, the "last" image the new
    // model's SO3 pre-alignment reads next frame IS this frame's intensity pyramid (same kernels, same bits)
    *out = fm;
    return MMF_OK;
}

// ---- processFrame (MultiMotionFusion.cpp:207-854), stage by stage ----------------------------------------------------------
// With several models a frame waits for the thread that enqueues its work: which launches, events and waits the stages
// below enqueue, and in what order, is the frame's speed.

// what the stages of one processFrame call hand on to each other
struct FrameRun {
    const mmf_frame* fr = nullptr;
    std::chrono::steady_clock::time_point t_begin;
    bool host_trace = false;  // MMF_HOST_TRACE
    bool have_init = false;   // odom_cfg.init == "kp"
    bool track = false;       // :299 "regular execution"
    bool prefetched = false;  // the filter (:262) and the input-side preparation ran on the side stream
    const OdomState* so3_stage = nullptr;  // this frame's own SO3 pre-alignment, computed ahead
    // tracking
    bool one_pass = false;    // one model: its sensor side and model side share the launches of one preparation
    bool lanes_wait = false;  // other streams wait for ev_frame_ready
    int owned = 0;            // models this rank runs, before the tracking
    bool will_batch = false;  // the tracked models will share one chain led by the camera model
    int early_image = 0;      // where the next frame's image side is enqueued (MMF_EARLY_IMAGE: 2 start, 1 chain, 0 off)
    bool next_from_host = false, image_early_any = false, image_early_ok = false;
    std::vector<FusionModel*> tracked;
    bool batched = false;  // one chain for all tracked models is planned ...
    bool batch_ok = false;  // ... and runs
    mmf_model early_snapshot;  // the model's host bookkeeping before the passes enqueued ahead of the pose (fusion_retrack)
    bool early_snapshot_valid = false;
    int pass_mode = 0;  // fusion_batch_mode, once the frame's model list is final
    bool superpixels = false;  // the super-pixel engine runs for this frame (its lane is open)
    bool flow = false;         // the optical-flow engine runs for this frame (its lane is open) ...
    bool flow_enqueued = false;  // ... and its launches are on the flow stream
    bool ferns = false;        // the fern database ran for this frame (its lane is closed, not yet joined)

    // MMF_HOST_TRACE=1: where the calling thread is, in us after the call began (averages over 100 calls)
    void stamp(mmf_fusion* f, int i) const {
        if (host_trace) f->trace_us[i] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count();
    }
};

// a pose's translation and rotation (row-major 3 x 3), as a tracking starts from them
static void pose_trans_rot(const float* pose, float* trans, float* rot) {
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) rot[r * 3 + q] = pose[r * 4 + q];
        trans[r] = pose[r * 4 + 3];
    }
}

// Model::initICP's model side (initICPModel / initRGBModel, Model.cpp:396-401) of one model from `pose`, into `stages`
// (side PREP_ALL: this frame's sensor side as well).  requiresFillIn (:380, :877-895) is decided on the device, from the
// count of covered thumbnail samples the prediction's resolve left (surfel_kernels.hpp: thumbnail_count_px).  `boxed`: an
// object model notes its extents under ext_gen (extent.hpp) and covers only the box its prediction is non-zero in.  The
// end-of-frame preparation of a rank's only model is not boxed: that model's odom->sparse may still be set from its tracking
// (an object model, on a sharded rank).
static void fusion_collect_prep(mmf_fusion* f, PrepStages& stages, FusionModel* fm, const float* pose, int side, bool boxed,
                                unsigned ext_gen) {
    const mmf_fusion_config& g = f->cfg;
    const mmf_model* m = fm->model;
    PrepPrediction p;
    p.vertex = (const float*)m->vertexConf, p.normal = (const float*)m->normalRadius;
    p.image = (const uint8_t*)((g.frame_to_frame_rgb && fm->fill_in) ? m->fill_image : m->image);
    p.channels = 4;
    p.pose = pose;
    p.depth_l0 = f->depth_filtered;
    p.sel = fm->fill_in ? reinterpret_cast<const int*>(model_latest_thumb_count(m)) : nullptr;
    p.alt_vertex = (const float*)m->fill_vertex, p.alt_normal = (const float*)m->fill_normal, p.alt_image = (const uint8_t*)m->fill_image;
    p.sel_total = (m->width / 20) * (m->height / 20), p.sel_ratio = 0.75f;
    p.ext_gen = boxed && fm->odom->sparse ? ext_gen : 0u;
    if (side == PREP_ALL) {
        PrepSensorFrame fr;
        fr.depth_filtered = f->depth_filtered, fr.depth_cutoff = g.max_depth_processed;
        fr.rgb = f->frame_rgb, fr.channels = 3;
        prep_collect_all(stages, fm->odom, fr, p);
    } else {
        p.pred_box = boxed ? fusion_pred_box(fm) : nullptr;
        prep_collect_model(stages, fm->odom, p);
    }
}

// The Gauss-Newton chains (Model::performTracking, Model.cpp:409-433) of n tracked models, from their poses or, on a retrack,
// from the poses the frame started with (fm->last_pose).  batch: ONE chain for all of them on the first one's stream
// (gridDim.y = model), the other models' streams continuing behind it; else one chain per model on the model's stream.
static int fusion_enqueue_chains(mmf_fusion* f, FusionModel* const* fms, size_t n, bool batch, bool from_last_pose) {
    const mmf_fusion_config& g = f->cfg;
    const TrackMode tm = track_mode(g.rgb_only, g.icp_weight, g.pyramid, g.fast_odom, g.so3);
    float pose[16];
    auto start_pose = [&](FusionModel* fm) -> const float* {
        if (from_last_pose) return fm->last_pose;
        mmf_model_get_pose(fm->model, pose);
        return pose;
    };
    if (!batch) {
        for (size_t k = 0; k < n; ++k) {
            float trans[3], rot[9];
            pose_trans_rot(start_pose(fms[k]), trans, rot);
            int rc = odom_enqueue_tracking(fms[k]->odom, trans, rot, tm, fms[k]->icp_error, fms[k]->rgb_error);
            if (rc) return rc;
        }
        return MMF_OK;
    }
    FusionModel* lead = fms[0];
    hipStream_t st = lead->lane->stream;
    TrackBatch tb;
    tb.n = (int)n;
    std::memset(&tb.bd, 0, sizeof(tb.bd));
    for (int k = 0; k < tb.n; ++k) {
        tb.o[k] = fms[k]->odom;
        tb.bd.d[k] = odom_slab_delta(fms[k]->odom, lead->odom);
        pose_trans_rot(start_pose(fms[k]), tb.poses.trans[k], tb.poses.rot[k]);
    }
    int rc = odom_enqueue_tracking(lead->odom, tb.poses.trans[0], tb.poses.rot[0], tm, lead->icp_error, lead->rgb_error, &tb);
    if (rc) return rc;
    // the lanes continue after the chain.  With a segmentation every lane waits for ev_frame_ready before its passes anyway,
    // and that event is recorded on this very stream (the camera model's) behind the chain (the mask's upload, frame_segment):
    // an event and a wait per model here would be fourteen host calls and seven barrier packets for nothing
    for (size_t k = 1; k < n && !(g.enable_multiple_models && st == f->ctx->stream); ++k)
        MMF_HIP_TRY(order(st, fms[k]->ev_done.get(), fms[k]->lane->stream));
    return MMF_OK;
}

// :209-283: the prefetch hand-over, the bilateral filter (:262), the mask, the scheduled deactivations
static int frame_begin(mmf_fusion* f, FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    mmf_ctx* c = f->ctx;
    if (f->pre.valid) {  // whatever was prefetched has to be complete before this frame touches the same buffers
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->pre.done.get(), 0));  // (recorded behind BOTH side streams' work)
        r.prefetched = f->pre.rgb == fr->rgb && f->pre.depth == fr->depth;
        f->pre.valid = false;
    }
    // a prefetched SO3 pre-alignment only counts for the frame it was computed for, and only when that frame is tracked
    const int so3_ready = f->pre.so3_ready;
    f->pre.so3_ready = -1;
    f->pre.image_rgb = nullptr;
    if (so3_ready >= 0 && r.prefetched && r.track && !(r.have_init && !fr->icp_refine)) r.so3_stage = f->pre.so3_stage[so3_ready];
    for (FusionModel* fm : f->models) fm->odom->so3.prefetched = false, fm->odom->so3.stage = nullptr;
    if (r.prefetched) {  // the filter (:262) and the input-side preparation already ran on the side stream
        f->pre.cur ^= 1;
        f->depth_filtered = f->pre.filtered[f->pre.cur].get();
        odom_adopt_gradients(f->models[0]->odom);
    } else {
        int rc = mmf_filter_depth(c, fr->depth, f->width, f->height, g.depth_cutoff, f->depth_filtered);  // :262
        if (rc) return rc;
    }
    f->frame_rgb = fr->rgb, f->frame_depth = fr->depth;
    f->pre.inputs_free_recorded = false;  // (set again by the stages that record ev_inputs_free)
    f->up.host_caught_up = false;
    if (!g.enable_multiple_models && !f->mask_is_zero) {  // :268-275: everything is background
        MMF_HIP_TRY(hipMemsetAsync(f->mask.get(), 0, (size_t)f->width * f->height, c->stream));
        f->mask_is_zero = true;
    }
    for (int id : f->scheduled_deactivation)  // :279-283
        if (FusionModel* fm = fusion_find(f, id)) {
            int rc = fusion_inactivate(f, fm);
            if (rc) return rc;
        }
    f->scheduled_deactivation.clear();
    return MMF_OK;
}

// :290-296
static int frame_first(mmf_fusion* f, const FrameRun& r) {
    const mmf_frame* fr = r.fr;
    mmf_ctx* c = f->ctx;
    if (fusion_owns(f, 0)) {
        int rc = mmf_model_initialise(f->models[0]->model, fr->rgb, fr->depth, f->depth_filtered, f->tick, f->cfg.max_depth_processed);
        if (rc) return rc;
    }
    int rc = mmf_odom_init_first_rgb(f->models[0]->odom, fr->rgb, 0, 3);  // sensor side: every rank
    if (rc) return rc;
    MMF_HIP_TRY(hipEventRecord(f->pre.inputs_free.get(), c->stream));
    f->pre.inputs_free_recorded = true;
    MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready.get(), c->stream));
    return MMF_OK;
}

// generateCUDATextures (:302) + the sensor side of Model::initICP (Model.cpp:402-403: initICP, initRGB), once for all models,
// and the next frame's image side if it goes out before the chains.  One model without pose initialisation: sensor side and
// model side share four launches.
static int frame_track_sensor_side(mmf_fusion* f, FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    mmf_ctx* c = f->ctx;
    FusionModel* global = f->models[0];
    const size_t n_models = f->models.size();
    for (size_t k = 0; k < n_models; ++k) {  // is last frame's end-of-frame preparation of a model still good?
        FusionModel* fm = f->models[k];
        float pose_now[16];
        mmf_model_get_pose(fm->model, pose_now);
        fm->spec_hit = fm->spec_valid && fusion_owns(f, k) && !r.have_init && std::memcmp(pose_now, fm->spec_pose, sizeof(pose_now)) == 0 &&
                       fm->model->gen.tex == fm->spec_tex_gen && fm->spec_f2f == g.frame_to_frame_rgb && fm->odom->in.prep_batched;
        fm->spec_valid = false;
        fm->odom->spec.ok = fm->spec_hit;  // (the tracking's beginning rode that preparation: odom_begin_rider)
        fm->early_done = fm->early_fused = false;
    }
    r.one_pass = n_models == 1 && !r.have_init && fusion_owns(f, 0) && !global->spec_hit;
    if (!r.prefetched && !r.one_pass) {
        PrepSensorFrame sf;
        sf.depth_filtered = f->depth_filtered, sf.depth_cutoff = g.max_depth_processed;
        sf.rgb = fr->rgb, sf.channels = 3;
        int rc = odom_prepare_sensor(global->odom, sf, PREP_INPUT_IMAGE | PREP_INPUT_DEPTH);
        if (rc) return rc;
        odom_adopt_gradients(global->odom);
    }
    // (waited for by the other models' streams only: one model and no segmentation = no marker on the model's stream)
    r.lanes_wait = g.enable_multiple_models || n_models > 1;
    if (!r.one_pass && r.lanes_wait) MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready.get(), c->stream));
    // Round 3: the IMAGE side of the next frame -- intensity pyramid, gradients, SO3 pre-alignment: sixteen launches --
    // depends on nothing the chains read or write (the image ring and the gradients are double buffered, the
    // pre-alignment runs in a state of its own), so it need not wait behind the pose, where its enqueue was the longest
    // part of the host's tail (93 us) and its stream the last thing the next frame's chain waited for.
    //   MMF_EARLY_IMAGE=start (default): enqueued HERE, before this frame's chain: the GPU is still working off the
    //     last frame's tail then, and the image side runs beside that, not beside the latency-bound chain;
    //   =chain: after the chain's enqueue, while the host would only wait (runs beside the chain: +5..35 us on it);
    //   =off: at the end of the call with the depth side.
    // so3_stage: this frame's own pre-alignment ran ahead as well -- inside the chain it reads the LAST frame's level-2
    // image, the half of the image ring the next frame's pyramid is written to.
    // (-1, the default: `start` with one or two models on this GPU -- the GPU is still busy when the call begins --,
    // `chain` from three on: there the GPU waits for the chain's first launch when the call begins, and sixteen
    // launches enqueued in front of it are 50-80 us of that wait: 4 models 0.617 -> 0.558 ms, 8 models 0.70 -> 0.69)
    r.owned = 0;
    for (size_t k = 0; k < n_models; ++k) r.owned += fusion_owns(f, k) ? 1 : 0;
    r.early_image = tunables().early_image >= 0 ? tunables().early_image : (r.owned >= 3 ? 1 : 2);
    r.next_from_host = f->up.next.slot >= 0 && f->up.dev[0].get() != nullptr;  // (a frame still being uploaded)
    r.image_early_any = fr->next_rgb && fr->next_depth && f->pre.side2.get() && g.so3 && r.so3_stage != nullptr;
    r.image_early_ok = r.image_early_any && !r.next_from_host;
    if (r.early_image == 2 && r.image_early_ok) {
        // the ring as it will be once this frame's chain is enqueued (RGBDOdometry.cpp:469-473; odom_enqueue_tracking)
        mmf_odom* go = global->odom;
        for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(go->last_next_image[i], go->next_image[i]);
        int rc = fusion_prefetch_image(f, fr->next_rgb, f->tick + 1, true);
        for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(go->last_next_image[i], go->next_image[i]);
        if (rc) return rc;
    }
    return MMF_OK;
}

// :312-387 up to the tracking itself: each model's stream, the initialisation by track transformation, the list of models
// whose tracking is enqueued next (r.tracked)
static int frame_init_poses(mmf_fusion* f, FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    FusionModel* global = f->models[0];
    // Several models in one chain (fusion_enqueue_chains): an object model's stream gets its next work behind that chain -- it
    // waits for an event recorded there -- so the wait for the frame's sensor side here would be a second barrier packet per
    // stream and two host calls per model at the point of the call where the GPU waits for the calling thread.
    // (only where the camera model leads the chain: its stream is the one the sensor side and the end-of-frame preparation
    // are ordered on; a rank of a sharded run that holds object models only keeps every wait)
    r.will_batch = r.owned > 1 && r.owned <= kMaxBatch && !r.have_init && g.batch_tracking && fusion_owns(f, 0);
    for (size_t k = 0; k < f->models.size(); ++k) {
        FusionModel* fm = f->models[k];
        fm->tracking = false;
        if (!fusion_owns(f, k)) continue;
        mmf_model_get_pose(fm->model, fm->prev_pose);  // (before the initialisation below replaces pose and last_pose)
        if (k > 0) {
            if (!r.will_batch) {
                int rc = lane_wait(fm, f->ev_frame_ready.get());
                if (rc) return rc;
            }
            odom_alias_sensor_side(fm->odom, global->odom);
        }
        bool do_icp = true;
        if (r.have_init) {  // initialise by track transformation (:316-376)
            do_icp = fr->icp_refine != 0;
            float pose[16], tnew[16];
            mmf_model_get_pose(fm->model, pose);
            const float* T = fr->init_transforms + 16 * (k < (size_t)fr->n_init_transforms ? k : 0);
            if (k >= (size_t)fr->n_init_transforms) {
                std::memcpy(tnew, pose, sizeof(pose));  // no transformation for this model: keep its pose
            } else if (fm->model->id == 0) {
                mmf::host::matmul4(pose, T, tnew);  // Tnew = model->getPose() * T (:331)
            } else {
                mmf::host::matmul4(T, pose, tnew);  // Tnew = T * model->getPose() (:334)
            }
            mmf_model_set_pose(fm->model, tnew);  // overridePose: pose = lastPose = Tnew (:350, Model.h:301-304)
            std::memcpy(fm->last_pose, tnew, sizeof(tnew));
            int rc = fusion_predict_model(f, fm);  // :353-355
            if (rc) return rc;
            // Model::fuse(..., weightMultiplier) applies computeFusionWeight(weightMultiplier) (:359-360, Model.cpp:918)
            rc = fusion_fuse_clean_model(f, fm, fusion_weight(tnew, fm->last_pose, fr->weight_multiplier));  // :357-366
            if (rc) return rc;
        }
        if (!do_icp) continue;  // no refinement, use the initial pose directly (:382-385)
        // Model::performTracking (Model.cpp:409-433) with Model::initICP (:390-407)
        float pose[16];
        mmf_model_get_pose(fm->model, pose);
        std::memcpy(fm->last_pose, pose, sizeof(pose));  // lastPose = pose (Model.cpp:412)
        fm->tracking = true;
        r.tracked.push_back(fm);
    }
    return MMF_OK;
}

// the tracked models' model-side preparation and chains.  ONE chain of launches for all tracked models (gridDim.y = model)
// when every level runs on the fused producer path and no model went through a pose-initialisation round on its own stream;
// else one chain per model on the model's stream.  Either way nothing waits here.
static int frame_enqueue_tracking(mmf_fusion* f, FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    FusionModel* global = f->models[0];
    const std::vector<FusionModel*>& tracked = r.tracked;
    if (r.so3_stage)  // every chain enqueued below starts from the prefetched pre-alignment
        for (FusionModel* fm : tracked) fm->odom->so3.prefetched = true, fm->odom->so3.stage = r.so3_stage;
    r.batched = tracked.size() > 1 && tracked.size() <= (size_t)kMaxBatch && !r.have_init && g.batch_tracking;
    const unsigned ext_gen = ++f->extent_seq;
    for (FusionModel* fm : tracked) fm->odom->sparse = fm != global && !fm->fill_in;  // an object model: extent.hpp, ChainGeom
    r.batch_ok = r.batched;
    if (r.batched) {  // (one_pass is one model: a batch is never prepared with the sensor side)
        FusionModel* lead = tracked[0];
        hipStream_t st = lead->lane->stream;
        for (size_t k = 1; k < tracked.size(); ++k) {  // the other models' last work (previous frame's predict) precedes
            // (a model prepared at the end of the last call, behind the join of all streams there, and untouched since:
            // nothing enqueued below reads what its stream may still hold)
            if (tracked[k]->spec_hit) continue;
            MMF_HIP_TRY(order(tracked[k]->lane->stream, tracked[k]->ev_done.get(), st));
        }
        PrepStages stages;
        stages.set_critical(true);  // the model's stream
        for (FusionModel* fm : tracked) {
            if (fm->spec_hit) {
                fm->odom->in.depth_l0 = f->depth_filtered;
                continue;
            }
            float pose[16];
            mmf_model_get_pose(fm->model, pose);
            fusion_collect_prep(f, stages, fm, pose, PREP_MODEL_SIDE, true, ext_gen);
        }
        int rc = stages.launch(st);
        if (rc) return rc;
        r.stamp(f, 8);
        r.batch_ok = odom_batchable(lead->odom, track_mode(g.rgb_only, g.icp_weight, g.pyramid, g.fast_odom, g.so3));
        if (r.batch_ok) {
            lead->odom->exclusive_chain = true;  // one chain for all of them
            return fusion_enqueue_chains(f, tracked.data(), tracked.size(), true, false);
        }
    }
    for (size_t k = 0; k < tracked.size(); ++k) {
        FusionModel* fm = tracked[k];
        const bool prep_all = fm == global && r.one_pass && !r.prefetched;
        if (r.will_batch && fm != global) {  // (the wait frame_init_poses skipped)
            int rc = lane_wait(fm, f->ev_frame_ready.get());
            if (rc) return rc;
        }
        if (fm->spec_hit) {  // the model side was prepared at the end of the last frame; the sensor side by the prefetch
            fm->odom->in.depth_l0 = f->depth_filtered;  // (or in frame_track_sensor_side)
        } else if (!r.batched) {  // (a failed batch has prepared every model already)
            PrepStages stages;
            stages.set_critical(true);  // the model's stream
            float pose[16];
            mmf_model_get_pose(fm->model, pose);
            fusion_collect_prep(f, stages, fm, pose, prep_all ? PREP_ALL : PREP_MODEL_SIDE, true, ext_gen);
            int rc = stages.launch(fm->lane->stream);
            if (rc) return rc;
            if (prep_all) odom_adopt_gradients(global->odom);  // (PREP_ALL: this frame's image side as well)
        } else if (k > 0) {  // prepared on the leader's stream
            MMF_HIP_TRY(order(tracked[0]->lane->stream, fm->ev_done.get(), fm->lane->stream));
        }
        fm->odom->exclusive_chain = tracked.size() == 1;  // several chains side by side: no in-launch barriers
        // The frame's first projection, enqueued right behind this chain (frame_enqueue_ahead), carries the hand-over to the
        // host and the fusion weight on one extra workgroup (frame_rider.hpp): the chain's last launch is the solve alone (13
        // -> 5.7 us on the stream a frame waits for).
        fm->odom->defer_publish = tracked.size() == 1 && !fr->bootstrap && !r.have_init && !g.rgb_only && f->tracking_ok && !f->fi.on;
        int rc = fusion_enqueue_chains(f, &fm, 1, false, false);
        if (rc) return rc;
    }
    return MMF_OK;
}

// One model on the context's stream, nothing between its tracking and its fusion that the host decides: the frame's first
// projections -- predict() (:675) and the first predictIndices (:792) -- are enqueued right here, behind the chain and the
// copy of its result, with the inverse pose read from the odometry's device state.  They run while the host picks the pose
// up and prepares the fusion passes (that turnaround used to be ~25 us of idle GPU per frame).
// (With several models it is one model per process in the sharded configuration: the segmentation between tracking and
// fusion touches masks, thresholds and the list, none of which a projection reads.)
static int frame_enqueue_ahead(mmf_fusion* f, FrameRun& r) {
    const mmf_fusion_config& g = f->cfg;
    static_assert(std::is_trivially_copyable<mmf_model>::value, "the speculation rollback copies mmf_model by value");
    if (!(r.tracked.size() == 1 && !r.fr->bootstrap && !r.have_init && !g.rgb_only && f->tracking_ok)) return MMF_OK;
    if (f->fi.on) return MMF_OK;  // (the flow inference reads the prediction the frame was tracked against: frame_flow_inference)
    FusionModel* fm = r.tracked[0];
    mmf_model* m = fm->model;
    r.early_snapshot = *m, r.early_snapshot_valid = true;
    m->dev.abort = &fm->odom->state->gn_fault;
    // "nothing enqueued so far reads the odometries' sensor-side buffers or the other filtered-depth buffer" holds
    // HERE, behind the one chain of this process; the passes enqueued next do not read them either.  No event
    // says so any more (see frame_track: the host knows when it has the pose; a marker behind the chain cost the
    // model's stream ~4 us in front of the frame's first projection).
    m->dev.t_inv = fm->odom->state->pose_inv;
    m->dev.rider = fm->odom->rider;
    fm->odom->rider = FrameRider();
    int rc = fusion_mid_predict() ? fusion_predict_model(f, fm) : MMF_OK;
    if (rc == MMF_OK) rc = mmf_model_predict_indices(m, f->tick, g.max_depth_processed, g.time_delta);
    MMF_REQUIRE(rc != MMF_OK || m->dev.rider.st == nullptr, "mmf_fusion_process_frame: the tracking result was not handed over");
    fm->early_done = rc == MMF_OK;
    // Without a segmentation the mask of the frame is known (all zeros) and nothing the host decides lies
    // between tracking and fusion: fuse -> predictIndices -> clean (:791-816) follow at once, with the pose and
    // Model::computeFusionWeight taken from the device state (odom_end, odom_fusion_weight_kernel).
    if (rc == MMF_OK && !g.enable_multiple_models) {
        m->dev.pose = fm->odom->state->pose_out, m->dev.weight = &fm->odom->state->fusion_weight;
        rc = fusion_fuse_clean_model(f, fm, r.fr->weight_multiplier, true);
        fm->early_fused = rc == MMF_OK;
    }
    m->dev.reset();
    return rc;
}

// The one-launch chain can give up (its count barrier needs every workgroup of a launch resident: another process on the GPU
// can prevent that; OdomState::gn_fault).  Then nothing of the chain's result is valid and the passes enqueued ahead of the
// pose have done nothing (MMF_SPECULATION_GUARD): the model's host bookkeeping goes back to where it was, the process stops
// using that chain, and the frame's tracking is enqueued again -- the two-launch chain, from the poses the frame started with
// (fm->last_pose) -- before the results are picked up a second time.
static int fusion_retrack(mmf_fusion* f, FrameRun& r) {
    std::vector<mmf_odom*> odoms;
    for (FusionModel* fm : r.tracked) odoms.push_back(fm->odom);
    odom_retrack_prepare(odoms.data(), (int)odoms.size(), f->cfg.so3);
    if (r.early_snapshot_valid) {
        *r.tracked[0]->model = r.early_snapshot;
        r.tracked[0]->early_done = r.tracked[0]->early_fused = false;
        r.early_snapshot_valid = false;
    }
    for (FusionModel* fm : r.tracked) fm->odom->defer_publish = false, fm->odom->rider = FrameRider();
    return fusion_enqueue_chains(f, r.tracked.data(), r.tracked.size(), r.batch_ok, true);
}

// the tracking results, model by model
static int frame_pick_up_poses(mmf_fusion* f, FrameRun& r) {
    bool retracked = false;
    for (size_t k = 0; k < f->models.size(); ++k) {
        FusionModel* fm = f->models[k];
        float pose[16];
        mmf_model_get_pose(fm->model, pose);
        if (!fm->tracking) continue;
        float trans[3], rot[9];
        int rc = odom_finish_tracking(fm->odom, trans, rot);
        if (rc == kGnRetry && !retracked) {  // (at most once: the two-launch chain has no way to give up)
            // every chain of the frame is void with it (a batch is one chain; chains side by side are two-launch chains)
            for (FusionModel* t : r.tracked)
                if (t->tracking && t != fm && t->odom->call.result_of) {  // drain what the other lanes' chains still publish
                    float tt[3], rr[9];
                    (void)odom_finish_tracking(t->odom, tt, rr);
                }
            rc = fusion_retrack(f, r);
            if (rc) return rc;
            retracked = true;
            for (FusionModel* t : r.tracked) {  // poses already taken over from the void chain: back to the frame's start
                mmf_model_set_pose(t->model, t->last_pose);
                t->tracking = true;
            }
            k = (size_t)-1;  // pick the results up again, from the first model
            continue;
        }
        if (rc == kGnRetry) return gn_retry_twice();
        if (rc) return rc;
        for (int i = 0; i < 3; ++i) {
            for (int q = 0; q < 3; ++q) pose[i * 4 + q] = rot[i * 3 + q];
            pose[i * 4 + 3] = trans[i];
        }
        mmf_model_set_pose(fm->model, pose);
        fm->tracking = false;
        if (fm->lane->stream == f->ctx->stream) f->up.host_caught_up = true;
    }
    return MMF_OK;
}

// :299-400: every model's tracking, enqueued before the first result is awaited, then the bootstrap
static int frame_track(mmf_fusion* f, FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    FusionModel* global = f->models[0];
    MMF_REQUIRE(!r.have_init || !g.frame_to_frame_rgb, "ICP initialisation not supported in frame-to-frame mode");  // :370
    const auto t_track = std::chrono::steady_clock::now();
    int rc = frame_track_sensor_side(f, r);
    if (rc) return rc;
    r.stamp(f, 6);
    rc = frame_init_poses(f, r);
    if (rc) return rc;
    r.stamp(f, 7);
    rc = frame_enqueue_tracking(f, r);
    if (rc) return rc;
    rc = frame_enqueue_ahead(f, r);
    if (rc) return rc;
    // the sensor-side image ring (this frame's / last frame's intensity pyramid, RGBDOdometry.cpp:469-473) lives in
    // the global odometry and advances when its chain is enqueued: when its owner is another rank, the swap
    // happens here, whether or not this rank tracked anything (every rank's ring must advance with the global model's)
    const bool global_tracks_somewhere = !(r.have_init && !fr->icp_refine);
    if (g.so3 && global_tracks_somewhere && !global->tracking)
        for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(global->odom->last_next_image[i], global->odom->next_image[i]);
    if (r.early_image == 1 && r.image_early_ok && !r.tracked.empty()) {  // (see frame_track_sensor_side)
        rc = fusion_prefetch_image(f, fr->next_rgb, f->tick + 1, true);
        if (rc) return rc;
    }
    if (r.superpixels) {  // the super-pixel engine, beside the chains
        rc = frame_superpixels_enqueue(f, fr->rgb);
        if (rc) return rc;
    }
    if (r.flow) {  // the optical-flow engine, beside the chains
        rc = frame_flow_enqueue(f, fr->rgb);
        if (rc) return rc;
        r.flow_enqueued = true;
    }
    r.stamp(f, 0);
    // a host frame announced for the next call: staged and sent up now, while the GPU tracks and the host would only wait
    // (its colour image first; the depth image is joined where the depth side is enqueued, behind the pose)
    rc = fusion_stage_host_rgb(f);
    if (rc) return rc;
    // ... and its image side behind the upload (an announced HOST frame cannot have it at the start of the call: its
    // copy into pinned memory has only just begun then), beside the chain instead of behind the pose
    if (r.early_image != 0 && r.image_early_any && r.next_from_host && !r.tracked.empty() && f->up.next.rgb_staged) {
        MMF_HIP_TRY(fusion_wait_unless_done(f->pre.side2.get(), f->up.ev_rgb[f->up.next.slot].get()));
        rc = fusion_prefetch_image(f, fr->next_rgb, f->tick + 1, true);
        if (rc) return rc;
    }
    rc = frame_pick_up_poses(f, r);
    if (rc) return rc;
    f->t_tracking_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_track).count();
    r.stamp(f, 1);
    if (fr->bootstrap) {  // :397-400
        MMF_REQUIRE(fr->in_pose != nullptr, "mmf_fusion_process_frame: bootstrap needs in_pose");
        float pose[16], np[16];
        mmf_model_get_pose(global->model, pose);
        mmf::host::matmul4(pose, fr->in_pose, np);
        mmf_model_set_pose(global->model, np);  // overridePose
        std::memcpy(global->last_pose, np, sizeof(np));
    }
    // from here on nothing enqueued reads the odometries' sensor-side buffers or the other filtered-depth
    // buffer, and the HOST knows it: every chain's result has been received, so every chain -- and whatever its
    // stream held before it, e.g. this frame's own image-side preparation -- has run.  The next frame's side-stream
    // work, enqueued from here on, needs no event to wait for (inputs_free_recorded stays false).
    if (r.one_pass && r.lanes_wait) MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready.get(), f->ctx->stream));
    return MMF_OK;
}

// :407-622: the segmentation's mask, a new model's first surfels, models that leave the list, confidence thresholds
static int frame_segment(mmf_fusion* f, const FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    mmf_ctx* c = f->ctx;
    mmf_segmentation seg_cb;
    const mmf_segmentation* seg = fr->segmentation;
    // a frame that brings raw labels (Segmentation.cpp:89: `frame.mask.total()` is tested before anything else)
    const bool from_labels = f->seg.mask_on && seg && seg->mask && !seg->model_data;
    // ... and one that brings nothing while the flow_crf mode is on (mmf_fusion_set_flow_segmentation)
    const bool from_flow = !from_labels && !seg && f->fseg.on;
    const int spawn_after = from_labels ? f->seg.mask_cfg.model_spawn_offset
                                        : (from_flow ? f->fseg.cfg.model_spawn_offset : f->seg.crf_cfg.model_spawn_offset);
    if (f->seg.spawn_offset < (unsigned)spawn_after) f->seg.spawn_offset++;  // (:410)
    if (from_labels) {
        int rc = fusion_mask_segment(f, seg->mask, &seg_cb);
        if (rc) return rc;
        seg = &seg_cb;
    } else if (from_flow) {
        int rc = fusion_flow_segment(f, &seg_cb);
        if (rc) return rc;
        seg = &seg_cb;
    } else if (!seg && f->seg.fn) {  // performSegmentation(frame) (:412)
        std::memset(&seg_cb, 0, sizeof(seg_cb));
        if (f->seg.fn(f->seg.user, f, fr, &seg_cb)) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the segmentation callback failed");
        seg = &seg_cb;
    } else if (!seg && f->seg.crf_on) {
        int rc = fusion_crf_segment(f, &seg_cb);
        if (rc) return rc;
        seg = &seg_cb;
    }
    MMF_REQUIRE(seg && seg->mask, "mmf_fusion_process_frame: enableMultipleModels needs a segmentation "
                                  "(mmf_frame::segmentation, mmf_fusion_set_segmentation_callback, mmf_fusion_set_crf_segmentation, "
                                  "mmf_fusion_set_flow_segmentation or, for a frame that brings its labels, mmf_fusion_set_mask_segmentation)");
    // textures[MASK]->Upload(fullSegmentation) (:416)
    if (seg->mask != f->mask.get())
        MMF_HIP_TRY(hipMemcpyAsync(f->mask.get(), seg->mask, (size_t)f->width * f->height, hipMemcpyDeviceToDevice, c->stream));
    f->mask_is_zero = false;
    MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready.get(), c->stream));
    // fewer entries than models (none at all from the flow_crf mode on a frame without an inference result): the models
    // without an entry keep their max depth, unseen count and confidence threshold -- every loop below ends at n_data
    const int n_data = seg->model_data ? seg->n_models : 0;
    // redetection via keypoints (:489-559) runs BEFORE a model is spawned: a label it cancels (:522-524) consumes neither an id
    // nor a preallocated model (the reference spawns first and abandons newModel, :468-487, :565)
    bool has_new = seg->has_new_label != 0;
    {
        int rc = frame_redetect(f, &has_new);
        if (rc) return rc;
    }
    if (seg->has_new_label && !has_new) f->seg.spawn_offset = 0;  // (the reference had spawned already: :484)
    FusionModel* fresh = nullptr;
    if (has_new) {  // :469-487
        int rc = fusion_spawn(f, &fresh);
        if (rc) return rc;
        f->seg.spawn_offset = 0;  // (:484)
        if (n_data > 0) fresh->model->max_depth = seg_max_depth(seg->model_data[n_data - 1]);
    }
    // Set max-depth (:585-586)
    for (size_t i = 1; i < f->models.size() && (int)i < n_data; ++i) f->models[i]->model->max_depth = seg_max_depth(seg->model_data[i]);
    if (fresh && !fusion_owns_model(f, fresh)) {
        f->models.push_back(fresh);  // another rank's model: bookkeeping only
    } else if (fresh) {  // :588-601: the first surfels of the new model, then it joins the list
        int rc = lane_wait(fresh, f->ev_frame_ready.get());
        if (rc) return rc;
        identity16(fresh->last_pose);
        float pose[16];
        mmf_model_get_pose(fresh->model, pose);
        rc = mmf_model_predict_indices(fresh->model, f->tick, g.max_depth_processed, g.time_delta);
        if (rc) return rc;
        rc = mmf_model_fuse(fresh->model, f->tick, f->frame_rgb, f->mask.get(), f->frame_depth, f->depth_filtered, g.max_depth_processed,
                            fusion_weight(pose, fresh->last_pose, 100.f));  // fuse(..., 100) (:591-592)
        if (rc) return rc;
        // (the second predictIndices is commented out in the reference, :594)
        rc = mmf_model_clean(fresh->model, f->tick, g.time_delta, g.max_depth_processed, f->depth_filtered, f->mask.get(), g.outlier_coeff);
        if (rc) return rc;
        f->models.push_back(fresh);  // moveNewModelToList (:600)
        f->kp.spawned_id = (int)fresh->model->id;
    }
    // unseen models leave the list (:606-613); the confidence of object models rises (:616-620)
    std::vector<FusionModel*> lost;
    for (int i = 0; i < n_data; ++i) {
        FusionModel* fm = fusion_find(f, (int)seg->model_data[i].id);
        if (!fm || fm == fresh) continue;
        if (seg->model_data[i].super_pixel_count <= 0 && ++fm->unseen > 0 && fm->model->id != 0) lost.push_back(fm);
    }
    for (FusionModel* fm : lost) {
        int rc = fusion_inactivate(f, fm);
        if (rc) return rc;
    }
    for (size_t i = 1; i < f->models.size() && (int)i < n_data; ++i) {
        const float old_conf = f->models[i]->model->conf_threshold;
        const float avg = seg->model_data[i].avg_confidence;
        const float m1 = old_conf < avg ? avg : old_conf;
        f->models[i]->model->conf_threshold = 9.0f < m1 ? 9.0f : m1;
    }
    return MMF_OK;
}

// globalModel->overridePose(*inPose) (:670)
static int frame_dictated_pose(mmf_fusion* f, const FrameRun& r) {
    FusionModel* global = f->models[0];
    float pose[16];
    std::memcpy(pose, r.fr->in_pose, sizeof(pose));
    mmf_model_set_pose(global->model, pose);
    std::memcpy(global->last_pose, pose, sizeof(pose));
    MMF_HIP_TRY(hipEventRecord(f->pre.inputs_free.get(), f->ctx->stream));
    f->pre.inputs_free_recorded = true;
    MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready.get(), f->ctx->stream));
    return MMF_OK;
}

// The OBJECT models whose passes go out as one launch per pass for all of them on the first one's stream (pass mode 2): ~9
// launches per model and frame otherwise, and with seven objects the calling thread's launch rate set the pace of that part
// of the frame.  At least two, at most kMaxPassBatch, no fill-in: the camera model keeps its own stream and kernels (riders,
// fill-in).  The fuse / clean batch leaves out a model whose passes went out ahead of its pose; the predict batch leaves out
// deep stores and models with device-side inputs (model_predict_batchable).  So a model fused in the batch can be predicted
// on its own stream, and a predict batch can be led by another object: both read the maps the fuse / clean batch wrote, and
// every object's stream continues behind a batch (fusion_pass_batch).
static void fusion_pass_batch_members(const mmf_fusion* f, bool predict, std::vector<FusionModel*>& objs) {
    for (size_t k = 1; k < f->models.size(); ++k) {
        FusionModel* fm = f->models[k];
        if (!fusion_owns(f, k) || fm->fill_in || (int)objs.size() >= kMaxPassBatch) continue;
        if (predict ? !model_predict_batchable(fm->model) : (fm->early_done || fm->early_fused)) continue;
        objs.push_back(fm);
    }
    if (objs.size() < 2) objs.clear();
}
// one batch on objs[0]'s stream: it waits for whatever the other objects' streams still hold (fusion_lanes_join),
// enqueue(models, n, stream) enqueues the passes, and the other objects' streams continue behind the batch
template <typename Enqueue>
static int fusion_pass_batch(const std::vector<FusionModel*>& objs, Enqueue&& enqueue) {
    hipStream_t st = objs[0]->lane->stream;
    int rc = fusion_lanes_join(objs, st);
    if (rc) return rc;
    mmf_model* ms[kMaxPassBatch];
    for (size_t k = 0; k < objs.size(); ++k) ms[k] = objs[k]->model;
    rc = enqueue(ms, (int)objs.size(), st);
    if (rc) return rc;
    MMF_HIP_TRY(hipEventRecord(objs[0]->ev_done.get(), st));
    for (size_t k = 1; k < objs.size(); ++k) MMF_HIP_TRY(hipStreamWaitEvent(objs[k]->lane->stream, objs[0]->ev_done.get(), 0));
    return MMF_OK;
}

// predict() (:675), then predictIndices -> fuse -> predictIndices -> clean (:791-816) of every model
static int frame_fuse_clean(mmf_fusion* f, const FrameRun& r) {
    const mmf_fusion_config& g = f->cfg;
    const float weight_multiplier = r.fr->weight_multiplier;
    const bool fuse_now = !g.rgb_only && f->tracking_ok;
    std::vector<FusionModel*> objs;
    if (r.pass_mode != 0 && fuse_now && !fusion_mid_predict()) fusion_pass_batch_members(f, false, objs);
    for (size_t k = 0; k < f->models.size(); ++k) {  // model by model
        FusionModel* fm = f->models[k];
        if (!fusion_owns(f, k)) continue;
        if (std::find(objs.begin(), objs.end(), fm) != objs.end()) continue;  // (batched below)
        if (k > 0) {
            int rc = lane_wait(fm, f->ev_frame_ready.get());
            if (rc) return rc;
        }
        const bool early = fm->early_done;  // its predict + predictIndices are already enqueued
        fm->early_done = false;
        if (!early && fusion_mid_predict()) {
            int rc = fusion_predict_model(f, fm);
            if (rc) return rc;
        }
        if (fuse_now && !fm->early_fused) {
            float pose[16];
            mmf_model_get_pose(fm->model, pose);
            int rc = fusion_fuse_clean_model(f, fm, fusion_weight(pose, fm->last_pose, weight_multiplier), early);
            if (rc) return rc;
        }
        fm->early_fused = false;
    }
    if (objs.empty()) return MMF_OK;
    int rc = lane_wait(objs[0], f->ev_frame_ready.get());
    if (rc) return rc;
    return fusion_pass_batch(objs, [&](mmf_model* const* ms, int n, hipStream_t st) {
        float wts[kMaxPassBatch];
        for (int k = 0; k < n; ++k) {
            float pose[16];
            mmf_model_get_pose(ms[k], pose);
            wts[k] = fusion_weight(pose, objs[k]->last_pose, weight_multiplier);
        }
        int rc2 = fusion_note_mask_boxes(f, st);
        if (rc2) return rc2;
        return models_fuse_clean_rect(ms, n, st, f->tick, g.time_delta, g.max_depth_processed, f->frame_rgb, f->mask.get(), f->frame_depth,
                                      f->depth_filtered, g.outlier_coeff, wts, f->mask_boxes.get(), f->mask_gen);
    });
}

// predict() (:821): the object models in a batch, the others one by one
static int frame_predict(mmf_fusion* f, const FrameRun& r) {
    const mmf_fusion_config& g = f->cfg;
    std::vector<FusionModel*> objs;
    if (r.pass_mode != 0) fusion_pass_batch_members(f, true, objs);
    for (size_t k = 0; k < f->models.size(); ++k) {
        if (!fusion_owns(f, k)) continue;
        if (std::find(objs.begin(), objs.end(), f->models[k]) != objs.end()) continue;
        int rc = fusion_predict_model(f, f->models[k]);
        if (rc) return rc;
    }
    if (objs.empty()) return MMF_OK;
    return fusion_pass_batch(objs, [&](mmf_model* const* ms, int n, hipStream_t st) {
        return models_combined_predict_rect(ms, n, st, g.max_depth_processed, f->tick, f->tick, g.time_delta);
    });
}

// :829-846: pose log (camera->world for the first model, object->world for the others)
static void frame_log_poses(mmf_fusion* f, const FrameRun& r) {
    float global_pose[16];
    mmf_model_get_pose(f->models[0]->model, global_pose);
    for (size_t k = 0; k < f->models.size(); ++k) {
        FusionModel* fm = f->models[k];
        if (fm->pose_log.capacity() == 0) continue;  // isLoggingPoses()
        // sharded: a model is logged by the rank that runs it -- the copies other ranks keep as bookkeeping hold poses that
        // arrive with the exchange, one to three frames late under mmf_shard_gather_poses_begin / _end (mmf_hip.h)
        if (f->shard_world > 1 && !fusion_owns(f, k)) continue;
        float T[16];
        if (k == 0) {
            std::memcpy(T, global_pose, sizeof(T));
        } else {
            float pose[16], inv[16];
            mmf_model_get_pose(fm->model, pose);
            inverse4f_host(pose, inv);
            mmf::host::matmul4(global_pose, inv, T);
        }
        PoseLogItem item;
        item.ts = r.fr->timestamp;
        pose_to_log7(T, item.p);
        fm->pose_log.push_back(item);
    }
}

// the next frame's model-side preparation, at the end of this one (see FusionModel::spec_valid)
static int frame_prepare_next(mmf_fusion* f, const FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    FusionModel* global = f->models[0];
    FusionModel* only = nullptr;
    int owned = 0;
    for (size_t k = 0; k < f->models.size(); ++k)
        if (fusion_owns(f, k)) only = f->models[k], ++owned;
    if (owned == 1) {
        const mmf_model* m = only->model;
        hipStream_t st = only->lane->stream;
        PrepStages stages;
        stages.set_critical(true);  // the model's stream
        mmf_model_get_pose(only->model, only->spec_pose);
        fusion_collect_prep(f, stages, only, only->spec_pose, PREP_MODEL_SIDE, false, 0u);
        // ... and the beginning of that tracking (odom_begin_kernel: the pose it starts from is this one, the pre-alignment
        // of the next frame sits staged since the start of this call) on one more workgroup of the preparation's last launch
        BeginRider rider;
        bool ride = false;
        if (only == global && !stages.empty() && fr->next_rgb && f->pre.image_rgb == fr->next_rgb && !g.rgb_only) {
            const OdomState* stage = (g.so3 && f->pre.so3_ready >= 0) ? f->pre.so3_stage[f->pre.so3_ready] : nullptr;
            if (!g.so3 || stage != nullptr) {
                if (stage) MMF_HIP_TRY(fusion_wait_unless_done(st, f->pre.done2.get()));  // (the staged pre-alignment is complete)
                ride = odom_begin_rider(only->odom, only->spec_pose, track_mode(g.rgb_only, g.icp_weight, g.pyramid, g.fast_odom, g.so3),
                                        stage, &rider);
            }
        }
        if (!ride) only->odom->spec.valid = false;
        int rc = stages.launch(st, ride ? &rider : nullptr);
        if (rc) return rc;
        only->spec_tex_gen = m->gen.tex;
        only->spec_f2f = g.frame_to_frame_rgb;
        only->spec_valid = true;
    } else if (owned >= std::max(2, tunables().spec_prep_all) && f->shard_world <= 1 && g.batch_tracking && owned <= kMaxBatch && tunables().spec_prep_all) {
        // Several models on this GPU: the same for all of them, in the launches they will share (the batched chain's
        // preparation: one set of stages, every model's jobs).  At the start of the next call these ~50 jobs were what the
        // calling thread enqueued first -- 130 us of it and as much of the GPU's -- while the GPU had nothing else to do; here
        // they queue up behind the frame's last passes.  A model whose pose or prediction changes before it is tracked
        // (a pose initialisation, a caller's predict()) is prepared again then (spec_hit).  From two models on (round 4: from
        // four -- with two or three the early preparation measured 6 % slower while every model's stream was joined by an
        // event in front of the chain; a model prepared HERE needs no such wait, and it is 4-7 % faster: LABNOTES r5).
        PrepStages stages;
        stages.set_critical(true);
        const unsigned ext_gen = ++f->extent_seq;
        for (size_t k = 0; k < f->models.size(); ++k) {
            if (!fusion_owns(f, k)) continue;
            FusionModel* fm = f->models[k];
            fm->odom->sparse = fm != global && !fm->fill_in;
            mmf_model_get_pose(fm->model, fm->spec_pose);
            fusion_collect_prep(f, stages, fm, fm->spec_pose, PREP_MODEL_SIDE, true, ext_gen);
            fm->spec_tex_gen = fm->model->gen.tex;
            fm->spec_f2f = g.frame_to_frame_rgb;
            fm->spec_valid = true;
        }
        int rc = stages.launch(f->ctx->stream);  // (every lane has joined this stream in frame_end)
        if (rc) return rc;
    }
    return MMF_OK;
}

// the end of the call: the lanes join, the next frame's prefetch, its model-side preparation
static int frame_end(mmf_fusion* f, const FrameRun& r) {
    const mmf_frame* fr = r.fr;
    // the fusion's stream continues only after every lane: the next frame's filter, prefetch and mask upload
    // overwrite what the lanes read
    for (size_t k = 1; k < f->models.size(); ++k) {
        FusionModel* fm = f->models[k];
        if (fusion_owns(f, k)) MMF_HIP_TRY(order(fm->lane->stream, fm->ev_done.get(), f->ctx->stream));
    }
    if (fr->next_rgb && fr->next_depth) {  // (first frame, dictated pose, several lanes)
        int rc = fusion_prefetch_impl(f, fr->next_rgb, fr->next_depth, f->tick);
        if (rc) return rc;
    }
    // behind the prefetch's enqueue: the side streams have the longer way to go
    return frame_prepare_next(f, r);
}

static int fusion_process_frame_impl(mmf_fusion* f, const mmf_frame* fr) {
    MMF_REQUIRE(f != nullptr && fr != nullptr, "mmf_fusion_process_frame: null argument");
    if (!fr->rgb || !fr->depth || fr->timestamp < 0)  // MultiMotionFusion.cpp:209-212
        return fail(MMF_ERR_INVALID, "invalid image data");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    FrameRun r;
    r.fr = fr;
    r.t_begin = std::chrono::steady_clock::now();
    r.host_trace = tunables().host_trace;
    r.have_init = fr->init_transforms != nullptr && fr->n_init_transforms > 0;
    r.track = f->tick > 1 && (fr->bootstrap || !fr->in_pose);
    if (f->kp.frontend && !(f->kp.tracker && r.have_init)) {  // (a frame the check below refuses adds nothing)
        int rc = frame_keypoints(f, fr);
        if (rc) return rc;
    }
    mmf_frame fr_kp;  // the frame with the transformations of the attached tracker (odom_cfg.init == "kp")
    if (f->kp.tracker) {
        MMF_REQUIRE(!r.have_init, "mmf_fusion_process_frame: a tracker is attached (mmf_fusion_set_tracker): the frame cannot bring init_transforms");
        f->kp.T.clear();
        if (f->kp.init_kp && r.track) {
            int rc = frame_track_transforms(f);
            if (rc) return rc;
            fr_kp = *fr;
            fr_kp.init_transforms = f->kp.T.data(), fr_kp.n_init_transforms = (int)(f->kp.T.size() / 16);
            fr_kp.icp_refine = f->kp.icp_refine ? 1 : 0;
            fr = &fr_kp, r.fr = fr, r.have_init = true;
        }
    }
    f->t_tracking_s = 0;
    f->rd.last.clear();  // (mmf_fusion_last_redetections speaks of this call)
    f->kp.stored_ids.clear(), f->kp.stored_views.clear(), f->kp.stored_rows.clear();
    f->kp.spawned_id = -1, f->kp.backdated_id = -1, f->kp.backdated.clear();
    int rc = MMF_OK;
    if (f->flow.engine) {
        f->fi.has = false;
        MMF_HIP_TRY(f->flow.lane.open(f->ctx->stream));  // (pending: a frame that failed between the enqueue and the join)
        r.flow = true;
    }
    rc = frame_begin(f, r);
    if (rc) return rc;
    const bool first = f->tick == 1;
    if (r.flow && (first || !r.track)) {  // (a tracked frame enqueues it behind its chains: frame_track)
        rc = frame_flow_enqueue(f, fr->rgb);
        if (rc) return rc;
        r.flow_enqueued = true;
    }
    if (first) {
        rc = frame_first(f, r);
        if (rc) return rc;
    } else {
        f->tracking_ok = 1;
        if (f->sp.engine && r.track && f->cfg.enable_multiple_models && !fr->segmentation && !f->fseg.on && !f->seg.fn && f->seg.crf_on && !f->sp.next) {
            rc = frame_superpixels_begin(f);
            if (rc) return rc;
            r.superpixels = true;
        }
        rc = r.track ? frame_track(f, r) : frame_dictated_pose(f, r);
        if (rc) return rc;
        if (r.track) fusion_note_view_poses(f, true);
        if (f->fi.on && r.track && r.flow_enqueued && f->flow.has) {
            rc = frame_flow_inference(f);
            if (rc) return rc;
        }
        if (r.track && f->cfg.enable_multiple_models) {
            rc = frame_segment(f, r);
            if (rc) return rc;
        }
        r.stamp(f, 2);
    }
    if (f->kp.tracker) {
        if (r.track && !first) fusion_note_view_poses(f, false);
        rc = frame_associate_tracks(f, first || !f->cfg.enable_multiple_models, r.track);
        if (rc) return rc;
        if (f->kp.backdate_history && f->kp.spawned_id >= 0 && r.track && !first) {  // refineTrackSubset (:596-599)
            rc = frame_backdate(f);
            if (rc) return rc;
        }
    }
    f->sp.next = false;  // (mmf_fusion_set_superpixels: this call's labels only, whichever segmentation ran)
    f->rd.kp_next = false;  // (mmf_fusion_set_keypoints: this call's keypoints only, whether or not a segmentation ran)
    r.pass_mode = fusion_batch_mode(f);  // (the model list stays as it is from here to the end of the call)
    if (!first) {
        rc = frame_fuse_clean(f, r);
        if (rc) return rc;
    }
    r.stamp(f, 3);
    rc = frame_predict(f, r);
    if (rc) return rc;
    r.stamp(f, 4);
    if (f->ferns.engine) {  // processFerns() (:824): behind predict(), with the tick the frame ran under
        rc = frame_ferns(f);
        if (rc) return rc;
        r.ferns = true;
    }
    f->tick++;  // :825
    frame_log_poses(f, r);
    rc = frame_end(f, r);
    if (rc) return rc;
    if (r.flow_enqueued) MMF_HIP_TRY(f->flow.lane.join(f->ctx->stream));
    if (r.ferns) MMF_HIP_TRY(f->ferns.lane.join(f->ctx->stream));
    r.stamp(f, 5);
    if (r.host_trace && ++f->trace_calls % 100 == 0) {
        std::fprintf(stderr, "host us from call start: next image side enqueued %.0f, lanes waiting %.0f, preparation enqueued %.0f (batched chains), chains enqueued %.0f, "
                             "poses here %.0f, segmentation handled %.0f, per-model passes enqueued %.0f, final predicts enqueued %.0f, end %.0f\n",
                     f->trace_us[6] / 100, f->trace_us[7] / 100, f->trace_us[8] / 100, f->trace_us[0] / 100, f->trace_us[1] / 100, f->trace_us[2] / 100,
                     f->trace_us[3] / 100, f->trace_us[4] / 100, f->trace_us[5] / 100);
        for (double& a : f->trace_us) a = 0;
    }
    f->t_frame_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - r.t_begin).count();
    return MMF_OK;
}

extern "C" int mmf_fusion_process_frame_ex(mmf_fusion* f, const mmf_frame* frame) { return fusion_process_frame_impl(f, frame); }

extern "C" int mmf_fusion_process_frame(mmf_fusion* f, const uint8_t* rgb, const float* depth, long long timestamp,
                                        const float* in_pose, float weight_multiplier, int bootstrap) {
    mmf_frame fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.rgb = rgb, fr.depth = depth, fr.timestamp = timestamp;
    fr.in_pose = in_pose, fr.weight_multiplier = weight_multiplier, fr.bootstrap = bootstrap;
    fr.icp_refine = 1;
    return fusion_process_frame_impl(f, &fr);
}

extern "C" int mmf_fusion_process_frame_init(mmf_fusion* f, const uint8_t* rgb, const float* depth, long long timestamp,
                                             const float* init_transform, int icp_refine, float weight_multiplier) {
    MMF_REQUIRE(init_transform != nullptr, "mmf_fusion_process_frame_init: null transformation");
    mmf_frame fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.rgb = rgb, fr.depth = depth, fr.timestamp = timestamp;
    fr.weight_multiplier = weight_multiplier;
    fr.init_transforms = init_transform, fr.n_init_transforms = 1, fr.icp_refine = icp_refine;
    return fusion_process_frame_impl(f, &fr);
}

// MultiMotionFusion::predict (:863-875) as a public call (the GUI re-predicts when a view changes)
extern "C" int mmf_fusion_predict(mmf_fusion* f) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_predict: null fusion object");
    MMF_REQUIRE(f->frame_rgb != nullptr, "mmf_fusion_predict: no frame has been processed yet");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    for (size_t k = 0; k < f->models.size(); ++k) {
        FusionModel* fm = f->models[k];
        if (!fusion_owns(f, k)) continue;
        int rc = fusion_predict_model(f, fm);
        if (rc) return rc;
        if (k > 0) MMF_HIP_TRY(order(fm->lane->stream, fm->ev_done.get(), f->ctx->stream));
    }
    return MMF_OK;
}
