// fusion_hooks.hpp -- where a frame's segmentation comes from (callback, built-in CRF, the frame's label image) and the side
// engines that run on streams of their own beside the tracking chains (super-pixel engine, optical flow, flow-CRF
// inference, fern keyframe database): their setters and getters, fusion_crf_segment / fusion_mask_segment, and the
// frame_superpixels_*, frame_flow_* and frame_ferns stages of processFrame.  Textually included by mmf_hip.hip behind fusion_state.hpp.
#pragma once

extern "C" int mmf_fusion_set_segmentation_callback(mmf_fusion* f, mmf_segmentation_fn fn, void* user) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_segmentation_callback: null fusion object");
    f->seg.fn = fn, f->seg.user = user;
    return MMF_OK;
}
extern "C" int mmf_fusion_set_crf_segmentation(mmf_fusion* f, const mmf_crf_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_crf_segmentation: null fusion object");
    if (!cfg) {
        f->seg.crf_on = false;
        return MMF_OK;
    }
    if (int rc = crf_check_config(cfg, "mmf_fusion_set_crf_segmentation")) return rc;
    f->seg.crf_cfg = *cfg, f->seg.crf_on = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_set_mask_segmentation(mmf_fusion* f, const mmf_mask_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_mask_segmentation: null fusion object");
    if (!cfg) {
        f->seg.mask_on = false;
        return MMF_OK;
    }
    MMF_REQUIRE(cfg->model_spawn_offset >= 0, "mmf_fusion_set_mask_segmentation: model_spawn_offset must not be negative");
    if (f->shard_world != 1)
        return fail(MMF_ERR_STATE, "mmf_fusion_set_mask_segmentation: needs world == 1 (a sharded front end calls mmf_mask_segment "
                                   "in its segmentation callback)");
    f->seg.mask_cfg = *cfg, f->seg.mask_on = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_mask_mapping(mmf_fusion* f, uint8_t mapping_out[256]) {
    MMF_REQUIRE(f && mapping_out, "mmf_fusion_mask_mapping: null argument");
    std::memcpy(mapping_out, f->seg.mask_map, 256);
    return MMF_OK;
}
extern "C" int mmf_fusion_last_mask_segmentation(mmf_fusion* f, mmf_mask_info* info, mmf_segmentation_model* models, int capacity) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_mask_segmentation: null fusion object");
    if (!f->seg.mask_valid) return fail(MMF_ERR_STATE, "mmf_fusion_last_mask_segmentation: no frame has been segmented from its labels yet");
    if (info) *info = f->seg.mask_info;
    if (models)
        for (int i = 0; i < (int)f->seg.mask_models.size() && i < capacity; ++i) models[i] = f->seg.mask_models[(size_t)i];
    return MMF_OK;
}
extern "C" int mmf_fusion_set_superpixels(mmf_fusion* f, const int* labels) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_superpixels: null fusion object");
    f->sp.next = false;
    if (!labels) return MMF_OK;
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->sp.last == f->sp.labels.get()) f->sp.last = nullptr;  // (the copy the last segmentation used is about to be replaced)
    if (!f->sp.labels) MMF_HIP_TRY(f->sp.labels.create((size_t)f->width * f->height));
    MMF_HIP_TRY(hipMemcpyAsync(f->sp.labels.get(), labels, (size_t)f->width * f->height * sizeof(int), hipMemcpyDeviceToDevice, f->ctx->stream));
    f->sp.next = true;
    return MMF_OK;
}
// the engine's streams and label image for the fusion's frame size and the CRF configuration's super-pixel size
static int fusion_sp_engine_prepare(mmf_fusion* f, const char* who) {
    if (int rc = slic_engine_check(f->width, f->height, f->seg.crf_cfg.spixel_size, who)) return rc;
    const int S = f->seg.crf_cfg.spixel_size;
    const size_t cells = (size_t)(f->width / S) * (f->height / S), pixels = (size_t)f->width * f->height;
    if (!f->sp.lane.stream) MMF_HIP_TRY(f->sp.lane.create());
    if (cells > f->sp.ws.cells || pixels > f->sp.ws.pixels) {  // (the setter, or a CRF configuration with a smaller S since)
        MMF_HIP_TRY(hipStreamSynchronize(f->sp.lane.stream.get()));
        if (f->sp.ws.mem && f->sp.last == f->sp.ws.labels()) f->sp.last = nullptr;
        if (int rc = slic_engine_workspace(&f->sp.ws, cells, pixels, f->ctx->stream)) return rc;
    }
    return MMF_OK;
}
extern "C" int mmf_fusion_set_superpixel_engine(mmf_fusion* f, int mode) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_superpixel_engine: null fusion object");
    MMF_REQUIRE(mode == 0 || mode == 1, "mmf_fusion_set_superpixel_engine: mode is 0 (off) or 1 (SLIC from the frame's RGB)");
    if (mode == 0) {
        f->sp.engine = 0;
        return MMF_OK;
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (int rc = fusion_sp_engine_prepare(f, "mmf_fusion_set_superpixel_engine")) return rc;
    f->sp.engine = 1;
    return MMF_OK;
}
extern "C" int mmf_fusion_last_superpixels(mmf_fusion* f, int* labels_out) {
    MMF_REQUIRE(f && labels_out, "mmf_fusion_last_superpixels: null argument");
    if (!f->sp.last) return fail(MMF_ERR_STATE, "mmf_fusion_last_superpixels: no segmentation has run on this fusion (or its labels were replaced)");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(labels_out, f->sp.last, (size_t)f->width * f->height * sizeof(int), hipMemcpyDeviceToDevice, f->ctx->stream));
    MMF_HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return MMF_OK;
}
// The optical-flow hook: cfg != NULL creates the fusion's own engine for its frame size (a second call replaces it: a new
// sequence), NULL frees it with its stream and events.  Off by default; while off no frame allocates, enqueues or waits for
// anything of it.  The configuration is checked before the device is touched.  The flow-inference hook lives on the engine
// that leaves: NULL switches it off as well; a replacement at div 4 switches it on again with the configuration it had (a new
// sequence for it too: no result until the second frame), a replacement at another div leaves it off.
extern "C" int mmf_fusion_set_optical_flow(mmf_fusion* f, const mmf_flow_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_optical_flow: null fusion object");
    if (cfg) {
        if (int rc = flow_check_config(f->width, f->height, cfg, "mmf_fusion_set_optical_flow")) return rc;
        if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_optical_flow: not available on a sharded fusion");
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    const bool rearm = f->fi.on && cfg && cfg->div == 4;
    const mmf_flowcrf_config fi_cfg = f->fi.cfg;
    f->fseg.reset();                 // (the flow_crf mode reads the inference: a replaced flow engine ends it as well)
    f->fi.reset(), f->flow.reset();  // (the inference lives on the flow's stream and reads the flow: it goes first)
    if (!cfg) return MMF_OK;
    if (int rc = flow_create_impl(f->ctx, f->width, f->height, cfg, &f->flow.engine, "mmf_fusion_set_optical_flow")) return rc;
    const hipError_t e = f->flow.lane.create();
    if (e != hipSuccess) {
        f->flow.reset();
        return fail(MMF_ERR_HIP, std::string("mmf_fusion_set_optical_flow: ") + hipGetErrorString(e));
    }
    return rearm ? mmf_fusion_set_flow_inference(f, &fi_cfg) : MMF_OK;
}
// The flow of the last processFrame call from the frame before it: DEVICE pointers into the hook's engine (flow [h][w][2],
// magnitude and motion [h][w]), complete for work enqueued on the context's stream behind that call (or after
// mmf_ctx_synchronize) and valid until the next frame, reset or setter call.  *has_flow = 0 (and null pointers) after the
// first frame of a sequence.  MMF_ERR_STATE while the hook is off.
extern "C" int mmf_fusion_last_flow(mmf_fusion* f, const float** flow_dev, const float** magnitude_dev, const float** motion_dev, int* w,
                                    int* h, int* has_flow) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_flow: null fusion object");
    if (!f->flow.engine) return fail(MMF_ERR_STATE, "mmf_fusion_last_flow: the optical-flow hook is off (mmf_fusion_set_optical_flow)");
    if (flow_dev) *flow_dev = nullptr;
    if (magnitude_dev) *magnitude_dev = nullptr;
    if (motion_dev) *motion_dev = nullptr;
    if (w) *w = f->flow.engine->geo.W;
    if (h) *h = f->flow.engine->geo.H;
    if (has_flow) *has_flow = f->flow.has ? 1 : 0;
    if (!f->flow.has) return MMF_OK;
    return mmf_flow_result(f->flow.engine, flow_dev, magnitude_dev, motion_dev, nullptr, nullptr);
}

// The flow-CRF inference hook: cfg != NULL switches it on (a second call replaces the configuration), NULL off -- the engine
// and its events are freed, and no frame allocates, enqueues or waits for anything.  It reads the optical-flow hook's result.
extern "C" int mmf_fusion_set_flow_inference(mmf_fusion* f, const mmf_flowcrf_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_flow_inference: null fusion object");
    if (cfg) {
        if (int rc = flowcrf_check_config(f->width, f->height, mmf::kCrfMaxLabels, 0, cfg, "mmf_fusion_set_flow_inference")) return rc;
        if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_inference: not available on a sharded fusion");
        if (!f->flow.engine) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_inference: the optical-flow hook is off (mmf_fusion_set_optical_flow)");
        if (f->flow.engine->cfg.div != 4) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_inference: the optical-flow hook must run at div 4");
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (!cfg) f->fseg.reset();  // (the flow_crf mode reads this hook's id image)
    f->fi.reset();
    if (!cfg) return MMF_OK;
    hipError_t e = f->fi.begin.create();
    if (e == hipSuccess) e = f->fi.inputs.create();
    if (e != hipSuccess) {
        f->fi.reset();
        return fail(MMF_ERR_HIP, std::string("mmf_fusion_set_flow_inference: ") + hipGetErrorString(e));
    }
    f->fi.cfg = *cfg, f->fi.stream = f->flow.lane.stream.get(), f->fi.on = true;
    return MMF_OK;
}

// The id images of the last processFrame call: DEVICE pointers into the hook's engine (ids [h][w], ids_full [height][width]),
// complete on the fusion's stream and valid until the next frame, reset or setter call.  *has_result = 0 (and null pointers)
// after a frame without a flow (the first of a sequence) or without tracking.
extern "C" int mmf_fusion_last_flow_inference(mmf_fusion* f, const uint8_t** ids_dev, const uint8_t** ids_full_dev, int* w, int* h,
                                              int* n_labels, int* has_result) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_flow_inference: null fusion object");
    if (!f->fi.on) return fail(MMF_ERR_STATE, "mmf_fusion_last_flow_inference: the flow-inference hook is off (mmf_fusion_set_flow_inference)");
    if (ids_dev) *ids_dev = nullptr;
    if (ids_full_dev) *ids_full_dev = nullptr;
    if (w) *w = f->width / 4;
    if (h) *h = f->height / 4;
    if (n_labels) *n_labels = 0;
    if (has_result) *has_result = f->fi.has ? 1 : 0;
    if (!f->fi.has) return MMF_OK;
    return mmf_flowcrf_result(f->fi.engine, ids_dev, ids_full_dev, nullptr, nullptr, nullptr, nullptr, n_labels);
}
// A stage image of the last call's inference to HOST memory, as mmf_flowcrf_download (tests: "E" shows the poses and the track
// table the hook handed its engine).  MMF_ERR_STATE while the hook is off and after a frame without a result.
extern "C" int mmf_fusion_flow_inference_download(mmf_fusion* f, const char* name, void* host_dst, size_t bytes) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_flow_inference_download: null fusion object");
    if (!f->fi.on) return fail(MMF_ERR_STATE, "mmf_fusion_flow_inference_download: the flow-inference hook is off (mmf_fusion_set_flow_inference)");
    if (!f->fi.has) return fail(MMF_ERR_STATE, "mmf_fusion_flow_inference_download: the last frame has no result");
    return mmf_flowcrf_download(f->fi.engine, name, host_dst, bytes);
}
extern "C" int mmf_fusion_last_segmentation(mmf_fusion* f, mmf_crf_info* info, mmf_segmentation_model* models, int capacity,
                                            float* unaries, float* q, uint8_t* raw_map, uint8_t* map) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_segmentation: null fusion object");
    return mmf_crf_last(f->ctx, info, models, capacity, unaries, q, raw_map, map);
}

// The engine's label image of this frame.  It depends on the frame's RGB only, so it runs on a lane of its own beside the
// tracking chains and fusion_crf_segment joins it in front of stage 1.  Two halves: the lane is opened on the fusion's
// stream when the frame begins (the RGB is there; the last segmentation that read the label image ended in a host wait),
// the twelve launches are enqueued once the chains are, while the host would only wait for the poses -- in front of the
// chains their enqueue is host time the whole frame waits for.  Only when this frame's segmentation will be the built-in
// one on the engine's labels.
static int frame_superpixels_begin(mmf_fusion* f) {
    if (int rc = fusion_sp_engine_prepare(f, "mmf_fusion_process_frame (super-pixel engine)")) return rc;
    MMF_HIP_TRY(f->sp.lane.open(f->ctx->stream));  // (pending: a frame that failed between the engine and its segmentation)
    return MMF_OK;
}
static int frame_superpixels_enqueue(mmf_fusion* f, const uint8_t* rgb) {
    MMF_HIP_TRY(f->sp.lane.enter());
    if (int rc = slic_engine_enqueue(f->sp.ws, f->sp.lane.stream.get(), rgb, f->width, f->height, f->seg.crf_cfg.spixel_size, 5, nullptr,
                                     nullptr, nullptr, nullptr))
        return rc;
    MMF_HIP_TRY(f->sp.lane.close());
    return MMF_OK;
}

// The optical flow of this frame from the one before it (mmf_fusion_set_optical_flow).  Like the label image it depends on
// the frame's RGB only.  The flow's lane is opened on the fusion's stream when the call begins: the RGB is on the device
// there (a host frame's upload has been joined), and whatever read the last frame's flow on that stream is done.  The
// launches go to the lane behind that -- on a tracked frame once the chains are enqueued, as the super-pixel engine's do --
// and the fusion's stream joins the lane at the end of the call.
static int frame_flow_enqueue(mmf_fusion* f, const uint8_t* rgb) {
    MMF_HIP_TRY(f->flow.lane.enter());
    int has = 0;
    f->flow.has = false;
    if (int rc = flow_next_on(f->flow.engine, rgb, f->flow.lane.stream.get(), &has)) return rc;
    MMF_HIP_TRY(f->flow.lane.close());
    f->flow.has = has != 0;
    return MMF_OK;
}

// The flow-CRF inference of this frame (mmf_fusion_set_flow_inference), where the reference segments: behind the tracking, on
// the predictions the frame was tracked against (nothing has rewritten them yet: frame_enqueue_ahead stands back while the
// hook is on).  The active models in list order, the new label when models may spawn; T_start = prev_pose pose^-1 and
// T_end = pose pose^-1 (Model.cpp:556-557: poses.back() is this frame's pose, tracked or -- with the refinement off --
// initialised; poses[-2] is the pose the frame before ended with, whatever overridePose has done to lastPose since); the
// attached tracker's table, if any.  On the flow stream behind the flow; the fusion's stream and the models' streams wait
// until the inference has read the predictions and the table (two launches), the rest is joined with the flow's lane.
// A frame with more labels than the engine takes has no result (has_result 0): the hook fails no frame.
static int frame_flow_inference(mmf_fusion* f) {
    mmf_ctx* c = f->ctx;
    // under the flow_crf mode the new label is there when a model may spawn (MultiMotionFusion.cpp:148, with the count
    // frame_segment is about to give this frame, :410), else whenever models may spawn at all
    const bool mode = f->fseg.on && f->cfg.enable_multiple_models;
    const int M = (int)f->models.size();
    const unsigned spawn_after = (unsigned)f->fseg.cfg.model_spawn_offset;
    const int allow_new = mode ? (f->seg.spawn_offset + (f->seg.spawn_offset < spawn_after ? 1u : 0u) >= spawn_after ? 1 : 0)
                               : (f->cfg.enable_multiple_models ? 1 : 0);
    const int L = M + allow_new;
    if (L > mmf::kCrfMaxLabels) return MMF_OK;
    const int cap = f->kp.tracker ? f->kp.tracker->capacity : 0;
    if (!f->fi.engine || f->fi.engine->max_labels < L || f->fi.engine->max_tracks < cap) {
        if (f->fi.engine) flowcrf_destroy_on(f->fi.engine, f->flow.lane.stream.get());
        f->fi.engine = nullptr;
        int rc = flowcrf_create_impl(c, f->width, f->height, std::max(4, flowcrf_pad_labels(L)), cap, f->fx, f->fy, f->cx, f->cy, &f->fi.cfg,
                                     &f->fi.engine, "mmf_fusion_process_frame (flow inference)");
        if (rc) return rc;
    }
    unsigned char ids[mmf::kCrfMaxLabels];
    const float* vertex[mmf::kCrfMaxLabels];
    std::vector<float> T((size_t)2 * 16 * M);
    for (int k = 0; k < M; ++k) {
        FusionModel* fm = f->models[(size_t)k];
        float pose[16], inv[16];
        mmf_model_get_pose(fm->model, pose);
        inverse4f_host(pose, inv);
        mmf::host::matmul4(fm->prev_pose, inv, T.data() + 16 * (size_t)k);
        mmf::host::matmul4(pose, inv, T.data() + 16 * (size_t)(M + k));
        ids[k] = fm->model->id;
        vertex[k] = reinterpret_cast<const float*>(fm->model->vertexConf);
        if (fm->lane->stream != c->stream)  // (its last prediction ran there)
            MMF_HIP_TRY(order(fm->lane->stream, fm->ev_done.get(), f->flow.lane.stream.get()));
    }
    mmf_flowcrf_input in;
    std::memset(&in, 0, sizeof(in));
    in.n_models = M, in.allow_new = allow_new, in.new_id = (unsigned)mmf_fusion_next_model_id(f), in.ids = ids;
    in.T_start = T.data(), in.T_end = T.data() + 16 * (size_t)M, in.vertex = vertex, in.depth = f->frame_depth;
    int rc = mmf_flow_result(f->flow.engine, &in.flow, nullptr, &in.motion, nullptr, nullptr);
    if (rc) return rc;
    if (int bad = flowcrf_check_input(f->fi.engine, &in, "mmf_fusion_process_frame (flow inference)")) return bad;
    mmf::FcrfTracks tr;
    rc = flowcrf_tracker_view(f->fi.engine, f->kp.tracker, &tr, "mmf_fusion_process_frame (flow inference)");
    if (rc) return rc;
    MMF_HIP_TRY(order(c->stream, f->fi.begin.get(), f->flow.lane.stream.get()));
    rc = flowcrf_run_on(f->fi.engine, &in, tr, f->flow.lane.stream.get(), f->fi.inputs.get());
    if (rc) return rc;
    MMF_HIP_TRY(f->flow.lane.close());  // (again: the join at the end of the call waits for the inference as well)
    MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->fi.inputs.get(), 0));
    for (FusionModel* fm : f->models)
        if (fm->lane->stream != c->stream) MMF_HIP_TRY(hipStreamWaitEvent(fm->lane->stream, f->fi.inputs.get(), 0));
    f->fi.has = true;
    f->fi.allow_new = allow_new;
    return MMF_OK;
}

// What both built-in segmentations start from: world == 1 (`sharded`: the path's own message), the active models' ids in
// list order, the id a new segment gets, and whether one may appear (`spawn_after`: the path's model_spawn_offset, :148)
struct SegLabels {
    std::vector<unsigned> ids;
    unsigned next_id = 0;
    int allow_new = 0;
};
static int fusion_seg_labels(mmf_fusion* f, const char* sharded, int spawn_after, SegLabels* l) {
    if (f->shard_world != 1) return fail(MMF_ERR_STATE, sharded);
    for (const FusionModel* fm : f->models) l->ids.push_back((unsigned)fm->model->id);
    l->next_id = (unsigned)mmf_fusion_next_model_id(f);
    l->allow_new = f->seg.spawn_offset >= (unsigned)spawn_after ? 1 : 0;
    return MMF_OK;
}
// ... and end with: textures[MASK], the summary's flag, and the path's own list of model entries
static void fusion_seg_result(mmf_fusion* f, int has_new_label, const std::vector<mmf_segmentation_model>& models, mmf_segmentation* out) {
    std::memset(out, 0, sizeof(*out));
    out->mask = f->mask.get();
    out->has_new_label = has_new_label;
    out->n_models = (int)models.size();
    out->model_data = models.data();
}

// performSegmentationCRF (Segmentation.cpp:159-740) on the fusion's stream, into textures[MASK]: stage 1 from every model's
// ICP-error image and the confidence of its splat (the previous frame's prediction), then crf_enqueue; one pinned read of
// the summary.  `out` points at f->mask and f->seg.crf_models.
static int fusion_crf_segment(mmf_fusion* f, mmf_segmentation* out) {
    mmf_ctx* c = f->ctx;
    const mmf_crf_config& cfg = f->seg.crf_cfg;
    SegLabels l;
    if (int rc = fusion_seg_labels(f, "mmf_fusion_process_frame: the built-in segmentation needs world == 1 (a sharded front end "
                                      "calls mmf_crf_segment in its segmentation callback)", cfg.model_spawn_offset, &l))
        return rc;
    const int M = (int)l.ids.size(), W = f->width, H = f->height, S = cfg.spixel_size;
    CrfWs* w = nullptr;
    const int* labels = nullptr;
    // labels handed in for this frame, then the engine's, then the grid (B3)
    const bool engine = !f->sp.next && f->sp.engine;
    if (engine && !f->sp.lane.pending) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the super-pixel engine did not run for this frame");
    int rc = crf_begin(c, &cfg, f->sp.next ? f->sp.labels.get() : (engine ? f->sp.ws.labels() : nullptr), W, H, l.ids.data(), M, l.next_id,
                       l.allow_new, "mmf_fusion_process_frame (segmentation)", &w, &labels);
    if (rc) return rc;
    f->sp.last = labels;
    if (engine) MMF_HIP_TRY(f->sp.lane.join(c->stream));
    // behind every model's tracking chain: the chains write the ICP-error images on the models' streams
    for (FusionModel* fm : f->models)
        if (fm->lane->stream != c->stream) MMF_HIP_TRY(order(fm->lane->stream, fm->ev_done.get(), c->stream));
    const int N = (W / S) * (H / S);
    rc = mmf_slic_downsample(c, labels, W, H, S, f->frame_depth, 1, 0, 1, 0.02f, w->low_depth, nullptr);  // :178
    for (int i = 0; i < M && rc == MMF_OK; ++i) {  // :218-219
        FusionModel* fm = f->models[(size_t)i];
        if (!fm->icp_error) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the built-in segmentation needs error_recording");
        rc = mmf_slic_downsample(c, labels, W, H, S, fm->icp_error, 1, 0, 0, 0.f, w->maps + (size_t)i * 2 * N, nullptr);
        if (rc == MMF_OK)
            rc = mmf_slic_downsample(c, labels, W, H, S, reinterpret_cast<const float*>(fm->model->vertexConf), 4, 3, 0, 0.f,
                                     w->maps + ((size_t)i * 2 + 1) * N, nullptr);
    }
    if (rc) return rc;
    rc = crf_enqueue(c, w, &cfg, labels, W, H, f->frame_rgb, w->maps, l.ids.data(), M, l.next_id, l.allow_new, f->mask.get());
    if (rc) return rc;
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    const mmf::CrfSummary& s = *w->sum_host;
    f->seg.crf_models.assign(s.models, s.models + s.n_models_out);
    // inhibitModels (:413-415): the mask and the entry stay
    fusion_seg_result(f, s.has_new_label && !cfg.inhibit_new, f->seg.crf_models, out);
    return MMF_OK;
}

// The `frame.mask` branch of performSegmentation (Segmentation.cpp:89-147) on the fusion's stream: `labels` (the frame's raw
// label image, uploaded on this stream or handed in as a device image) into textures[MASK], one pinned read of the summary.
// `out` points at f->mask and f->seg.mask_models.
static int fusion_mask_segment(mmf_fusion* f, const uint8_t* labels, mmf_segmentation* out) {
    mmf_ctx* c = f->ctx;
    SegLabels l;
    if (int rc = fusion_seg_labels(f, "mmf_fusion_process_frame: the segmentation from the frame's labels needs world == 1 (a sharded "
                                      "front end calls mmf_mask_segment in its segmentation callback)", f->seg.mask_cfg.model_spawn_offset, &l))
        return rc;
    MaskWs* w = nullptr;
    int rc = mask_enqueue(c, f->width, f->height, labels, f->frame_depth, l.ids.data(), (int)l.ids.size(), l.next_id, l.allow_new,
                          f->seg.mask_map, f->mask.get(), "mmf_fusion_process_frame (segmentation from labels)", &w);
    if (rc) return rc;
    MMF_HIP_TRY(wait_stream(c->stream));
    const mmf::MaskSummary& s = *w->sum_host;
    std::memcpy(f->seg.mask_map, s.mapping, 256);
    f->seg.mask_models.assign(s.models, s.models + s.n_models_out);
    // inhibitModels (:413-415): the mask and the entry stay
    fusion_seg_result(f, s.has_new_label && !f->seg.mask_cfg.inhibit_new, f->seg.mask_models, out);
    f->seg.mask_info.n_models = s.n_models_out, f->seg.mask_info.allow_new = l.allow_new;
    f->seg.mask_info.has_new_label = out->has_new_label, f->seg.mask_info.new_label = s.new_label;
    f->seg.mask_valid = true;
    return MMF_OK;
}

// The flow_crf mode (mmf_fusion_set_flow_segmentation): cfg != NULL switches it on (a second call replaces the configuration),
// NULL off -- the engine is freed, and no frame allocates, enqueues or waits for anything.  It reads the inference hook's ids.
extern "C" int mmf_fusion_set_flow_segmentation(mmf_fusion* f, const mmf_flowseg_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_flow_segmentation: null fusion object");
    if (cfg) {
        if (int rc = flowseg_check_config(f->width, f->height, mmf::kCrfMaxLabels, cfg, "mmf_fusion_set_flow_segmentation")) return rc;
        if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_segmentation: not available on a sharded fusion");
        if (!f->fi.on) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_segmentation: the flow-inference hook is off (mmf_fusion_set_flow_inference)");
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    f->fseg.reset();
    if (!cfg) return MMF_OK;
    f->fseg.cfg = *cfg, f->fseg.on = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_last_flow_segmentation(mmf_fusion* f, mmf_flowseg_summary* summary, int* has_result) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_flow_segmentation: null fusion object");
    if (!f->fseg.valid) return fail(MMF_ERR_STATE, "mmf_fusion_last_flow_segmentation: no frame has been segmented by the flow_crf mode yet");
    if (summary) *summary = f->fseg.last;
    if (has_result) *has_result = f->fseg.has ? 1 : 0;
    return MMF_OK;
}

// Segmentation.cpp:1270-1324 on the fusion's stream, into textures[MASK]: the blob stage on the id image the inference of this
// frame left on the flow's lane (frame_flow_inference: the lane's event is joined here), one pinned read of the summary.  `out`
// points at f->mask and f->fseg.models.  A frame without an inference result -- no flow yet, more than 32 labels -- gets a
// zero mask, no entries and no new label (deviation 1): frame_segment then moves nobody's unseen count, max
// depth or confidence threshold.
static int fusion_flow_segment(mmf_fusion* f, mmf_segmentation* out) {
    mmf_ctx* c = f->ctx;
    std::memset(&f->fseg.last, 0, sizeof(f->fseg.last));
    f->fseg.models.clear();
    f->fseg.valid = true, f->fseg.has = false;
    if (!f->fi.has) {
        MMF_HIP_TRY(hipMemsetAsync(f->mask.get(), 0, (size_t)f->width * f->height, c->stream));
        fusion_seg_result(f, 0, f->fseg.models, out);
        out->model_data = nullptr;  // (an empty vector's data() may be anything)
        return MMF_OK;
    }
    SegLabels l;
    if (int rc = fusion_seg_labels(f, "mmf_fusion_process_frame: the flow_crf mode needs world == 1", f->fseg.cfg.model_spawn_offset, &l)) return rc;
    const int M = (int)l.ids.size(), allow_new = f->fi.allow_new, L = M + allow_new;
    if (!f->fseg.engine || f->fseg.engine->max_labels < L) {
        flowseg_destroy_on(f->fseg.engine, nullptr);
        f->fseg.engine = nullptr;
        int rc = flowseg_create_impl(c, f->width, f->height, std::max(4, flowcrf_pad_labels(L)), &f->fseg.cfg, &f->fseg.engine,
                                     "mmf_fusion_process_frame (flow_crf mode)");
        if (rc) return rc;
    }
    unsigned char ids[mmf::kCrfMaxLabels];
    for (int k = 0; k < M; ++k) ids[k] = (unsigned char)l.ids[(size_t)k];
    mmf::FsegTable tab;
    if (int rc = flowseg_table(f->fseg.engine, ids, M, allow_new, l.next_id, &tab, "mmf_fusion_process_frame (flow_crf mode)")) return rc;
    const uint8_t* ids_dev = nullptr;
    if (int rc = mmf_flowcrf_result(f->fi.engine, &ids_dev, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    MMF_HIP_TRY(f->flow.lane.join(c->stream));  // the inference is complete before the blob stage reads its ids
    if (int rc = flowseg_run_on(f->fseg.engine, ids_dev, f->frame_depth, tab, c->stream, f->mask.get())) return rc;
    MMF_HIP_TRY(wait_stream(c->stream));
    mmf_flowseg_summary s = *f->fseg.engine->sum_host;
    f->fseg.models.assign(s.models, s.models + s.n_entries);
    // inhibitModels (:413-415): the mask and the entry stay
    s.has_new_label = s.has_new_label && !f->fseg.cfg.inhibit_new ? 1 : 0;
    fusion_seg_result(f, s.has_new_label, f->fseg.models, out);
    f->fseg.last = s, f->fseg.has = true;
    return MMF_OK;
}

// The fern keyframe database hook: cfg != NULL creates the fusion's own engine for its frame size (a second call replaces it:
// an empty database), NULL frees it with its stream and events.  Off by default; while off no frame allocates, enqueues or
// waits for anything of it.  The configuration and the table are checked before the device is touched.
extern "C" int mmf_fusion_set_fern_database(mmf_fusion* f, const mmf_ferns_config* cfg, const int* table) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_fern_database: null fusion object");
    std::vector<int> own;
    if (cfg) {
        if (int rc = ferns_check_config(f->width, f->height, cfg, table, "mmf_fusion_set_fern_database")) return rc;
        if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_fern_database: not available on a sharded fusion");
        if (!f->models[0]->fill_in) return fail(MMF_ERR_STATE, "mmf_fusion_set_fern_database: the camera model has no fill-in images");
        if (!table) {
            own.resize((size_t)cfg->num * 6);
            if (int rc = mmf_ferns_make_table(0ull, cfg->num, f->width / 8, f->height / 8, cfg->max_depth_mm, own.data())) return rc;
            table = own.data();
        }
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    f->ferns.reset();
    if (!cfg) return MMF_OK;
    if (int rc = ferns_create_impl(f->ctx, f->width, f->height, cfg, table, &f->ferns.engine, "mmf_fusion_set_fern_database")) return rc;
    const hipError_t e = f->ferns.lane.create();
    if (e != hipSuccess) {
        f->ferns.reset();
        return fail(MMF_ERR_HIP, std::string("mmf_fusion_set_fern_database: ") + hipGetErrorString(e));
    }
    return MMF_OK;
}
extern "C" int mmf_fusion_last_fern_result(mmf_fusion* f, mmf_ferns_result_t* out) {
    MMF_REQUIRE(f != nullptr && out != nullptr, "mmf_fusion_last_fern_result: null argument");
    if (!f->ferns.engine) return fail(MMF_ERR_STATE, "mmf_fusion_last_fern_result: the fern database is off (mmf_fusion_set_fern_database)");
    if (!f->ferns.has) return fail(MMF_ERR_STATE, "mmf_fusion_last_fern_result: no frame has run since the hook went on or the last reset");
    return mmf_ferns_result(f->ferns.engine, out);
}
extern "C" mmf_ferns* mmf_fusion_fern_database(mmf_fusion* f) { return f ? f->ferns.engine : nullptr; }

// processFerns() (MultiMotionFusion.cpp:824, :856-860) with the query of findFrame (:682-685) in front of it: process(FIND | ADD)
// on the camera model's fill-in images, its pose and the frame's tick.  Behind the end-of-frame predict(): the lane opens on the
// camera model's stream, where that prediction has just been enqueued; the fusion's stream joins the lane at the end of the
// call, in front of whatever rewrites those images.
static int frame_ferns(mmf_fusion* f) {
    FusionModel* cam = f->models[0];
    const mmf_model* m = cam->model;
    float pose[16];
    mmf_model_get_pose(cam->model, pose);
    MMF_HIP_TRY(f->ferns.lane.open(cam->lane->stream));  // (pending: a frame that failed between the enqueue and the join)
    MMF_HIP_TRY(f->ferns.lane.enter());
    int rc = ferns_process_on(f->ferns.engine, m->fill_image, m->fill_vertex, m->fill_normal, pose, f->tick, MMF_FERNS_FIND | MMF_FERNS_ADD,
                              f->ferns.lane.stream.get(), "mmf_fusion_process_frame (fern database)");
    if (rc) return rc;
    MMF_HIP_TRY(f->ferns.lane.close());
    f->ferns.has = true;
    return MMF_OK;
}
