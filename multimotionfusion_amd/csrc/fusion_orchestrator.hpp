// fusion_orchestrator.hpp -- MultiMotionFusion::processFrame / predict (Core/MultiMotionFusion.cpp:207-854,
// 863-875) for a list of rigid-body models: the global (camera) model plus the object models the segmentation
// spawns.  Textually included at the end of mmf_hip.hip (it uses that file's static helpers and
// model_host.hpp's enqueuers of the surfel passes).
//
// The segmentation is handed in per frame (mmf_segmentation: the reference's gSLICr + dense CRF), pulled through a
// callback at the point where the reference calls performSegmentation (:412), computed from the frame's raw label image
// (mask_kernels.hpp, mmf_fusion_set_mask_segmentation: the `frame.mask` branch of Segmentation.cpp:89-147, which comes
// first as it does there) or by the built-in dense CRF (crf_kernels.hpp, mmf_fusion_set_crf_segmentation).  What stays
// with the caller: relocalisation, ferns, deformation (closeLoops / reloc off).
//
// MI355X mapping: every model owns a LANE (a child context: its own stream + reduction scratch), so the
// latency-bound Gauss-Newton chains of different models (19 x two small launches each) overlap on the device;
// the chains of all models are enqueued before the first result is awaited.  What depends on the sensor frame
// only (bilateral filter, depth / intensity pyramids, vertex / normal maps, gradients) is computed ONCE on the
// fusion's own stream and aliased by every model's odometry -- the reference shares just the depth pyramid
// (Model::GPUSetup::depth_tmp, Model.h:103) and recomputes the rest per model.
#pragma once

#include <chrono>
#include <vector>

struct PoseLogItem {  // Model::PoseLogItem (Model.h:326-329)
    long long ts;
    float p[7];  // x y z qx qy qz qw
};

struct FusionModel {  // one ModelPointer of the reference's `models` list
    mmf_ctx* lane = nullptr;  // stream + reduction scratch (models[0]: the fusion's own context)
    bool own_lane = false;
    mmf_model* model = nullptr;
    mmf_odom* odom = nullptr;  // Model::frameToModel
    float last_pose[16];       // Model::lastPose
    // the pose the model came into the running frame with, i.e. the one the frame before left it (frame_init_poses): while a
    // frame runs this is the reference's poses[-2] -- overridePose changes pose and lastPose but logs nothing; every frame
    // logs one pose per model, tracked (Model.cpp:430) or not (MultiMotionFusion.cpp:385).  Read by the flow inference only.
    float prev_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int fill_in = 0;           // Model::allowsFillIn()
    long long unseen = 0;      // Model::unseenCount
    float* icp_error = nullptr;  // Model::icpError / rgbError (R32F, enableErrorRecording)
    float* rgb_error = nullptr;
    hipEvent_t ev_done = nullptr;
    bool tracking = false;  // a tracking call is in flight on the lane
    bool early_done = false;  // this frame's predict() + first predictIndices went out before the pose reached the host
    bool early_fused = false;  // ... and so did its fuse / predictIndices / clean
    // The model side of the tracker's preparation (prediction -> model pyramids in the global frame, point clouds,
    // intensity pyramid: Model::initICP's initICPModel / initRGBModel, Model.cpp:396-401) needs nothing of the next
    // sensor frame.  When this process runs ONE model it is enqueued at the END of a frame, behind the final predict(),
    // where the model's stream would otherwise idle until the side streams have finished the next frame's sensor side;
    // the next processFrame uses it if nothing it was computed from has changed since (pose, images, mode), else
    // prepares as before.
    bool spec_valid = false, spec_hit = false;
    float spec_pose[16];
    unsigned long long spec_tex_gen = 0;
    int spec_f2f = 0;
    std::vector<PoseLogItem> pose_log;
};

struct mmf_fusion {
    mmf_ctx* ctx = nullptr;
    mmf_fusion_config cfg;
    int width = 0, height = 0;
    float cx = 0, cy = 0, fx = 0, fy = 0;
    std::vector<FusionModel*> models;        // active; models[0] = globalModel
    std::vector<FusionModel*> preallocated;  // preallocatedModels (MultiMotionFusion.h:349)
    std::vector<FusionModel*> inactive;      // inactiveModels
    std::vector<int> scheduled_deactivation;
    int next_id = 0;                  // nextID (getNextModelID)
    // per-rigid-body shard: this process owns the models whose id has id % shard_world == shard_rank
    // (fusion_owner_of) and runs their track / predict / fuse / clean; the others only exist as bookkeeping here (ids,
    // thresholds, poses handed in through mmf_fusion_set_model_pose) -- their owners run on other GPUs
    int shard_rank = 0, shard_world = 1;
    double t_tracking_s = 0, t_frame_s = 0;  // host wall clock of the last processFrame: tracking phase, whole call
    double trace_us[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // MMF_HOST_TRACE
    long trace_calls = 0;
    float* depth_filtered = nullptr;  // = filtered[cur]
    uint8_t* mask = nullptr;          // textures[MASK]: all zeros unless enableMultipleModels
    bool mask_is_zero = false;
    int tick = 1;                     // MultiMotionFusion.cpp:36
    unsigned extent_seq = 0;          // number of the frame whose model-side preparation notes extents (extent.hpp): only ever grows
    unsigned long long* mask_boxes = nullptr;  // pass_rect.hpp: the boxes of the ids of the frame's id image (device, 256 x 4 words)
    unsigned mask_gen = 0;
    int tracking_ok = 1;
    const uint8_t* frame_rgb = nullptr;  // this frame's inputs (device), kept for predict()
    const float* frame_depth = nullptr;
    mmf_segmentation_fn seg_fn = nullptr;
    void* seg_user = nullptr;
    // the built-in segmentation (mmf_fusion_set_crf_segmentation): off unless configured
    bool crf_on = false;
    mmf_crf_config crf_cfg;          // (mmf_crf_default_config at creation: model_spawn_offset is read either way)
    unsigned spawn_offset = 0;       // MultiMotionFusion::spawnOffset (MultiMotionFusion.h:433)
    int* sp_labels = nullptr;        // mmf_fusion_set_superpixels: the next frame's label image (a copy)
    bool sp_next = false;
    // the super-pixel engine (mmf_fusion_set_superpixel_engine): the frame's label image from its RGB, on a stream of its
    // own beside the tracking chains; nothing below exists until the engine is switched on
    int sp_engine = 0;
    SlicEngineWs sp_ws;
    hipStream_t sp_stream = nullptr;
    hipEvent_t ev_sp_begin = nullptr;  // fusion stream: the frame's RGB is there, the last segmentation has read the labels
    hipEvent_t ev_sp_done = nullptr;   // engine stream: this frame's labels are complete
    bool sp_enqueued = false;          // ev_sp_done is recorded and nothing has waited for it yet
    const int* sp_last = nullptr;      // the label image the last segmentation used (handed in, the engine's, or the grid)
    // the optical-flow engine (mmf_fusion_set_optical_flow; flow_host.hpp): every frame's dense flow from the frame before
    // it, on a stream of its own beside the tracking chains; nothing below exists while the hook is off
    mmf_flow* flow = nullptr;            // owned
    hipStream_t flow_stream = nullptr;
    hipEvent_t ev_flow_begin = nullptr;  // fusion stream: the frame's RGB is on the device, the last flow's readers are done
    hipEvent_t ev_flow_done = nullptr;   // flow stream: this frame's flow is complete
    bool flow_pending = false;           // ev_flow_done is recorded and the fusion's stream has not waited for it yet
    bool flow_has = false;               // the last frame produced a flow (not the first frame, nor the first after a reset)
    // the flow-CRF inference (mmf_fusion_set_flow_inference; flowcrf_host.hpp): on the flow stream behind the flow, on every
    // tracked frame that has one; observational.  Nothing below exists while the hook is off
    bool fi_on = false;
    mmf_flowcrf_config fi_cfg{};
    mmf_flowcrf* fi = nullptr;          // owned; created by the first frame that needs it, for its labels and the tracker's capacity
    hipEvent_t ev_fi_begin = nullptr;   // fusion stream: the tracking is done, the track table and the predictions are as the frame met them
    hipEvent_t ev_fi_inputs = nullptr;  // flow stream: the inference has read them
    bool fi_has = false;                // the last frame produced an id image
    std::vector<mmf_segmentation_model> crf_models;
    // the segmentation from the frame's raw label image (mmf_fusion_set_mask_segmentation): off unless configured
    bool mask_on = false;
    mmf_mask_config mask_cfg;
    uint8_t mask_map[256] = {0};     // Segmentation.cpp:92: input label -> model id, from frame to frame
    bool mask_valid = false;         // a frame went through this path (mmf_fusion_last_mask_segmentation)
    mmf_mask_info mask_info;
    std::vector<mmf_segmentation_model> mask_models;
    // keypoint redetection of inactive models (MultiMotionFusion.cpp:489-559; redetect_host.hpp): off unless switched on
    bool redetect_on = false;
    int redetect_verifier = 0;             // mmf_fusion_set_redetection_verifier: 0 = host, 1 = device
    mmf_ransac_batch* verifier = nullptr;  // owned; attached to `views` while the mode is 1
    int host_verified = 0;                 // segments too large for the verifier, verified on the host under its rule
    mmf_viewstore* views = nullptr;  // the stored keypoint views of the inactive models (created on first use)
    bool kp_next = false;            // mmf_fusion_set_keypoints: the NEXT frame's keypoints
    std::vector<int> kp_xy;
    std::vector<float> kp_coord, kp_desc;
    int *kp_xy_pin = nullptr, *kp_label_pin = nullptr;  // host memory the gather kernel reads / writes
    size_t kp_cap = 0;
    std::vector<mmf_redetection> redetections;  // what the last frame's redetection did
    // keypoint tracks (tracker_host.hpp; mmf_fusion_set_tracker): not owned, off unless attached
    mmf_tracker* tracker = nullptr;
    bool trk_init_kp = false, trk_icp_refine = true;
    std::vector<int> trk_ids;      // the active models' ids at the last association
    std::vector<float> trk_T;      // the transformations the last frame's models were initialised with, list order
    // the keypoint front end inside processFrame (mmf_fusion_set_keypoint_frontend): not owned, off unless set
    mmf_superpoint* kpfe_sp = nullptr;
    mmf_keypoint_frontend_config kpfe_cfg{};
    long long kpfe_caller_adds = 0;  // the tracker's caller_adds when the front end last looked
    // the models' keypoint views on deactivation (Model::store, Model.cpp:1617-1644): active only with redetection on and an
    // attached tracker that keeps a view log.  Per object model the list of (tracker stamp, pose after that frame's tracking)
    // -- Model::poses, host memory, trimmed to the log's length -- and what the last frame stored
    struct ViewPose {
        int stamp;
        float pose[16];
    };
    std::map<int, std::vector<ViewPose>> view_poses;
    std::vector<int> stored_ids, stored_views, stored_rows;
    hipEvent_t ev_frame_ready = nullptr;  // fusion stream: the frame's shared inputs are complete
    // next-frame prefetch (mmf_fusion_prefetch_frame): the filter and the input-side preparation of frame t+1 run
    // on `side` while frame t is fused on the context's stream.  Two filtered-depth buffers: frame t's fuse /
    // clean / fill-in read one while frame t+1's filter writes the other.
    float* filtered[2] = {nullptr, nullptr};
    int cur = 0;
    // The next frame's SO3 pre-alignment runs in one of two states of its own (by the parity of the frame it is for): no
    // chain reads or writes them, so it can run while the current frame's chain is still at work; the chain's first launch
    // copies the result into every tracked model's state (BeginArgs::so3_stage).
    OdomState* so3_stage[2] = {nullptr, nullptr};
    int so3_stage_ready = -1;               // which of the two holds the pre-alignment of the upcoming frame; -1: none
    const uint8_t* image_pre_rgb = nullptr;  // the image side of this frame (intensity pyramid, gradients, SO3) is enqueued already
    hipStream_t side = nullptr;   // depth chain: filter, depth pyramid, vertex / normal maps
    hipStream_t side2 = nullptr;  // image chain: intensity pyramid, gradients, SO3 pre-alignment
    float* side_partials = nullptr;   // reduction scratch of the SO3 launches on side2 (never the context's: the
    unsigned* side_ticket = nullptr;  // main stream may be inside a reduction of its own at the same time)
    hipEvent_t ev_prefetch2_done = nullptr;
    hipEvent_t ev_inputs_free = nullptr;    // fusion stream: enqueued work no longer reads the odometry's input-side
                                            // buffers nor filtered[1 - cur]
    hipEvent_t ev_prefetch_done = nullptr;  // side stream: the prefetch has been enqueued up to here
    bool inputs_free_recorded = false;
    bool pre_valid = false;
    const uint8_t* pre_rgb = nullptr;
    const float* pre_depth = nullptr;
    // host FrameData hand-over (mmf_fusion_process_frame_host[_next]): pinned staging + device copies in a ring of three
    // (the frame being processed, the next one being uploaded, one whose readers may still be running), uploads on a
    // stream of their own
    static constexpr int kUp = 3;
    uint8_t* up_pin[kUp] = {nullptr, nullptr, nullptr};
    uint8_t* up_dev[kUp] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_up[kUp] = {nullptr, nullptr, nullptr};      // upload stream: slot k is on the device
    hipEvent_t ev_up_rgb[kUp] = {nullptr, nullptr, nullptr};  // ... its colour image is (sent first: the image side needs only that)
    bool up_recorded[kUp] = {false, false, false};
    hipStream_t up_stream = nullptr;
    hipEvent_t ev_up_begin = nullptr;  // fusion stream -> upload stream
    int up_cur = 0;
    // the last call waited on the host for a pose that came off the fusion's stream: everything enqueued before that call is
    // done, a slot of the ring can be refilled without an event from the fusion's stream (a marker on the stream a frame waits for)
    bool host_caught_up = false;
    // the NEXT call's host frame, handed in as a hint: staged and uploaded while the host would only wait for this
    // frame's pose (fusion_stage_host_next), its sensor-side preparation enqueued like a device-side hint's
    struct HostNext {
        const uint8_t* rgb = nullptr;
        const float* depth = nullptr;
        int slot = -1;
        bool pending = false;     // handed to the staging thread, not yet joined
        bool rgb_staged = false;  // its colour image is on its way (ev_up_rgb[slot] recorded)
        bool staged = false;      // all of it is on its way to (or on) the device in `slot`
    } host_next;
    // The copy of an announced frame into its pinned slot (2.15 MB at 640x480: ~150 us of one core) and the enqueue of its
    // upload run on a thread of their own, started when the call that announces the frame begins: on the calling thread the
    // copy was longer than the wait for the pose it was meant to hide in (announced frames ran 7 % behind device frames).
    struct Stager {
        std::thread thread;
        std::mutex mu;
        std::condition_variable cv;
        bool stop = false, busy = false;
        bool rgb_done = false;  // the job's colour image has been copied and its upload enqueued
        bool after_begin = true;  // the upload waits for ev_up_begin
        int slot = 0;
        const uint8_t* rgb = nullptr;
        const float* depth = nullptr;
        int rc = MMF_OK;
        std::string error;
    } stager;
};

static void identity16(float* m) {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
}

extern "C" int mmf_fusion_default_config(mmf_fusion_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_fusion_default_config: null argument");
    cfg->time_delta = 200;          // GUI/MainController.cpp:333 (timeDelta flag default)
    cfg->conf_global_init = 10.0f;  // GUI default confGlobalInit
    cfg->icp_weight = 10.0f;        // GUI default icpWeight
    cfg->depth_cutoff = 15.0f;      // GUI default depthCutoff (bilateral filter maxD)
    cfg->max_depth_processed = 20.0f;  // MultiMotionFusion.cpp:53
    cfg->rgb_only = 0;
    cfg->pyramid = 1;
    cfg->fast_odom = 0;
    cfg->so3 = 1;
    cfg->frame_to_frame_rgb = 0;
    cfg->outlier_coeff = 3.0f;      // GPUSetup::outlierCoefficient GUI default
    cfg->fill_in = 1;               // the global model is created with fill-in enabled
    cfg->max_surfels = 0;
    cfg->conf_object_init = 0.01f;  // GUI/MainController.cpp:333 (-confO)
    cfg->enable_multiple_models = 0;
    cfg->preallocated_models = 0;   // GUI/MainController.cpp:339 (-a)
    cfg->error_recording = 1;       // every Model is created with enableErrorRecording (MultiMotionFusion.cpp:70,128,944)
    cfg->pose_logging = 0;          // enablePoseLogging
    cfg->max_object_surfels = 0;
    cfg->batch_tracking = 1;
    return MMF_OK;
}

static void fusion_model_destroy(FusionModel* fm) {
    if (!fm) return;
    mmf_model_destroy(fm->model);
    mmf_odom_destroy(fm->odom);
    if (fm->ev_done) (void)hipEventDestroy(fm->ev_done);
    if (fm->own_lane) mmf_ctx_destroy(fm->lane);
    delete fm;
}

// std::make_shared<Model>(id, confidence, odom_cfg, enableFillIn, enableErrorRecording, ...) (Model.cpp:147-262)
static int fusion_model_create(mmf_fusion* f, int id, float conf, int fill_in, bool own_lane, FusionModel** out) {
    FusionModel* fm = new (std::nothrow) FusionModel();
    MMF_REQUIRE(fm != nullptr, "mmf_fusion: out of host memory");
    int rc = MMF_OK;
    // a rigid body another rank owns (ownership is by id: fusion_owner_of) is bookkeeping here: id, thresholds, pose,
    // statistics -- no surfel store, no odometry slab, no stream.  (The global model's odometry holds the sensor side of
    // every rank: it is always the real thing.)
    if (f->shard_world > 1 && id != 0 && id % f->shard_world != f->shard_rank) {
        fm->lane = f->ctx;
        rc = model_create_bookkeeping(f->ctx, f->width, f->height, f->cx, f->cy, f->fx, f->fy, (unsigned char)id, conf, &fm->model);
        if (rc == MMF_OK) rc = odom_create_bookkeeping(f->ctx, f->width, f->height, f->cx, f->cy, f->fx, f->fy, &fm->odom);
        if (rc != MMF_OK) {
            const std::string keep = g_last_error;
            fusion_model_destroy(fm);
            return fail(rc, keep);
        }
        fm->fill_in = fill_in;
        identity16(fm->last_pose);
        if (f->cfg.pose_logging) fm->pose_log.reserve(1000);  // Model.cpp:177
        *out = fm;
        return MMF_OK;
    }
    if (own_lane) {
        rc = mmf_ctx_create(f->ctx->device, nullptr, 1, &fm->lane);
        fm->own_lane = rc == MMF_OK;
    } else {
        fm->lane = f->ctx;
    }
    const int cap = id == 0 ? f->cfg.max_surfels : (f->cfg.max_object_surfels ? f->cfg.max_object_surfels : f->cfg.max_surfels);
    if (rc == MMF_OK)
        rc = mmf_model_create(fm->lane, f->width, f->height, f->cx, f->cy, f->fx, f->fy, (unsigned char)id, conf, cap, &fm->model);
    if (rc == MMF_OK)
        rc = mmf_odom_create(fm->lane, f->width, f->height, f->cx, f->cy, f->fx, f->fy, 0.10f,
                             std::sin(20.f * 3.14159254f / 180.f), &fm->odom);
    if (rc == MMF_OK && f->cfg.error_recording)  // Model::icpError / rgbError: images inside the odometry's slab
        fm->icp_error = fm->odom->icp_err, fm->rgb_error = fm->odom->rgb_err;
    if (rc == MMF_OK && hipEventCreateWithFlags(&fm->ev_done, hipEventDisableTiming) != hipSuccess)
        rc = fail(MMF_ERR_HIP, "mmf_fusion: hipEventCreate failed");
    if (rc != MMF_OK) {
        const std::string keep = g_last_error;
        fusion_model_destroy(fm);
        return fail(rc, keep);
    }
    // the prediction images (model slab) and the filtered depth (the fusion's buffer) are not written
    // between the init* calls of a frame and the end of its tracking
    fm->odom->alias_inputs = true;
    fm->fill_in = fill_in;
    identity16(fm->last_pose);
    if (f->cfg.pose_logging) fm->pose_log.reserve(1000);  // Model.cpp:177
    *out = fm;
    return MMF_OK;
}

// MultiMotionFusion::getNextModelID (MultiMotionFusion.cpp:983-999)
static int fusion_next_model_id(mmf_fusion* f, bool assign) {
    const int next = f->next_id;
    if (assign) {
        while (true) {
            f->next_id = (f->next_id + 1) & 255;
            bool occupied = false;
            for (FusionModel* m : f->models)
                if (f->next_id == (int)m->model->id) occupied = true;
            if (!occupied) break;
        }
    }
    return next;
}

extern "C" int mmf_fusion_create(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy,
                                 const mmf_fusion_config* cfg, mmf_fusion** out) {
    MMF_REQUIRE(c && out, "mmf_fusion_create: null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_fusion* f = new (std::nothrow) mmf_fusion();
    MMF_REQUIRE(f != nullptr, "mmf_fusion_create: out of host memory");
    f->ctx = c;
    if (cfg)
        f->cfg = *cfg;
    else
        mmf_fusion_default_config(&f->cfg);
    mmf_crf_default_config(&f->crf_cfg);
    mmf_mask_default_config(&f->mask_cfg);
    f->width = width, f->height = height;
    f->cx = cx, f->cy = cy, f->fx = fx, f->fy = fy;
    FusionModel* global = nullptr;
    // globalModel (MultiMotionFusion.cpp:69-71): id 0, fill-in, on the fusion's own stream
    int rc = fusion_model_create(f, fusion_next_model_id(f, true), f->cfg.conf_global_init, f->cfg.fill_in, false, &global);
    if (rc != MMF_OK) {
        delete f;
        return rc;
    }
    f->models.push_back(global);
    const size_t npix = (size_t)width * height;
    // from here on every failure leaves through mmf_fusion_destroy (it tolerates members that were never created)
    auto device_side = [&]() -> int {
        MMF_HIP_TRY(hipMalloc(&f->filtered[0], npix * 4));
        MMF_HIP_TRY(hipMalloc(&f->filtered[1], npix * 4));
        f->depth_filtered = f->filtered[0];
        // the side streams and events of the prefetch are created by its first call
        MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_inputs_free, hipEventDisableTiming));
        MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_frame_ready, hipEventDisableTiming));
        MMF_HIP_TRY(hipMalloc(&f->mask, npix));
        MMF_HIP_TRY(hipMemsetAsync(f->mask, 0, npix, c->stream));
        f->mask_is_zero = true;
        return MMF_OK;
    };
    rc = device_side();
    if (rc == MMF_OK)
        rc = mmf_fusion_preallocate_models(f, (unsigned)(f->cfg.preallocated_models > 0 ? f->cfg.preallocated_models : 0));
    if (rc != MMF_OK) {
        const std::string keep = g_last_error;
        mmf_fusion_destroy(f);
        return fail(rc, keep);
    }
    *out = f;
    return MMF_OK;
}

// preallocateModels(count) (MultiMotionFusion.cpp:125-131): object models created ahead of their first use
extern "C" int mmf_fusion_preallocate_models(mmf_fusion* f, unsigned count) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_preallocate_models: null fusion object");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    for (unsigned i = 0; i < count; ++i) {
        FusionModel* fm = nullptr;
        int rc = fusion_model_create(f, fusion_next_model_id(f, true), f->cfg.conf_object_init, 0, true, &fm);
        if (rc) return rc;
        f->preallocated.push_back(fm);
    }
    return MMF_OK;
}

// the flow-inference hook's engine and events, once the flow's stream has run dry
static void fusion_flow_inference_release(mmf_fusion* f) {
    if (!f->fi_on) return;
    if (f->fi) flowcrf_destroy_on(f->fi, f->flow_stream);
    (void)hipStreamSynchronize(f->flow_stream);
    (void)hipEventDestroy(f->ev_fi_begin);
    (void)hipEventDestroy(f->ev_fi_inputs);
    f->fi = nullptr, f->ev_fi_begin = f->ev_fi_inputs = nullptr;
    f->fi_on = f->fi_has = false;
}
// the optical-flow hook's engine, stream and events, once the stream has run dry
static void fusion_flow_release(mmf_fusion* f) {
    if (!f->flow) return;
    fusion_flow_inference_release(f);  // (it lives on the flow's stream and reads the flow)
    flow_destroy_on(f->flow, f->flow_stream);
    (void)hipEventDestroy(f->ev_flow_begin);
    (void)hipEventDestroy(f->ev_flow_done);
    (void)hipStreamDestroy(f->flow_stream);
    f->flow = nullptr, f->flow_stream = nullptr, f->ev_flow_begin = f->ev_flow_done = nullptr;
    f->flow_pending = f->flow_has = false;
}

extern "C" void mmf_fusion_destroy(mmf_fusion* f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    if (f->side) (void)hipStreamSynchronize(f->side);
    if (f->side2) (void)hipStreamSynchronize(f->side2);
    for (auto* list : {&f->models, &f->preallocated, &f->inactive}) {
        for (FusionModel* fm : *list) fusion_model_destroy(fm);
        list->clear();
    }
    (void)hipFree(f->filtered[0]);
    (void)hipFree(f->filtered[1]);
    (void)hipFree(f->mask);
    (void)hipFree(f->sp_labels);
    if (f->sp_stream) (void)hipStreamSynchronize(f->sp_stream);
    (void)hipFree(f->sp_ws.mem);
    if (f->ev_sp_begin) (void)hipEventDestroy(f->ev_sp_begin);
    if (f->ev_sp_done) (void)hipEventDestroy(f->ev_sp_done);
    if (f->sp_stream) (void)hipStreamDestroy(f->sp_stream);
    fusion_flow_release(f);
    mmf_viewstore_destroy(f->views);
    mmf_ransac_batch_destroy(f->verifier);
    if (f->kp_xy_pin) (void)hipHostFree(f->kp_xy_pin);
    if (f->kp_label_pin) (void)hipHostFree(f->kp_label_pin);
    (void)hipFree(f->mask_boxes);
    (void)hipFree(f->side_partials);
    (void)hipFree(f->side_ticket);
    if (f->stager.thread.joinable()) {
        {
            std::lock_guard<std::mutex> lock(f->stager.mu);
            f->stager.stop = true;
        }
        f->stager.cv.notify_all();
        f->stager.thread.join();
    }
    if (f->up_stream) (void)hipStreamSynchronize(f->up_stream);
    for (int i = 0; i < mmf_fusion::kUp; ++i) {
        if (f->up_pin[i]) (void)hipHostFree(f->up_pin[i]);
        (void)hipFree(f->up_dev[i]);
        if (f->ev_up[i]) (void)hipEventDestroy(f->ev_up[i]);
        if (f->ev_up_rgb[i]) (void)hipEventDestroy(f->ev_up_rgb[i]);
    }
    if (f->up_stream) (void)hipStreamDestroy(f->up_stream);
    if (f->ev_up_begin) (void)hipEventDestroy(f->ev_up_begin);
    (void)hipFree(f->so3_stage[0]);
    if (f->ev_inputs_free) (void)hipEventDestroy(f->ev_inputs_free);
    if (f->ev_frame_ready) (void)hipEventDestroy(f->ev_frame_ready);
    if (f->ev_prefetch_done) (void)hipEventDestroy(f->ev_prefetch_done);
    if (f->side) (void)hipStreamDestroy(f->side);
    if (f->ev_prefetch2_done) (void)hipEventDestroy(f->ev_prefetch2_done);
    if (f->side2) (void)hipStreamDestroy(f->side2);
    delete f;
}

extern "C" mmf_model* mmf_fusion_model(mmf_fusion* f) { return f ? f->models[0]->model : nullptr; }
extern "C" mmf_odom* mmf_fusion_odometry(mmf_fusion* f) { return f ? f->models[0]->odom : nullptr; }
extern "C" int mmf_fusion_tick(mmf_fusion* f) { return f ? f->tick : -1; }
extern "C" const float* mmf_fusion_depth_filtered(mmf_fusion* f) { return f ? f->depth_filtered : nullptr; }

// getModels() (MultiMotionFusion.h:107): the active list in its order, index 0 = the global model
extern "C" int mmf_fusion_num_models(mmf_fusion* f) { return f ? (int)f->models.size() : -1; }
extern "C" mmf_model* mmf_fusion_model_at(mmf_fusion* f, int index) {
    return (f && index >= 0 && index < (int)f->models.size()) ? f->models[index]->model : nullptr;
}
extern "C" mmf_odom* mmf_fusion_odometry_at(mmf_fusion* f, int index) {
    return (f && index >= 0 && index < (int)f->models.size()) ? f->models[index]->odom : nullptr;
}
extern "C" int mmf_fusion_num_inactive_models(mmf_fusion* f) { return f ? (int)f->inactive.size() : -1; }
extern "C" mmf_model* mmf_fusion_inactive_model_at(mmf_fusion* f, int index) {
    return (f && index >= 0 && index < (int)f->inactive.size()) ? f->inactive[index]->model : nullptr;
}
// The id the next spawned model will carry = the label a new segment must have in the id image.  The reference
// hands getNextModelID() to the segmentation (:148) but spawns the FRONT of preallocatedModels when there is one
// (:940-942), whose id was assigned at preallocation: with `-a N` its new segment is labelled with an id no model
// has.  Here the label and the spawned model always agree.
extern "C" int mmf_fusion_next_model_id(mmf_fusion* f) {
    if (!f) return -1;
    return f->preallocated.empty() ? f->next_id : (int)f->preallocated.front()->model->id;
}

// A model belongs to the rank its ID selects (id % world; the global model, id 0, to rank 0): fixed when the model is
// created and the same on every rank, whatever happens to the list around it -- a model that leaves the list (lost segment,
// scheduled deactivation) does not hand the models behind it to other ranks, which a rule by list position would.
static inline int fusion_owner_of(const mmf_fusion* f, const FusionModel* fm) { return (int)((unsigned)fm->model->id % (unsigned)f->shard_world); }
static inline bool fusion_owns_model(const mmf_fusion* f, const FusionModel* fm) { return fusion_owner_of(f, fm) == f->shard_rank; }
static inline bool fusion_owns(const mmf_fusion* f, size_t index) { return index < f->models.size() && fusion_owns_model(f, f->models[index]); }

extern "C" int mmf_fusion_set_shard(mmf_fusion* f, int rank, int world) {
    MMF_REQUIRE(f && world >= 1 && rank >= 0 && rank < world, "mmf_fusion_set_shard: bad argument");
    MMF_REQUIRE(f->models.size() == 1 && f->inactive.empty(), "mmf_fusion_set_shard: call it before the first object model is spawned");
    if (world > 1 && f->redetect_on) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: redetection is on (sharded redetection is not supported)");
    if (world > 1 && f->redetect_verifier) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: the redetection verifier is on (not supported on a shard)");
    if (world > 1 && f->flow) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: the optical-flow hook is on (not supported on a shard)");
    f->shard_rank = rank, f->shard_world = world;
    // models created ahead of their use (preallocateModels): the ones this rank will not own shrink to bookkeeping
    for (FusionModel*& fm : f->preallocated) {
        const int id = (int)fm->model->id;
        const bool is_light = fm->model->slab == nullptr, want_light = world > 1 && id % world != rank;
        if (is_light == want_light) continue;
        FusionModel* again = nullptr;
        const float conf = fm->model->conf_threshold;
        const int fill_in = fm->fill_in;
        fusion_model_destroy(fm);
        fm = nullptr;
        int rc = fusion_model_create(f, id, conf, fill_in, true, &again);
        if (rc) return rc;
        fm = again;
    }
    return MMF_OK;
}
extern "C" int mmf_fusion_owns_model(mmf_fusion* f, int index) {
    return (f && index >= 0 && fusion_owns(f, (size_t)index)) ? 1 : 0;
}
// the pose of a model another rank owns, as gathered from its owner (Model::overridePose semantics)
extern "C" int mmf_fusion_set_model_pose(mmf_fusion* f, int index, const float pose[16]) {
    MMF_REQUIRE(f && pose && index >= 0 && index < (int)f->models.size(), "mmf_fusion_set_model_pose: bad argument");
    std::memcpy(f->models[index]->model->pose, pose, sizeof(float) * 16);
    std::memcpy(f->models[index]->last_pose, pose, sizeof(float) * 16);
    return MMF_OK;
}
extern "C" int mmf_fusion_last_timings(mmf_fusion* f, double* tracking_s, double* frame_s) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_timings: null fusion object");
    if (tracking_s) *tracking_s = f->t_tracking_s;
    if (frame_s) *frame_s = f->t_frame_s;
    return MMF_OK;
}

static FusionModel* fusion_find(mmf_fusion* f, int id) {
    for (FusionModel* m : f->models)
        if ((int)m->model->id == id) return m;
    return nullptr;
}

// Model::getICPErrorTexture / getRGBErrorTexture (Model.h:232-236): R32F images written by the last level-0
// iteration of the model's tracking (reduce.cu:275,299; RGBDOdometry.cpp:369,408)
extern "C" int mmf_fusion_error_texture(mmf_fusion* f, int index, int which, float** dev_ptr) {
    MMF_REQUIRE(f && dev_ptr && index >= 0 && index < (int)f->models.size(), "mmf_fusion_error_texture: bad argument");
    *dev_ptr = which == 0 ? f->models[index]->icp_error : f->models[index]->rgb_error;
    MMF_REQUIRE(*dev_ptr != nullptr, "mmf_fusion_error_texture: error recording is off");
    return MMF_OK;
}

// getTextures() (MultiMotionFusion.h:124): the raw input images of the current frame as device images
extern "C" int mmf_fusion_texture(mmf_fusion* f, const char* name, const void** dev_ptr, size_t* bytes) {
    MMF_REQUIRE(f && name && dev_ptr && bytes, "mmf_fusion_texture: null argument");
    const size_t npix = (size_t)f->width * f->height;
    const std::string s(name);
    if (s == "RGB") *dev_ptr = f->frame_rgb, *bytes = npix * 3;                      // GPUTexture::RGB
    else if (s == "DEPTH_METRIC") *dev_ptr = f->frame_depth, *bytes = npix * 4;      // GPUTexture::DEPTH_METRIC
    else if (s == "DEPTH_METRIC_FILTERED") *dev_ptr = f->depth_filtered, *bytes = npix * 4;
    else if (s == "MASK") *dev_ptr = f->mask, *bytes = npix;
    else return fail(MMF_ERR_INVALID, "mmf_fusion_texture: unknown name '" + s + "'");
    return MMF_OK;
}

// ---- runtime setters the front end pushes every GUI tick (MultiMotionFusion.cpp:1064-1116, GUI/MainController.cpp:641-670)
#define MMF_FUSION_SETTER(name, field, type)                              \
    extern "C" int mmf_fusion_set_##name(mmf_fusion* f, type val) {       \
        MMF_REQUIRE(f != nullptr, "mmf_fusion_set_" #name ": null fusion object"); \
        f->cfg.field = val;                                               \
        return MMF_OK;                                                    \
    }
MMF_FUSION_SETTER(rgb_only, rgb_only, int)
MMF_FUSION_SETTER(icp_weight, icp_weight, float)
MMF_FUSION_SETTER(outlier_coefficient, outlier_coeff, float)
MMF_FUSION_SETTER(pyramid, pyramid, int)
MMF_FUSION_SETTER(fast_odom, fast_odom, int)
MMF_FUSION_SETTER(so3, so3, int)
MMF_FUSION_SETTER(frame_to_frame_rgb, frame_to_frame_rgb, int)
MMF_FUSION_SETTER(depth_cutoff, depth_cutoff, float)
MMF_FUSION_SETTER(enable_multiple_models, enable_multiple_models, int)
#undef MMF_FUSION_SETTER
// setConfidenceThreshold is declared by the reference (MultiMotionFusion.h:168) but has no definition: the
// threshold lives in each Model (Model.h:222-224)
extern "C" int mmf_fusion_set_confidence_threshold(mmf_fusion* f, float val) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_confidence_threshold: null fusion object");
    f->models[0]->model->conf_threshold = val;
    return MMF_OK;
}
extern "C" int mmf_fusion_set_tick(mmf_fusion* f, int val) {  // :1116
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_tick: null fusion object");
    f->tick = val;
    return MMF_OK;
}
extern "C" int mmf_fusion_get_config(mmf_fusion* f, mmf_fusion_config* out) {
    MMF_REQUIRE(f && out, "mmf_fusion_get_config: null argument");
    *out = f->cfg;
    return MMF_OK;
}
extern "C" int mmf_fusion_set_segmentation_callback(mmf_fusion* f, mmf_segmentation_fn fn, void* user) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_segmentation_callback: null fusion object");
    f->seg_fn = fn, f->seg_user = user;
    return MMF_OK;
}
extern "C" int mmf_fusion_set_crf_segmentation(mmf_fusion* f, const mmf_crf_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_crf_segmentation: null fusion object");
    if (!cfg) {
        f->crf_on = false;
        return MMF_OK;
    }
    if (int rc = crf_check_config(cfg, "mmf_fusion_set_crf_segmentation")) return rc;
    f->crf_cfg = *cfg, f->crf_on = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_set_mask_segmentation(mmf_fusion* f, const mmf_mask_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_mask_segmentation: null fusion object");
    if (!cfg) {
        f->mask_on = false;
        return MMF_OK;
    }
    MMF_REQUIRE(cfg->model_spawn_offset >= 0, "mmf_fusion_set_mask_segmentation: model_spawn_offset must not be negative");
    if (f->shard_world != 1)
        return fail(MMF_ERR_STATE, "mmf_fusion_set_mask_segmentation: needs world == 1 (a sharded front end calls mmf_mask_segment "
                                   "in its segmentation callback)");
    f->mask_cfg = *cfg, f->mask_on = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_mask_mapping(mmf_fusion* f, uint8_t mapping_out[256]) {
    MMF_REQUIRE(f && mapping_out, "mmf_fusion_mask_mapping: null argument");
    std::memcpy(mapping_out, f->mask_map, 256);
    return MMF_OK;
}
extern "C" int mmf_fusion_last_mask_segmentation(mmf_fusion* f, mmf_mask_info* info, mmf_segmentation_model* models, int capacity) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_mask_segmentation: null fusion object");
    if (!f->mask_valid) return fail(MMF_ERR_STATE, "mmf_fusion_last_mask_segmentation: no frame has been segmented from its labels yet");
    if (info) *info = f->mask_info;
    if (models)
        for (int i = 0; i < (int)f->mask_models.size() && i < capacity; ++i) models[i] = f->mask_models[(size_t)i];
    return MMF_OK;
}
extern "C" int mmf_fusion_set_superpixels(mmf_fusion* f, const int* labels) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_superpixels: null fusion object");
    f->sp_next = false;
    if (!labels) return MMF_OK;
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->sp_last == f->sp_labels) f->sp_last = nullptr;  // (the copy the last segmentation used is about to be replaced)
    if (!f->sp_labels) MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&f->sp_labels), (size_t)f->width * f->height * sizeof(int)));
    MMF_HIP_TRY(hipMemcpyAsync(f->sp_labels, labels, (size_t)f->width * f->height * sizeof(int), hipMemcpyDeviceToDevice, f->ctx->stream));
    f->sp_next = true;
    return MMF_OK;
}
// the engine's streams and label image for the fusion's frame size and the CRF configuration's super-pixel size
static int fusion_sp_engine_prepare(mmf_fusion* f, const char* who) {
    if (int rc = slic_engine_check(f->width, f->height, f->crf_cfg.spixel_size, who)) return rc;
    const int S = f->crf_cfg.spixel_size;
    const size_t cells = (size_t)(f->width / S) * (f->height / S), pixels = (size_t)f->width * f->height;
    if (!f->sp_stream) {
        MMF_HIP_TRY(hipStreamCreateWithFlags(&f->sp_stream, hipStreamNonBlocking));
        MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_sp_begin, hipEventDisableTiming));
        MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_sp_done, hipEventDisableTiming));
    }
    if (cells > f->sp_ws.cells || pixels > f->sp_ws.pixels) {  // (the setter, or a CRF configuration with a smaller S since)
        MMF_HIP_TRY(hipStreamSynchronize(f->sp_stream));
        if (f->sp_ws.mem && f->sp_last == f->sp_ws.labels()) f->sp_last = nullptr;
        if (int rc = slic_engine_workspace(&f->sp_ws, cells, pixels, f->ctx->stream)) return rc;
    }
    return MMF_OK;
}
extern "C" int mmf_fusion_set_superpixel_engine(mmf_fusion* f, int mode) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_superpixel_engine: null fusion object");
    MMF_REQUIRE(mode == 0 || mode == 1, "mmf_fusion_set_superpixel_engine: mode is 0 (off) or 1 (SLIC from the frame's RGB)");
    if (mode == 0) {
        f->sp_engine = 0;
        return MMF_OK;
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (int rc = fusion_sp_engine_prepare(f, "mmf_fusion_set_superpixel_engine")) return rc;
    f->sp_engine = 1;
    return MMF_OK;
}
extern "C" int mmf_fusion_last_superpixels(mmf_fusion* f, int* labels_out) {
    MMF_REQUIRE(f && labels_out, "mmf_fusion_last_superpixels: null argument");
    if (!f->sp_last) return fail(MMF_ERR_STATE, "mmf_fusion_last_superpixels: no segmentation has run on this fusion (or its labels were replaced)");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(labels_out, f->sp_last, (size_t)f->width * f->height * sizeof(int), hipMemcpyDeviceToDevice, f->ctx->stream));
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
    const bool rearm = f->fi_on && cfg && cfg->div == 4;
    const mmf_flowcrf_config fi_cfg = f->fi_cfg;
    fusion_flow_release(f);
    if (!cfg) return MMF_OK;
    if (int rc = flow_create_impl(f->ctx, f->width, f->height, cfg, &f->flow, "mmf_fusion_set_optical_flow")) return rc;
    hipError_t e = hipStreamCreateWithFlags(&f->flow_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_flow_begin, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_flow_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (f->ev_flow_begin) (void)hipEventDestroy(f->ev_flow_begin);
        if (f->flow_stream) (void)hipStreamDestroy(f->flow_stream);
        flow_destroy_on(f->flow, nullptr);
        f->flow = nullptr, f->flow_stream = nullptr, f->ev_flow_begin = f->ev_flow_done = nullptr;
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
    if (!f->flow) return fail(MMF_ERR_STATE, "mmf_fusion_last_flow: the optical-flow hook is off (mmf_fusion_set_optical_flow)");
    if (flow_dev) *flow_dev = nullptr;
    if (magnitude_dev) *magnitude_dev = nullptr;
    if (motion_dev) *motion_dev = nullptr;
    if (w) *w = f->flow->geo.W;
    if (h) *h = f->flow->geo.H;
    if (has_flow) *has_flow = f->flow_has ? 1 : 0;
    if (!f->flow_has) return MMF_OK;
    return mmf_flow_result(f->flow, flow_dev, magnitude_dev, motion_dev, nullptr, nullptr);
}

// The flow-CRF inference hook: cfg != NULL switches it on (a second call replaces the configuration), NULL off -- the engine
// and its events are freed, and no frame allocates, enqueues or waits for anything.  It reads the optical-flow hook's result.
extern "C" int mmf_fusion_set_flow_inference(mmf_fusion* f, const mmf_flowcrf_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_flow_inference: null fusion object");
    if (cfg) {
        if (int rc = flowcrf_check_config(f->width, f->height, mmf::kCrfMaxLabels, 0, cfg, "mmf_fusion_set_flow_inference")) return rc;
        if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_inference: not available on a sharded fusion");
        if (!f->flow) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_inference: the optical-flow hook is off (mmf_fusion_set_optical_flow)");
        if (f->flow->cfg.div != 4) return fail(MMF_ERR_STATE, "mmf_fusion_set_flow_inference: the optical-flow hook must run at div 4");
    }
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    fusion_flow_inference_release(f);
    if (!cfg) return MMF_OK;
    hipError_t e = hipEventCreateWithFlags(&f->ev_fi_begin, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_fi_inputs, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (f->ev_fi_begin) (void)hipEventDestroy(f->ev_fi_begin);
        f->ev_fi_begin = f->ev_fi_inputs = nullptr;
        return fail(MMF_ERR_HIP, std::string("mmf_fusion_set_flow_inference: ") + hipGetErrorString(e));
    }
    f->fi_cfg = *cfg, f->fi_on = true;
    return MMF_OK;
}

// The id images of the last processFrame call: DEVICE pointers into the hook's engine (ids [h][w], ids_full [height][width]),
// complete on the fusion's stream and valid until the next frame, reset or setter call.  *has_result = 0 (and null pointers)
// after a frame without a flow (the first of a sequence) or without tracking.
extern "C" int mmf_fusion_last_flow_inference(mmf_fusion* f, const uint8_t** ids_dev, const uint8_t** ids_full_dev, int* w, int* h,
                                              int* n_labels, int* has_result) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_flow_inference: null fusion object");
    if (!f->fi_on) return fail(MMF_ERR_STATE, "mmf_fusion_last_flow_inference: the flow-inference hook is off (mmf_fusion_set_flow_inference)");
    if (ids_dev) *ids_dev = nullptr;
    if (ids_full_dev) *ids_full_dev = nullptr;
    if (w) *w = f->width / 4;
    if (h) *h = f->height / 4;
    if (n_labels) *n_labels = 0;
    if (has_result) *has_result = f->fi_has ? 1 : 0;
    if (!f->fi_has) return MMF_OK;
    return mmf_flowcrf_result(f->fi, ids_dev, ids_full_dev, nullptr, nullptr, nullptr, nullptr, n_labels);
}
// A stage image of the last call's inference to HOST memory, as mmf_flowcrf_download (tests: "E" shows the poses and the track
// table the hook handed its engine).  MMF_ERR_STATE while the hook is off and after a frame without a result.
extern "C" int mmf_fusion_flow_inference_download(mmf_fusion* f, const char* name, void* host_dst, size_t bytes) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_flow_inference_download: null fusion object");
    if (!f->fi_on) return fail(MMF_ERR_STATE, "mmf_fusion_flow_inference_download: the flow-inference hook is off (mmf_fusion_set_flow_inference)");
    if (!f->fi_has) return fail(MMF_ERR_STATE, "mmf_fusion_flow_inference_download: the last frame has no result");
    return mmf_flowcrf_download(f->fi, name, host_dst, bytes);
}
extern "C" int mmf_fusion_last_segmentation(mmf_fusion* f, mmf_crf_info* info, mmf_segmentation_model* models, int capacity,
                                            float* unaries, float* q, uint8_t* raw_map, uint8_t* map) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_last_segmentation: null fusion object");
    return mmf_crf_last(f->ctx, info, models, capacity, unaries, q, raw_map, map);
}
// scheduleDeactivation (MultiMotionFusion.cpp: scheduled_model_deactivation, applied at the next frame :279-283)
extern "C" int mmf_fusion_schedule_deactivation(mmf_fusion* f, int id) {
    MMF_REQUIRE(f != nullptr && id > 0, "mmf_fusion_schedule_deactivation: bad argument (the global model stays)");
    f->scheduled_deactivation.push_back(id);
    return MMF_OK;
}

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
    o->depth_l0 = primary->depth_l0;
}

// where an OBJECT model's latest prediction is non-zero (device, PassBoxes::spl_nz of its last resolve), for a model-side
// preparation that may then leave the rest of the frame alone; null: unknown, or not such a model
static const int* fusion_pred_box(const FusionModel* fm) {
    const mmf_model* m = fm->model;
    if (fm->fill_in || !fm->odom->sparse || !m->boxes || !m->spl_nz_known) return nullptr;
    return m->boxes->spl_nz[m->sgen & 1u];
}
// the covered thumbnail samples of a model's latest prediction (thumbnail_count_px)
static const int* fusion_thumb_count(const mmf_model* m) {
    return reinterpret_cast<const int*>(&m->totals[4 + (m->thumb_gen & 1)]);
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
// way, and tests/test_gpu_fusion.py compares the two).  MMF_MID_PREDICT=1 runs it as the reference does.
static std::atomic<int> g_mid_predict{-1};  // -1: MMF_MID_PREDICT decides (default off); 0 / 1: mmf_debug_set_mid_predict
extern "C" int mmf_debug_set_mid_predict(int on) {
    g_mid_predict.store(on < 0 ? -1 : (on ? 1 : 0));
    return MMF_OK;
}
static bool fusion_mid_predict() {
    return g_mid_predict.load() > 0;
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
    rc = model_fuse(fm->model, f->tick, f->frame_rgb, f->mask, f->frame_depth, f->depth_filtered, g.max_depth_processed, weighting,
                    merged ? &ia : nullptr);
    if (rc) return rc;
    rc = model_predict_indices(fm->model, f->tick, g.max_depth_processed, g.time_delta, merged);
    if (rc) return rc;
    return mmf_model_clean(fm->model, f->tick, g.time_delta, g.max_depth_processed, f->depth_filtered, f->mask, g.outlier_coeff);
}

// getMaxDepth (:408): float operands, double arithmetic (1.2 is a double literal), returned as float
static float seg_max_depth(const mmf_segmentation_model& d) { return (float)((double)d.depth_mean + (double)d.depth_std * 1.2); }

// test / A-B hook: how the object models' passes go out (fusion_batch_mode)
static std::atomic<int> g_batch_passes{-1};  // -1: MMF_PASS_BATCH / the number of object models decide
extern "C" int mmf_debug_set_pass_batch(int mode) {
    MMF_REQUIRE(mode == -1 || mode == 0 || mode == 2, "mmf_debug_set_pass_batch: mode must be -1, 0 or 2");
    g_batch_passes.store(mode);
    return MMF_OK;
}
// 0: model by model; 2: one launch per pass, restricted to where the models are (pass_rect.hpp).  Neither the hook nor
// MMF_PASS_BATCH says: by the number of object models this GPU runs -- model by model on the models' own streams up to three
// of them, restricted launches from four on
// (measured, LABNOTES r5: 8 models 0.69-0.70 against 0.76-0.78 ms, 5 models 0.60-0.62 against 0.65-0.67, 4 models 0.575-0.58
// against 0.55-0.59)
constexpr int kRectPassObjects = 4;
static int fusion_batch_mode(const mmf_fusion* f) {
    int v = g_batch_passes.load();
    if (v < 0) v = tunables().pass_batch;
    if (v >= 0) return v;
    int objects = 0;
    for (size_t k = 1; k < f->models.size(); ++k) objects += fusion_owns(f, k) ? 1 : 0;
    return objects >= kRectPassObjects ? 2 : 0;
}
// the boxes of the ids of the frame's id image (pass_rect.hpp: mask_boxes_kernel), on `st`
static int fusion_note_mask_boxes(mmf_fusion* f, hipStream_t st) {
    if (!f->mask_boxes) {
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&f->mask_boxes), 256 * 4 * sizeof(unsigned long long)));
        MMF_HIP_TRY(hipMemsetAsync(f->mask_boxes, 0, 256 * 4 * sizeof(unsigned long long), st));
    }
    ++f->mask_gen;
    const int tiles = ((f->width + 63) / 64) * ((f->height + 15) / 16);
    hipLaunchKernelGGL(mask_boxes_kernel, dim3(tiles), dim3(256), 0, st, f->mask, f->width, f->height, f->mask_boxes, f->mask_gen);
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
        MMF_HIP_TRY(hipEventRecord(objs[k]->ev_done, ls));
        MMF_HIP_TRY(hipStreamWaitEvent(st, objs[k]->ev_done, 0));
    }
    return MMF_OK;
}

static int lane_wait(FusionModel* fm, hipEvent_t ev) {
    MMF_HIP_TRY(hipStreamWaitEvent(fm->lane->stream, ev, 0));
    return MMF_OK;
}

static bool fusion_view_log_on(const mmf_fusion* f) { return f->redetect_on && f->views && f->tracker && f->tracker->log.frames > 0; }

// Model::appendPoses: one (stamp, pose) entry per object model and tracked frame.  after_tracking: every active object model
// gets this frame's entry; otherwise (the end of the frame) only the models that have none yet -- the one spawned in it.
// Stamps that do not ascend mean the tracker was reset: the list restarts.
static void fusion_note_view_poses(mmf_fusion* f, bool after_tracking) {
    if (!fusion_view_log_on(f)) return;
    const int stamp = (int)f->tracker->frame;
    for (size_t k = 1; k < f->models.size(); ++k) {
        std::vector<mmf_fusion::ViewPose>& list = f->view_poses[(int)f->models[k]->model->id];
        if (!list.empty() && list.back().stamp > stamp) list.clear();
        if (!list.empty() && list.back().stamp == stamp) {
            if (after_tracking) mmf_model_get_pose(f->models[k]->model, list.back().pose);
            continue;
        }
        mmf_fusion::ViewPose e;
        e.stamp = stamp;
        mmf_model_get_pose(f->models[k]->model, e.pose);
        list.push_back(e);
        if ((int)list.size() > f->tracker->log.frames) list.erase(list.begin(), list.end() - f->tracker->log.frames);
    }
}

// Model::store (Model.cpp:1617-1644) without the files: the model's views from the tracker's log (mmf_tracker_model_views),
// its pose entries paired with the log's frames BY STAMP, into the view store without passing through the host
// (mmf_viewstore_store_device).  One host wait in each.  A model that has stored views stores nothing (:1618-1621).
static int fusion_store_views(mmf_fusion* f, FusionModel* fm) {
    const int id = (int)fm->model->id;
    if (!fusion_view_log_on(f) || id <= 0 || id >= mmf::kTrkMaxModels || viewstore_has_model(f->views, id)) return MMF_OK;
    std::vector<int> frames;
    std::vector<float> poses;
    auto it = f->view_poses.find(id);
    if (it != f->view_poses.end())
        for (const mmf_fusion::ViewPose& e : it->second) {
            frames.push_back(e.stamp);
            poses.insert(poses.end(), e.pose, e.pose + 16);
        }
    const int n = (int)frames.size();
    if (n == 0) return MMF_OK;  // (no tracked frame since the log is kept: nothing is known of the model)
    const int* counts = nullptr;
    const float *desc = nullptr, *coord = nullptr;
    int rc = mmf_tracker_model_views(f->tracker, id, n, frames.data(), poses.data(), &counts, &desc, &coord, nullptr);
    if (rc) return rc;
    int stored = 0;
    rc = mmf_viewstore_store_device(f->views, id, n, counts, desc, coord, &stored);
    if (rc) return rc;
    if (stored) {
        int rows = 0;
        for (int v = 0; v < n; ++v) rows += counts[v];
        f->stored_ids.push_back(id), f->stored_views.push_back(n), f->stored_rows.push_back(rows);
    }
    f->view_poses.erase(id);
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

static int fusion_prefetch_impl(mmf_fusion* f, const uint8_t* rgb, const float* depth, int tick_at_use);
static int fusion_prefetch_image(mmf_fusion* f, const uint8_t* rgb, int tick_at_use, bool ahead);
static int fusion_stage_host_next(mmf_fusion* f);
// a stream waits for an event only when the event has not happened yet (a wait is a barrier packet on the queue either way)
static hipError_t fusion_wait_unless_done(hipStream_t s, hipEvent_t e) {
    if (hipEventQuery(e) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    return hipStreamWaitEvent(s, e, 0);
}
static int fusion_stage_host_rgb(mmf_fusion* f);

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
    bool superpixels = false;  // the super-pixel engine runs for this frame (ev_sp_begin is recorded)
    bool flow = false;         // the optical-flow engine runs for this frame (ev_flow_begin is recorded) ...
    bool flow_enqueued = false;  // ... and its launches are on the flow stream

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
    p.sel = fm->fill_in ? fusion_thumb_count(m) : nullptr;
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
        tb.bd.d[k] = (long long)(reinterpret_cast<char*>(fms[k]->odom->slab) - reinterpret_cast<char*>(lead->odom->slab));
        pose_trans_rot(start_pose(fms[k]), tb.poses.trans[k], tb.poses.rot[k]);
    }
    int rc = odom_enqueue_tracking(lead->odom, tb.poses.trans[0], tb.poses.rot[0], tm, lead->icp_error, lead->rgb_error, &tb);
    if (rc) return rc;
    // the lanes continue after the chain.  With a segmentation every lane waits for ev_frame_ready before its passes anyway,
    // and that event is recorded on this very stream (the camera model's) behind the chain (the mask's upload, frame_segment):
    // an event and a wait per model here would be fourteen host calls and seven barrier packets for nothing
    for (size_t k = 1; k < n && !(g.enable_multiple_models && st == f->ctx->stream); ++k) {
        MMF_HIP_TRY(hipEventRecord(fms[k]->ev_done, st));
        MMF_HIP_TRY(hipStreamWaitEvent(fms[k]->lane->stream, fms[k]->ev_done, 0));
    }
    return MMF_OK;
}

// :209-283: the prefetch hand-over, the bilateral filter (:262), the mask, the scheduled deactivations
static int frame_begin(mmf_fusion* f, FrameRun& r) {
    const mmf_frame* fr = r.fr;
    const mmf_fusion_config& g = f->cfg;
    mmf_ctx* c = f->ctx;
    if (f->pre_valid) {  // whatever was prefetched has to be complete before this frame touches the same buffers
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->ev_prefetch_done, 0));  // (recorded behind BOTH side streams' work)
        r.prefetched = f->pre_rgb == fr->rgb && f->pre_depth == fr->depth;
        f->pre_valid = false;
    }
    // a prefetched SO3 pre-alignment only counts for the frame it was computed for, and only when that frame is tracked
    const int so3_ready = f->so3_stage_ready;
    f->so3_stage_ready = -1;
    f->image_pre_rgb = nullptr;
    if (so3_ready >= 0 && r.prefetched && r.track && !(r.have_init && !fr->icp_refine)) r.so3_stage = f->so3_stage[so3_ready];
    for (FusionModel* fm : f->models) fm->odom->so3_prefetched = false, fm->odom->so3_stage = nullptr;
    if (r.prefetched) {  // the filter (:262) and the input-side preparation already ran on the side stream
        f->cur ^= 1;
        f->depth_filtered = f->filtered[f->cur];
        odom_adopt_gradients(f->models[0]->odom);
    } else {
        int rc = mmf_filter_depth(c, fr->depth, f->width, f->height, g.depth_cutoff, f->depth_filtered);  // :262
        if (rc) return rc;
    }
    f->frame_rgb = fr->rgb, f->frame_depth = fr->depth;
    f->inputs_free_recorded = false;  // (set again by the stages that record ev_inputs_free)
    f->host_caught_up = false;
    if (!g.enable_multiple_models && !f->mask_is_zero) {  // :268-275: everything is background
        MMF_HIP_TRY(hipMemsetAsync(f->mask, 0, (size_t)f->width * f->height, c->stream));
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
    MMF_HIP_TRY(hipEventRecord(f->ev_inputs_free, c->stream));
    f->inputs_free_recorded = true;
    MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready, c->stream));
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
                       fm->model->tex_gen == fm->spec_tex_gen && fm->spec_f2f == g.frame_to_frame_rgb && fm->odom->prep_batched;
        fm->spec_valid = false;
        fm->odom->begin_spec_ok = fm->spec_hit;  // (the tracking's beginning rode that preparation: odom_begin_rider)
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
    if (!r.one_pass && r.lanes_wait) MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready, c->stream));
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
    r.next_from_host = f->host_next.slot >= 0 && f->up_dev[0] != nullptr;  // (a frame still being uploaded)
    r.image_early_any = fr->next_rgb && fr->next_depth && f->side2 && g.so3 && r.so3_stage != nullptr;
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
                int rc = lane_wait(fm, f->ev_frame_ready);
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
        for (FusionModel* fm : tracked) fm->odom->so3_prefetched = true, fm->odom->so3_stage = r.so3_stage;
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
            MMF_HIP_TRY(hipEventRecord(tracked[k]->ev_done, tracked[k]->lane->stream));
            MMF_HIP_TRY(hipStreamWaitEvent(st, tracked[k]->ev_done, 0));
        }
        PrepStages stages;
        stages.set_critical(true);  // the model's stream
        for (FusionModel* fm : tracked) {
            if (fm->spec_hit) {
                fm->odom->depth_l0 = f->depth_filtered;
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
            int rc = lane_wait(fm, f->ev_frame_ready);
            if (rc) return rc;
        }
        if (fm->spec_hit) {  // the model side was prepared at the end of the last frame; the sensor side by the prefetch
            fm->odom->depth_l0 = f->depth_filtered;  // (or in frame_track_sensor_side)
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
            MMF_HIP_TRY(hipEventRecord(fm->ev_done, tracked[0]->lane->stream));
            MMF_HIP_TRY(hipStreamWaitEvent(fm->lane->stream, fm->ev_done, 0));
        }
        fm->odom->exclusive_chain = tracked.size() == 1;  // several chains side by side: no in-launch barriers
        // The frame's first projection, enqueued right behind this chain (frame_enqueue_ahead), carries the hand-over to the
        // host and the fusion weight on one extra workgroup (frame_rider.hpp): the chain's last launch is the solve alone (13
        // -> 5.7 us on the stream a frame waits for).
        fm->odom->defer_publish = tracked.size() == 1 && !fr->bootstrap && !r.have_init && !g.rgb_only && f->tracking_ok && !f->fi_on;
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
    if (f->fi_on) return MMF_OK;  // (the flow inference reads the prediction the frame was tracked against: frame_flow_inference)
    FusionModel* fm = r.tracked[0];
    mmf_model* m = fm->model;
    r.early_snapshot = *m, r.early_snapshot_valid = true;
    m->abort_dev = &fm->odom->state->gn_fault;
    // "nothing enqueued so far reads the odometries' sensor-side buffers or the other filtered-depth buffer" holds
    // HERE, behind the one chain of this process; the passes enqueued next do not read them either.  No event
    // says so any more (see frame_track: the host knows when it has the pose; a marker behind the chain cost the
    // model's stream ~4 us in front of the frame's first projection).
    m->t_inv_dev = fm->odom->state->pose_inv;
    m->rider = fm->odom->rider;
    fm->odom->rider = FrameRider();
    int rc = fusion_mid_predict() ? fusion_predict_model(f, fm) : MMF_OK;
    if (rc == MMF_OK) rc = mmf_model_predict_indices(m, f->tick, g.max_depth_processed, g.time_delta);
    MMF_REQUIRE(rc != MMF_OK || m->rider.st == nullptr, "mmf_fusion_process_frame: the tracking result was not handed over");
    fm->early_done = rc == MMF_OK;
    // Without a segmentation the mask of the frame is known (all zeros) and nothing the host decides lies
    // between tracking and fusion: fuse -> predictIndices -> clean (:791-816) follow at once, with the pose and
    // Model::computeFusionWeight taken from the device state (odom_end, odom_fusion_weight_kernel).
    if (rc == MMF_OK && !g.enable_multiple_models) {
        m->pose_dev = fm->odom->state->pose_out, m->weight_dev = &fm->odom->state->fusion_weight;
        rc = fusion_fuse_clean_model(f, fm, r.fr->weight_multiplier, true);
        fm->early_fused = rc == MMF_OK;
    }
    m->t_inv_dev = m->pose_dev = m->weight_dev = nullptr;
    m->abort_dev = nullptr;
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
                if (t->tracking && t != fm && t->odom->result_of) {  // drain what the other lanes' chains still publish
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
        if (fm->lane->stream == f->ctx->stream) f->host_caught_up = true;
    }
    return MMF_OK;
}

// The engine's label image of this frame.  It depends on the frame's RGB only, so it runs on a stream of its own beside the
// tracking chains and fusion_crf_segment joins it in front of stage 1.  Two halves: ev_sp_begin is recorded on the fusion's
// stream when the frame begins (the RGB is there; the last segmentation that read the label image ended in a host wait),
// the twelve launches are enqueued once the chains are, while the host would only wait for the poses -- in front of the
// chains their enqueue is host time the whole frame waits for.  Only when this frame's segmentation will be the built-in
// one on the engine's labels.
static int frame_superpixels_begin(mmf_fusion* f, FrameRun& r) {
    mmf_ctx* c = f->ctx;
    if (f->sp_enqueued) {  // a frame that failed between the engine and its segmentation
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->ev_sp_done, 0));
        f->sp_enqueued = false;
    }
    if (int rc = fusion_sp_engine_prepare(f, "mmf_fusion_process_frame (super-pixel engine)")) return rc;
    MMF_HIP_TRY(hipEventRecord(f->ev_sp_begin, c->stream));
    r.superpixels = true;
    return MMF_OK;
}
static int frame_superpixels_enqueue(mmf_fusion* f, const FrameRun& r) {
    MMF_HIP_TRY(hipStreamWaitEvent(f->sp_stream, f->ev_sp_begin, 0));
    if (int rc = slic_engine_enqueue(f->sp_ws, f->sp_stream, r.fr->rgb, f->width, f->height, f->crf_cfg.spixel_size, 5, nullptr, nullptr,
                                     nullptr, nullptr))
        return rc;
    MMF_HIP_TRY(hipEventRecord(f->ev_sp_done, f->sp_stream));
    f->sp_enqueued = true;
    return MMF_OK;
}

// The optical flow of this frame from the one before it (mmf_fusion_set_optical_flow).  Like the label image it depends on
// the frame's RGB only.  ev_flow_begin is recorded on the fusion's stream when the call begins: the RGB is on the device
// there (a host frame's upload has been joined), and whatever read the last frame's flow on that stream is done.  The
// launches go to the flow stream behind that event -- on a tracked frame once the chains are enqueued, as the super-pixel
// engine's do -- and the fusion's stream joins them at the end of the call (frame_flow_join).
static int frame_flow_begin(mmf_fusion* f, FrameRun& r) {
    mmf_ctx* c = f->ctx;
    if (f->flow_pending) {  // a frame that failed between the enqueue and the join
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->ev_flow_done, 0));
        f->flow_pending = false;
    }
    MMF_HIP_TRY(hipEventRecord(f->ev_flow_begin, c->stream));
    r.flow = true;
    return MMF_OK;
}
static int frame_flow_enqueue(mmf_fusion* f, FrameRun& r) {
    MMF_HIP_TRY(hipStreamWaitEvent(f->flow_stream, f->ev_flow_begin, 0));
    int has = 0;
    f->flow_has = false;
    if (int rc = flow_next_on(f->flow, r.fr->rgb, f->flow_stream, &has)) return rc;
    MMF_HIP_TRY(hipEventRecord(f->ev_flow_done, f->flow_stream));
    f->flow_pending = true, f->flow_has = has != 0;
    r.flow_enqueued = true;
    return MMF_OK;
}
static int frame_flow_join(mmf_fusion* f) {
    MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, f->ev_flow_done, 0));
    f->flow_pending = false;
    return MMF_OK;
}

// The flow-CRF inference of this frame (mmf_fusion_set_flow_inference), where the reference segments: behind the tracking, on
// the predictions the frame was tracked against (nothing has rewritten them yet: frame_enqueue_ahead stands back while the
// hook is on).  The active models in list order, the new label when models may spawn; T_start = prev_pose pose^-1 and
// T_end = pose pose^-1 (Model.cpp:556-557: poses.back() is this frame's pose, tracked or -- with the refinement off --
// initialised; poses[-2] is the pose the frame before ended with, whatever overridePose has done to lastPose since); the
// attached tracker's table, if any.  On the flow stream behind the flow; the fusion's stream and the models' streams wait
// until the inference has read the predictions and the table (two launches), the rest is joined with the flow
// (frame_flow_join).  A frame with more labels than the engine takes has no result (has_result 0): the hook fails no frame.
static int frame_flow_inference(mmf_fusion* f) {
    mmf_ctx* c = f->ctx;
    const int M = (int)f->models.size(), allow_new = f->cfg.enable_multiple_models ? 1 : 0, L = M + allow_new;
    if (L > mmf::kCrfMaxLabels) return MMF_OK;
    const int cap = f->tracker ? f->tracker->capacity : 0;
    if (!f->fi || f->fi->max_labels < L || f->fi->max_tracks < cap) {
        if (f->fi) flowcrf_destroy_on(f->fi, f->flow_stream);
        f->fi = nullptr;
        int rc = flowcrf_create_impl(c, f->width, f->height, std::max(4, flowcrf_pad_labels(L)), cap, f->fx, f->fy, f->cx, f->cy, &f->fi_cfg,
                                     &f->fi, "mmf_fusion_process_frame (flow inference)");
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
        if (fm->lane->stream != c->stream) {  // (its last prediction ran there)
            MMF_HIP_TRY(hipEventRecord(fm->ev_done, fm->lane->stream));
            MMF_HIP_TRY(hipStreamWaitEvent(f->flow_stream, fm->ev_done, 0));
        }
    }
    mmf_flowcrf_input in;
    std::memset(&in, 0, sizeof(in));
    in.n_models = M, in.allow_new = allow_new, in.new_id = (unsigned)mmf_fusion_next_model_id(f), in.ids = ids;
    in.T_start = T.data(), in.T_end = T.data() + 16 * (size_t)M, in.vertex = vertex, in.depth = f->frame_depth;
    int rc = mmf_flow_result(f->flow, &in.flow, nullptr, &in.motion, nullptr, nullptr);
    if (rc) return rc;
    if (int bad = flowcrf_check_input(f->fi, &in, "mmf_fusion_process_frame (flow inference)")) return bad;
    mmf::FcrfTracks tr;
    rc = flowcrf_tracker_view(f->fi, f->tracker, &tr, "mmf_fusion_process_frame (flow inference)");
    if (rc) return rc;
    MMF_HIP_TRY(hipEventRecord(f->ev_fi_begin, c->stream));
    MMF_HIP_TRY(hipStreamWaitEvent(f->flow_stream, f->ev_fi_begin, 0));
    rc = flowcrf_run_on(f->fi, &in, tr, f->flow_stream, f->ev_fi_inputs);
    if (rc) return rc;
    MMF_HIP_TRY(hipEventRecord(f->ev_flow_done, f->flow_stream));  // (frame_flow_join waits for the inference as well)
    MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->ev_fi_inputs, 0));
    for (FusionModel* fm : f->models)
        if (fm->lane->stream != c->stream) MMF_HIP_TRY(hipStreamWaitEvent(fm->lane->stream, f->ev_fi_inputs, 0));
    f->fi_has = true;
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
        rc = frame_superpixels_enqueue(f, r);
        if (rc) return rc;
    }
    if (r.flow) {  // the optical-flow engine, beside the chains
        rc = frame_flow_enqueue(f, r);
        if (rc) return rc;
    }
    r.stamp(f, 0);
    // a host frame announced for the next call: staged and sent up now, while the GPU tracks and the host would only wait
    // (its colour image first; the depth image is joined where the depth side is enqueued, behind the pose)
    rc = fusion_stage_host_rgb(f);
    if (rc) return rc;
    // ... and its image side behind the upload (an announced HOST frame cannot have it at the start of the call: its
    // copy into pinned memory has only just begun then), beside the chain instead of behind the pose
    if (r.early_image != 0 && r.image_early_any && r.next_from_host && !r.tracked.empty() && f->host_next.rgb_staged) {
        MMF_HIP_TRY(fusion_wait_unless_done(f->side2, f->ev_up_rgb[f->host_next.slot]));
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
    if (r.one_pass && r.lanes_wait) MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready, f->ctx->stream));
    return MMF_OK;
}

// performSegmentationCRF (Segmentation.cpp:159-740) on the fusion's stream, into textures[MASK]: stage 1 from every model's
// ICP-error image and the confidence of its splat (the previous frame's prediction), then crf_enqueue; one pinned read of
// the summary.  `out` points at f->mask and f->crf_models.
static int fusion_crf_segment(mmf_fusion* f, mmf_segmentation* out) {
    if (f->shard_world != 1)
        return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the built-in segmentation needs world == 1 (a sharded front end "
                                   "calls mmf_crf_segment in its segmentation callback)");
    mmf_ctx* c = f->ctx;
    const mmf_crf_config& cfg = f->crf_cfg;
    const int M = (int)f->models.size(), W = f->width, H = f->height, S = cfg.spixel_size;
    std::vector<unsigned> ids((size_t)M);
    for (int i = 0; i < M; ++i) ids[(size_t)i] = (unsigned)f->models[(size_t)i]->model->id;
    const unsigned next_id = (unsigned)mmf_fusion_next_model_id(f);
    const int allow_new = f->spawn_offset >= (unsigned)cfg.model_spawn_offset ? 1 : 0;  // (:148)
    CrfWs* w = nullptr;
    const int* labels = nullptr;
    // labels handed in for this frame, then the engine's, then the grid (B3)
    const bool engine = !f->sp_next && f->sp_engine;
    if (engine && !f->sp_enqueued) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the super-pixel engine did not run for this frame");
    int rc = crf_begin(c, &cfg, f->sp_next ? f->sp_labels : (engine ? f->sp_ws.labels() : nullptr), W, H, ids.data(), M, next_id,
                       allow_new, "mmf_fusion_process_frame (segmentation)", &w, &labels);
    if (rc) return rc;
    f->sp_last = labels;
    if (engine) {
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->ev_sp_done, 0));
        f->sp_enqueued = false;
    }
    // behind every model's tracking chain: the chains write the ICP-error images on the models' streams
    for (FusionModel* fm : f->models) {
        hipStream_t ls = fm->lane->stream;
        if (ls == c->stream) continue;
        MMF_HIP_TRY(hipEventRecord(fm->ev_done, ls));
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, fm->ev_done, 0));
    }
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
    rc = crf_enqueue(c, w, &cfg, labels, W, H, f->frame_rgb, w->maps, ids.data(), M, next_id, allow_new, f->mask);
    if (rc) return rc;
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    const mmf::CrfSummary& s = *w->sum_host;
    f->crf_models.assign(s.models, s.models + s.n_models_out);
    std::memset(out, 0, sizeof(*out));
    out->mask = f->mask;
    out->has_new_label = s.has_new_label && !cfg.inhibit_new;  // inhibitModels (:413-415): the mask and the entry stay
    out->n_models = s.n_models_out;
    out->model_data = f->crf_models.data();
    return MMF_OK;
}

// The `frame.mask` branch of performSegmentation (Segmentation.cpp:89-147) on the fusion's stream: `labels` (the frame's raw
// label image, uploaded on this stream or handed in as a device image) into textures[MASK], one pinned read of the summary.
// `out` points at f->mask and f->mask_models.
static int fusion_mask_segment(mmf_fusion* f, const uint8_t* labels, mmf_segmentation* out) {
    if (f->shard_world != 1)
        return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the segmentation from the frame's labels needs world == 1 (a sharded "
                                   "front end calls mmf_mask_segment in its segmentation callback)");
    mmf_ctx* c = f->ctx;
    const int M = (int)f->models.size();
    std::vector<unsigned> ids((size_t)M);
    for (int i = 0; i < M; ++i) ids[(size_t)i] = (unsigned)f->models[(size_t)i]->model->id;
    const unsigned next_id = (unsigned)mmf_fusion_next_model_id(f);
    const int allow_new = f->spawn_offset >= (unsigned)f->mask_cfg.model_spawn_offset ? 1 : 0;  // (:148)
    MaskWs* w = nullptr;
    int rc = mask_enqueue(c, f->width, f->height, labels, f->frame_depth, ids.data(), M, next_id, allow_new, f->mask_map, f->mask,
                          "mmf_fusion_process_frame (segmentation from labels)", &w);
    if (rc) return rc;
    MMF_HIP_TRY(wait_stream(c->stream));
    const mmf::MaskSummary& s = *w->sum_host;
    std::memcpy(f->mask_map, s.mapping, 256);
    f->mask_models.assign(s.models, s.models + s.n_models_out);
    std::memset(out, 0, sizeof(*out));
    out->mask = f->mask;
    out->has_new_label = s.has_new_label && !f->mask_cfg.inhibit_new;  // inhibitModels (:413-415): the mask and the entry stay
    out->n_models = s.n_models_out;
    out->model_data = f->mask_models.data();
    f->mask_info.n_models = s.n_models_out, f->mask_info.allow_new = allow_new;
    f->mask_info.has_new_label = out->has_new_label, f->mask_info.new_label = s.new_label;
    f->mask_valid = true;
    return MMF_OK;
}

// ---- keypoint tracks (MultiMotionFusion.cpp:312-335, 425-436, 584-604, 622-627; tracker_host.hpp) ------------------------------
extern "C" int mmf_fusion_set_tracker(mmf_fusion* f, mmf_tracker* tracker, int odom_init_kp, int icp_refine) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_tracker: null fusion object");
    if (tracker && f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_tracker: sharded use is not supported (world > 1)");
    MMF_REQUIRE(!tracker || (tracker->ctx == f->ctx && tracker->width == f->width && tracker->height == f->height),
                "mmf_fusion_set_tracker: the tracker must share the fusion's context and image size");
    f->tracker = tracker;
    f->kpfe_sp = nullptr;  // (the in-frame front end belongs to the tracker that leaves)
    f->trk_init_kp = tracker && odom_init_kp != 0, f->trk_icp_refine = icp_refine != 0;
    f->trk_ids.clear(), f->trk_T.clear();
    f->view_poses.clear();  // (the entries carry the stamps of the tracker that leaves)
    return MMF_OK;
}

// ---- the keypoint front end inside processFrame (MultiMotionFusion.cpp:223-248) -------------------------------------------
extern "C" int mmf_keypoint_frontend_default_config(mmf_keypoint_frontend_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_keypoint_frontend_default_config: null argument");
    cfg->conf_thresh = 0.015f, cfg->nms_dist = 4, cfg->border = 4;
    cfg->min_feature_distance = 0.7f, cfg->history = 30;  // addKeypoints(..., 0.7f, 30), :240
    cfg->prune_min_kps = 30, cfg->prune_window_ns = 1000000000ll;  // prune(30, t - 1 s), :246
    return MMF_OK;
}

extern "C" int mmf_fusion_set_keypoint_frontend(mmf_fusion* f, mmf_superpoint* sp, const mmf_keypoint_frontend_config* cfg) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_keypoint_frontend: null fusion object");
    if (!sp) {
        f->kpfe_sp = nullptr;
        return MMF_OK;
    }
    MMF_REQUIRE(cfg != nullptr, "mmf_fusion_set_keypoint_frontend: null configuration");
    if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_keypoint_frontend: sharded use is not supported (world > 1)");
    if (!f->tracker) return fail(MMF_ERR_STATE, "mmf_fusion_set_keypoint_frontend: no tracker is attached (mmf_fusion_set_tracker)");
    MMF_REQUIRE(sp->ctx == f->ctx, "mmf_fusion_set_keypoint_frontend: the network must share the fusion's context");
    MMF_REQUIRE(f->width <= sp->max_w && f->height <= sp->max_h && f->width % 8 == 0 && f->height % 8 == 0,
                "mmf_fusion_set_keypoint_frontend: the frame is larger than the network was created for (or its sides are no multiples of 8)");
    MMF_REQUIRE(sp->max_kp <= f->tracker->max_keypoints, "mmf_fusion_set_keypoint_frontend: the network returns more keypoints than the tracker takes");
    MMF_REQUIRE(cfg->nms_dist >= 0 && cfg->border >= 0 && cfg->history >= 0, "mmf_fusion_set_keypoint_frontend: negative radius or history");
    f->kpfe_sp = sp, f->kpfe_cfg = *cfg;
    f->kpfe_caller_adds = f->tracker->caller_adds;
    return MMF_OK;
}

// the frame's keypoints, first thing in the call: features, add, prune on the frame's own device buffers -- all of it
// enqueued, none of it awaited (the frame's first wait stays the pairs call of frame_track_transforms)
static int frame_keypoints(mmf_fusion* f, const mmf_frame* fr) {
    mmf_tracker* t = f->tracker;
    if (!t) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the keypoint front end is on but no tracker is attached");
    if (t->caller_adds != f->kpfe_caller_adds) {
        f->kpfe_caller_adds = t->caller_adds;
        return fail(MMF_ERR_INVALID, "mmf_fusion_process_frame: the keypoint front end is on (mmf_fusion_set_keypoint_frontend): "
                                     "the caller must not add keypoints to the tracker itself");
    }
    const mmf_keypoint_frontend_config& k = f->kpfe_cfg;
    mmf_superpoint* sp = f->kpfe_sp;
    int rc = mmf_superpoint_get_features_device(sp, fr->rgb, f->width, f->height, 3, k.conf_thresh, k.nms_dist, k.border);
    if (rc) return rc;
    rc = tracker_add_counted(t, reinterpret_cast<const int*>(&sp->counters[4]), reinterpret_cast<const int*>(&sp->counters[5]),
                             sp->sel_xy, sp->kp_desc, fr->depth, fr->timestamp, k.min_feature_distance, k.history);
    if (rc) return rc;
    return mmf_tracker_prune(t, k.prune_min_kps, std::max(fr->timestamp - k.prune_window_ns, 0ll));
}

// what the last frame stored on deactivation: per model its id, the number of views and their rows in all
extern "C" int mmf_fusion_last_stored_views(mmf_fusion* f, int* model_ids, int* n_views, int* rows, int capacity, int* n_out) {
    MMF_REQUIRE(f && n_out && capacity >= 0, "mmf_fusion_last_stored_views: bad argument");
    *n_out = (int)f->stored_ids.size();
    for (int i = 0; i < *n_out && i < capacity; ++i) {
        if (model_ids) model_ids[i] = f->stored_ids[(size_t)i];
        if (n_views) n_views[i] = f->stored_views[(size_t)i];
        if (rows) rows[i] = f->stored_rows[(size_t)i];
    }
    return MMF_OK;
}
extern "C" int mmf_fusion_last_track_transforms(mmf_fusion* f, float* T, int capacity, int* n_out) {
    MMF_REQUIRE(f && n_out && capacity >= 0 && (T || capacity == 0), "mmf_fusion_last_track_transforms: bad argument");
    *n_out = (int)(f->trk_T.size() / 16);
    for (int i = 0; i < *n_out && i < capacity; ++i) std::memcpy(T + 16 * i, f->trk_T.data() + 16 * (size_t)i, 16 * sizeof(float));
    return MMF_OK;
}

// model->getLastTrackTransform() of every active model (:322), list order: one pairs launch, one wait, RANSAC on the host
static int frame_track_transforms(mmf_fusion* f) {
    std::vector<int> ids;
    for (FusionModel* fm : f->models) ids.push_back((int)fm->model->id);
    const float *p0 = nullptr, *p1 = nullptr;
    const int* counts = nullptr;
    int stride = 0;
    int rc = mmf_tracker_last_pairs(f->tracker, ids.data(), (int)ids.size(), &p0, &p1, &counts, &stride);
    if (rc) return rc;
    f->trk_T.resize(16 * ids.size());
    for (size_t k = 0; k < ids.size(); ++k) {
        const mmf::RigidRANSAC::Result res = tracker_transform(p0 + k * (size_t)stride * 3, p1 + k * (size_t)stride * 3, counts[k], kTrackRansac);
        isometry_to_4x4(res.transformation, f->trk_T.data() + 16 * k);
    }
    return MMF_OK;
}

// the models' track sets after the frame's segmentation, spawn and redetection (:584-604; one model: :622-627; the first
// frame: initGlobalTracks); a model that left the active list since the last association is forgotten
static int frame_associate_tracks(mmf_fusion* f, bool all, bool by_mask) {
    std::vector<int> ids;
    for (FusionModel* fm : f->models) ids.push_back((int)fm->model->id);
    for (int old : f->trk_ids)
        if (std::find(ids.begin(), ids.end(), old) == ids.end()) {
            int rc = mmf_tracker_forget_model(f->tracker, old);
            if (rc) return rc;
        }
    f->trk_ids = ids;
    if (all) return mmf_tracker_associate_all(f->tracker, ids.data(), (int)ids.size());
    if (by_mask) return mmf_tracker_associate(f->tracker, f->mask, ids.data(), (int)ids.size());
    return MMF_OK;  // (a frame with a dictated pose has no segmentation)
}

// ---- keypoint redetection (MultiMotionFusion.cpp:425-436, 489-559) ----------------------------------------------------------
static int fusion_viewstore(mmf_fusion* f) {
    if (f->views) return MMF_OK;
    return mmf_viewstore_create(f->ctx, &f->views);
}
extern "C" mmf_viewstore* mmf_fusion_viewstore(mmf_fusion* f) {
    if (!f || fusion_viewstore(f) != MMF_OK) return nullptr;
    return f->views;
}
// setEnableRedetection (MultiMotionFusion.h:414 defaults to true; here OFF by default: every call behaves as before)
extern "C" int mmf_fusion_set_redetection(mmf_fusion* f, int on) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_redetection: null fusion object");
    if (on && f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_redetection: sharded redetection is not supported (world > 1)");
    if (on) {
        int rc = fusion_viewstore(f);
        if (rc) return rc;
    }
    f->redetect_on = on != 0;
    return MMF_OK;
}
// where the geometric verification of the redetection candidates runs: 0 = on the host, one RigidRANSAC per (segment, model)
// running on from view to view (the default); 1 = on the device, a fresh one per view (ransac_kernels.hpp)
static std::atomic<int> g_redetect_max_points{mmf::kRansacMaxPoints};
extern "C" int mmf_debug_set_redetect_max_points(int max_points) {
    MMF_REQUIRE(max_points >= 3 && max_points <= mmf::kRansacMaxPoints, "mmf_debug_set_redetect_max_points: 3 .. 1024");
    g_redetect_max_points.store(max_points);
    return MMF_OK;
}
extern "C" int mmf_fusion_set_redetection_verifier(mmf_fusion* f, int mode) {
    MMF_REQUIRE(f && (mode == 0 || mode == 1), "mmf_fusion_set_redetection_verifier: mode is 0 (host) or 1 (device)");
    if (mode && f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_redetection_verifier: not supported on a shard (world > 1)");
    if (mode == f->redetect_verifier) return MMF_OK;
    int rc = fusion_viewstore(f);
    if (rc) return rc;
    if (mode) {
        const mmf_ransac_config cfg{kRedetectRansac.iterations, kRedetectRansac.inlier_threshold, kRedetectRansac.inlier_fraction};
        rc = mmf_ransac_batch_create(f->ctx, &cfg, g_redetect_max_points.load(), &f->verifier);
        if (rc) return rc;
        rc = mmf_viewstore_set_verifier(f->views, f->verifier);
        if (rc) return rc;
    } else {
        rc = mmf_viewstore_set_verifier(f->views, nullptr);
        if (rc) return rc;
        mmf_ransac_batch_destroy(f->verifier);  // (waits for the stream)
        f->verifier = nullptr;
    }
    f->redetect_verifier = mode;
    return MMF_OK;
}
extern "C" int mmf_fusion_redetection_host_verified(mmf_fusion* f) { return f ? f->host_verified : -1; }

// the last keypoint of every currently visible track (track->back(), :428-436) for the NEXT processFrame only: HOST arrays
// xy [n][2] integer pixels, coordinate [n][3] camera frame (non-finite allowed), descriptor [n][256].  Copied.
extern "C" int mmf_fusion_set_keypoints(mmf_fusion* f, int n, const int* xy, const float* coordinate, const float* descriptor) {
    MMF_REQUIRE(f && n >= 0 && ((xy && coordinate && descriptor) || n == 0), "mmf_fusion_set_keypoints: bad argument");
    f->kp_xy.assign(xy, xy + 2 * (size_t)n);
    f->kp_coord.assign(coordinate, coordinate + 3 * (size_t)n);
    f->kp_desc.assign(descriptor, descriptor + (size_t)kRdDim * (size_t)n);
    f->kp_next = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_last_redetections(mmf_fusion* f, mmf_redetection* out, int capacity, int* n_out) {
    MMF_REQUIRE(f && n_out && capacity >= 0 && (out || capacity == 0), "mmf_fusion_last_redetections: bad argument");
    *n_out = (int)f->redetections.size();
    for (int i = 0; i < *n_out && i < capacity; ++i) out[i] = f->redetections[(size_t)i];
    return MMF_OK;
}

// Isometry3f::inverse(): [R^T | -(R^T t)], float, sums left to right
static void redetect_inverse_pose(const mmf::Isometry3f& T, float pose[16]) {
    identity16(pose);
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) pose[r * 4 + q] = T.R[q * 3 + r];
        float s = T.R[0 * 3 + r] * T.t[0];
        s = s + T.R[1 * 3 + r] * T.t[1];
        s = s + T.R[2 * 3 + r] * T.t[2];
        pose[r * 4 + 3] = -s;
    }
}

// models.remove(model_act_rm) (:542): the reference drops the model; freed once nothing enqueued uses it
static int redetect_drop_active(mmf_fusion* f, FusionModel* fm) {
    f->models.erase(std::find(f->models.begin(), f->models.end(), fm));
    MMF_HIP_TRY(hipStreamSynchronize(fm->lane->stream));
    MMF_HIP_TRY(hipStreamSynchronize(f->ctx->stream));  // (batched passes and the segmentation read it from there)
    for (FusionModel* m : f->models)
        if (m->lane->stream != f->ctx->stream) MMF_HIP_TRY(hipStreamSynchronize(m->lane->stream));  // (a batch led by another object)
    if (f->views) mmf_viewstore_forget(f->views, (int)fm->model->id);
    fusion_model_destroy(fm);
    return MMF_OK;
}

// Model::activate(pose, timestamp) (Model.cpp:1646-1656) + models.push_back (:544): the model is in the state
// overridePose leaves (pose == lastPose), nothing prepared ahead is valid, and its stream -- idle since it left the list --
// continues behind this frame's inputs.  Its extents (extent.hpp) need nothing: they are stamped with the frame that noted them.
static int redetect_activate(mmf_fusion* f, FusionModel* fm, const float pose[16]) {
    mmf_model_set_pose(fm->model, pose);
    std::memcpy(fm->last_pose, pose, sizeof(float) * 16);
    fm->unseen = 0;
    fm->tracking = false, fm->early_done = false, fm->early_fused = false;
    fm->spec_valid = false, fm->spec_hit = false;
    fm->odom->so3_prefetched = false, fm->odom->so3_stage = nullptr;
    f->inactive.erase(std::find(f->inactive.begin(), f->inactive.end(), fm));
    f->models.push_back(fm);
    if (fusion_view_log_on(f)) {  // Model::activate (:1646-1656): one pose, the activation's
        mmf_fusion::ViewPose e;
        e.stamp = (int)f->tracker->frame;
        std::memcpy(e.pose, pose, sizeof(e.pose));
        f->view_poses[(int)fm->model->id].assign(1, e);
    }
    if (fm->lane->stream != f->ctx->stream) return lane_wait(fm, f->ev_frame_ready);
    return MMF_OK;
}

// :425-436 + :489-559.  Waits on the host twice: for the keypoints' labels, then for the matches of all segments.
// *has_new: segmentationResult.hasNewLabel, cancelled by an accepted match (:522-524).
static int frame_redetect(mmf_fusion* f, bool* has_new) {
    const bool have_kp = f->kp_next;
    f->kp_next = false;  // (for this frame only)
    if (!f->redetect_on || !(have_kp || f->tracker) || f->inactive.empty() || !f->views || f->views->views.empty()) return MMF_OK;
    if (!have_kp) {  // no mmf_fusion_set_keypoints for this frame: the attached tracker's visible set (:428-431)
        int nv = 0;
        int rc = tracker_visible_device(f->tracker, &nv);
        if (rc) return rc;
        f->kp_xy.resize(2 * (size_t)nv), f->kp_coord.resize(3 * (size_t)nv), f->kp_desc.resize((size_t)kRdDim * (size_t)nv);
        if (nv > 0) {
            MMF_HIP_TRY(hipMemcpy(f->kp_xy.data(), f->tracker->vis_xy, f->kp_xy.size() * sizeof(int), hipMemcpyDeviceToHost));
            MMF_HIP_TRY(hipMemcpy(f->kp_coord.data(), f->tracker->vis_co, f->kp_coord.size() * sizeof(float), hipMemcpyDeviceToHost));
            MMF_HIP_TRY(hipMemcpy(f->kp_desc.data(), f->tracker->vis_desc, f->kp_desc.size() * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    mmf_ctx* c = f->ctx;
    mmf_viewstore* vs = f->views;
    const size_t n = f->kp_xy.size() / 2;
    if (n == 0) return MMF_OK;
    if (n > f->kp_cap) {
        if (f->kp_xy_pin) (void)hipHostFree(f->kp_xy_pin);
        if (f->kp_label_pin) (void)hipHostFree(f->kp_label_pin);
        f->kp_xy_pin = f->kp_label_pin = nullptr, f->kp_cap = 0;
        const size_t cap = n + n / 2 + 64;
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&f->kp_xy_pin), cap * 2 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&f->kp_label_pin), cap * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        f->kp_cap = cap;
    }
    std::memcpy(f->kp_xy_pin, f->kp_xy.data(), n * 2 * sizeof(int));
    hipLaunchKernelGGL(mmf::rd_gather_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)f->mask,
                       f->width, f->height, (const int*)f->kp_xy_pin, (int)n, f->kp_label_pin);
    MMF_HIP_TRY(hipGetLastError());
    MMF_HIP_TRY(wait_stream(c->stream));  // wait 1: the labels
    // per label other than 0 and 255 the keypoints with finite coordinates (:494-507), labels ascending
    std::vector<std::vector<int>> by_label(256);
    for (size_t i = 0; i < n; ++i) {
        const int l = f->kp_label_pin[i];
        const float* p = f->kp_coord.data() + 3 * i;
        if (l <= 0 || l >= 255) continue;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
        by_label[(size_t)l].push_back((int)i);
    }
    std::vector<RdSet> sets;
    std::vector<int> set_label;
    size_t total_q = 0;
    for (int l = 1; l < 255; ++l) {
        if (by_label[(size_t)l].size() < 3) continue;  // min_tracks (:493, :507)
        sets.push_back(RdSet{nullptr, (int)by_label[(size_t)l].size(), total_q});
        set_label.push_back(l);
        total_q += by_label[(size_t)l].size();
    }
    if (sets.empty()) return MMF_OK;
    int rc = viewstore_stage(vs, total_q);
    if (rc) return rc;
    std::vector<float> coords(total_q * 3);
    for (size_t s = 0; s < sets.size(); ++s) {
        sets[s].q = vs->q_dev + sets[s].q0 * kRdDim;
        const std::vector<int>& idx = by_label[(size_t)set_label[s]];
        for (size_t k = 0; k < idx.size(); ++k) {
            std::memcpy(vs->q_pin + (sets[s].q0 + k) * kRdDim, f->kp_desc.data() + (size_t)idx[k] * kRdDim, kRdDim * sizeof(float));
            std::memcpy(coords.data() + (sets[s].q0 + k) * 3, f->kp_coord.data() + (size_t)idx[k] * 3, 3 * sizeof(float));
        }
    }
    MMF_HIP_TRY(hipMemcpyAsync(vs->q_dev, vs->q_pin, total_q * kRdDim * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const bool on_device = f->redetect_verifier == 1 && vs->verifier;
    if (on_device) {  // the segments' coordinates travel with their descriptors
        if (total_q * 3 > vs->qc_cap) {  // (every earlier verification has been awaited)
            if (vs->qc_pin) (void)hipHostFree(vs->qc_pin);
            (void)hipFree(vs->qc_dev);
            vs->qc_pin = vs->qc_dev = nullptr, vs->qc_cap = 0;
            const size_t cap = total_q * 3 + total_q * 3 / 2 + 192;
            MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&vs->qc_pin), cap * sizeof(float), hipHostMallocDefault));
            MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&vs->qc_dev), cap * sizeof(float)));
            vs->qc_cap = cap;
        }
        std::memcpy(vs->qc_pin, coords.data(), total_q * 3 * sizeof(float));
        MMF_HIP_TRY(hipMemcpyAsync(vs->qc_dev, vs->qc_pin, total_q * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    rc = viewstore_enqueue(vs, c->stream, sets.data(), (int)sets.size());
    if (rc) return rc;
    // device verifier: behind the matches of all segments the two verification launches for ALL (segment, inactive model)
    // pairs of the frame, before the one wait.  (No match launched -- a store of empty views: nothing can be found.)
    std::vector<int> asked;
    const bool verified = on_device && vs->last_launches > 0;
    if (verified) {
        std::vector<mmf::RdVerifySet> vsets(sets.size());
        for (size_t s = 0; s < sets.size(); ++s) vsets[s] = mmf::RdVerifySet{vs->qc_dev + sets[s].q0 * 3, sets[s].nq, (int)sets[s].q0};
        for (const FusionModel* im : f->inactive) asked.push_back((int)im->model->id);
        rc = viewstore_enqueue_verify(vs, c->stream, vsets.data(), (int)vsets.size(), asked.data(), (int)asked.size());
        if (rc) return rc;
    }
    MMF_HIP_TRY(wait_stream(c->stream));  // wait 2: the matches of every segment against every view (and their verification)
    for (size_t s = 0; s < sets.size(); ++s) {
        const int label = set_label[s];
        const bool too_large = on_device && sets[s].nq > vs->verifier->max_points;  // verified here, under the verifier's rule
        if (too_large) ++f->host_verified;
        for (size_t mi = 0; mi < f->inactive.size();) {
            FusionModel* im = f->inactive[mi];
            RdBest best;
            if (!on_device) {
                best = viewstore_best(vs, (int)im->model->id, sets[s], coords.data() + sets[s].q0 * 3, kRedetectRansac);
            } else if (too_large) {
                best = viewstore_best_fresh(vs, (int)im->model->id, sets[s], coords.data() + sets[s].q0 * 3, vs->verifier->cfg);
            } else if (verified) {  // the record of (segment, model): a model an earlier segment activated has left the list
                const size_t a = (size_t)(std::find(asked.begin(), asked.end(), (int)im->model->id) - asked.begin());
                const mmf::RdRecord& rec = vs->rec_pin[s * asked.size() + a];
                best.found = rec.found != 0, best.error = rec.error, best.inliers = rec.inliers, best.view = rec.view, best.n_matches = rec.n_matches;
                for (int r = 0; r < 3; ++r) {
                    for (int q = 0; q < 3; ++q) best.transformation.R[r * 3 + q] = rec.T[r * 4 + q];
                    best.transformation.t[r] = rec.T[r * 4 + 3];
                }
            }
            if (!(best.found && (double)best.error < 0.01 && best.inliers > 5)) {  // :516
                ++mi;
                continue;
            }
            *has_new = false;  // :522-524
            mmf_redetection rd;
            std::memset(&rd, 0, sizeof(rd));
            rd.label = label, rd.model_id = (int)im->model->id, rd.removed_id = -1, rd.activated = 0;
            rd.error = best.error, rd.inliers = best.inliers, rd.view = best.view;
            isometry_to_4x4(best.transformation, rd.transformation);
            FusionModel* act = fusion_find(f, label);
            if (act && act->model->id < im->model->id) {  // an older model is not replaced by a newer one (:537-541)
                f->redetections.push_back(rd);
                ++mi;
                continue;
            }
            if (act) {
                rd.removed_id = (int)act->model->id;
                rc = redetect_drop_active(f, act);
                if (rc) return rc;
            }
            float pose[16];
            redetect_inverse_pose(best.transformation, pose);  // activate(best.transformation.inverse(), ...) (:545)
            rc = redetect_activate(f, im, pose);  // (leaves the inactive list: inactive[mi] is the next one)
            if (rc) return rc;
            rd.activated = 1;
            f->redetections.push_back(rd);
        }
    }
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
    const bool from_labels = f->mask_on && seg && seg->mask && !seg->model_data;
    const int spawn_after = from_labels ? f->mask_cfg.model_spawn_offset : f->crf_cfg.model_spawn_offset;
    if (f->spawn_offset < (unsigned)spawn_after) f->spawn_offset++;  // (:410)
    if (from_labels) {
        int rc = fusion_mask_segment(f, seg->mask, &seg_cb);
        if (rc) return rc;
        seg = &seg_cb;
    } else if (!seg && f->seg_fn) {  // performSegmentation(frame) (:412)
        std::memset(&seg_cb, 0, sizeof(seg_cb));
        if (f->seg_fn(f->seg_user, f, fr, &seg_cb)) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the segmentation callback failed");
        seg = &seg_cb;
    } else if (!seg && f->crf_on) {
        int rc = fusion_crf_segment(f, &seg_cb);
        if (rc) return rc;
        seg = &seg_cb;
    }
    MMF_REQUIRE(seg && seg->mask, "mmf_fusion_process_frame: enableMultipleModels needs a segmentation "
                                  "(mmf_frame::segmentation, mmf_fusion_set_segmentation_callback, mmf_fusion_set_crf_segmentation "
                                  "or, for a frame that brings its labels, mmf_fusion_set_mask_segmentation)");
    // textures[MASK]->Upload(fullSegmentation) (:416)
    if (seg->mask != f->mask)
        MMF_HIP_TRY(hipMemcpyAsync(f->mask, seg->mask, (size_t)f->width * f->height, hipMemcpyDeviceToDevice, c->stream));
    f->mask_is_zero = false;
    MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready, c->stream));
    const int n_data = seg->model_data ? seg->n_models : 0;
    // redetection via keypoints (:489-559) runs BEFORE a model is spawned: a label it cancels (:522-524) consumes neither an id
    // nor a preallocated model (the reference spawns first and abandons newModel, :468-487, :565)
    bool has_new = seg->has_new_label != 0;
    {
        int rc = frame_redetect(f, &has_new);
        if (rc) return rc;
    }
    if (seg->has_new_label && !has_new) f->spawn_offset = 0;  // (the reference had spawned already: :484)
    FusionModel* fresh = nullptr;
    if (has_new) {  // :469-487
        int rc = fusion_spawn(f, &fresh);
        if (rc) return rc;
        f->spawn_offset = 0;  // (:484)
        if (n_data > 0) fresh->model->max_depth = seg_max_depth(seg->model_data[n_data - 1]);
    }
    // Set max-depth (:585-586)
    for (size_t i = 1; i < f->models.size() && (int)i < n_data; ++i) f->models[i]->model->max_depth = seg_max_depth(seg->model_data[i]);
    if (fresh && !fusion_owns_model(f, fresh)) {
        f->models.push_back(fresh);  // another rank's model: bookkeeping only
    } else if (fresh) {  // :588-601: the first surfels of the new model, then it joins the list
        int rc = lane_wait(fresh, f->ev_frame_ready);
        if (rc) return rc;
        identity16(fresh->last_pose);
        float pose[16];
        mmf_model_get_pose(fresh->model, pose);
        rc = mmf_model_predict_indices(fresh->model, f->tick, g.max_depth_processed, g.time_delta);
        if (rc) return rc;
        rc = mmf_model_fuse(fresh->model, f->tick, f->frame_rgb, f->mask, f->frame_depth, f->depth_filtered, g.max_depth_processed,
                            fusion_weight(pose, fresh->last_pose, 100.f));  // fuse(..., 100) (:591-592)
        if (rc) return rc;
        // (the second predictIndices is commented out in the reference, :594)
        rc = mmf_model_clean(fresh->model, f->tick, g.time_delta, g.max_depth_processed, f->depth_filtered, f->mask, g.outlier_coeff);
        if (rc) return rc;
        f->models.push_back(fresh);  // moveNewModelToList (:600)
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
    MMF_HIP_TRY(hipEventRecord(f->ev_inputs_free, f->ctx->stream));
    f->inputs_free_recorded = true;
    MMF_HIP_TRY(hipEventRecord(f->ev_frame_ready, f->ctx->stream));
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
    MMF_HIP_TRY(hipEventRecord(objs[0]->ev_done, st));
    for (size_t k = 1; k < objs.size(); ++k) MMF_HIP_TRY(hipStreamWaitEvent(objs[k]->lane->stream, objs[0]->ev_done, 0));
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
            int rc = lane_wait(fm, f->ev_frame_ready);
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
    int rc = lane_wait(objs[0], f->ev_frame_ready);
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
        return models_fuse_clean_rect(ms, n, st, f->tick, g.time_delta, g.max_depth_processed, f->frame_rgb, f->mask, f->frame_depth,
                                      f->depth_filtered, g.outlier_coeff, wts, f->mask_boxes, f->mask_gen);
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
        if (only == global && !stages.empty() && fr->next_rgb && f->image_pre_rgb == fr->next_rgb && !g.rgb_only) {
            const OdomState* stage = (g.so3 && f->so3_stage_ready >= 0) ? f->so3_stage[f->so3_stage_ready] : nullptr;
            if (!g.so3 || stage != nullptr) {
                if (stage) MMF_HIP_TRY(fusion_wait_unless_done(st, f->ev_prefetch2_done));  // (the staged pre-alignment is complete)
                ride = odom_begin_rider(only->odom, only->spec_pose, track_mode(g.rgb_only, g.icp_weight, g.pyramid, g.fast_odom, g.so3),
                                        stage, &rider);
            }
        }
        if (!ride) only->odom->begin_spec_valid = false;
        int rc = stages.launch(st, ride ? &rider : nullptr);
        if (rc) return rc;
        only->spec_tex_gen = m->tex_gen;
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
            fm->spec_tex_gen = fm->model->tex_gen;
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
        if (!fusion_owns(f, k)) continue;
        MMF_HIP_TRY(hipEventRecord(fm->ev_done, fm->lane->stream));
        MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, fm->ev_done, 0));
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
    if (f->kpfe_sp && !(f->tracker && r.have_init)) {  // (a frame the check below refuses adds nothing)
        int rc = frame_keypoints(f, fr);
        if (rc) return rc;
    }
    mmf_frame fr_kp;  // the frame with the transformations of the attached tracker (odom_cfg.init == "kp")
    if (f->tracker) {
        MMF_REQUIRE(!r.have_init, "mmf_fusion_process_frame: a tracker is attached (mmf_fusion_set_tracker): the frame cannot bring init_transforms");
        f->trk_T.clear();
        if (f->trk_init_kp && r.track) {
            int rc = frame_track_transforms(f);
            if (rc) return rc;
            fr_kp = *fr;
            fr_kp.init_transforms = f->trk_T.data(), fr_kp.n_init_transforms = (int)(f->trk_T.size() / 16);
            fr_kp.icp_refine = f->trk_icp_refine ? 1 : 0;
            fr = &fr_kp, r.fr = fr, r.have_init = true;
        }
    }
    f->t_tracking_s = 0;
    f->redetections.clear();  // (mmf_fusion_last_redetections speaks of this call)
    f->stored_ids.clear(), f->stored_views.clear(), f->stored_rows.clear();
    int rc = MMF_OK;
    if (f->flow) {
        f->fi_has = false;
        rc = frame_flow_begin(f, r);
        if (rc) return rc;
    }
    rc = frame_begin(f, r);
    if (rc) return rc;
    const bool first = f->tick == 1;
    if (r.flow && (first || !r.track)) {  // (a tracked frame enqueues it behind its chains: frame_track)
        rc = frame_flow_enqueue(f, r);
        if (rc) return rc;
    }
    if (first) {
        rc = frame_first(f, r);
        if (rc) return rc;
    } else {
        f->tracking_ok = 1;
        if (f->sp_engine && r.track && f->cfg.enable_multiple_models && !fr->segmentation && !f->seg_fn && f->crf_on && !f->sp_next) {
            rc = frame_superpixels_begin(f, r);
            if (rc) return rc;
        }
        rc = r.track ? frame_track(f, r) : frame_dictated_pose(f, r);
        if (rc) return rc;
        if (r.track) fusion_note_view_poses(f, true);
        if (f->fi_on && r.track && r.flow_enqueued && f->flow_has) {
            rc = frame_flow_inference(f);
            if (rc) return rc;
        }
        if (r.track && f->cfg.enable_multiple_models) {
            rc = frame_segment(f, r);
            if (rc) return rc;
        }
        r.stamp(f, 2);
    }
    if (f->tracker) {
        if (r.track && !first) fusion_note_view_poses(f, false);
        rc = frame_associate_tracks(f, first || !f->cfg.enable_multiple_models, r.track);
        if (rc) return rc;
    }
    f->sp_next = false;  // (mmf_fusion_set_superpixels: this call's labels only, whichever segmentation ran)
    f->kp_next = false;  // (mmf_fusion_set_keypoints: this call's keypoints only, whether or not a segmentation ran)
    r.pass_mode = fusion_batch_mode(f);  // (the model list stays as it is from here to the end of the call)
    if (!first) {
        rc = frame_fuse_clean(f, r);
        if (rc) return rc;
    }
    r.stamp(f, 3);
    rc = frame_predict(f, r);
    if (rc) return rc;
    r.stamp(f, 4);
    f->tick++;  // :825
    frame_log_poses(f, r);
    rc = frame_end(f, r);
    if (rc) return rc;
    if (r.flow_enqueued) {
        rc = frame_flow_join(f);
        if (rc) return rc;
    }
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

// ---- processFrame(const FrameData&) with the frame still in host memory ------------------------------------------
// The reference uploads FrameData::rgb / depth to GL textures at :221, :261.  Here rgb, depth (and the optional id image)
// go through pinned staging buffers into device copies, three deep, on a stream of their own.
static int fusion_up_init(mmf_fusion* f) {
    if (f->up_pin[0]) return MMF_OK;
    const size_t total = (size_t)f->width * f->height * 8;  // 8 B/px: depth f32, rgb u8 x 3, id u8
    for (int i = 0; i < mmf_fusion::kUp; ++i) {
        MMF_HIP_TRY(hipHostMalloc((void**)&f->up_pin[i], total, hipHostMallocDefault));
        MMF_HIP_TRY(hipMalloc((void**)&f->up_dev[i], total));
        MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_up[i], hipEventDisableTiming));
        MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_up_rgb[i], hipEventDisableTiming));
    }
    MMF_HIP_TRY(hipStreamCreateWithFlags(&f->up_stream, hipStreamNonBlocking));
    MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_up_begin, hipEventDisableTiming));
    return MMF_OK;
}
// host -> pinned -> device of rgb, then depth, into `slot`, on the upload stream; ev_up_rgb[slot] / ev_up[slot] mark the
// arrivals.  The colour image goes first: the next frame's image side (intensity pyramid, gradients, SO3) needs only that
// and runs beside the chain, the depth side is enqueued behind the pose.  after_begin: see mmf_fusion::host_caught_up.
static int fusion_up_stage(mmf_fusion* f, int slot, const uint8_t* rgb_host, const float* depth_host, bool after_begin,
                           mmf_fusion::Stager* announce) {
    const size_t npix = (size_t)f->width * f->height;
    // the staging buffer's previous upload must have left it (round-2 advisor finding: nothing made sure of that)
    if (f->up_recorded[slot]) MMF_HIP_TRY(hipEventSynchronize(f->ev_up[slot]));
    std::memcpy(f->up_pin[slot] + npix * 4, rgb_host, npix * 3);
    // the device copy's last readers are frames enqueued before this call (ev_up_begin: recorded when the call began --
    // NOT now: by now this frame's whole tracking chain sits on the fusion's stream and the upload is meant to overlap it)
    if (after_begin) MMF_HIP_TRY(hipStreamWaitEvent(f->up_stream, f->ev_up_begin, 0));
    MMF_HIP_TRY(hipMemcpyAsync(f->up_dev[slot] + npix * 4, f->up_pin[slot] + npix * 4, npix * 3, hipMemcpyHostToDevice, f->up_stream));
    MMF_HIP_TRY(hipEventRecord(f->ev_up_rgb[slot], f->up_stream));
    if (announce) {
        {
            std::lock_guard<std::mutex> lock(announce->mu);
            announce->rgb_done = true;
        }
        announce->cv.notify_all();
    }
    std::memcpy(f->up_pin[slot], depth_host, npix * 4);
    MMF_HIP_TRY(hipMemcpyAsync(f->up_dev[slot], f->up_pin[slot], npix * 4, hipMemcpyHostToDevice, f->up_stream));
    MMF_HIP_TRY(hipEventRecord(f->ev_up[slot], f->up_stream));
    f->up_recorded[slot] = true;
    return MMF_OK;
}
// the staging thread: one job at a time (mmf_fusion::Stager)
static void fusion_stager_main(mmf_fusion* f) {
    mmf_fusion::Stager& s = f->stager;
    (void)hipSetDevice(f->ctx->device);
    std::unique_lock<std::mutex> lock(s.mu);
    for (;;) {
        s.cv.wait(lock, [&] { return s.stop || s.busy; });
        if (s.stop) return;
        const int slot = s.slot;
        const uint8_t* rgb = s.rgb;
        const float* depth = s.depth;
        const bool after_begin = s.after_begin;
        lock.unlock();
        const int rc = fusion_up_stage(f, slot, rgb, depth, after_begin, &s);
        const std::string err = rc ? std::string(mmf_last_error()) : std::string();  // (the error text is per thread)
        lock.lock();
        s.rc = rc, s.error = err, s.busy = false, s.rgb_done = true;
        s.cv.notify_all();
    }
}
// hands the announced frame to the staging thread (started on first use)
static int fusion_stage_host_begin(mmf_fusion* f, bool after_begin) {
    mmf_fusion::HostNext& hn = f->host_next;
    mmf_fusion::Stager& s = f->stager;
    if (!s.thread.joinable()) s.thread = std::thread(fusion_stager_main, f);
    {
        std::lock_guard<std::mutex> lock(s.mu);
        s.slot = hn.slot, s.rgb = hn.rgb, s.depth = hn.depth, s.busy = true, s.rgb_done = false, s.after_begin = after_begin;
    }
    s.cv.notify_all();
    hn.pending = true;
    return MMF_OK;
}
// the hinted next frame's upload has been enqueued when this returns (ev_up[slot] recorded): called before anything is told
// to wait for that event -- inside processFrame where the host would only wait for the pose, in the prefetch, or at the
// latest when the call returns
static int fusion_stage_host_next(mmf_fusion* f) {
    mmf_fusion::HostNext& hn = f->host_next;
    if (!hn.pending) return MMF_OK;
    hn.pending = false;
    mmf_fusion::Stager& s = f->stager;
    std::unique_lock<std::mutex> lock(s.mu);
    s.cv.wait(lock, [&] { return !s.busy; });
    if (s.rc) return fail(s.rc, s.error);
    hn.staged = hn.rgb_staged = true;
    return MMF_OK;
}
// ... only its colour image's (ev_up_rgb[slot] recorded): what the image side enqueued beside the chain waits for
static int fusion_stage_host_rgb(mmf_fusion* f) {
    mmf_fusion::HostNext& hn = f->host_next;
    if (!hn.pending || hn.rgb_staged) return MMF_OK;
    mmf_fusion::Stager& s = f->stager;
    std::unique_lock<std::mutex> lock(s.mu);
    s.cv.wait(lock, [&] { return s.rgb_done; });
    if (!s.busy && s.rc) return MMF_OK;  // (the join reports it)
    hn.rgb_staged = true;
    return MMF_OK;
}

// next_rgb_host / next_depth_host (both or neither): the frame the NEXT call will be given (same pointers, contents
// unchanged until then) -- the host-memory form of mmf_frame::next_*: it is staged and uploaded during this call and its
// sensor-side preparation overlaps this frame's fusion, so the next call starts with its frame on the device.
extern "C" int mmf_fusion_process_frame_host_next(mmf_fusion* f, const uint8_t* rgb_host, const float* depth_host,
                                                  const uint8_t* mask_host, int has_new_label, long long timestamp,
                                                  const float* in_pose, float weight_multiplier, int bootstrap,
                                                  const uint8_t* next_rgb_host, const float* next_depth_host) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_process_frame_host: null fusion object");
    if (!rgb_host || !depth_host || timestamp < 0) return fail(MMF_ERR_INVALID, "invalid image data");  // :209-212
    mmf_ctx* c = f->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (int rc = fusion_up_init(f)) return rc;
    const size_t npix = (size_t)f->width * f->height;
    const size_t o_depth = 0, o_rgb = npix * 4, o_mask = npix * 7;
    mmf_fusion::HostNext& hn = f->host_next;
    if (int rc = fusion_stage_host_next(f)) return rc;  // (nothing of an earlier announcement is still being staged)
    // what a refilled slot's upload has to wait for: the work enqueued before this call -- nothing, when the last call
    // ended with the host holding a pose from the fusion's stream (every lane joins that stream at the end of a frame)
    const bool host_knows = !tunables().host_up_events;
    const bool after_begin = !(host_knows && f->host_caught_up);
    if (after_begin) MMF_HIP_TRY(hipEventRecord(f->ev_up_begin, c->stream));
    int slot;
    if (hn.staged && hn.rgb == rgb_host && hn.depth == depth_host) {  // announced by the previous call: already on its way
        slot = hn.slot;
    } else {
        if (hn.staged || hn.pending) f->pre_rgb = nullptr, f->pre_depth = nullptr;  // what was prepared belongs to a frame that never came
        slot = f->up_cur;                                                          // (its device buffer is about to be reused)
        if (int rc = fusion_up_stage(f, slot, rgb_host, depth_host, after_begin, nullptr)) return rc;
    }
    hn = mmf_fusion::HostNext();
    f->up_cur = (slot + 1) % mmf_fusion::kUp;
    // (an announced frame arrived during the last call as a rule: then the fusion's stream gets no barrier packet)
    if (host_knows)
        MMF_HIP_TRY(fusion_wait_unless_done(c->stream, f->ev_up[slot]));
    else
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->ev_up[slot], 0));
    mmf_frame fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.rgb = f->up_dev[slot] + o_rgb, fr.depth = (const float*)(f->up_dev[slot] + o_depth), fr.timestamp = timestamp;
    fr.in_pose = in_pose, fr.weight_multiplier = weight_multiplier, fr.bootstrap = bootstrap;
    fr.icp_refine = 1;
    mmf_segmentation seg;
    std::memset(&seg, 0, sizeof(seg));
    if (mask_host) {  // the id image is this frame's segmentation result: it cannot be announced a frame ahead
        std::memcpy(f->up_pin[slot] + o_mask, mask_host, npix);
        MMF_HIP_TRY(hipMemcpyAsync(f->up_dev[slot] + o_mask, f->up_pin[slot] + o_mask, npix, hipMemcpyHostToDevice, c->stream));
        seg.mask = f->up_dev[slot] + o_mask, seg.has_new_label = has_new_label;
        fr.segmentation = &seg;
    }
    if (next_rgb_host && next_depth_host) {
        hn.rgb = next_rgb_host, hn.depth = next_depth_host, hn.slot = f->up_cur;
        fr.next_rgb = f->up_dev[hn.slot] + o_rgb, fr.next_depth = (const float*)(f->up_dev[hn.slot] + o_depth);
        if (int rc = fusion_stage_host_begin(f, after_begin)) return rc;  // staged and sent up beside this call's own work
    }
    int rc = fusion_process_frame_impl(f, &fr);
    if (rc) {  // the staging thread may still be reading the caller's next_* buffers: not past this call's return
        const std::string why = mmf_last_error();
        (void)fusion_stage_host_next(f);
        return fail(rc, why);
    }
    return fusion_stage_host_next(f);  // (paths that enqueue no prefetch never reached the staging point)
}

extern "C" int mmf_fusion_process_frame_host(mmf_fusion* f, const uint8_t* rgb_host, const float* depth_host,
                                             const uint8_t* mask_host, int has_new_label, long long timestamp,
                                             const float* in_pose, float weight_multiplier, int bootstrap) {
    return mmf_fusion_process_frame_host_next(f, rgb_host, depth_host, mask_host, has_new_label, timestamp, in_pose,
                                              weight_multiplier, bootstrap, nullptr, nullptr);
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
        if (k > 0) {
            MMF_HIP_TRY(hipEventRecord(fm->ev_done, fm->lane->stream));
            MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, fm->ev_done, 0));
        }
    }
    return MMF_OK;
}

// The filter and the input-side preparation (vertex / normal maps, depth and intensity pyramids, gradients) of the
// NEXT frame, enqueued on a second stream so that they run while the current frame is still being fused.
// rgb / depth must stay unchanged until the mmf_fusion_process_frame call that consumes them (same pointers).
// `tick_at_use`: the tick of the processFrame call these buffers are for
static int fusion_prefetch_init(mmf_fusion* f) {
    if (f->side != nullptr) return MMF_OK;
    MMF_HIP_TRY(hipStreamCreateWithFlags(&f->side, hipStreamNonBlocking));
    MMF_HIP_TRY(hipStreamCreateWithFlags(&f->side2, hipStreamNonBlocking));
    MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_prefetch_done, hipEventDisableTiming));
    MMF_HIP_TRY(hipEventCreateWithFlags(&f->ev_prefetch2_done, hipEventDisableTiming));
    MMF_HIP_TRY(hipMalloc(&f->side_partials, sizeof(float) * kMaxGrid * kPartialStride));
    MMF_HIP_TRY(hipMalloc(&f->side_ticket, sizeof(unsigned) * kTicketWords));
    MMF_HIP_TRY(hipMemsetAsync(f->side_ticket, 0, sizeof(unsigned) * kTicketWords, f->side2));
    MMF_HIP_TRY(hipMalloc(&f->so3_stage[0], 2 * sizeof(OdomState)));
    f->so3_stage[1] = f->so3_stage[0] + 1;
    MMF_HIP_TRY(hipMemsetAsync(f->so3_stage[0], 0, 2 * sizeof(OdomState), f->side2));
    return MMF_OK;
}

// The image side of the frame the call with tick `tick_at_use` will be given: intensity pyramid + gradients into the
// free halves of their double buffers, then the SO3 pre-alignment (this frame's against the last frame's level-2 image:
// no model, no pose) in the staging state of that tick's parity.  Second side stream; needs the streams to exist.
// ahead: enqueued at the start of a frame whose own image side was prepared on this same stream (nothing to wait for);
// else behind ev_inputs_free where a frame recorded it (the first frame's intensity pyramid and an untracked frame's
// preparation are written on the fusion's stream; after a tracked frame the host has the poses: everything is done)
static int fusion_prefetch_image(mmf_fusion* f, const uint8_t* rgb, int tick_at_use, bool ahead) {
    const mmf_fusion_config& g = f->cfg;
    mmf_odom* odom = f->models[0]->odom;
    hipStream_t img_stream = f->side2;
    if (!ahead && f->inputs_free_recorded) MMF_HIP_TRY(hipStreamWaitEvent(img_stream, f->ev_inputs_free, 0));
    Enqueuer qi(img_stream);
    PrepSensorFrame sf;
    sf.rgb = rgb, sf.channels = 3;
    int rc = odom_prepare_sensor(odom, sf, PREP_INPUT_IMAGE, &qi);
    if (rc) return rc;
    f->so3_stage_ready = -1;
    if (g.so3 && tick_at_use > 1) {  // a model exists: the frame will be tracked, SO3 first
        const int s = tick_at_use & 1;
        rc = odom_prefetch_so3(odom, qi, f->side_partials, f->side_ticket, f->so3_stage[s]);
        if (rc) return rc;
        f->so3_stage_ready = s;
    }
    MMF_HIP_TRY(qi.flush());
    MMF_HIP_TRY(hipEventRecord(f->ev_prefetch2_done, img_stream));
    f->image_pre_rgb = rgb;
    return MMF_OK;
}

static int fusion_prefetch_impl(mmf_fusion* f, const uint8_t* rgb, const float* depth, int tick_at_use) {
    mmf_ctx* c = f->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_odom* odom = f->models[0]->odom;
    if (int rc0 = fusion_prefetch_init(f)) return rc0;
    f->pre_valid = false;  // an earlier prefetch is simply overwritten: same streams, same order
    if (f->host_next.slot >= 0 && f->up_dev[0] && rgb == f->up_dev[f->host_next.slot] + (size_t)f->width * f->height * 4) {
        // the hinted frame comes from host memory (mmf_fusion_process_frame_host_next): behind its upload
        if (int rc0 = fusion_stage_host_next(f)) return rc0;
        if (hipEventQuery(f->ev_up[f->host_next.slot]) != hipSuccess) {  // (as a rule it arrived long ago: no barrier packets)
            (void)hipGetLastError();
            MMF_HIP_TRY(hipStreamWaitEvent(f->side, f->ev_up[f->host_next.slot], 0));
            MMF_HIP_TRY(hipStreamWaitEvent(f->side2, f->ev_up[f->host_next.slot], 0));
        }
    }
    if (f->inputs_free_recorded) MMF_HIP_TRY(hipStreamWaitEvent(f->side, f->ev_inputs_free, 0));
    const mmf_fusion_config& g = f->cfg;
    // depth chain (first side stream): filter, depth pyramid, vertex and normal maps -- what the chains' ICP term reads,
    // hence behind ev_inputs_free.  Enqueued before the image chain when that is still to come: it is five launches that
    // start with the 40 us filter, the image chain fifteen short ones.
    float* target = f->filtered[1 - f->cur];
    Enqueuer qd(f->side);
    int rc = filter_depth_on(c, qd, depth, f->width, f->height, g.depth_cutoff, target);
    if (rc) return rc;
    PrepSensorFrame sf;
    sf.depth_filtered = target, sf.depth_cutoff = g.max_depth_processed;
    rc = odom_prepare_sensor(odom, sf, PREP_INPUT_DEPTH, &qd);
    if (rc) return rc;
    MMF_HIP_TRY(qd.flush());
    if (f->image_pre_rgb != rgb) {  // (else: enqueued at the start of the frame)
        rc = fusion_prefetch_image(f, rgb, tick_at_use, false);
        if (rc) return rc;
    }
    // ONE event for the consumer: the first side stream takes in the second's (one wait less on the model's stream)
    MMF_HIP_TRY(hipStreamWaitEvent(f->side, f->ev_prefetch2_done, 0));
    MMF_HIP_TRY(hipEventRecord(f->ev_prefetch_done, f->side));
    f->pre_valid = true, f->pre_rgb = rgb, f->pre_depth = depth;
    return MMF_OK;
}

extern "C" int mmf_fusion_prefetch_frame(mmf_fusion* f, const uint8_t* rgb, const float* depth) {
    MMF_REQUIRE(f && rgb && depth, "mmf_fusion_prefetch_frame: null argument");
    return fusion_prefetch_impl(f, rgb, depth, f->tick);
}

extern "C" int mmf_fusion_get_pose(mmf_fusion* f, float pose[16]) {
    MMF_REQUIRE(f && pose, "mmf_fusion_get_pose: null argument");
    return mmf_model_get_pose(f->models[0]->model, pose);
}

static int model_reset_store(mmf_model* m) {
    if (int rc = model_resolve_count(m)) return rc;  // lets an in-flight count land before it is dropped
    m->count = 0, m->count_pending = false, m->count_bound = 0;
    if (m->slab) MMF_HIP_TRY(hipMemsetAsync(m->totals, 0, 16, m->ctx->stream));  // (no slab: another rank's model)
    identity16(m->pose);
    m->max_depth = FLT_MAX;
    return MMF_OK;
}

// start a new map: empty surfel stores, identity poses, tick = 1, only the global model active (what
// constructing a fresh MultiMotionFusion does, MultiMotionFusion.cpp:21-97); object models return to the
// preallocated pool
extern "C" int mmf_fusion_reset(mmf_fusion* f) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_reset: null fusion object");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->pre_valid) {  // a prefetched frame belongs to the sequence that ends here
        MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, f->ev_prefetch_done, 0));
        MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, f->ev_prefetch2_done, 0));
        f->pre_valid = false;
    }
    for (auto* list : {&f->models, &f->inactive})
        for (size_t k = (list == &f->models ? 1 : 0); k < list->size(); ++k) f->preallocated.push_back((*list)[k]);
    f->models.resize(1);
    f->inactive.clear();
    f->scheduled_deactivation.clear();
    if (f->views)  // the stored views belonged to the models of the map that ends here
        for (RdView& v : f->views->views) v.model = -1;
    f->kp_next = false;
    f->redetections.clear();
    f->trk_ids.clear(), f->trk_T.clear();
    f->view_poses.clear(), f->stored_ids.clear(), f->stored_views.clear(), f->stored_rows.clear();
    std::memset(f->mask_map, 0, sizeof(f->mask_map));  // (the table speaks of the models of the map that ends here)
    f->mask_valid = false;
    std::vector<FusionModel*> all(f->preallocated);
    all.push_back(f->models[0]);
    for (FusionModel* fm : all) {
        int rc = model_reset_store(fm->model);
        if (rc) return rc;
        fm->model->conf_threshold = fm->model->id == 0 ? f->cfg.conf_global_init : f->cfg.conf_object_init;
        identity16(fm->last_pose);
        fm->odom->so3_prefetched = false, fm->odom->so3_stage = nullptr;
        fm->odom->have_tmp = false;
        fm->unseen = 0;
        fm->pose_log.clear();
    }
    for (FusionModel* fm : all) fm->spec_valid = false;
    f->so3_stage_ready = -1, f->image_pre_rgb = nullptr;
    if (f->flow) {  // the next frame is the first of a sequence: it yields no flow
        (void)mmf_flow_reset(f->flow);
        f->flow_has = f->fi_has = false;
    }
    f->tick = 1;
    return MMF_OK;
}

// MultiMotionFusion::exportPoses (:1020-1045): one file per pose-logging model, `poses-<id>.txt` in export_dir,
// lines `ts x y z qx qy qz qw` (operator<< formatting: 6 significant digits)
extern "C" int mmf_fusion_export_poses(mmf_fusion* f, const char* export_dir) {
    MMF_REQUIRE(f && export_dir, "mmf_fusion_export_poses: null argument");
    for (auto* list : {&f->models, &f->inactive})
        for (FusionModel* fm : *list) {
            if (fm->pose_log.capacity() == 0) continue;
            const std::string name = std::string(export_dir) + "poses-" + std::to_string((int)fm->model->id) + ".txt";
            FILE* fp = std::fopen(name.c_str(), "w");
            if (!fp) return fail(MMF_ERR_INVALID, "mmf_fusion_export_poses: cannot open " + name);
            for (const PoseLogItem& it : fm->pose_log) {
                std::fprintf(fp, "%lld", it.ts);
                for (int i = 0; i < 7; ++i) std::fprintf(fp, " %g", (double)it.p[i]);
                std::fprintf(fp, "\n");
            }
            std::fclose(fp);
        }
    return MMF_OK;
}

// the pose log of one active model (Model::getPoseLog): n entries of {ts, x y z qx qy qz qw}
extern "C" int mmf_fusion_pose_log(mmf_fusion* f, int index, long long* ts, float* p7, int max_entries, int* n_out) {
    MMF_REQUIRE(f && n_out && index >= 0 && index < (int)f->models.size(), "mmf_fusion_pose_log: bad argument");
    const std::vector<PoseLogItem>& log = f->models[index]->pose_log;
    *n_out = (int)log.size();
    for (int i = 0; i < (int)log.size() && i < max_entries; ++i) {
        if (ts) ts[i] = log[i].ts;
        if (p7) std::memcpy(p7 + 7 * i, log[i].p, sizeof(float) * 7);
    }
    return MMF_OK;
}
