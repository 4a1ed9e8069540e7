// fusion_state.hpp -- the fusion object of fusion_orchestrator.hpp: the models of the reference's list (FusionModel), struct
// mmf_fusion with one member struct per concern, each owning what it creates (stream_lane.hpp), and what does not enqueue a
// frame: create / destroy / preallocate, accessors, runtime and shard setters, reset, pose export, pose log.  Textually
// included by mmf_hip.hip behind stream_lane.hpp.
#pragma once

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
    // its surfels came from a cloud.ply (mmf_fusion_load_models_ex, MMF_LOAD_DENSE) and it has not been active since: the
    // frame that activates it sets their timestamps to its tick (redetect_activate), once
    bool restored_dense = false;
    float* icp_error = nullptr;  // Model::icpError / rgbError (R32F, enableErrorRecording)
    float* rgb_error = nullptr;
    Event ev_done;
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

// ---- the members of mmf_fusion: one struct per concern, each releasing what it holds ----------------------------------------

// where a frame's segmentation comes from when the frame does not bring it: a callback, the built-in CRF
// (mmf_fusion_set_crf_segmentation) or the frame's raw label image (mmf_fusion_set_mask_segmentation)
struct Segmentation {
    mmf_segmentation_fn fn = nullptr;
    void* user = nullptr;
    bool crf_on = false;          // the built-in segmentation: off unless configured
    mmf_crf_config crf_cfg;       // (mmf_crf_default_config at creation: model_spawn_offset is read either way)
    unsigned spawn_offset = 0;    // MultiMotionFusion::spawnOffset (MultiMotionFusion.h:433)
    std::vector<mmf_segmentation_model> crf_models;
    bool mask_on = false;         // the segmentation from the frame's raw label image: off unless configured
    mmf_mask_config mask_cfg;
    uint8_t mask_map[256] = {0};  // Segmentation.cpp:92: input label -> model id, from frame to frame
    bool mask_valid = false;      // a frame went through this path (mmf_fusion_last_mask_segmentation)
    mmf_mask_info mask_info;
    std::vector<mmf_segmentation_model> mask_models;
};

// the super-pixel input (mmf_fusion_set_superpixels) and engine (mmf_fusion_set_superpixel_engine): the frame's label image
// from its RGB, on a lane of its own beside the tracking chains; lane and workspace exist once the engine has been on
struct SuperPixels {
    DeviceBuf<int> labels;      // mmf_fusion_set_superpixels: the next frame's label image (a copy)
    bool next = false;
    int engine = 0;
    SlicEngineWs ws;
    SideLane lane;              // begin: the frame's RGB is there, the last segmentation has read the labels
    const int* last = nullptr;  // the label image the last segmentation used (handed in, the engine's, or the grid)
    ~SuperPixels() {
        lane.stream.drain();  // (the engine's launches write the workspace)
        (void)hipFree(ws.mem);
    }
};

// the optical-flow hook (mmf_fusion_set_optical_flow; flow_host.hpp): every frame's dense flow from the frame before it, on a
// lane of its own beside the tracking chains; nothing exists while the hook is off
struct FlowHook {
    mmf_flow* engine = nullptr;  // owned
    SideLane lane;               // begin: the frame's RGB is on the device, the last flow's readers are done
    bool has = false;            // the last frame produced a flow (not the first frame, nor the first after a reset)
    void reset() {
        flow_destroy_on(engine, lane.stream.get());  // (once the context's stream and the lane have run dry)
        engine = nullptr, has = false;
        lane.reset();
    }
    ~FlowHook() { reset(); }
};

// the flow-CRF inference (mmf_fusion_set_flow_inference; flowcrf_host.hpp): on the flow's lane behind the flow, on every
// tracked frame that has one; observational.  Nothing exists while the hook is off
struct FlowInference {
    bool on = false;
    mmf_flowcrf_config cfg{};
    mmf_flowcrf* engine = nullptr;  // owned; created by the first frame that needs it, for its labels and the tracker's capacity
    hipStream_t stream = nullptr;   // the flow's lane, where the engine runs (not owned; set while the hook is on)
    Event begin;                    // fusion stream: the tracking is done, the track table and the predictions are as the frame met them
    Event inputs;                   // flow stream: the inference has read them
    bool has = false;               // the last frame produced an id image
    int allow_new = 0;              // ... with the new label as its last
    void reset() {
        if (on) {  // (once the flow's stream has run dry)
            flowcrf_destroy_on(engine, stream);
            (void)hipStreamSynchronize(stream);
        }
        begin.reset(), inputs.reset();
        engine = nullptr, stream = nullptr, on = has = false;
    }
    ~FlowInference() { reset(); }
};

// the flow_crf segmentation mode (mmf_fusion_set_flow_segmentation; flowseg_host.hpp): the blob stage on the fusion's stream
// behind the inference, for a frame that brings no segmentation of its own.  Nothing exists while the mode is off
struct FlowSegmentation {
    bool on = false;
    mmf_flowseg_config cfg{};
    mmf_flowseg* engine = nullptr;  // owned; created by the first frame that needs it, for its labels
    bool valid = false;             // a frame went through this path (mmf_fusion_last_flow_segmentation)
    bool has = false;               // ... and had an inference result
    mmf_flowseg_summary last{};
    std::vector<mmf_segmentation_model> models;
    void reset() {
        flowseg_destroy_on(engine, nullptr);
        engine = nullptr, on = valid = has = false;
        models.clear();
    }
    ~FlowSegmentation() { reset(); }
};

// the fern keyframe database (mmf_fusion_set_fern_database; ferns_host.hpp): behind the end-of-frame predict(), on a lane of
// its own; observational.  Nothing exists while the hook is off
struct FernHook {
    mmf_ferns* engine = nullptr;  // owned
    SideLane lane;                // begin: the camera model's fill-in images of this frame are complete
    bool has = false;             // a frame has run since the hook went on / the last reset
    void reset() {
        ferns_destroy_on(engine, lane.stream.get());  // (once the context's stream and the lane have run dry)
        engine = nullptr, has = false;
        lane.reset();
    }
    ~FernHook() { reset(); }
};

// keypoint redetection of inactive models (MultiMotionFusion.cpp:489-559; redetect_host.hpp): off unless switched on
struct Redetection {
    bool on = false;
    int verifier_mode = 0;                 // mmf_fusion_set_redetection_verifier: 0 = host, 1 = device
    mmf_ransac_batch* verifier = nullptr;  // owned; attached to `views` while the mode is 1
    int host_verified = 0;                 // segments too large for the verifier, verified on the host under its rule
    mmf_viewstore* views = nullptr;        // owned: the stored keypoint views of the inactive models (created on first use)
    bool kp_next = false;                  // mmf_fusion_set_keypoints: the NEXT frame's keypoints
    std::vector<int> kp_xy;
    std::vector<float> kp_coord, kp_desc;
    PinnedBuf<int> xy_pin, label_pin;      // host memory the gather kernel reads / writes
    size_t kp_cap = 0;
    std::vector<mmf_redetection> last;     // what the last frame's redetection did
    ~Redetection() {
        mmf_viewstore_destroy(views);
        mmf_ransac_batch_destroy(verifier);
    }
};

// keypoint tracks (tracker_host.hpp; mmf_fusion_set_tracker), the keypoint front end inside processFrame
// (mmf_fusion_set_keypoint_frontend) and the models' view-pose log: nothing here is owned
struct Keypoints {
    mmf_tracker* tracker = nullptr;  // off unless attached
    bool init_kp = false, icp_refine = true;
    std::vector<int> ids;                // the active models' ids at the last association
    std::vector<float> T;                // the transformations the last frame's models were initialised with, list order
    mmf_superpoint* frontend = nullptr;  // off unless set
    mmf_keypoint_frontend_config frontend_cfg{};
    long long caller_adds = 0;           // the tracker's caller_adds when the front end last looked
    // the models' keypoint views on deactivation (Model::store, Model.cpp:1617-1644): active only with redetection on and an
    // attached tracker that keeps a view log.  Per object model the list of (tracker stamp, pose after that frame's tracking)
    // -- Model::poses, host memory, trimmed to the log's length -- and what the last frame stored
    struct ViewPose {
        int stamp;
        float pose[16];
    };
    std::map<int, std::vector<ViewPose>> view_poses;
    std::vector<int> stored_ids, stored_views, stored_rows;
    // back-dating of a spawned model's poses from its tracks (mmf_fusion_set_track_backdating; Model::refineTrackSubset,
    // Model.cpp:649-737): off unless a history is set.  The batch object is the one thing here that is owned
    int backdate_history = 0;
    mmf_ransac_batch* backdate_batch = nullptr;  // created by the setter, never per frame
    int spawned_id = -1;                         // the model this call's segmentation spawned on this rank, -1: none
    int backdated_id = -1;                       // what this call back-dated (mmf_fusion_last_backdated_poses)
    std::vector<mmf_backdated_pose> backdated;
    ~Keypoints() { mmf_ransac_batch_destroy(backdate_batch); }
};

// next-frame prefetch (mmf_fusion_prefetch_frame): the filter and the input-side preparation of frame t+1 run on `side` and
// `side2` while frame t is fused on the context's stream.  The streams, their events and scratch are created by its first call
struct Prefetch {
    // two filtered-depth buffers: frame t's fuse / clean / fill-in read one while frame t+1's filter writes the other
    DeviceBuf<float> filtered[2];
    int cur = 0;
    // The next frame's SO3 pre-alignment runs in one of two states of its own (by the parity of the frame it is for): no
    // chain reads or writes them, so it can run while the current frame's chain is still at work; the chain's first launch
    // copies the result into every tracked model's state (BeginArgs::so3_stage).
    DeviceBuf<OdomState> so3_mem;  // both of them
    OdomState* so3_stage[2] = {nullptr, nullptr};
    int so3_ready = -1;                  // which of the two holds the pre-alignment of the upcoming frame; -1: none
    const uint8_t* image_rgb = nullptr;  // the image side of this frame (intensity pyramid, gradients, SO3) is enqueued already
    Stream side;                         // depth chain: filter, depth pyramid, vertex / normal maps
    Stream side2;                        // image chain: intensity pyramid, gradients, SO3 pre-alignment
    DeviceBuf<float> partials;           // reduction scratch of the SO3 launches on side2 (never the context's: the
    DeviceBuf<unsigned> ticket;          // main stream may be inside a reduction of its own at the same time)
    Event done2;                         // side2: the image chain has been enqueued up to here
    Event inputs_free;  // fusion stream: enqueued work no longer reads the odometry's input-side buffers nor filtered[1 - cur]
    Event done;         // side stream: the prefetch has been enqueued up to here
    bool inputs_free_recorded = false;
    bool valid = false;
    const uint8_t* rgb = nullptr;
    const float* depth = nullptr;
    ~Prefetch() { side.drain(), side2.drain(); }  // every side stream runs dry before a buffer that work on it reads is freed
};

// host FrameData hand-over (mmf_fusion_process_frame_host[_next]): pinned staging + device copies in a ring of three (the
// frame being processed, the next one being uploaded, one whose readers may still be running), uploads on a stream of their own
struct HostRing {
    static constexpr int kUp = 3;
    PinnedBuf<uint8_t> pin[kUp];
    DeviceBuf<uint8_t> dev[kUp];
    Event ev[kUp];      // upload stream: slot k is on the device
    Event ev_rgb[kUp];  // ... its colour image is (sent first: the image side needs only that)
    bool recorded[kUp] = {false, false, false};
    Stream stream;
    Event begin;  // fusion stream -> upload stream
    int cur = 0;
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
        bool rgb_staged = false;  // its colour image is on its way (ev_rgb[slot] recorded)
        bool staged = false;      // all of it is on its way to (or on) the device in `slot`
    } next;
    // The copy of an announced frame into its pinned slot (2.15 MB at 640x480: ~150 us of one core) and the enqueue of its
    // upload run on a thread of their own, started when the call that announces the frame begins: on the calling thread the
    // copy was longer than the wait for the pose it was meant to hide in (announced frames ran 7 % behind device frames).
    struct Stager {
        std::thread thread;
        std::mutex mu;
        std::condition_variable cv;
        bool stop = false, busy = false;
        bool rgb_done = false;    // the job's colour image has been copied and its upload enqueued
        bool after_begin = true;  // the upload waits for `begin`
        int slot = 0;
        const uint8_t* rgb = nullptr;
        const float* depth = nullptr;
        int rc = MMF_OK;
        std::string error;
        void join() {
            if (!thread.joinable()) return;
            {
                std::lock_guard<std::mutex> lock(mu);
                stop = true;
            }
            cv.notify_all();
            thread.join();
        }
    } stager;
    // the stager thread is joined before the upload ring, its events and its stream go; the stream runs dry before the buffers
    ~HostRing() {
        stager.join();
        stream.drain();
    }
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
    float* depth_filtered = nullptr;  // = pre.filtered[pre.cur]
    DeviceBuf<uint8_t> mask;          // textures[MASK]: all zeros unless enableMultipleModels
    bool mask_is_zero = false;
    int tick = 1;                     // MultiMotionFusion.cpp:36
    unsigned extent_seq = 0;          // number of the frame whose model-side preparation notes extents (extent.hpp): only ever grows
    DeviceBuf<unsigned long long> mask_boxes;  // pass_rect.hpp: the boxes of the ids of the frame's id image (device, 256 x 4 words)
    unsigned mask_gen = 0;
    int tracking_ok = 1;
    const uint8_t* frame_rgb = nullptr;  // this frame's inputs (device), kept for predict()
    const float* frame_depth = nullptr;
    Event ev_frame_ready;  // fusion stream: the frame's shared inputs are complete
    Segmentation seg;      // where the segmentation comes from: callback, built-in CRF, the frame's labels
    SuperPixels sp;        // the super-pixel input and engine
    FlowHook flow;         // the optical-flow hook
    FlowInference fi;      // the flow inference.  Behind `flow`: it is released before the flow engine and the flow's stream
    FlowSegmentation fseg; // the flow_crf mode: the blob stage behind the inference
    FernHook ferns;        // the fern keyframe database
    std::vector<mmf_dense_restore> dense_restores;  // modeldb_host.hpp: per model of the last load call
    Redetection rd;        // redetection: view store, verifier, keypoint hand-over
    Keypoints kp;          // tracker, keypoint front end, view-pose log
    Prefetch pre;          // the next frame's prefetch on the side streams
    HostRing up;           // the host-frame ring and its staging thread
};

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
    fm->ev_done.reset();
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
    } else {
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
        if (rc == MMF_OK && fm->ev_done.create() != hipSuccess) rc = fail(MMF_ERR_HIP, "mmf_fusion: hipEventCreate failed");
        // the prediction images (model slab) and the filtered depth (the fusion's buffer) are not written
        // between the init* calls of a frame and the end of its tracking
        if (rc == MMF_OK) fm->odom->in.alias_inputs = true;
    }
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
    mmf_crf_default_config(&f->seg.crf_cfg);
    mmf_mask_default_config(&f->seg.mask_cfg);
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
    // from here on every failure leaves through mmf_fusion_destroy
    auto device_side = [&]() -> int {
        MMF_HIP_TRY(f->pre.filtered[0].create(npix));
        MMF_HIP_TRY(f->pre.filtered[1].create(npix));
        f->depth_filtered = f->pre.filtered[0].get();
        // the side streams and events of the prefetch are created by its first call
        MMF_HIP_TRY(f->pre.inputs_free.create());
        MMF_HIP_TRY(f->ev_frame_ready.create());
        MMF_HIP_TRY(f->mask.create(npix));
        MMF_HIP_TRY(hipMemsetAsync(f->mask.get(), 0, npix, c->stream));
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

extern "C" void mmf_fusion_destroy(mmf_fusion* f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    f->pre.side.drain(), f->pre.side2.drain();
    f->up.stager.join();  // (the thread works on the fusion object)
    for (auto* list : {&f->models, &f->preallocated, &f->inactive})
        for (FusionModel* fm : *list) fusion_model_destroy(fm);
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
    if (world > 1 && f->rd.on) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: redetection is on (sharded redetection is not supported)");
    if (world > 1 && f->rd.verifier_mode) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: the redetection verifier is on (not supported on a shard)");
    if (world > 1 && f->flow.engine) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: the optical-flow hook is on (not supported on a shard)");
    if (world > 1 && f->ferns.engine) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: the fern database is on (not supported on a shard)");
    if (world > 1 && f->kp.backdate_history) return fail(MMF_ERR_STATE, "mmf_fusion_set_shard: track back-dating is on (not supported on a shard)");
    f->shard_rank = rank, f->shard_world = world;
    // models created ahead of their use (preallocateModels): the ones this rank will not own shrink to bookkeeping
    for (FusionModel*& fm : f->preallocated) {
        const int id = (int)fm->model->id;
        const bool is_light = model_is_bookkeeping(fm->model), want_light = world > 1 && id % world != rank;
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
    else if (s == "MASK") *dev_ptr = f->mask.get(), *bytes = npix;
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

// scheduleDeactivation (MultiMotionFusion.cpp: scheduled_model_deactivation, applied at the next frame :279-283)
extern "C" int mmf_fusion_schedule_deactivation(mmf_fusion* f, int id) {
    MMF_REQUIRE(f != nullptr && id > 0, "mmf_fusion_schedule_deactivation: bad argument (the global model stays)");
    f->scheduled_deactivation.push_back(id);
    return MMF_OK;
}

static int lane_wait(FusionModel* fm, hipEvent_t ev) {
    MMF_HIP_TRY(hipStreamWaitEvent(fm->lane->stream, ev, 0));
    return MMF_OK;
}

extern "C" int mmf_fusion_get_pose(mmf_fusion* f, float pose[16]) {
    MMF_REQUIRE(f && pose, "mmf_fusion_get_pose: null argument");
    return mmf_model_get_pose(f->models[0]->model, pose);
}

// start a new map: empty surfel stores, identity poses, tick = 1, only the global model active (what
// constructing a fresh MultiMotionFusion does, MultiMotionFusion.cpp:21-97); object models return to the
// preallocated pool
extern "C" int mmf_fusion_reset(mmf_fusion* f) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_reset: null fusion object");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->pre.valid) {  // a prefetched frame belongs to the sequence that ends here
        MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, f->pre.done.get(), 0));
        MMF_HIP_TRY(hipStreamWaitEvent(f->ctx->stream, f->pre.done2.get(), 0));
        f->pre.valid = false;
    }
    for (auto* list : {&f->models, &f->inactive})
        for (size_t k = (list == &f->models ? 1 : 0); k < list->size(); ++k) f->preallocated.push_back((*list)[k]);
    f->models.resize(1);
    f->inactive.clear();
    f->scheduled_deactivation.clear();
    if (f->rd.views)  // the stored views belonged to the models of the map that ends here
        for (RdView& v : f->rd.views->books.views) v.model = -1;
    f->rd.kp_next = false;
    f->rd.last.clear();
    f->kp.ids.clear(), f->kp.T.clear();
    f->kp.view_poses.clear(), f->kp.stored_ids.clear(), f->kp.stored_views.clear(), f->kp.stored_rows.clear();
    std::memset(f->seg.mask_map, 0, sizeof(f->seg.mask_map));  // (the table speaks of the models of the map that ends here)
    f->seg.mask_valid = false;
    f->fseg.valid = f->fseg.has = false;
    std::vector<FusionModel*> all(f->preallocated);
    all.push_back(f->models[0]);
    for (FusionModel* fm : all) {
        int rc = model_reset_store(fm->model);
        if (rc) return rc;
        fm->model->conf_threshold = fm->model->id == 0 ? f->cfg.conf_global_init : f->cfg.conf_object_init;
        identity16(fm->last_pose);
        fm->odom->so3.prefetched = false, fm->odom->so3.stage = nullptr;
        fm->odom->in.have_tmp = false;
        fm->unseen = 0;
        fm->restored_dense = false;  // (its store is empty now)
        fm->pose_log.clear();
    }
    for (FusionModel* fm : all) fm->spec_valid = false;
    f->pre.so3_ready = -1, f->pre.image_rgb = nullptr;
    if (f->flow.engine) {  // the next frame is the first of a sequence: it yields no flow
        (void)mmf_flow_reset(f->flow.engine);
        f->flow.has = f->fi.has = false;
    }
    if (f->ferns.engine) {  // the keyframes belonged to the map that ends here (every frame's lane has been joined by this stream)
        int rc = ferns_reset_on(f->ferns.engine, f->ctx->stream);
        if (rc) return rc;
        f->ferns.has = false;
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
