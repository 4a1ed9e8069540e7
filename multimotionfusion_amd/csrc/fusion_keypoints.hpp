// fusion_keypoints.hpp -- the keypoint side of processFrame: the attached tracker and the in-frame front end, the models'
// view log and stored views, and the redetection of inactive models (frame_redetect).  Textually included by mmf_hip.hip
// behind fusion_hooks.hpp.
#pragma once

// ---- keypoint tracks (MultiMotionFusion.cpp:312-335, 425-436, 584-604, 622-627; tracker_host.hpp) ------------------------------
extern "C" int mmf_fusion_set_tracker(mmf_fusion* f, mmf_tracker* tracker, int odom_init_kp, int icp_refine) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_tracker: null fusion object");
    if (tracker && f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_tracker: sharded use is not supported (world > 1)");
    MMF_REQUIRE(!tracker || (tracker->ctx == f->ctx && tracker->width == f->width && tracker->height == f->height),
                "mmf_fusion_set_tracker: the tracker must share the fusion's context and image size");
    f->kp.tracker = tracker;
    f->kp.frontend = nullptr;  // (the in-frame front end belongs to the tracker that leaves)
    f->kp.init_kp = tracker && odom_init_kp != 0, f->kp.icp_refine = icp_refine != 0;
    f->kp.ids.clear(), f->kp.T.clear();
    f->kp.view_poses.clear();  // (the entries carry the stamps of the tracker that leaves)
    if (tracker && f->kp.backdate_history) return mmf_tracker_reserve_backdate(tracker, f->kp.backdate_history);  // (here, not in a frame)
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
        f->kp.frontend = nullptr;
        return MMF_OK;
    }
    MMF_REQUIRE(cfg != nullptr, "mmf_fusion_set_keypoint_frontend: null configuration");
    if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_keypoint_frontend: sharded use is not supported (world > 1)");
    if (!f->kp.tracker) return fail(MMF_ERR_STATE, "mmf_fusion_set_keypoint_frontend: no tracker is attached (mmf_fusion_set_tracker)");
    MMF_REQUIRE(sp->ctx == f->ctx, "mmf_fusion_set_keypoint_frontend: the network must share the fusion's context");
    MMF_REQUIRE(f->width <= sp->max_w && f->height <= sp->max_h && f->width % 8 == 0 && f->height % 8 == 0,
                "mmf_fusion_set_keypoint_frontend: the frame is larger than the network was created for (or its sides are no multiples of 8)");
    MMF_REQUIRE(sp->max_kp <= f->kp.tracker->max_keypoints, "mmf_fusion_set_keypoint_frontend: the network returns more keypoints than the tracker takes");
    MMF_REQUIRE(cfg->nms_dist >= 0 && cfg->border >= 0 && cfg->history >= 0, "mmf_fusion_set_keypoint_frontend: negative radius or history");
    f->kp.frontend = sp, f->kp.frontend_cfg = *cfg;
    f->kp.caller_adds = f->kp.tracker->caller_adds;
    return MMF_OK;
}

// the frame's keypoints, first thing in the call: features, add, prune on the frame's own device buffers -- all of it
// enqueued, none of it awaited (the frame's first wait stays the pairs call of frame_track_transforms)
static int frame_keypoints(mmf_fusion* f, const mmf_frame* fr) {
    mmf_tracker* t = f->kp.tracker;
    if (!t) return fail(MMF_ERR_STATE, "mmf_fusion_process_frame: the keypoint front end is on but no tracker is attached");
    if (t->caller_adds != f->kp.caller_adds) {
        f->kp.caller_adds = t->caller_adds;
        return fail(MMF_ERR_INVALID, "mmf_fusion_process_frame: the keypoint front end is on (mmf_fusion_set_keypoint_frontend): "
                                     "the caller must not add keypoints to the tracker itself");
    }
    const mmf_keypoint_frontend_config& k = f->kp.frontend_cfg;
    mmf_superpoint* sp = f->kp.frontend;
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
    *n_out = (int)f->kp.stored_ids.size();
    for (int i = 0; i < *n_out && i < capacity; ++i) {
        if (model_ids) model_ids[i] = f->kp.stored_ids[(size_t)i];
        if (n_views) n_views[i] = f->kp.stored_views[(size_t)i];
        if (rows) rows[i] = f->kp.stored_rows[(size_t)i];
    }
    return MMF_OK;
}
extern "C" int mmf_fusion_last_track_transforms(mmf_fusion* f, float* T, int capacity, int* n_out) {
    MMF_REQUIRE(f && n_out && capacity >= 0 && (T || capacity == 0), "mmf_fusion_last_track_transforms: bad argument");
    *n_out = (int)(f->kp.T.size() / 16);
    for (int i = 0; i < *n_out && i < capacity; ++i) std::memcpy(T + 16 * i, f->kp.T.data() + 16 * (size_t)i, 16 * sizeof(float));
    return MMF_OK;
}

// model->getLastTrackTransform() of every active model (:322), list order: one pairs launch, one wait, RANSAC on the host
static int frame_track_transforms(mmf_fusion* f) {
    std::vector<int> ids;
    for (FusionModel* fm : f->models) ids.push_back((int)fm->model->id);
    const float *p0 = nullptr, *p1 = nullptr;
    const int* counts = nullptr;
    int stride = 0;
    int rc = mmf_tracker_last_pairs(f->kp.tracker, ids.data(), (int)ids.size(), &p0, &p1, &counts, &stride);
    if (rc) return rc;
    f->kp.T.resize(16 * ids.size());
    for (size_t k = 0; k < ids.size(); ++k) {
        const mmf::RigidRANSAC::Result res = tracker_transform(p0 + k * (size_t)stride * 3, p1 + k * (size_t)stride * 3, counts[k], kTrackRansac);
        isometry_to_4x4(res.transformation, f->kp.T.data() + 16 * k);
    }
    return MMF_OK;
}

// the models' track sets after the frame's segmentation, spawn and redetection (:584-604; one model: :622-627; the first
// frame: initGlobalTracks); a model that left the active list since the last association is forgotten
static int frame_associate_tracks(mmf_fusion* f, bool all, bool by_mask) {
    std::vector<int> ids;
    for (FusionModel* fm : f->models) ids.push_back((int)fm->model->id);
    for (int old : f->kp.ids)
        if (std::find(ids.begin(), ids.end(), old) == ids.end()) {
            int rc = mmf_tracker_forget_model(f->kp.tracker, old);
            if (rc) return rc;
        }
    f->kp.ids = ids;
    if (all) return mmf_tracker_associate_all(f->kp.tracker, ids.data(), (int)ids.size());
    if (by_mask) return mmf_tracker_associate(f->kp.tracker, f->mask.get(), ids.data(), (int)ids.size());
    return MMF_OK;  // (a frame with a dictated pose has no segmentation)
}

static bool fusion_view_log_on(const mmf_fusion* f) { return f->rd.on && f->rd.views && f->kp.tracker && f->kp.tracker->log.frames > 0; }

// Model::appendPoses: one (stamp, pose) entry per object model and tracked frame.  after_tracking: every active object model
// gets this frame's entry; otherwise (the end of the frame) only the models that have none yet -- the one spawned in it.
// Stamps that do not ascend mean the tracker was reset: the list restarts.
static void fusion_note_view_poses(mmf_fusion* f, bool after_tracking) {
    if (!fusion_view_log_on(f)) return;
    const int stamp = (int)f->kp.tracker->frame;
    for (size_t k = 1; k < f->models.size(); ++k) {
        std::vector<Keypoints::ViewPose>& list = f->kp.view_poses[(int)f->models[k]->model->id];
        if (!list.empty() && list.back().stamp > stamp) list.clear();
        if (!list.empty() && list.back().stamp == stamp) {
            if (after_tracking) mmf_model_get_pose(f->models[k]->model, list.back().pose);
            continue;
        }
        Keypoints::ViewPose e;
        e.stamp = stamp;
        mmf_model_get_pose(f->models[k]->model, e.pose);
        list.push_back(e);
        if ((int)list.size() > f->kp.tracker->log.frames) list.erase(list.begin(), list.end() - f->kp.tracker->log.frames);
    }
}

// Model::store (Model.cpp:1617-1644) without the files: the model's views from the tracker's log (mmf_tracker_model_views),
// its pose entries paired with the log's frames BY STAMP, into the view store without passing through the host
// (mmf_viewstore_store_device).  One host wait in each.  A model that has stored views stores nothing (:1618-1621).
static int fusion_store_views(mmf_fusion* f, FusionModel* fm) {
    const int id = (int)fm->model->id;
    if (!fusion_view_log_on(f) || id <= 0 || id >= mmf::kTrkMaxModels || viewstore_has_model(f->rd.views, id)) return MMF_OK;
    std::vector<int> frames;
    std::vector<float> poses;
    auto it = f->kp.view_poses.find(id);
    if (it != f->kp.view_poses.end())
        for (const Keypoints::ViewPose& e : it->second) {
            frames.push_back(e.stamp);
            poses.insert(poses.end(), e.pose, e.pose + 16);
        }
    const int n = (int)frames.size();
    if (n == 0) return MMF_OK;  // (no tracked frame since the log is kept: nothing is known of the model)
    const int* counts = nullptr;
    const float *desc = nullptr, *coord = nullptr;
    int rc = mmf_tracker_model_views(f->kp.tracker, id, n, frames.data(), poses.data(), &counts, &desc, &coord, nullptr);
    if (rc) return rc;
    int stored = 0;
    rc = mmf_viewstore_store_device(f->rd.views, id, n, counts, desc, coord, &stored);
    if (rc) return rc;
    if (stored) {
        int rows = 0;
        for (int v = 0; v < n; ++v) rows += counts[v];
        f->kp.stored_ids.push_back(id), f->kp.stored_views.push_back(n), f->kp.stored_rows.push_back(rows);
    }
    f->kp.view_poses.erase(id);
    return MMF_OK;
}

// ---- back-dating a spawned model's poses (MultiMotionFusion.cpp:596-599; Model::refineTrackSubset, Model.cpp:649-737) ---------
extern "C" int mmf_fusion_set_track_backdating(mmf_fusion* f, int history) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_track_backdating: null fusion object");
    MMF_REQUIRE(history == 0 || (history >= 2 && history <= mmf::kTrkBackdateMax), "mmf_fusion_set_track_backdating: history is 0 (off) or 2 .. 256");
    if (history && f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_track_backdating: sharded use is not supported (world > 1)");
    if (history == 0) {
        mmf_ransac_batch_destroy(f->kp.backdate_batch);  // (waits for the stream)
        f->kp.backdate_batch = nullptr, f->kp.backdate_history = 0;
        f->kp.backdated.clear(), f->kp.backdated_id = -1;
        return MMF_OK;
    }
    if (!f->kp.backdate_batch) {
        const mmf_ransac_config cfg{kTrackRansac.iterations, kTrackRansac.inlier_threshold, kTrackRansac.inlier_fraction};  // (:665)
        int rc = mmf_ransac_batch_create(f->ctx, &cfg, mmf::kRansacMaxPoints, &f->kp.backdate_batch);
        if (rc) return rc;
    }
    if (f->kp.tracker) {  // (a tracker attached later gets its workspace in mmf_fusion_set_tracker)
        int rc = mmf_tracker_reserve_backdate(f->kp.tracker, history);
        if (rc) return rc;
    }
    f->kp.backdate_history = history;
    return MMF_OK;
}

extern "C" int mmf_fusion_last_backdated_poses(mmf_fusion* f, int* model_id, mmf_backdated_pose* out, int capacity, int* n_out) {
    MMF_REQUIRE(f && n_out && capacity >= 0 && (out || capacity == 0), "mmf_fusion_last_backdated_poses: bad argument");
    if (model_id) *model_id = f->kp.backdated_id;
    *n_out = (int)f->kp.backdated.size();
    for (int i = 0; i < *n_out && i < capacity; ++i) out[i] = f->kp.backdated[(size_t)i];
    return MMF_OK;
}

// directly behind the frame's association: the tracks that carry the spawned model's label say how it moved before it was
// segmented.  With the models' view-pose lists kept, entries 0 .. len - 2 go in front of the spawn frame's own entry
// (fusion_note_view_poses made it), so that fusion_store_views builds the earlier views too; the model's pose stays as it is.
static int frame_backdate(mmf_fusion* f) {
    mmf_tracker* t = f->kp.tracker;
    const int id = f->kp.spawned_id, history = f->kp.backdate_history;
    if (history < 2 || !f->kp.backdate_batch || !t || t->log.frames <= 0 || id <= 0 || id >= mmf::kTrkMaxModels) return MMF_OK;
    f->kp.backdated.resize((size_t)history);
    int n = 0;
    int rc = mmf_tracker_backdate(t, id, history, f->kp.backdate_batch, f->kp.backdated.data(), history, &n);
    if (rc) {
        f->kp.backdated.clear();
        return rc;
    }
    f->kp.backdated.resize((size_t)n), f->kp.backdated_id = id;
    if (!fusion_view_log_on(f)) return MMF_OK;
    std::vector<Keypoints::ViewPose>& list = f->kp.view_poses[id];
    if (list.size() != 1 || list.back().stamp != (int)t->frame) return MMF_OK;  // (only the spawn frame's own entry is expected)
    std::vector<Keypoints::ViewPose> front;
    for (int j = 0; j + 1 < n; ++j) {
        Keypoints::ViewPose e;
        e.stamp = f->kp.backdated[(size_t)j].stamp;
        std::memcpy(e.pose, f->kp.backdated[(size_t)j].pose, sizeof(e.pose));
        front.push_back(e);
    }
    list.insert(list.begin(), front.begin(), front.end());
    if ((int)list.size() > t->log.frames) list.erase(list.begin(), list.end() - t->log.frames);
    return MMF_OK;
}

// ---- keypoint redetection (MultiMotionFusion.cpp:425-436, 489-559) ----------------------------------------------------------
static int fusion_viewstore(mmf_fusion* f) {
    if (f->rd.views) return MMF_OK;
    return mmf_viewstore_create(f->ctx, &f->rd.views);
}
extern "C" mmf_viewstore* mmf_fusion_viewstore(mmf_fusion* f) {
    if (!f || fusion_viewstore(f) != MMF_OK) return nullptr;
    return f->rd.views;
}
// setEnableRedetection (MultiMotionFusion.h:414 defaults to true; here OFF by default: every call behaves as before)
extern "C" int mmf_fusion_set_redetection(mmf_fusion* f, int on) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_set_redetection: null fusion object");
    if (on && f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_set_redetection: sharded redetection is not supported (world > 1)");
    if (on) {
        int rc = fusion_viewstore(f);
        if (rc) return rc;
    }
    f->rd.on = on != 0;
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
    if (mode == f->rd.verifier_mode) return MMF_OK;
    int rc = fusion_viewstore(f);
    if (rc) return rc;
    if (mode) {
        const mmf_ransac_config cfg{kRedetectRansac.iterations, kRedetectRansac.inlier_threshold, kRedetectRansac.inlier_fraction};
        rc = mmf_ransac_batch_create(f->ctx, &cfg, g_redetect_max_points.load(), &f->rd.verifier);
        if (rc) return rc;
        rc = mmf_viewstore_set_verifier(f->rd.views, f->rd.verifier);
        if (rc) return rc;
    } else {
        rc = mmf_viewstore_set_verifier(f->rd.views, nullptr);
        if (rc) return rc;
        mmf_ransac_batch_destroy(f->rd.verifier);  // (waits for the stream)
        f->rd.verifier = nullptr;
    }
    f->rd.verifier_mode = mode;
    return MMF_OK;
}
extern "C" int mmf_fusion_redetection_host_verified(mmf_fusion* f) { return f ? f->rd.host_verified : -1; }

// the last keypoint of every currently visible track (track->back(), :428-436) for the NEXT processFrame only: HOST arrays
// xy [n][2] integer pixels, coordinate [n][3] camera frame (non-finite allowed), descriptor [n][256].  Copied.
extern "C" int mmf_fusion_set_keypoints(mmf_fusion* f, int n, const int* xy, const float* coordinate, const float* descriptor) {
    MMF_REQUIRE(f && n >= 0 && ((xy && coordinate && descriptor) || n == 0), "mmf_fusion_set_keypoints: bad argument");
    f->rd.kp_xy.assign(xy, xy + 2 * (size_t)n);
    f->rd.kp_coord.assign(coordinate, coordinate + 3 * (size_t)n);
    f->rd.kp_desc.assign(descriptor, descriptor + (size_t)kRdDim * (size_t)n);
    f->rd.kp_next = true;
    return MMF_OK;
}
extern "C" int mmf_fusion_last_redetections(mmf_fusion* f, mmf_redetection* out, int capacity, int* n_out) {
    MMF_REQUIRE(f && n_out && capacity >= 0 && (out || capacity == 0), "mmf_fusion_last_redetections: bad argument");
    *n_out = (int)f->rd.last.size();
    for (int i = 0; i < *n_out && i < capacity; ++i) out[i] = f->rd.last[(size_t)i];
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
    if (f->rd.views) mmf_viewstore_forget(f->rd.views, (int)fm->model->id);
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
    fm->odom->so3.prefetched = false, fm->odom->so3.stage = nullptr;
    f->inactive.erase(std::find(f->inactive.begin(), f->inactive.end(), fm));
    f->models.push_back(fm);
    if (fusion_view_log_on(f)) {  // Model::activate (:1646-1656): one pose, the activation's
        Keypoints::ViewPose e;
        e.stamp = (int)f->kp.tracker->frame;
        std::memcpy(e.pose, pose, sizeof(e.pose));
        f->kp.view_poses[(int)fm->model->id].assign(1, e);
    }
    if (fm->lane->stream != f->ctx->stream) {
        int rc = lane_wait(fm, f->ev_frame_ready.get());
        if (rc) return rc;
    }
    if (fm->restored_dense) {
        // surfels restored from a cloud.ply carry the tick of the load: into this frame's prediction window, once, in one
        // launch on the model's stream ahead of every pass of the frame (its count is exact: no pass has run on it)
        fm->restored_dense = false;
        return model_enqueue_timestamps(fm->model, (float)f->tick, fm->lane->stream);
    }
    return MMF_OK;
}

// :425-436 + :489-559.  Waits on the host twice: for the keypoints' labels, then for the matches of all segments.
// *has_new: segmentationResult.hasNewLabel, cancelled by an accepted match (:522-524).
static int frame_redetect(mmf_fusion* f, bool* has_new) {
    const bool have_kp = f->rd.kp_next;
    f->rd.kp_next = false;  // (for this frame only)
    if (!f->rd.on || !(have_kp || f->kp.tracker) || f->inactive.empty() || !f->rd.views || f->rd.views->books.views.empty()) return MMF_OK;
    if (!have_kp) {  // no mmf_fusion_set_keypoints for this frame: the attached tracker's visible set (:428-431)
        int nv = 0;
        int rc = tracker_visible_device(f->kp.tracker, &nv);
        if (rc) return rc;
        f->rd.kp_xy.resize(2 * (size_t)nv), f->rd.kp_coord.resize(3 * (size_t)nv), f->rd.kp_desc.resize((size_t)kRdDim * (size_t)nv);
        if (nv > 0) {
            MMF_HIP_TRY(hipMemcpy(f->rd.kp_xy.data(), f->kp.tracker->vis_xy, f->rd.kp_xy.size() * sizeof(int), hipMemcpyDeviceToHost));
            MMF_HIP_TRY(hipMemcpy(f->rd.kp_coord.data(), f->kp.tracker->vis_co, f->rd.kp_coord.size() * sizeof(float), hipMemcpyDeviceToHost));
            MMF_HIP_TRY(hipMemcpy(f->rd.kp_desc.data(), f->kp.tracker->vis_desc, f->rd.kp_desc.size() * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    mmf_ctx* c = f->ctx;
    mmf_viewstore* vs = f->rd.views;
    const size_t n = f->rd.kp_xy.size() / 2;
    if (n == 0) return MMF_OK;
    if (n > f->rd.kp_cap) {
        f->rd.kp_cap = 0;
        const size_t cap = n + n / 2 + 64;
        MMF_HIP_TRY(f->rd.xy_pin.create(cap * 2, hipHostMallocMapped | hipHostMallocCoherent));
        MMF_HIP_TRY(f->rd.label_pin.create(cap, hipHostMallocMapped | hipHostMallocCoherent));
        f->rd.kp_cap = cap;
    }
    std::memcpy(f->rd.xy_pin.get(), f->rd.kp_xy.data(), n * 2 * sizeof(int));
    hipLaunchKernelGGL(mmf::rd_gather_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)f->mask.get(),
                       f->width, f->height, (const int*)f->rd.xy_pin.get(), (int)n, f->rd.label_pin.get());
    MMF_HIP_TRY(hipGetLastError());
    MMF_HIP_TRY(wait_stream(c->stream));  // wait 1: the labels
    // per label other than 0 and 255 the keypoints with finite coordinates (:494-507), labels ascending
    std::vector<std::vector<int>> by_label(256);
    for (size_t i = 0; i < n; ++i) {
        const int l = f->rd.label_pin.get()[i];
        const float* p = f->rd.kp_coord.data() + 3 * i;
        if (l <= 0 || l >= 255) continue;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
        by_label[(size_t)l].push_back((int)i);
    }
    RdBatch batch;
    std::vector<int> set_label;
    size_t total_q = 0;
    for (int l = 1; l < 255; ++l) {
        if (by_label[(size_t)l].size() < 3) continue;  // min_tracks (:493, :507)
        batch.sets.push_back(RdSet{nullptr, (int)by_label[(size_t)l].size(), total_q});
        set_label.push_back(l);
        total_q += by_label[(size_t)l].size();
    }
    if (batch.sets.empty()) return MMF_OK;
    const bool on_device = f->rd.verifier_mode == 1 && vs->ver.verifier;  // the segments' coordinates travel with their descriptors
    // device verifier: behind the matches of all segments the two verification launches for ALL (segment, inactive model)
    // pairs of the frame, before the one wait (viewstore_batch_run, redetect_host.hpp)
    if (on_device)
        for (const FusionModel* im : f->inactive) batch.asked.push_back((int)im->model->id);
    int rc = viewstore_batch_run(vs, c->stream, &batch, on_device, [&](float* desc, float* coord) {
        for (size_t s = 0; s < batch.sets.size(); ++s) {
            const std::vector<int>& idx = by_label[(size_t)set_label[s]];
            for (size_t k = 0; k < idx.size(); ++k) {
                std::memcpy(desc + (batch.sets[s].q0 + k) * kRdDim, f->rd.kp_desc.data() + (size_t)idx[k] * kRdDim, kRdDim * sizeof(float));
                std::memcpy(coord + (batch.sets[s].q0 + k) * 3, f->rd.kp_coord.data() + (size_t)idx[k] * 3, 3 * sizeof(float));
            }
        }
    });  // wait 2: the matches of every segment against every view (and their verification)
    if (rc) return rc;
    for (size_t s = 0; s < batch.sets.size(); ++s) {
        const int label = set_label[s];
        if (viewstore_batch_too_large(vs, batch, s)) ++f->rd.host_verified;  // verified here, under the verifier's rule
        for (size_t mi = 0; mi < f->inactive.size();) {
            FusionModel* im = f->inactive[mi];
            // (with the device verifier the record of (segment, model): a model an earlier segment activated has left the list)
            const RdBest best = viewstore_batch_best(vs, batch, s, (int)im->model->id, false);
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
                f->rd.last.push_back(rd);
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
            f->rd.last.push_back(rd);
        }
    }
    return MMF_OK;
}
