// modeldb_host.hpp -- the model database on the fusion: MultiMotionFusion::savePly (Core/MultiMotionFusion.cpp:1001-1018) and
// loadModels (:131-145, `-restore`).  Textually included by mmf_hip.hip behind fusion_orchestrator.hpp.  Neither call is made by
// a frame; both are synchronous and leave nothing enqueued.
#pragma once

#include <filesystem>

static std::string modeldb_join(const std::string& dir, const std::string& name) {
    return (dir.empty() || dir.back() == '/') ? dir + name : dir + "/" + name;
}
static int modeldb_make_dirs(const std::string& dir) {
    std::error_code ec;
    std::filesystem::create_directories(dir, ec);
    if (ec && !std::filesystem::is_directory(dir)) return fail(MMF_ERR_INVALID, "mmf_fusion_save_models: cannot create " + dir + ": " + ec.message());
    return MMF_OK;
}

// the views of model `id` in the store, ascending, in the mmf_viewstore_store layout; false: the model has none
static int modeldb_model_views(mmf_viewstore* vs, int id, std::vector<int>* counts, std::vector<float>* desc, std::vector<float>* coord, bool* any) {
    counts->clear(), desc->clear(), coord->clear();
    *any = false;
    if (!vs) return MMF_OK;
    std::vector<int> which;
    size_t rows = 0;
    for (size_t v = 0; v < vs->books.views.size(); ++v)
        if (vs->books.views[v].model == id) which.push_back((int)v), rows += (size_t)vs->books.views[v].rows;
    if (which.empty()) return MMF_OK;
    *any = true;
    desc->resize(rows * kRdDim), coord->resize(rows * 3);
    size_t at = 0;
    for (int v : which) {
        const int n = vs->books.views[(size_t)v].rows;
        counts->push_back(n);
        if (int rc = mmf_viewstore_download_view(vs, v, n, desc->data() + at * kRdDim, coord->data() + at * 3)) return rc;
        at += (size_t)n;
    }
    return MMF_OK;
}

// savePly: every active model, then every inactive one (a model another rank owns has no store here and is left to its
// owner).  Per model P = global pose * pose^-1: `cloud-<id>.ply` under export_dir, `model_db/model-<id>/cloud.ply` with the
// same P and -- for a model with views in the fusion's store -- `model_db/model-<id>/tracks.ply` with P.  Observational.
extern "C" int mmf_fusion_save_models(mmf_fusion* f, const char* export_dir) {
    MMF_REQUIRE(f && export_dir, "mmf_fusion_save_models: null argument");
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    // the stores are written on the models' own streams and on those of batched passes: all of it has landed
    MMF_HIP_TRY(hipDeviceSynchronize());
    const std::string dir(export_dir), db = modeldb_join(dir, "model_db");
    if (int rc = modeldb_make_dirs(db)) return rc;
    float global_pose[16];
    mmf_model_get_pose(f->models[0]->model, global_pose);
    std::vector<int> counts;
    std::vector<float> desc, coord;
    for (auto* list : {&f->models, &f->inactive})
        for (FusionModel* fm : *list) {
            mmf_model* m = fm->model;
            if (model_is_bookkeeping(m)) continue;
            const std::string id = std::to_string((int)m->id), model_dir = modeldb_join(db, "model-" + id);
            float inv[16], P[16];
            inverse4f_host(m->pose, inv);
            mmf::host::matmul4(global_pose, inv, P);
            if (int rc = modeldb_make_dirs(model_dir)) return rc;
            if (int rc = mmf_model_export_ply(m, modeldb_join(dir, "cloud-" + id + ".ply").c_str(), P)) return rc;
            if (int rc = mmf_model_export_ply(m, modeldb_join(model_dir, "cloud.ply").c_str(), P)) return rc;
            bool any = false;
            if (int rc = modeldb_model_views(f->rd.views, (int)m->id, &counts, &desc, &coord, &any)) return rc;
            if (!any) continue;
            if (int rc = mmf_tracks_ply_write(modeldb_join(model_dir, "tracks.ply").c_str(), (int)counts.size(), counts.data(), desc.data(),
                                              coord.data(), P))
                return rc;
        }
    return MMF_OK;
}

// MMF_LOAD_DENSE for one loaded model: its cloud.ply into its store, the outcome into f->dense_restores; a file that cannot be
// used is named in *skipped and is no error
static int modeldb_restore_dense(mmf_fusion* f, FusionModel* fm, const std::string& path, std::string* skipped) {
    mmf_dense_restore r;
    r.model_id = (int)fm->model->id, r.surfels = 0, r.status = MMF_DENSE_RESTORED;
    std::error_code ec;
    if (!std::filesystem::exists(path, ec)) {
        r.status = MMF_DENSE_NO_FILE;
        *skipped = path + ": no such file";
    } else {
        unsigned n = 0;
        const int rc = model_import_ply(fm->model, path.c_str(), nullptr, fm->model->conf_threshold + 1.f, f->tick, &n);
        if (rc == MMF_ERR_INVALID) {
            r.status = n > (unsigned)fm->model->capacity ? MMF_DENSE_TOO_LARGE : MMF_DENSE_NO_PARSE;
            *skipped = path + ": " + g_last_error;
        } else if (rc != MMF_OK) {
            return rc;
        } else {
            r.surfels = n;
            fm->restored_dense = n > 0;
        }
    }
    f->dense_restores.push_back(r);
    return MMF_OK;
}

// loadModels: for id = 1 .. 255 ascending with a `model_db/model-<id>/tracks.ply`, an object model with the NEXT model id and
// conf_object_init, the file's views stored for that id, unseen count -5 (:141), at the end of the inactive list.  A file that
// does not parse is skipped: mmf_last_error names the last such file, the models before and behind it are loaded.
// flags 0: no dense surfels (as in the reference).  MMF_LOAD_DENSE (ours): the records of
// `model_db/model-<id>/cloud.ply` become the model's surfels under the identity (the file's frame is the frame of the
// restored views' coordinates), confidence = the model's threshold + 1 (strictly stable: drawn and exported again), both
// times = the tick now; the activating frame moves the timestamps into its window (redetect_activate).  A missing file,
// one that does not parse or one with more records than the model holds leaves the model without surfels -- it is loaded all
// the same, mmf_last_error names the file, mmf_fusion_last_dense_restores tells which it was.
extern "C" int mmf_fusion_load_models_ex(mmf_fusion* f, const char* export_dir, unsigned flags, int* n_loaded) {
    MMF_REQUIRE(f && export_dir, "mmf_fusion_load_models: null argument");
    if (n_loaded) *n_loaded = 0;
    MMF_REQUIRE((flags & ~(unsigned)MMF_LOAD_DENSE) == 0, "mmf_fusion_load_models: unknown flag");
    if (f->shard_world > 1) return fail(MMF_ERR_STATE, "mmf_fusion_load_models: not supported on a shard (world > 1)");
    f->dense_restores.clear();
    MMF_HIP_TRY(hipSetDevice(f->ctx->device));
    if (int rc = fusion_viewstore(f)) return rc;
    const std::string db = modeldb_join(export_dir, "model_db");
    std::string skipped;
    std::vector<int> counts;
    std::vector<float> desc, coord;
    for (int id = 1; id < 256; ++id) {
        const std::string model_dir = modeldb_join(db, "model-" + std::to_string(id)), path = modeldb_join(model_dir, "tracks.ply");
        std::error_code ec;
        if (!std::filesystem::exists(path, ec)) continue;
        int n_views = 0, n_rows = 0;
        int rc = mmf_tracks_ply_read(path.c_str(), 0, &n_views, nullptr, 0, &n_rows, nullptr, nullptr);
        if (rc == MMF_OK) {
            counts.assign((size_t)n_views, 0), desc.assign((size_t)n_rows * kRdDim, 0.f), coord.assign((size_t)n_rows * 3, 0.f);
            rc = mmf_tracks_ply_read(path.c_str(), n_views, &n_views, counts.data(), n_rows, &n_rows, desc.data(), coord.data());
        }
        if (rc != MMF_OK) {
            skipped = path + ": " + g_last_error;
            continue;
        }
        FusionModel* fm = nullptr;
        if (int rc_new = fusion_model_create(f, fusion_next_model_id(f, true), f->cfg.conf_object_init, 0, true, &fm)) return rc_new;
        int stored = 0;
        rc = mmf_viewstore_store(f->rd.views, (int)fm->model->id, n_views, counts.data(), desc.data(), coord.data(), &stored);
        if (rc != MMF_OK) {
            const std::string keep = g_last_error;
            fusion_model_destroy(fm);
            return fail(rc, keep);
        }
        fm->unseen = -5;
        f->inactive.push_back(fm);
        if (n_loaded) ++*n_loaded;
        if (flags & MMF_LOAD_DENSE)
            if (int rc_dense = modeldb_restore_dense(f, fm, modeldb_join(model_dir, "cloud.ply"), &skipped)) return rc_dense;
    }
    g_last_error = skipped.empty() ? std::string() : "mmf_fusion_load_models: skipped " + skipped;
    return MMF_OK;
}
extern "C" int mmf_fusion_load_models(mmf_fusion* f, const char* export_dir, int* n_loaded) {
    return mmf_fusion_load_models_ex(f, export_dir, 0, n_loaded);
}

// per model of the last load call with MMF_LOAD_DENSE, in load order: its id, the surfels it got, why it got none.
// *n is always the number of entries; at most `capacity` are written.  Observational
extern "C" int mmf_fusion_last_dense_restores(mmf_fusion* f, mmf_dense_restore* out, int capacity, int* n) {
    MMF_REQUIRE(f && n && (out || capacity <= 0), "mmf_fusion_last_dense_restores: null argument");
    *n = (int)f->dense_restores.size();
    for (int i = 0; i < *n && i < capacity; ++i) out[i] = f->dense_restores[(size_t)i];
    return MMF_OK;
}
