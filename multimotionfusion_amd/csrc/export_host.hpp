// export_host.hpp -- a model's stable surfels as PLY records (export_kernels.hpp) and the C ABI of the model database's files
// (modeldb_io.hpp).  Textually included by mmf_hip.hip behind model_host.hpp.  Nothing here is on a frame's path: a model's
// export workspace exists once its first export has asked for it, and goes with the model.
#pragma once

#include "export_kernels.hpp"
#include "modeldb_io.hpp"

constexpr int kExportLaunches = 3;  // count, scan, write -- whatever the store holds

static inline unsigned export_blocks(unsigned count) { return count ? (count + kExportBlock - 1) / kExportBlock : 1u; }

// the workspace of an export of `count` surfels: per-workgroup counts | the total | every surfel's record.  Grows only; the
// call that grows it has waited for every earlier export (they are synchronous)
static int model_export_workspace(mmf_model* m, unsigned count, unsigned** block_counts, unsigned** total, unsigned char** records) {
    const size_t counts_bytes = align_up((size_t)export_blocks(count) * sizeof(unsigned), 256);
    const size_t need = counts_bytes + 256 + align_up((size_t)count * kExportRecord + 4, 256);
    if (need > m->export_ws_bytes) {
        (void)hipFree(m->export_ws);
        m->export_ws = nullptr, m->export_ws_bytes = 0;
        MMF_HIP_TRY(hipMalloc(&m->export_ws, need + need / 2));
        m->export_ws_bytes = need + need / 2;
    }
    unsigned char* base = static_cast<unsigned char*>(m->export_ws);
    *block_counts = reinterpret_cast<unsigned*>(base);
    *total = reinterpret_cast<unsigned*>(base + counts_bytes);
    *records = base + counts_bytes + 256;
    return MMF_OK;
}

// Model::exportModelPLY's loop (Model.cpp:1547-1594): the surfels with conf > conf_threshold, ascending, as 31-byte records
// in HOST memory.  *n_valid is always written; capacity < *n_valid: MMF_ERR_INVALID and nothing is copied.  Synchronous;
// reads the store only (like mmf_model_download_map it first lets an in-flight count land).
extern "C" int mmf_model_export_cloud(mmf_model* m, const float pose[16], float conf_threshold, void* host_records, unsigned capacity,
                                      unsigned* n_valid) {
    MMF_REQUIRE(m && pose && n_valid && (host_records || capacity == 0), "mmf_model_export_cloud: null argument");
    *n_valid = 0;
    MMF_REQUIRE(!model_is_bookkeeping(m), "mmf_model_export_cloud: the model has no surfel store here (another rank owns it)");
    if (int rc0 = model_resolve_count(m)) return rc0;
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const unsigned count = m->count.value, blocks = export_blocks(count);
    unsigned *block_counts = nullptr, *total_dev = nullptr;
    unsigned char* records = nullptr;
    if (int rc = model_export_workspace(m, count, &block_counts, &total_dev, &records)) return rc;
    Mat4 P;
    std::memcpy(P.m, pose, sizeof(P.m));
    m->export_launches = 0;
    hipLaunchKernelGGL(export_count_kernel, dim3(blocks), dim3(kExportBlock), 0, c->stream, m->set[m->cur], count, conf_threshold,
                       block_counts);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kScanBlock), 0, c->stream, block_counts, blocks, total_dev);
    hipLaunchKernelGGL(export_write_kernel, dim3(blocks), dim3(kExportBlock), 0, c->stream, m->set[m->cur], count, conf_threshold, P,
                       (const unsigned*)block_counts, records);
    MMF_HIP_TRY(hipGetLastError());
    m->export_launches = kExportLaunches;
    unsigned total = 0;
    MMF_HIP_TRY(hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    MMF_REQUIRE(total <= count, "mmf_model_export_cloud: more records than surfels");
    *n_valid = total;
    MMF_REQUIRE(capacity >= total, "mmf_model_export_cloud: capacity below the number of stable surfels (mmf_model_count bounds it)");
    if (total) {
        MMF_HIP_TRY(hipMemcpyAsync(host_records, records, (size_t)total * kExportRecord, hipMemcpyDeviceToHost, c->stream));
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return MMF_OK;
}

extern "C" int mmf_model_export_last_launches(mmf_model* m) { return m ? m->export_launches : -1; }

// ---- the files (modeldb_io.hpp) ----------------------------------------------------------------------------------------------
static int modeldb_status(int rc, const std::string& err) { return rc == mmf::modeldb::kOk ? MMF_OK : fail(MMF_ERR_INVALID, err); }

extern "C" int mmf_ply_write_cloud(const char* path, const void* records, unsigned n) {
    std::string err;
    return modeldb_status(mmf::modeldb::write_cloud(path, records, n, &err), err);
}
extern "C" int mmf_ply_read_cloud(const char* path, void* records, unsigned capacity, unsigned* n) {
    std::string err;
    return modeldb_status(mmf::modeldb::read_cloud(path, records, capacity, n, &err), err);
}
extern "C" int mmf_tracks_ply_write(const char* path, int n_views, const int* counts, const float* descriptor, const float* coordinate,
                                    const float pose[16]) {
    std::string err;
    return modeldb_status(mmf::modeldb::write_tracks(path, n_views, counts, descriptor, coordinate, pose, &err), err);
}
extern "C" int mmf_tracks_ply_read(const char* path, int cap_views, int* n_views, int* counts, int cap_rows, int* n_rows,
                                   float* descriptor, float* coordinate) {
    std::string err;
    return modeldb_status(mmf::modeldb::read_tracks(path, cap_views, n_views, counts, cap_rows, n_rows, descriptor, coordinate, &err), err);
}

// a model's stable surfels (its own confidence threshold) under `pose`, as a PLY file at `path`
static int model_export_ply(mmf_model* m, const char* path, const float pose[16], float conf_threshold) {
    unsigned bound = 0, n = 0;
    if (int rc = mmf_model_count(m, &bound)) return rc;
    std::vector<unsigned char> records((size_t)bound * kExportRecord);
    if (int rc = mmf_model_export_cloud(m, pose, conf_threshold, records.data(), bound, &n)) return rc;
    return mmf_ply_write_cloud(path, records.data(), n);
}
// Model::exportModelPLY(surfels, getConfidenceThreshold(), path, pose) (Model.cpp:1510, :1604)
extern "C" int mmf_model_export_ply(mmf_model* m, const char* path, const float pose[16]) {
    MMF_REQUIRE(m && path && pose, "mmf_model_export_ply: null argument");
    return model_export_ply(m, path, pose, m->conf_threshold);
}
