// import_host.hpp -- PLY records back into a model's store (import_kernels.hpp): the inverse of mmf_model_export_cloud, and
// the timestamps of a store set to one time.  Textually included by mmf_hip.hip behind export_host.hpp, whose workspace the
// records are staged in.  The reference restores no surfels; what the file does not hold -- confidence and
// times -- is the caller's.
#pragma once

#include "import_kernels.hpp"

constexpr int kImportLaunches = 1;  // whatever the count

// import_stamp_kernel over the store's current content on `stream` (the caller has let an in-flight count land); enqueues only
static int model_enqueue_timestamps(mmf_model* m, float time, hipStream_t stream) {
    const unsigned count = m->count.value;
    if (!count) return MMF_OK;
    hipLaunchKernelGGL(import_stamp_kernel, dim3(export_blocks(count)), dim3(kExportBlock), 0, stream, m->set[m->cur].col, count, time);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// Record i of `host_records` (31 bytes each, mmf_model_export_cloud's layout) becomes surfel i of the store under `pose`
// (NULL: identity, the same arithmetic), with `confidence` and initTime = timestamp = (float)time.  REPLACES the store's
// content and leaves the model as mmf_model_upload_map leaves it for the same surfels.  n > capacity: MMF_ERR_INVALID and the
// store is untouched.  Synchronous; one launch.
extern "C" int mmf_model_import_cloud(mmf_model* m, const float pose[16], const void* host_records, unsigned n, float confidence, int time) {
    MMF_REQUIRE(m && (host_records || n == 0), "mmf_model_import_cloud: null argument");
    MMF_REQUIRE(!model_is_bookkeeping(m), "mmf_model_import_cloud: the model has no surfel store here (another rank owns it)");
    MMF_REQUIRE(n <= (unsigned)m->capacity, "mmf_model_import_cloud: more records than the model holds surfels");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (int rc0 = model_resolve_count(m)) return rc0;  // lets an in-flight count land before it is replaced
    m->import_launches = 0;
    // the export's workspace: its record area is 256-byte aligned and holds 31 n + 4 bytes or more, so the last whole dword of
    // the records lies inside it; what the bytes behind the records hold is never decoded
    unsigned *block_counts = nullptr, *total_dev = nullptr;
    unsigned char* records = nullptr;
    if (int rc = model_export_workspace(m, n, &block_counts, &total_dev, &records)) return rc;
    Mat4 Q;
    if (pose) std::memcpy(Q.m, pose, sizeof(Q.m));
    else identity16(Q.m);
    if (n) MMF_HIP_TRY(hipMemcpyAsync(records, host_records, (size_t)n * kExportRecord, hipMemcpyHostToDevice, c->stream));
    // (n = 0: one workgroup that finds nothing to do -- the launch count does not depend on the count)
    hipLaunchKernelGGL(import_unpack_kernel, dim3(export_blocks(n)), dim3(kExportBlock), 0, c->stream,
                       reinterpret_cast<const unsigned*>(records), n, Q, confidence, (float)time, m->set[m->cur]);
    MMF_HIP_TRY(hipGetLastError());
    m->import_launches = kImportLaunches;
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    m->count.value = n;
    return MMF_OK;
}

extern "C" int mmf_model_import_last_launches(mmf_model* m) { return m ? m->import_launches : -1; }

// the records of the PLY file at `path` (mmf_ply_read_cloud), then mmf_model_import_cloud.  A file that does not parse or holds
// more records than the model holds surfels: MMF_ERR_INVALID, the store is untouched.  *n_records (may be NULL): the file's
// count once its header has parsed, else 0
static int model_import_ply(mmf_model* m, const char* path, const float pose[16], float confidence, int time, unsigned* n_records) {
    unsigned n = 0;
    if (n_records) *n_records = 0;
    std::string err;
    // the count first: the status of this call speaks of the capacity, the header's verdict is in n and err
    const int rc_head = mmf::modeldb::read_cloud(path, nullptr, 0, &n, &err);
    if (n_records) *n_records = n;
    if (rc_head != mmf::modeldb::kOk && n == 0) return modeldb_status(rc_head, err);
    if (n > (unsigned)m->capacity)
        return fail(MMF_ERR_INVALID, std::string("mmf_model_import_ply: ") + path + " holds " + std::to_string(n) + " records, the model " +
                                         std::to_string(m->capacity) + " surfels");
    std::vector<unsigned char> records((size_t)n * kExportRecord);
    if (int rc = mmf_ply_read_cloud(path, records.data(), n, &n)) return rc;
    return mmf_model_import_cloud(m, pose, records.data(), n, confidence, time);
}
extern "C" int mmf_model_import_ply(mmf_model* m, const char* path, const float pose[16], float confidence, int time) {
    MMF_REQUIRE(m && path, "mmf_model_import_ply: null argument");
    return model_import_ply(m, path, pose, confidence, time, nullptr);
}

// timestamp = (float)time for every surfel of the store; initTime and everything else stay.  Synchronous; one launch
extern "C" int mmf_model_set_timestamps(mmf_model* m, int time) {
    MMF_REQUIRE(m != nullptr, "mmf_model_set_timestamps: null model");
    MMF_REQUIRE(!model_is_bookkeeping(m), "mmf_model_set_timestamps: the model has no surfel store here (another rank owns it)");
    mmf_ctx* c = m->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (int rc0 = model_resolve_count(m)) return rc0;
    if (int rc = model_enqueue_timestamps(m, (float)time, c->stream)) return rc;
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    return MMF_OK;
}
