// backdate_host.hpp -- Model::refineTrackSubset (Core/Model/Model.cpp:649-737) from the tracker's table and view log: the C ABI
// of backdate_kernels.hpp.  Textually included at the end of tracker_host.hpp.
//
// One call: three launches (mark, chain, gather), a wait for the counts, the batch object's one launch with its wait for the
// estimates, and the chain of 4 x 4 products on the host.  The workspace belongs to the tracker and is sized by
// mmf_tracker_reserve_backdate -- or by the first call that needs more --, never per frame.
#pragma once

// the frames s, s - 1, ... that are in the ring (tracker_in_log)
static int tracker_frames_in_log(const mmf_tracker* t) {
    if (t->log.frames <= 0) return 0;
    return (int)std::max<long long>(0, std::min<long long>(t->log.frames, t->frame - t->log_first + 1));
}

extern "C" int mmf_tracker_reserve_backdate(mmf_tracker* t, int history) {
    MMF_REQUIRE(t != nullptr, "mmf_tracker_reserve_backdate: null tracker");
    MMF_REQUIRE(history == 0 || (history >= 2 && history <= mmf::kTrkBackdateMax), "mmf_tracker_reserve_backdate: history is 0 (free) or 2 .. 256");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    if (history != 0 && history <= t->bd_history) return MMF_OK;
    if (history == 0 && t->bd_history == 0) return MMF_OK;
    MMF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));  // (a gather in flight may still write the old buffers)
    tracker_free_backdate(t);
    if (history == 0) return MMF_OK;
    // a problem's rows have a keypoint in their frame's slot and a row of the table: no more than either holds
    const size_t per_problem = (size_t)std::min(t->capacity, t->max_keypoints);
    const size_t rows = std::min<size_t>(per_problem * (size_t)(history - 1), (size_t)1 << 30);
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&t->bd_pin), sizeof(mmf::TrkBackdate), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->bd_dev), sizeof(mmf::TrkBackdate));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->bd_ent), (size_t)history * t->cap_pad * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->bd_p0), rows * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->bd_p1), rows * 3 * sizeof(float));
    if (e != hipSuccess) {
        tracker_free_backdate(t);
        MMF_HIP_TRY(e);
    }
    std::memset(t->bd_pin, 0, sizeof(mmf::TrkBackdate));
    t->bd_history = history, t->bd_row_cap = (int)rows;
    return MMF_OK;
}

// Isometry3f::inverse() of a row-major 4 x 4: [R^T | -(R^T t)], float, sums left to right (redetect_inverse_pose's arithmetic)
static void backdate_inverse16(const float* T, float out[16]) {
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) out[r * 4 + q] = T[q * 4 + r];
        float s = T[0 * 4 + r] * T[3];
        s = s + T[1 * 4 + r] * T[7];
        s = s + T[2 * 4 + r] * T[11];
        out[r * 4 + 3] = -s;
    }
    out[12] = out[13] = out[14] = 0.f, out[15] = 1.f;
}

static void backdate_identity16(float* m) {
    for (int k = 0; k < 16; ++k) m[k] = (k % 5 == 0) ? 1.f : 0.f;
}

extern "C" int mmf_tracker_backdate(mmf_tracker* t, int label, int history, mmf_ransac_batch* batch, mmf_backdated_pose* out,
                                    int capacity, int* n_out) {
    using namespace mmf;
    MMF_REQUIRE(t && batch && out && n_out && capacity >= 0, "mmf_tracker_backdate: bad argument");
    MMF_REQUIRE(label >= 0 && label < kTrkMaxModels, "mmf_tracker_backdate: labels are 0 .. 255");
    MMF_REQUIRE(history >= 2 && history <= kTrkBackdateMax, "mmf_tracker_backdate: history is 2 .. 256");
    if (t->log.frames <= 0) return fail(MMF_ERR_STATE, "mmf_tracker_backdate: the tracker keeps no view log (mmf_tracker_set_view_log)");
    MMF_REQUIRE(batch->ctx == t->ctx, "mmf_tracker_backdate: the batch object must share the tracker's context");
    const int bound = std::max(1, std::min(history, tracker_frames_in_log(t)));
    MMF_REQUIRE(capacity >= bound, "mmf_tracker_backdate: fewer entries than min(history, the frames in the log)");
    int rc = mmf_tracker_reserve_backdate(t, history);
    if (rc) return rc;
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    t->bd_valid = false;
    const long long newest = t->frame;
    hipLaunchKernelGGL(trk_backdate_mark_kernel, dim3((unsigned)bound), dim3(kTrkBlock), 0, st, t->T, t->log, label, bound, newest, t->bd_ent,
                       t->cap_pad);
    hipLaunchKernelGGL(trk_backdate_chain_kernel, dim3(1), dim3(kTrkBlock), 0, st, t->T, bound, (const int*)t->bd_ent, t->cap_pad, t->bd_pin,
                       t->bd_dev);
    hipLaunchKernelGGL(trk_backdate_gather_kernel, dim3((unsigned)std::max(bound - 1, 1)), dim3(kTrkBlock), 0, st, t->log,
                       (const TrkBackdate*)t->bd_dev, (const int*)t->bd_ent, t->cap_pad, newest, t->bd_p0, t->bd_p1, t->bd_row_cap);
    MMF_HIP_TRY(hipGetLastError());
    t->last_launches = 3;
    MMF_HIP_TRY(wait_stream(st));  // wait 1: the counts
    const TrkBackdate& R = t->bd_last = *t->bd_pin;
    MMF_REQUIRE(R.len >= 1 && R.len <= bound && R.rows >= 0 && R.rows <= t->bd_row_cap, "mmf_tracker_backdate: the record is out of range");
    const int len = R.len;
    // the problems, in entry order
    std::vector<int> entry, offsets(1, 0);
    for (int j = 1; j < len; ++j)
        if (R.status[j] == MMF_RANSAC_OK) {
            MMF_REQUIRE(R.nvalid[j] >= 3 && R.offset[j] == offsets.back(), "mmf_tracker_backdate: the record's offsets do not add up");
            entry.push_back(j), offsets.push_back(R.offset[j] + R.nvalid[j]);
        }
    MMF_REQUIRE(offsets.back() == R.rows && (int)entry.size() == R.n_problems, "mmf_tracker_backdate: the record's rows do not add up");
    std::vector<mmf_ransac_result> res(entry.size());
    if (!entry.empty()) {
        rc = mmf_ransac_batch_estimate(batch, t->bd_p0, t->bd_p1, offsets.data(), (int)entry.size(), res.data(), nullptr);  // wait 2
        if (rc) return rc;
    }
    std::vector<float> rel((size_t)len * 16);
    backdate_identity16(rel.data());
    size_t p = 0;
    for (int j = 0; j < len; ++j) {
        mmf_backdated_pose& o = out[j];
        std::memset(&o, 0, sizeof(o));
        const long long stamp = newest - len + 1 + j;
        o.stamp = (int)stamp;
        o.timestamp = tracker_in_log(t, stamp) ? t->add_ts[(size_t)(stamp % t->log.frames)] : 0;
        o.from = R.from[j], o.both = R.both[j], o.nvalid = R.nvalid[j], o.status = R.status[j];
        o.error = std::numeric_limits<float>::infinity();
        backdate_identity16(o.T);
        if (j == 0) continue;
        const float* prev = rel.data() + 16 * (size_t)std::min(std::max(R.from[j], 0), j - 1);
        if (R.status[j] != MMF_RANSAC_OK) {
            std::memcpy(rel.data() + 16 * (size_t)j, prev, 16 * sizeof(float));
            continue;
        }
        const mmf_ransac_result& r = res[p];
        const int n = R.nvalid[j];
        o.status = r.status;
        if (r.status == MMF_RANSAC_OK) {
            std::memcpy(o.T, r.T, sizeof(o.T));
            o.error = r.error, o.n_inliers = r.n_inliers;
        } else if (r.status == MMF_RANSAC_TOO_MANY && n <= 65535) {  // the same core on the host (the verifier's rule for such a set)
            std::vector<float> a((size_t)n * 3), b((size_t)n * 3);
            MMF_HIP_TRY(hipMemcpy(a.data(), t->bd_p0 + 3 * (size_t)offsets[p], a.size() * sizeof(float), hipMemcpyDeviceToHost));
            MMF_HIP_TRY(hipMemcpy(b.data(), t->bd_p1 + 3 * (size_t)offsets[p], b.size() * sizeof(float), hipMemcpyDeviceToHost));
            std::vector<unsigned short> triples(3 * (size_t)batch->cfg.iterations);
            ransac_triples(batch->cfg.iterations, n, triples.data());
            Isometry3f I;
            o.n_inliers = ransac_core_host(batch->cfg, triples.data(), a.data(), b.data(), n, &I, &o.error, nullptr);
            isometry_to_4x4(I, o.T);
            o.status = MMF_RANSAC_OK, o.host_estimated = 1;
        }
        mmf::host::matmul4(prev, o.T, rel.data() + 16 * (size_t)j);  // rel[jk] = rel[ik] * T_01 (:718)
        ++p;
    }
    float E[16];
    backdate_inverse16(rel.data() + 16 * (size_t)(len - 1), E);
    for (int j = 0; j + 1 < len; ++j) mmf::host::matmul4(E, rel.data() + 16 * (size_t)j, out[j].pose);  // (:728-730)
    backdate_identity16(out[len - 1].pose);
    *n_out = len;
    t->bd_valid = true;
    return MMF_OK;
}

// test accessor: the rows the last mmf_tracker_backdate handed the batch object for entry `entry` (HOST p0 / p1 [capacity][3])
extern "C" int mmf_tracker_backdate_rows(mmf_tracker* t, int entry, float* p0, float* p1, int capacity, int* n) {
    MMF_REQUIRE(t && n && capacity >= 0, "mmf_tracker_backdate_rows: bad argument");
    if (!t->bd_valid) return fail(MMF_ERR_STATE, "mmf_tracker_backdate_rows: no mmf_tracker_backdate since the workspace, the log or the tracker changed");
    const mmf::TrkBackdate& R = t->bd_last;
    MMF_REQUIRE(entry >= 0 && entry < R.len, "mmf_tracker_backdate_rows: no such entry");
    *n = (entry > 0 && R.status[entry] == MMF_RANSAC_OK) ? R.nvalid[entry] : 0;
    if (*n == 0) return MMF_OK;
    MMF_REQUIRE(*n <= capacity, "mmf_tracker_backdate_rows: more rows than the arrays hold");
    MMF_HIP_TRY(hipSetDevice(t->ctx->device));
    MMF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    if (p0) MMF_HIP_TRY(hipMemcpy(p0, t->bd_p0 + 3 * (size_t)R.offset[entry], (size_t)*n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (p1) MMF_HIP_TRY(hipMemcpy(p1, t->bd_p1 + 3 * (size_t)R.offset[entry], (size_t)*n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return MMF_OK;
}
