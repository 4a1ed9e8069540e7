// flowseg_host.hpp -- the host side of the blob stage of the flow_crf segmentation (flowseg_kernels.hpp): the
// object, the launches of one run and the C ABI (mmf_flowseg_*).  Included by mmf_hip.hip behind flowcrf_host.hpp.
//
// One run is 8 kernel launches, two memsets and one copy of the summary into pinned memory, whatever the image holds.  Nothing
// here waits but mmf_flowseg_result: the launches go to the stream they are given (the context's for the public calls, the
// fusion's inside processFrame).
#pragma once

struct mmf_flowseg {
    mmf_ctx* ctx = nullptr;
    mmf_flowseg_config cfg{};
    int W = 0, H = 0, w = 0, h = 0, N = 0, max_labels = 0, nwg = 0;
    std::vector<void*> allocs;
    int *label = nullptr, *comp = nullptr, *area2 = nullptr, *area2_cell = nullptr;
    unsigned long long* best = nullptr;  // [32] winners, then [32] unsigned pixels per entry: one memset
    unsigned* pix = nullptr;
    int8_t* cross = nullptr;
    uint8_t *ring = nullptr, *winner = nullptr, *segm = nullptr, *full = nullptr;
    double* slab = nullptr;
    mmf::FsegSummary *sum_dev = nullptr, *sum_host = nullptr;  // sum_host: pinned
    const uint8_t* full_last = nullptr;                        // where the last run wrote the full-size image
    bool have_result = false;
    int last_launches = 0;
};

static int flowseg_check_config(int width, int height, int max_labels, const mmf_flowseg_config* cfg, const char* who) {
    const std::string w(who);
    MMF_REQUIRE(cfg != nullptr, w + ": null configuration");
    MMF_REQUIRE(cfg->div == 4, w + ": div must be 4");
    MMF_REQUIRE(width > 0 && height > 0 && width % 4 == 0 && height % 4 == 0,
                w + ": 4 must divide the frame's width and height (" + std::to_string(width) + " x " + std::to_string(height) + ")");
    MMF_REQUIRE((long long)width * height <= (long long)INT_MAX / 64, w + ": frame too large");
    MMF_REQUIRE(max_labels >= 1 && max_labels <= mmf::kCrfMaxLabels, w + ": at most 32 labels (models and the new label)");
    MMF_REQUIRE(cfg->new_model_size >= 0.f && cfg->new_model_size < 1.f, w + ": new_model_size must be in [0, 1)");  // (NaN refused too)
    MMF_REQUIRE(cfg->avg_confidence >= 0.f, w + ": avg_confidence must not be negative");
    MMF_REQUIRE(cfg->model_spawn_offset >= 0, w + ": model_spawn_offset must not be negative");
    return MMF_OK;
}

extern "C" int mmf_flowseg_default_config(mmf_flowseg_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_flowseg_default_config: null configuration");
    // Segmentation.cpp:1302 (new_model_size), :1307 (avgConfidence); the spawn offset as mmf_crf_default_config
    cfg->div = 4, cfg->new_model_size = 0.05f, cfg->avg_confidence = 0.4f, cfg->model_spawn_offset = 22, cfg->inhibit_new = 0;
    return MMF_OK;
}

static void flowseg_destroy_on(mmf_flowseg* fs, hipStream_t st) {
    if (!fs) return;
    (void)hipSetDevice(fs->ctx->device);
    (void)hipStreamSynchronize(fs->ctx->stream);
    if (st) (void)hipStreamSynchronize(st);
    for (void* p : fs->allocs) (void)hipFree(p);
    if (fs->sum_host) (void)hipHostFree(fs->sum_host);
    delete fs;
}
extern "C" void mmf_flowseg_destroy(mmf_flowseg* fs) { flowseg_destroy_on(fs, nullptr); }

template <typename P>
static int flowseg_alloc(mmf_flowseg* fs, P** p, size_t count) {
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(P)));
    fs->allocs.push_back(*p);
    return MMF_OK;
}

static int flowseg_create_impl(mmf_ctx* c, int width, int height, int max_labels, const mmf_flowseg_config* cfg, mmf_flowseg** out,
                               const char* who) {
    if (int rc = flowseg_check_config(width, height, max_labels, cfg, who)) return rc;
    MMF_REQUIRE(c != nullptr && out != nullptr, std::string(who) + ": null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_flowseg* fs = new (std::nothrow) mmf_flowseg();
    MMF_REQUIRE(fs != nullptr, std::string(who) + ": out of host memory");
    fs->ctx = c, fs->cfg = *cfg, fs->W = width, fs->H = height, fs->w = width / 4, fs->h = height / 4, fs->N = fs->w * fs->h;
    fs->max_labels = max_labels;
    fs->nwg = (int)(((size_t)width * height + mmf::kFsegStatTile - 1) / mmf::kFsegStatTile);
    const size_t N = (size_t)fs->N;
    int rc = MMF_OK;
    auto A = [&](auto** p, size_t n) {
        if (rc == MMF_OK) rc = flowseg_alloc(fs, p, n);
    };
    A(&fs->label, N), A(&fs->comp, N), A(&fs->area2, N), A(&fs->area2_cell, N), A(&fs->best, (size_t)mmf::kCrfMaxLabels * 3 / 2);
    A(&fs->cross, (size_t)max_labels * N), A(&fs->ring, N), A(&fs->winner, N), A(&fs->segm, N), A(&fs->full, (size_t)width * height);
    A(&fs->slab, (size_t)fs->nwg * 2 * mmf::kCrfMaxLabels), A(&fs->sum_dev, 1);
    if (rc == MMF_OK) {
        fs->pix = reinterpret_cast<unsigned*>(fs->best + mmf::kCrfMaxLabels);
        if (hipHostMalloc(reinterpret_cast<void**>(&fs->sum_host), sizeof(mmf::FsegSummary), hipHostMallocDefault) != hipSuccess)
            rc = fail(MMF_ERR_HIP, std::string(who) + ": hipHostMalloc");
    }
    if (rc != MMF_OK) {
        const std::string msg = g_last_error;
        flowseg_destroy_on(fs, nullptr);
        return fail(rc, msg);
    }
    *out = fs;
    return MMF_OK;
}

extern "C" int mmf_flowseg_create(mmf_ctx* c, int width, int height, int max_labels, const mmf_flowseg_config* cfg, mmf_flowseg** out) {
    return flowseg_create_impl(c, width, height, max_labels, cfg, out, "mmf_flowseg_create");
}

// the label table of a run: the models' ids in list order, then the new id
static int flowseg_table(const mmf_flowseg* fs, const unsigned char* ids, int n_models, int allow_new, unsigned new_id, mmf::FsegTable* t,
                         const char* who) {
    const std::string w(who);
    MMF_REQUIRE(fs != nullptr && ids != nullptr, w + ": null argument");
    MMF_REQUIRE(n_models >= 1 && n_models + (allow_new ? 1 : 0) <= fs->max_labels,
                w + ": " + std::to_string(n_models) + " models" + (allow_new ? " and the new label" : "") + " with an engine for " +
                    std::to_string(fs->max_labels) + " labels");
    MMF_REQUIRE(new_id <= 255u, w + ": ids are 0 .. 255");
    std::memset(t, 0, sizeof(*t));
    std::memset(t->entry, mmf::kFsegNoEntry, sizeof(t->entry));
    t->L = n_models + (allow_new ? 1 : 0), t->allow_new = allow_new ? 1 : 0;
    for (int e = 0; e < t->L; ++e) {
        const uint8_t id = e < n_models ? ids[e] : (uint8_t)new_id;
        MMF_REQUIRE(t->entry[id] == mmf::kFsegNoEntry, w + ": id " + std::to_string((int)id) + " is in the table twice");
        t->id[e] = id, t->entry[id] = (uint8_t)e;
    }
    int k = 0;
    for (int id = 0; id < 256; ++id)
        if (t->entry[id] != mmf::kFsegNoEntry) t->order[k++] = t->entry[id];
    return MMF_OK;
}

// one run on `st`; full_out: where the full-size image goes (nullptr: the engine's own)
static int flowseg_run_on(mmf_flowseg* fs, const uint8_t* ids, const float* depth, const mmf::FsegTable& tab, hipStream_t st,
                          uint8_t* full_out) {
    using namespace mmf;
    const int N = fs->N, w = fs->w, h = fs->h;
    uint8_t* full = full_out ? full_out : fs->full;
    fs->have_result = false;
    MMF_HIP_TRY(hipMemsetAsync(fs->best, 0, (size_t)kCrfMaxLabels * 3 / 2 * sizeof(unsigned long long), st));
    MMF_HIP_TRY(hipMemsetAsync(fs->cross, 0, (size_t)tab.L * N, st));
    const dim3 cells((unsigned)((N + kFsegThreads - 1) / kFsegThreads)), block(kFsegThreads);
    hipLaunchKernelGGL(fseg_init_kernel, cells, block, 0, st, ids, tab, w, h, fs->label, fs->ring);
    hipLaunchKernelGGL(fseg_merge_kernel, cells, block, 0, st, ids, w, N, fs->label);
    hipLaunchKernelGGL(fseg_flatten_kernel, cells, block, 0, st, N, (const int*)fs->label, fs->comp);
    hipLaunchKernelGGL(fseg_trace_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, ids, (const int*)fs->comp,
                       (const uint8_t*)fs->ring, tab, w, h, fs->area2, fs->best);
    hipLaunchKernelGGL(fseg_mark_kernel, dim3(1), dim3(64), 0, st, (const uint8_t*)fs->ring, tab.L, w, h, (const unsigned long long*)fs->best, fs->cross);
    hipLaunchKernelGGL(fseg_compose_kernel, dim3((unsigned)h), dim3(64), 0, st, ids, (const int*)fs->comp, (const int*)fs->area2, tab, w, h,
                       (const unsigned long long*)fs->best, (const int8_t*)fs->cross, fs->segm, fs->area2_cell, fs->winner);
    const bool vec = (reinterpret_cast<uintptr_t>(depth) & 15u) == 0 && (reinterpret_cast<uintptr_t>(full) & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(fseg_stats_kernel<true>, dim3((unsigned)fs->nwg), block, 0, st, (const uint8_t*)fs->segm, depth, tab, fs->W, fs->H, full,
                           fs->slab, fs->pix);
    else
        hipLaunchKernelGGL(fseg_stats_kernel<false>, dim3((unsigned)fs->nwg), block, 0, st, (const uint8_t*)fs->segm, depth, tab, fs->W, fs->H, full,
                           fs->slab, fs->pix);
    hipLaunchKernelGGL(fseg_finish_kernel, dim3(1), dim3(64), 0, st, tab, w, h, fs->cfg.new_model_size, fs->cfg.avg_confidence,
                       (const double*)fs->slab, fs->nwg, (const unsigned*)fs->pix, (const unsigned long long*)fs->best, fs->sum_dev);
    MMF_HIP_TRY(hipGetLastError());
    MMF_HIP_TRY(hipMemcpyAsync(fs->sum_host, fs->sum_dev, sizeof(FsegSummary), hipMemcpyDeviceToHost, st));
    fs->full_last = full, fs->last_launches = 8, fs->have_result = true;
    return MMF_OK;
}

extern "C" int mmf_flowseg_run(mmf_flowseg* fs, const uint8_t* ids_dev, const float* depth_dev, const unsigned char* ids_host, int n_models,
                               int allow_new, unsigned new_id) {
    MMF_REQUIRE(fs && ids_dev && depth_dev, "mmf_flowseg_run: null argument");
    mmf::FsegTable tab;
    if (int rc = flowseg_table(fs, ids_host, n_models, allow_new, new_id, &tab, "mmf_flowseg_run")) return rc;
    MMF_HIP_TRY(hipSetDevice(fs->ctx->device));
    return flowseg_run_on(fs, ids_dev, depth_dev, tab, fs->ctx->stream, nullptr);
}

extern "C" int mmf_flowseg_result(mmf_flowseg* fs, const uint8_t** segm_dev, const uint8_t** full_dev, mmf_flowseg_summary* summary, int* w,
                                  int* h) {
    MMF_REQUIRE(fs != nullptr, "mmf_flowseg_result: null engine");
    if (w) *w = fs->w;
    if (h) *h = fs->h;
    if (!fs->have_result) return fail(MMF_ERR_STATE, "mmf_flowseg_result: nothing has run yet");
    MMF_HIP_TRY(hipSetDevice(fs->ctx->device));
    MMF_HIP_TRY(wait_stream(fs->ctx->stream));
    if (segm_dev) *segm_dev = fs->segm;
    if (full_dev) *full_dev = fs->full_last;
    if (summary) *summary = *fs->sum_host;
    return MMF_OK;
}

// the stage images of the last run, for tests.  Synchronous on the context's stream.
extern "C" int mmf_flowseg_download(mmf_flowseg* fs, const char* name, void* host_dst, size_t bytes) {
    MMF_REQUIRE(fs != nullptr && name != nullptr && host_dst != nullptr, "mmf_flowseg_download: null argument");
    if (!fs->have_result) return fail(MMF_ERR_STATE, "mmf_flowseg_download: nothing has run yet");
    const size_t N = (size_t)fs->N;
    const std::string s(name);
    const void* src = nullptr;
    size_t want = 0;
    if (s == "component") src = fs->comp, want = N * 4;
    else if (s == "area2") src = fs->area2_cell, want = N * 4;
    else if (s == "winner") src = fs->winner, want = N;
    else if (s == "segm") src = fs->segm, want = N;
    else if (s == "full") src = fs->full_last, want = (size_t)fs->W * fs->H;
    MMF_REQUIRE(src != nullptr, "mmf_flowseg_download: unknown image '" + s + "'");
    MMF_REQUIRE(bytes == want, "mmf_flowseg_download: '" + s + "' has " + std::to_string(want) + " bytes, the buffer " + std::to_string(bytes));
    MMF_HIP_TRY(hipSetDevice(fs->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(host_dst, src, want, hipMemcpyDeviceToHost, fs->ctx->stream));
    MMF_HIP_TRY(hipStreamSynchronize(fs->ctx->stream));
    return MMF_OK;
}

extern "C" int mmf_flowseg_last_launches(mmf_flowseg* fs) { return fs ? fs->last_launches : -1; }
