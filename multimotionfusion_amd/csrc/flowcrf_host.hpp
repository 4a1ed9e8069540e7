// flowcrf_host.hpp -- the host side of the flow-CRF inference engine (flowcrf_kernels.hpp): the object, the
// launches of one inference and the C ABI (mmf_flowcrf_*).  Included by mmf_hip.hip behind tracker_host.hpp.
//
// One inference is 5 + 3 * iterations kernel launches (4 at iterations 0) and one memset, whatever the image size, the number
// of labels and the number of tracks: tracks, prep, the normalisation's pair pass, the first softmax; per iteration the pair
// pass, the row blur and the update; the fusion.  Nothing here waits: the launches go to the stream they are given (the
// context's for the public calls, the fusion's flow stream inside processFrame).
#pragma once

struct mmf_flowcrf {
    mmf_ctx* ctx = nullptr;
    mmf::FcrfGeom geo{};
    mmf_flowcrf_config cfg{};
    mmf::FcrfTable tab{};
    int max_labels = 0, lp_max = 0, max_tracks = 0;
    std::vector<void*> allocs;
    int *claim = nullptr, *cell = nullptr, *label = nullptr;
    float *speed = nullptr, *E = nullptr, *U = nullptr, *proj = nullptr, *Q = nullptr, *prob = nullptr;
    float *Ds = nullptr, *Da = nullptr, *xs = nullptr, *xa = nullptr, *hb = nullptr, *partial = nullptr;
    float4* feat = nullptr;
    uint8_t *invalid = nullptr, *ids = nullptr, *ids_full = nullptr;
    int L = 0, M = 0;  // of the last inference
    bool have_result = false;
    int last_launches = 0;
};

static int flowcrf_pad_labels(int L) {
    int p = 1;
    while (p < L) p *= 2;
    return p;
}
static int flowcrf_ipl(int LP) { return LP <= 16 ? 4 : 2; }
// ranges of j per cell i: enough workgroups for every CU a few times over, never more than there are chunks
static int flowcrf_nsplit(int N, int LP) {
    const int tiles = (N + 64 * flowcrf_ipl(LP) - 1) / (64 * flowcrf_ipl(LP)), nchunk = (N + mmf::kFcrfTJ - 1) / mmf::kFcrfTJ;
    return std::max(1, std::min(nchunk, (768 + tiles - 1) / tiles));
}

// the split of fcrf_pair_kernel's sum over j as flowcrf_launch_pair launches it and the kernel walks it (host: no device needed)
extern "C" int mmf_debug_flowcrf_pair_geometry(int n_cells, int padded_labels, int* nsplit, int* nchunk, int* per) {
    MMF_REQUIRE(n_cells >= 1 && padded_labels >= 1 && padded_labels <= mmf::kCrfMaxLabels && flowcrf_pad_labels(padded_labels) == padded_labels,
                "mmf_debug_flowcrf_pair_geometry: cells >= 1 and a padded label width of 1, 2, 4, 8, 16 or 32");
    MMF_REQUIRE(nsplit && nchunk && per, "mmf_debug_flowcrf_pair_geometry: null argument");
    *nsplit = flowcrf_nsplit(n_cells, padded_labels);
    *nchunk = (n_cells + mmf::kFcrfTJ - 1) / mmf::kFcrfTJ;
    *per = (*nchunk + *nsplit - 1) / *nsplit;
    return MMF_OK;
}

static int flowcrf_check_config(int width, int height, int max_labels, int max_tracks, const mmf_flowcrf_config* cfg, const char* who) {
    const std::string w(who);
    MMF_REQUIRE(cfg != nullptr, w + ": null configuration");
    MMF_REQUIRE(cfg->div == 4, w + ": div must be 4");
    MMF_REQUIRE(width > 0 && height > 0 && width % 4 == 0 && height % 4 == 0,
                w + ": 4 must divide the frame's width and height (" + std::to_string(width) + " x " + std::to_string(height) + ")");
    MMF_REQUIRE((long long)width * height <= (long long)INT_MAX / 64, w + ": frame too large");
    MMF_REQUIRE(max_labels >= 1 && max_labels <= mmf::kCrfMaxLabels, w + ": at most 32 labels (models and the new label)");
    MMF_REQUIRE(max_tracks >= 0 && max_tracks <= (1 << 24), w + ": max_tracks out of range");
    MMF_REQUIRE(cfg->iterations >= 0 && cfg->iterations <= 50, w + ": iterations must be in [0, 50]");
    MMF_REQUIRE(cfg->weight_smoothness > 0.f && cfg->weight_appearance > 0.f, w + ": the weights must be positive");  // (NaN refused too)
    MMF_REQUIRE(cfg->threshold > 0.f && cfg->max_err > 0.f && cfg->min_proj_prob >= 0.f && cfg->min_proj_prob <= 1.f,
                w + ": threshold and max_err must be positive, min_proj_prob in [0, 1]");
    return MMF_OK;
}

extern "C" int mmf_flowcrf_default_config(mmf_flowcrf_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_flowcrf_default_config: null configuration");
    // Segmentation.h's crfIterations / weightSmoothness / weightAppearance; Segmentation.cpp:822 (max_err), :922 (threshold), :1169
    cfg->div = 4, cfg->iterations = 10, cfg->weight_smoothness = 40.f, cfg->weight_appearance = 40.f;
    cfg->threshold = 20.f, cfg->max_err = 0.03f, cfg->min_proj_prob = 0.3f;
    return MMF_OK;
}

template <typename P>
static int flowcrf_alloc(mmf_flowcrf* fc, P** p, size_t count) {
    MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(P)));
    fc->allocs.push_back(*p);
    return MMF_OK;
}

static void flowcrf_destroy_on(mmf_flowcrf* fc, hipStream_t st) {
    if (!fc) return;
    (void)hipSetDevice(fc->ctx->device);
    (void)hipStreamSynchronize(fc->ctx->stream);
    if (st) (void)hipStreamSynchronize(st);
    for (void* p : fc->allocs) (void)hipFree(p);
    delete fc;
}
extern "C" void mmf_flowcrf_destroy(mmf_flowcrf* fc) { flowcrf_destroy_on(fc, nullptr); }

static int flowcrf_create_impl(mmf_ctx* c, int width, int height, int max_labels, int max_tracks, float fx, float fy, float cx, float cy,
                               const mmf_flowcrf_config* cfg, mmf_flowcrf** out, const char* who) {
    if (int rc = flowcrf_check_config(width, height, max_labels, max_tracks, cfg, who)) return rc;
    MMF_REQUIRE(c != nullptr && out != nullptr, std::string(who) + ": null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_flowcrf* fc = new (std::nothrow) mmf_flowcrf();
    MMF_REQUIRE(fc != nullptr, std::string(who) + ": out of host memory");
    fc->ctx = c, fc->cfg = *cfg;
    fc->geo = mmf::FcrfGeom{width, height, width / 4, height / 4, (width / 4) * (height / 4), fx, fy, cx, cy};
    fc->max_labels = max_labels, fc->lp_max = flowcrf_pad_labels(max_labels), fc->max_tracks = std::max(max_tracks, 1);
    for (int d = 0; d <= mmf::kFcrfRadius; ++d) fc->tab.g[d] = (float)std::exp(-(double)(d * d) / 18.0);
    const size_t N = (size_t)fc->geo.N, Lm = (size_t)max_labels, LP = (size_t)fc->lp_max, T = (size_t)fc->max_tracks;
    size_t part = 0;
    for (int lp = 1; lp <= fc->lp_max; lp *= 2) part = std::max(part, (size_t)flowcrf_nsplit(fc->geo.N, lp) * lp);
    int rc = MMF_OK;
    auto A = [&](auto** p, size_t n) {
        if (rc == MMF_OK) rc = flowcrf_alloc(fc, p, n);
    };
    A(&fc->claim, Lm * N), A(&fc->cell, Lm * T), A(&fc->speed, Lm * T), A(&fc->label, N);
    A(&fc->E, Lm * N), A(&fc->U, Lm * N), A(&fc->proj, Lm * N), A(&fc->Q, Lm * N), A(&fc->prob, Lm * N);
    A(&fc->Ds, N), A(&fc->Da, N), A(&fc->xs, N * LP), A(&fc->xa, N * LP), A(&fc->hb, N * LP), A(&fc->partial, part * N);
    A(&fc->feat, N), A(&fc->invalid, N), A(&fc->ids, N), A(&fc->ids_full, (size_t)width * height);
    // (a track row the kernel never reaches reads "no sample" in the "cell" download)
    if (rc == MMF_OK && hipMemset(fc->cell, 0xFF, Lm * T * sizeof(int)) != hipSuccess) rc = fail(MMF_ERR_HIP, std::string(who) + ": hipMemset");
    if (rc != MMF_OK) {
        const std::string msg = g_last_error;
        flowcrf_destroy_on(fc, nullptr);
        return fail(rc, msg);
    }
    *out = fc;
    return MMF_OK;
}

extern "C" int mmf_flowcrf_create(mmf_ctx* c, int width, int height, int max_labels, int max_tracks, float fx, float fy, float cx, float cy,
                                  const mmf_flowcrf_config* cfg, mmf_flowcrf** out) {
    return flowcrf_create_impl(c, width, height, max_labels, max_tracks, fx, fy, cx, cy, cfg, out, "mmf_flowcrf_create");
}

template <int LMAX, int IPL>
static void flowcrf_launch_pair(const mmf_flowcrf* fc, const float* x, hipStream_t st) {
    const int N = fc->geo.N;
    const dim3 grid((unsigned)((N + 64 * IPL - 1) / (64 * IPL)), (unsigned)flowcrf_nsplit(N, LMAX));
    hipLaunchKernelGGL((mmf::fcrf_pair_kernel<LMAX, IPL>), grid, dim3(256), 0, st, (const float4*)fc->feat, x, N, (int)grid.y, fc->partial);
}
static void flowcrf_pair(const mmf_flowcrf* fc, int LP, const float* x, hipStream_t st) {
    switch (LP) {
        case 1: return flowcrf_launch_pair<1, 4>(fc, x, st);
        case 2: return flowcrf_launch_pair<2, 4>(fc, x, st);
        case 4: return flowcrf_launch_pair<4, 4>(fc, x, st);
        case 8: return flowcrf_launch_pair<8, 4>(fc, x, st);
        case 16: return flowcrf_launch_pair<16, 4>(fc, x, st);
        default: return flowcrf_launch_pair<32, 2>(fc, x, st);
    }
}
static void flowcrf_update(int LP, const mmf::FcrfUpdateArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + 255) / 256)), block(256);
    switch (LP) {
        case 1: hipLaunchKernelGGL(mmf::fcrf_update_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(mmf::fcrf_update_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(mmf::fcrf_update_kernel<4>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(mmf::fcrf_update_kernel<8>, grid, block, 0, st, a); break;
        case 16: hipLaunchKernelGGL(mmf::fcrf_update_kernel<16>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(mmf::fcrf_update_kernel<32>, grid, block, 0, st, a); break;
    }
}

static int flowcrf_check_input(const mmf_flowcrf* fc, const mmf_flowcrf_input* in, const char* who) {
    const std::string w(who);
    MMF_REQUIRE(fc != nullptr && in != nullptr, w + ": null argument");
    MMF_REQUIRE(in->n_models >= 1 && in->n_models + (in->allow_new ? 1 : 0) <= fc->max_labels,
                w + ": " + std::to_string(in->n_models) + " models" + (in->allow_new ? " and the new label" : "") + " with an engine for " +
                    std::to_string(fc->max_labels) + " labels");
    MMF_REQUIRE(in->ids && in->T_start && in->T_end && in->vertex && in->depth && in->flow && in->motion, w + ": null input");
    for (int m = 0; m < in->n_models; ++m) MMF_REQUIRE(in->vertex[m] != nullptr, w + ": null vertex image");
    MMF_REQUIRE(in->new_id <= 255u, w + ": ids are 0 .. 255");
    return MMF_OK;
}

// one inference on `st`.  `tr` holds device pointers (tr.n = 0: no tracks, the pointers are not read).  The tracks, the depth
// and the vertex images are read by the first two launches alone: `inputs_read`, if given, is recorded behind them (the fusion
// rewrites the predictions later in the frame).
static int flowcrf_run_on(mmf_flowcrf* fc, const mmf_flowcrf_input* in, const mmf::FcrfTracks& tr, hipStream_t st,
                          hipEvent_t inputs_read = nullptr) {
    using namespace mmf;
    const FcrfGeom& g = fc->geo;
    const int N = g.N, M = in->n_models, L = M + (in->allow_new ? 1 : 0), LP = flowcrf_pad_labels(L);
    fc->have_result = false;
    FcrfModels md{};
    md.M = M, md.L = L, md.allow_new = in->allow_new ? 1 : 0;
    for (int m = 0; m < M; ++m) {
        std::memcpy(md.T_start[m], in->T_start + 16 * m, 12 * sizeof(float));
        std::memcpy(md.T_end[m], in->T_end + 16 * m, 12 * sizeof(float));
    }
    MMF_HIP_TRY(hipMemsetAsync(fc->claim, 0xFF, (size_t)M * N * sizeof(int), st));  // -1: no track
    const unsigned blocks = (unsigned)std::max(1, (tr.n + 255) / 256);
    hipLaunchKernelGGL(fcrf_track_kernel, dim3(blocks, (unsigned)M), dim3(256), 0, st, g, md, tr, fc->max_tracks, fc->speed, fc->cell, fc->claim);
    FcrfPrepArgs pa{};
    pa.g = g, pa.M = M, pa.L = L, pa.allow_new = md.allow_new, pa.stride = fc->max_tracks;
    pa.threshold = fc->cfg.threshold, pa.max_err = fc->cfg.max_err, pa.min_proj = fc->cfg.min_proj_prob;
    pa.claim = fc->claim, pa.speed = fc->speed, pa.depth = in->depth, pa.flow = in->flow;
    for (int m = 0; m < M; ++m) pa.vert.v[m] = in->vertex[m];
    pa.E = fc->E, pa.U = fc->U, pa.proj = fc->proj, pa.invalid = fc->invalid, pa.feat = fc->feat;
    const dim3 cells((unsigned)((N + 255) / 256)), block(256);
    hipLaunchKernelGGL(fcrf_prep_kernel, cells, block, 0, st, pa);
    if (inputs_read) MMF_HIP_TRY(hipEventRecord(inputs_read, st));
    const int iters = fc->cfg.iterations;
    FcrfUpdateArgs ua{};
    ua.tab = fc->tab, ua.mode = 0, ua.w = g.w, ua.h = g.h, ua.N = N, ua.L = L;
    ua.w_smooth = 4.f * fc->cfg.weight_smoothness, ua.w_app = fc->cfg.weight_appearance;
    ua.U = fc->U, ua.Ds = fc->Ds, ua.Da = fc->Da, ua.Q = fc->Q, ua.xs = fc->xs, ua.xa = fc->xa, ua.hb = fc->hb;
    int launches = 2;
    if (iters > 0) {
        flowcrf_pair(fc, 1, nullptr, st);
        ua.partial = fc->partial, ua.nsplit = flowcrf_nsplit(N, 1);
        ++launches;
    }
    flowcrf_update(LP, ua, st);
    ++launches;
    ua.mode = 1, ua.partial = fc->partial, ua.nsplit = flowcrf_nsplit(N, LP);
    for (int it = 0; it < iters; ++it) {
        flowcrf_pair(fc, LP, fc->xa, st);
        hipLaunchKernelGGL(fcrf_hblur_kernel, dim3((unsigned)(((size_t)N * LP + 255) / 256)), block, 0, st, fc->tab, g.w, N, LP,
                           (const float*)fc->xs, fc->hb);
        flowcrf_update(LP, ua, st);
        launches += 3;
    }
    FcrfFuseArgs fa{};
    fa.g = g, fa.L = L;
    for (int m = 0; m < M; ++m) fa.id[m] = in->ids[m];
    if (in->allow_new) fa.id[M] = (uint8_t)in->new_id;
    fa.Q = fc->Q, fa.proj = fc->proj, fa.motion = in->motion, fa.prob = fc->prob, fa.label = fc->label, fa.ids = fc->ids, fa.ids_full = fc->ids_full;
    hipLaunchKernelGGL(fcrf_fuse_kernel, cells, block, 0, st, fa);
    ++launches;
    MMF_HIP_TRY(hipGetLastError());
    fc->L = L, fc->M = M, fc->last_launches = launches, fc->have_result = true;
    return MMF_OK;
}

extern "C" int mmf_flowcrf_infer(mmf_flowcrf* fc, const mmf_flowcrf_input* in, const mmf_flowcrf_tracks* tracks) {
    if (int rc = flowcrf_check_input(fc, in, "mmf_flowcrf_infer")) return rc;
    mmf::FcrfTracks tr{};
    if (tracks && tracks->count > 0) {
        MMF_REQUIRE(tracks->count <= fc->max_tracks, "mmf_flowcrf_infer: more tracks than the engine was created for");
        MMF_REQUIRE(tracks->xy_cur && tracks->co_cur && tracks->ts_cur && tracks->ok_cur && tracks->xy_prev && tracks->co_prev &&
                        tracks->ts_prev && tracks->ok_prev,
                    "mmf_flowcrf_infer: null track array");
        tr.xy[0] = tracks->xy_cur, tr.co[0] = tracks->co_cur, tr.ts[0] = tracks->ts_cur, tr.ok[0] = tracks->ok_cur;
        tr.xy[1] = tracks->xy_prev, tr.co[1] = tracks->co_prev, tr.ts[1] = tracks->ts_prev, tr.ok[1] = tracks->ok_prev;
        tr.n = tracks->count;
    }
    MMF_HIP_TRY(hipSetDevice(fc->ctx->device));
    return flowcrf_run_on(fc, in, tr, fc->ctx->stream);
}

static int flowcrf_tracker_view(const mmf_flowcrf* fc, const mmf_tracker* t, mmf::FcrfTracks* tr, const char* who) {
    *tr = mmf::FcrfTracks{};
    if (!t) return MMF_OK;
    MMF_REQUIRE(t->ctx == fc->ctx, std::string(who) + ": the tracker belongs to another context");
    MMF_REQUIRE(t->capacity <= fc->max_tracks, std::string(who) + ": the tracker's capacity exceeds the engine's max_tracks");
    for (int s = 0; s < 2; ++s) tr->xy[s] = t->T.xy[s], tr->co[s] = t->T.co[s], tr->ts[s] = t->T.ts[s], tr->ok[s] = t->T.ok[s];
    tr->n_dev = &t->T.head->n_tracks, tr->n = t->capacity;
    return MMF_OK;
}

extern "C" int mmf_flowcrf_infer_tracker(mmf_flowcrf* fc, const mmf_flowcrf_input* in, mmf_tracker* tracker) {
    if (int rc = flowcrf_check_input(fc, in, "mmf_flowcrf_infer_tracker")) return rc;
    mmf::FcrfTracks tr;
    if (int rc = flowcrf_tracker_view(fc, tracker, &tr, "mmf_flowcrf_infer_tracker")) return rc;
    MMF_HIP_TRY(hipSetDevice(fc->ctx->device));
    return flowcrf_run_on(fc, in, tr, fc->ctx->stream);
}

extern "C" int mmf_flowcrf_result(mmf_flowcrf* fc, const uint8_t** ids_dev, const uint8_t** ids_full_dev, const float** prob_dev,
                                  const float** q_dev, int* w, int* h, int* n_labels) {
    MMF_REQUIRE(fc != nullptr, "mmf_flowcrf_result: null engine");
    if (w) *w = fc->geo.w;
    if (h) *h = fc->geo.h;
    if (!fc->have_result) return fail(MMF_ERR_STATE, "mmf_flowcrf_result: nothing has been inferred yet");
    if (ids_dev) *ids_dev = fc->ids;
    if (ids_full_dev) *ids_full_dev = fc->ids_full;
    if (prob_dev) *prob_dev = fc->prob;
    if (q_dev) *q_dev = fc->Q;
    if (n_labels) *n_labels = fc->L;
    return MMF_OK;
}

// the stage images of the last inference, for tests.  Synchronous on the context's stream.
extern "C" int mmf_flowcrf_download(mmf_flowcrf* fc, const char* name, void* host_dst, size_t bytes) {
    MMF_REQUIRE(fc != nullptr && name != nullptr && host_dst != nullptr, "mmf_flowcrf_download: null argument");
    if (!fc->have_result) return fail(MMF_ERR_STATE, "mmf_flowcrf_download: nothing has been inferred yet");
    const size_t N = (size_t)fc->geo.N, L = (size_t)fc->L, M = (size_t)fc->M;
    const std::string s(name);
    const void* src = nullptr;
    size_t want = 0;
    if (s == "E") src = fc->E, want = L * N * 4;
    else if (s == "U") src = fc->U, want = L * N * 4;
    else if (s == "proj") src = fc->proj, want = L * N * 4;
    else if (s == "Q") src = fc->Q, want = L * N * 4;
    else if (s == "prob") src = fc->prob, want = L * N * 4;
    else if (s == "label") src = fc->label, want = N * 4;
    else if (s == "ids") src = fc->ids, want = N;
    else if (s == "ids_full") src = fc->ids_full, want = (size_t)fc->geo.W * fc->geo.H;
    else if (s == "invalid") src = fc->invalid, want = N;
    else if (s == "cell") src = fc->cell, want = M * (size_t)fc->max_tracks * 4;  // int [M][max_tracks]
    MMF_REQUIRE(src != nullptr, "mmf_flowcrf_download: unknown image '" + s + "'");
    MMF_REQUIRE(bytes == want, "mmf_flowcrf_download: '" + s + "' has " + std::to_string(want) + " bytes, the buffer " + std::to_string(bytes));
    MMF_HIP_TRY(hipSetDevice(fc->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(host_dst, src, want, hipMemcpyDeviceToHost, fc->ctx->stream));
    MMF_HIP_TRY(hipStreamSynchronize(fc->ctx->stream));
    return MMF_OK;
}

extern "C" int mmf_flowcrf_last_launches(mmf_flowcrf* fc) { return fc ? fc->last_launches : -1; }
