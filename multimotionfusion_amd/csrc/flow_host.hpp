// flow_host.hpp -- the host side of the optical-flow engine (flow_kernels.hpp): the object, its tables, the
// launches of a frame pair and the C ABI (mmf_flow_*).  Included by mmf_hip.hip.
//
// An engine owns two sets of stage images (grey, smoothed, expansion) and swaps them from frame to frame: a frame pays stages
// 1-4 once.  A pair is 1 + 2 * iterations launches whatever the size: one expansion launch (both frames of a stateless pair
// share it), then per iteration the matrices and the blur-and-solve; the last of them writes magnitude and motion as well.
// Nothing here waits: the launches go to the stream they are given (the context's for the public calls, the fusion's flow
// stream inside processFrame).
#pragma once

struct mmf_flow {
    mmf_ctx* ctx = nullptr;
    mmf::FlowGeom geo{};
    mmf_flow_config cfg{};
    mmf::FlowTables tab{};
    void* mem = nullptr;  // every buffer below, one allocation
    uint8_t* gray[2] = {nullptr, nullptr};
    float* smooth[2] = {nullptr, nullptr};
    float* R[2] = {nullptr, nullptr};
    float* M = nullptr;           // the matrices the last iteration's blur read
    float* flow_it = nullptr;     // [iterations][H][W][2]: the flow behind every iteration
    float *magnitude = nullptr, *motion = nullptr;
    int cur = 0;              // the set that holds the latest frame
    bool have_frame = false;  // `cur` holds a frame of the running sequence (mmf_flow_next)
    bool have_flow = false;   // the result buffers hold a pair's flow; R[1 - cur] is its first frame
    int last_launches = 0;
    float* result() const { return flow_it + (size_t)(cfg.iterations - 1) * geo.W * geo.H * 2; }
};

// Refusals, before any device is touched.  `who` names the public function.
static int flow_check_config(int width, int height, const mmf_flow_config* cfg, const char* who) {
    const std::string w(who);
    MMF_REQUIRE(cfg != nullptr, w + ": null configuration");
    MMF_REQUIRE(cfg->levels == 1, w + ": levels must be 1 (pyramids are not supported)");
    MMF_REQUIRE(cfg->div == 1 || cfg->div == 2 || cfg->div == 4, w + ": div must be 1, 2 or 4");
    MMF_REQUIRE(width > 0 && height > 0 && width % cfg->div == 0 && height % cfg->div == 0,
                w + ": div must divide the frame's width and height (" + std::to_string(width) + " x " + std::to_string(height) + ", div " +
                    std::to_string(cfg->div) + ")");
    MMF_REQUIRE(width / cfg->div >= 8 && height / cfg->div >= 8, w + ": the flow image must be at least 8 x 8");
    MMF_REQUIRE((long long)width * height <= (long long)INT_MAX / 16, w + ": frame too large");
    MMF_REQUIRE(cfg->winsize >= 2 && cfg->winsize <= 2 * mmf::kFlowMaxM + 1, w + ": winsize must be in [2, 33]");
    MMF_REQUIRE(cfg->poly_n >= 3 && cfg->poly_n <= mmf::kFlowMaxN, w + ": poly_n must be in [3, 7]");
    MMF_REQUIRE(cfg->iterations >= 1 && cfg->iterations <= 10, w + ": iterations must be in [1, 10]");
    MMF_REQUIRE(cfg->poly_sigma > 0.f, w + ": poly_sigma must be positive");  // (a NaN is refused too)
    return MMF_OK;
}

// The expansion's tables: the Gaussian normalised over -n..n and its first two moments, and four entries of the inverse of
// the 6 x 6 moment matrix of the basis (1, x, y, x^2, y^2, xy).  That matrix couples only {1, x^2, y^2}:
//   [a b b; b c d; b d c],  a = sum g g, b = sum g g x^2, c = sum g g x^4, d = sum g g x^2 y^2;  G(x,x) = G(y,y) = b, G(xy,xy) = d
// so its inverse is written out.  Double throughout, rounded to float once.
static void flow_make_tables(int n, double sigma, mmf::FlowTables* t) {
    double g[mmf::kFlowMaxN + 1], s = 0.0;
    for (int k = 0; k <= n; ++k) {
        g[k] = std::exp(-(double)(k * k) / (2.0 * sigma * sigma));
        s += k == 0 ? g[k] : 2.0 * g[k];
    }
    *t = mmf::FlowTables{};
    for (int k = 0; k <= n; ++k) {
        g[k] /= s;
        t->g[k] = (float)g[k], t->xg[k] = (float)(k * g[k]), t->xxg[k] = (float)((double)(k * k) * g[k]);
    }
    double a = 0, b = 0, c = 0, d = 0;
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const double w = g[std::abs(y)] * g[std::abs(x)];
            a += w, b += w * x * x, c += w * x * x * x * x, d += w * x * x * y * y;
        }
    const double e = a * (c + d) - 2.0 * b * b;
    t->ig[0] = (float)(1.0 / b);                         // ig11
    t->ig[1] = (float)(-b / e);                          // ig03
    t->ig[2] = (float)((a * c - b * b) / ((c - d) * e));  // ig33
    t->ig[3] = (float)(1.0 / d);                         // ig55
}

static mmf::FlowFrameOut flow_frame_out(const mmf_flow* fl, int set, const uint8_t* rgb) {
    return mmf::FlowFrameOut{rgb, fl->gray[set], fl->smooth[set], fl->R[set]};
}

// stages 5-8 of the pair (R[1 - cur], R[cur]) on `st`: 2 * iterations launches
static void flow_enqueue_iterations(mmf_flow* fl, hipStream_t st) {
    using namespace mmf;
    const FlowGeom& g = fl->geo;
    const size_t px = (size_t)g.W * g.H;
    const dim3 tiles((g.W + kFlowTX - 1) / kFlowTX, (g.H + kFlowTY - 1) / kFlowTY), block(kFlowTX, kFlowTY);
    const float *R0 = fl->R[1 - fl->cur], *R1 = fl->R[fl->cur];
    for (int it = 0; it < fl->cfg.iterations; ++it) {
        const float* prev = it == 0 ? nullptr : fl->flow_it + (size_t)(it - 1) * px * 2;
        const bool last = it == fl->cfg.iterations - 1;
        hipLaunchKernelGGL(flow_matrices_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, g, R0, R1, prev, fl->M);
        hipLaunchKernelGGL(flow_blur_solve_kernel, tiles, block, 0, st, g, (const float*)fl->M, fl->flow_it + (size_t)it * px * 2,
                           last ? fl->magnitude : nullptr, last ? fl->motion : nullptr);
    }
}

static dim3 flow_expand_grid(const mmf_flow* fl, int frames) {
    return dim3((fl->geo.W + mmf::kFlowTX - 1) / mmf::kFlowTX, (fl->geo.H + mmf::kFlowTY - 1) / mmf::kFlowTY, frames);
}

// the next frame of the sequence on `st`: its expansion, and from the second frame on the flow from the frame before it
static int flow_next_on(mmf_flow* fl, const uint8_t* rgb, hipStream_t st, int* has_flow) {
    const int set = fl->have_frame ? 1 - fl->cur : 0;
    const mmf::FlowFrameOut out = flow_frame_out(fl, set, rgb);
    hipLaunchKernelGGL(mmf::flow_expand_kernel, flow_expand_grid(fl, 1), dim3(mmf::kFlowTX, mmf::kFlowTY), 0, st, fl->geo, fl->tab, out, out);
    fl->last_launches = 1;
    const bool pair = fl->have_frame;
    fl->cur = set, fl->have_frame = true, fl->have_flow = false;
    if (pair) {
        flow_enqueue_iterations(fl, st);
        fl->last_launches += 2 * fl->cfg.iterations;
    }
    MMF_HIP_TRY(hipGetLastError());
    fl->have_flow = pair;
    if (has_flow) *has_flow = pair ? 1 : 0;
    return MMF_OK;
}

extern "C" int mmf_flow_default_config(mmf_flow_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_flow_default_config: null configuration");
    // Segmentation.cpp:779-804: the pair scaled down by 4; calcOpticalFlowFarneback(.., 0.2, 1, 20, 2, 5, 15 / 50.0, 0)
    cfg->div = 4, cfg->levels = 1, cfg->winsize = 20, cfg->iterations = 2, cfg->poly_n = 5, cfg->poly_sigma = 0.3f;
    return MMF_OK;
}

static int flow_create_impl(mmf_ctx* c, int width, int height, const mmf_flow_config* cfg, mmf_flow** out, const char* who) {
    if (int rc = flow_check_config(width, height, cfg, who)) return rc;
    MMF_REQUIRE(c != nullptr && out != nullptr, std::string(who) + ": null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_flow* fl = new (std::nothrow) mmf_flow();
    MMF_REQUIRE(fl != nullptr, std::string(who) + ": out of host memory");
    fl->ctx = c, fl->cfg = *cfg;
    fl->geo = mmf::FlowGeom{width, height, cfg->div, width / cfg->div, height / cfg->div, cfg->poly_n, cfg->winsize / 2};
    flow_make_tables(cfg->poly_n, (double)cfg->poly_sigma, &fl->tab);
    const size_t px = (size_t)fl->geo.W * fl->geo.H;
    // floats first (16-byte aligned pieces are not needed: every access is scalar), the two grey images behind them
    const size_t floats = px * (2 * 1 + 2 * 5 + 5 + 2 * (size_t)cfg->iterations + 2);
    const hipError_t e = hipMalloc(&fl->mem, floats * sizeof(float) + 2 * px);
    if (e != hipSuccess) {
        delete fl;
        return fail(MMF_ERR_HIP, std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    }
    float* p = static_cast<float*>(fl->mem);
    for (int s = 0; s < 2; ++s) fl->smooth[s] = p, p += px;
    for (int s = 0; s < 2; ++s) fl->R[s] = p, p += 5 * px;
    fl->M = p, p += 5 * px;
    fl->flow_it = p, p += 2 * px * (size_t)cfg->iterations;
    fl->magnitude = p, p += px;
    fl->motion = p, p += px;
    fl->gray[0] = reinterpret_cast<uint8_t*>(p), fl->gray[1] = fl->gray[0] + px;
    *out = fl;
    return MMF_OK;
}

extern "C" int mmf_flow_create(mmf_ctx* c, int width, int height, const mmf_flow_config* cfg, mmf_flow** out) {
    return flow_create_impl(c, width, height, cfg, out, "mmf_flow_create");
}

// `st`: a further stream whose enqueued work may still use the buffers (the fusion's flow stream), or nullptr
static void flow_destroy_on(mmf_flow* fl, hipStream_t st) {
    if (!fl) return;
    (void)hipSetDevice(fl->ctx->device);
    (void)hipStreamSynchronize(fl->ctx->stream);
    if (st) (void)hipStreamSynchronize(st);
    (void)hipFree(fl->mem);
    delete fl;
}
extern "C" void mmf_flow_destroy(mmf_flow* fl) { flow_destroy_on(fl, nullptr); }

extern "C" int mmf_flow_reset(mmf_flow* fl) {
    MMF_REQUIRE(fl != nullptr, "mmf_flow_reset: null engine");
    fl->have_frame = fl->have_flow = false;
    return MMF_OK;
}

extern "C" int mmf_flow_next(mmf_flow* fl, const uint8_t* rgb, int* has_flow) {
    MMF_REQUIRE(fl != nullptr && rgb != nullptr, "mmf_flow_next: null argument");
    MMF_HIP_TRY(hipSetDevice(fl->ctx->device));
    return flow_next_on(fl, rgb, fl->ctx->stream, has_flow);
}

// A stateless pair: both frames are expanded in one launch.  The running sequence of mmf_flow_next ends here (the next call
// of it starts a new one): the pair uses the sequence's buffers.
extern "C" int mmf_flow_compute(mmf_flow* fl, const uint8_t* prev_rgb, const uint8_t* next_rgb) {
    MMF_REQUIRE(fl != nullptr && prev_rgb != nullptr && next_rgb != nullptr, "mmf_flow_compute: null argument");
    MMF_HIP_TRY(hipSetDevice(fl->ctx->device));
    hipStream_t st = fl->ctx->stream;
    fl->have_frame = fl->have_flow = false;
    fl->cur = 1;
    hipLaunchKernelGGL(mmf::flow_expand_kernel, flow_expand_grid(fl, 2), dim3(mmf::kFlowTX, mmf::kFlowTY), 0, st, fl->geo, fl->tab,
                       flow_frame_out(fl, 0, prev_rgb), flow_frame_out(fl, 1, next_rgb));
    flow_enqueue_iterations(fl, st);
    fl->last_launches = 1 + 2 * fl->cfg.iterations;
    MMF_HIP_TRY(hipGetLastError());
    fl->have_flow = true;
    return MMF_OK;
}

extern "C" int mmf_flow_result(mmf_flow* fl, const float** flow_dev, const float** magnitude_dev, const float** motion_dev, int* w, int* h) {
    MMF_REQUIRE(fl != nullptr, "mmf_flow_result: null engine");
    if (w) *w = fl->geo.W;
    if (h) *h = fl->geo.H;
    if (!fl->have_flow) return fail(MMF_ERR_STATE, "mmf_flow_result: no pair has been computed since creation or the last reset");
    if (flow_dev) *flow_dev = fl->result();
    if (magnitude_dev) *magnitude_dev = fl->magnitude;
    if (motion_dev) *motion_dev = fl->motion;
    return MMF_OK;
}

// the stage images, for tests: gray / smooth (the latest frame; gray0 / smooth0: the pair's first frame), R0 / R1 (the
// pair's expansions), M, flow_<i> (behind iteration i), magnitude, motion.  Synchronous on the context's stream.
extern "C" int mmf_flow_download(mmf_flow* fl, const char* name, void* host_dst, size_t bytes) {
    MMF_REQUIRE(fl != nullptr && name != nullptr && host_dst != nullptr, "mmf_flow_download: null argument");
    const size_t px = (size_t)fl->geo.W * fl->geo.H;
    const std::string s(name);
    const void* src = nullptr;
    size_t want = 0;
    const bool frame_image = s == "gray" || s == "smooth";
    if (frame_image ? !fl->have_frame && !fl->have_flow : !fl->have_flow)
        return fail(MMF_ERR_STATE, "mmf_flow_download: '" + s + "' has not been computed yet");
    const int cur = fl->cur, old = 1 - fl->cur;
    if (s == "gray") src = fl->gray[cur], want = px;
    else if (s == "gray0") src = fl->gray[old], want = px;
    else if (s == "smooth") src = fl->smooth[cur], want = px * 4;
    else if (s == "smooth0") src = fl->smooth[old], want = px * 4;
    else if (s == "R0") src = fl->R[old], want = px * 20;
    else if (s == "R1") src = fl->R[cur], want = px * 20;
    else if (s == "M") src = fl->M, want = px * 20;
    else if (s == "magnitude") src = fl->magnitude, want = px * 4;
    else if (s == "motion") src = fl->motion, want = px * 4;
    else if (s.rfind("flow_", 0) == 0 && s.size() > 5 && s.size() <= 7 && s.find_first_not_of("0123456789", 5) == std::string::npos) {
        const int it = std::atoi(s.c_str() + 5);
        MMF_REQUIRE(it >= 0 && it < fl->cfg.iterations, "mmf_flow_download: no such iteration: " + s);
        src = fl->flow_it + (size_t)it * px * 2, want = px * 8;
    }
    MMF_REQUIRE(src != nullptr, "mmf_flow_download: unknown image '" + s + "'");
    MMF_REQUIRE(bytes == want, "mmf_flow_download: '" + s + "' has " + std::to_string(want) + " bytes, the buffer " + std::to_string(bytes));
    MMF_HIP_TRY(hipSetDevice(fl->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(host_dst, src, want, hipMemcpyDeviceToHost, fl->ctx->stream));
    MMF_HIP_TRY(hipStreamSynchronize(fl->ctx->stream));
    return MMF_OK;
}

static void flow_copy_tables(const mmf::FlowTables& t, int n, float* g, float* xg, float* xxg, float* ig) {
    for (int k = 0; k <= n; ++k) {
        if (g) g[k] = t.g[k];
        if (xg) xg[k] = t.xg[k];
        if (xxg) xxg[k] = t.xxg[k];
    }
    if (ig)
        for (int k = 0; k < 4; ++k) ig[k] = t.ig[k];
}
// the tables the engine's kernels read: g, xg, xxg [poly_n + 1], ig [4] = {ig11, ig03, ig33, ig55}
extern "C" int mmf_flow_tables(mmf_flow* fl, float* g, float* xg, float* xxg, float* ig) {
    MMF_REQUIRE(fl != nullptr, "mmf_flow_tables: null engine");
    flow_copy_tables(fl->tab, fl->cfg.poly_n, g, xg, xxg, ig);
    return MMF_OK;
}
// ... and what an engine with (poly_n, poly_sigma) would hold: host arithmetic, no device
extern "C" int mmf_flow_make_tables(int poly_n, float poly_sigma, float* g, float* xg, float* xxg, float* ig) {
    MMF_REQUIRE(poly_n >= 3 && poly_n <= mmf::kFlowMaxN, "mmf_flow_make_tables: poly_n must be in [3, 7]");
    MMF_REQUIRE(poly_sigma > 0.f, "mmf_flow_make_tables: poly_sigma must be positive");
    mmf::FlowTables t;
    flow_make_tables(poly_n, (double)poly_sigma, &t);
    flow_copy_tables(t, poly_n, g, xg, xxg, ig);
    return MMF_OK;
}

extern "C" int mmf_flow_last_launches(mmf_flow* fl) { return fl ? fl->last_launches : -1; }
