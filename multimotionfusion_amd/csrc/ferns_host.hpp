// ferns_host.hpp -- the host side of the fern keyframe database (ferns_kernels.hpp): the object, the table of
// ferns, the three launches of a process call and the C ABI (mmf_ferns_*).  Included by mmf_hip.hip.
//
// A process call enqueues encode, search and select on the stream it is given (the context's for the public call, the hook's
// lane inside processFrame) and returns: the number of keyframes, the drop count and the result record stay on the device.
// The calls that hand something to the host (result, keyframe, download) wait for that stream and read through pinned memory.
#pragma once

struct mmf_ferns {
    mmf_ctx* ctx = nullptr;
    mmf::FernsGeom geo{};
    mmf_ferns_config cfg{};
    DeviceBuf<int> table;       // [num][6]
    DeviceBuf<uchar4> cur_image;  // the current frame's small images, codes and per-wave counts
    DeviceBuf<float4> cur_vert, cur_norm;
    DeviceBuf<uint8_t> cur_codes;
    DeviceBuf<int> wave_good;
    DeviceBuf<uint8_t> db_codes;  // the keyframes, slot by slot
    DeviceBuf<int> db_good, db_times;
    DeviceBuf<float> db_poses;
    DeviceBuf<uchar4> db_image;
    DeviceBuf<float4> db_vert, db_norm;
    DeviceBuf<int> counters;  // {keyframes stored, frames dropped}
    DeviceBuf<int> co, both;  // the last search
    DeviceBuf<float> dissim;
    DeviceBuf<mmf_ferns_result_t> record;
    struct Pinned {  // what result / keyframe read back
        mmf_ferns_result_t record;
        int counters[2];
        float pose[16];
        int time, good;
    };
    PinnedBuf<Pinned> pin;
    hipStream_t last_stream = nullptr;  // where the last process call went
    bool processed = false;
    int last_launches = 0;

    mmf::FernsCur cur() const {
        return mmf::FernsCur{cur_image.get(), cur_vert.get(), cur_norm.get(), cur_codes.get(), wave_good.get()};
    }
    mmf::FernsDb db() const {
        return mmf::FernsDb{db_codes.get(), db_good.get(), db_times.get(), db_poses.get(), db_image.get(),
                            db_vert.get(),  db_norm.get(), counters.get(), counters.get() + 1};
    }
    hipStream_t stream() const { return last_stream ? last_stream : ctx->stream; }
};

// splitmix64: the sequence mmf_ferns_make_table draws from
static inline unsigned long long ferns_next(unsigned long long& state) {
    state += 0x9E3779B97F4A7C15ull;
    unsigned long long z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Refusals, before any device is touched.  `who` names the public function; table == nullptr: not checked.
static int ferns_check_config(int width, int height, const mmf_ferns_config* cfg, const int* table, const char* who) {
    const std::string w(who);
    MMF_REQUIRE(cfg != nullptr, w + ": null configuration");
    MMF_REQUIRE(width >= 8 && height >= 8, w + ": the frame must be at least 8 x 8");
    MMF_REQUIRE((long long)width * height <= (long long)INT_MAX / 16, w + ": frame too large");
    MMF_REQUIRE(cfg->num >= 1 && cfg->num <= mmf::kFernsMaxNum, w + ": num must be in [1, " + std::to_string(mmf::kFernsMaxNum) + "]");
    MMF_REQUIRE(cfg->max_depth_mm >= 400, w + ": max_depth_mm must be at least 400");
    MMF_REQUIRE(cfg->capacity >= 1, w + ": capacity must be at least 1");
    MMF_REQUIRE((long long)cfg->capacity * (width / 8) * (height / 8) <= (long long)INT_MAX / 16, w + ": capacity too large for this frame size");
    MMF_REQUIRE(cfg->threshold == cfg->threshold && cfg->min_similarity == cfg->min_similarity, w + ": a threshold is NaN");
    if (!table) return MMF_OK;
    const int sw = width / 8, sh = height / 8;
    for (int i = 0; i < cfg->num; ++i) {
        const int* f = table + 6 * (size_t)i;
        const bool ok = f[0] >= 0 && f[0] < sw && f[1] >= 0 && f[1] < sh && f[2] >= 0 && f[2] <= 255 && f[3] >= 0 && f[3] <= 255 && f[4] >= 0 &&
                        f[4] <= 255 && f[5] >= 400 && f[5] <= cfg->max_depth_mm;
        MMF_REQUIRE(ok, w + ": fern " + std::to_string(i) + " is outside its ranges");
    }
    return MMF_OK;
}

extern "C" int mmf_ferns_default_config(mmf_ferns_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_ferns_default_config: null configuration");
    // MultiMotionFusion.cpp:33: ferns(500, depthCut * 1000, photoThresh), depthCut = the GUI's depth cutoff (GUI/Tools/GUI.h:203:
    // 15.0; MainController.cpp:515); Ferns.cpp:193 (300), :203 (0.3); MultiMotionFusion.h:57 (fernThresh 0.3095)
    cfg->num = 500, cfg->max_depth_mm = 15000, cfg->capacity = 1024, cfg->min_time_gap = 300;
    cfg->threshold = 0.3095f, cfg->min_similarity = 0.3f;
    return MMF_OK;
}

// Ferns::generateFerns (Ferns.cpp:56-70): per fern x, y, three colour thresholds and a depth threshold, uniform over the
// reference's ranges -- from a sequence of this library's own (the reference seeds std::mt19937 with time(0))
extern "C" int mmf_ferns_make_table(unsigned long long seed, int num, int w, int h, int max_depth_mm, int* table_out) {
    MMF_REQUIRE(table_out != nullptr, "mmf_ferns_make_table: null table");
    MMF_REQUIRE(num >= 1 && w >= 1 && h >= 1 && max_depth_mm >= 400, "mmf_ferns_make_table: num, w, h must be at least 1, max_depth_mm at least 400");
    unsigned long long state = seed;
    auto draw = [&state](int lo, int hi) { return lo + (int)(ferns_next(state) % (unsigned long long)(hi - lo + 1)); };
    for (int i = 0; i < num; ++i) {
        int* f = table_out + 6 * (size_t)i;
        f[0] = draw(0, w - 1), f[1] = draw(0, h - 1);
        f[2] = draw(0, 255), f[3] = draw(0, 255), f[4] = draw(0, 255);
        f[5] = draw(400, max_depth_mm);
    }
    return MMF_OK;
}

static int ferns_create_impl(mmf_ctx* c, int width, int height, const mmf_ferns_config* cfg, const int* table, mmf_ferns** out, const char* who) {
    MMF_REQUIRE(table != nullptr, std::string(who) + ": null table");
    if (int rc = ferns_check_config(width, height, cfg, table, who)) return rc;
    MMF_REQUIRE(c != nullptr && out != nullptr, std::string(who) + ": null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_ferns* fe = new (std::nothrow) mmf_ferns();
    MMF_REQUIRE(fe != nullptr, std::string(who) + ": out of host memory");
    fe->ctx = c, fe->cfg = *cfg;
    mmf::FernsGeom& g = fe->geo;
    g.width = width, g.height = height, g.w = width / 8, g.h = height / 8;
    g.num = cfg->num, g.stride = (cfg->num + 3) & ~3, g.capacity = cfg->capacity;
    g.image_blocks = (g.w * g.h + mmf::kFernsThreads - 1) / mmf::kFernsThreads;
    g.code_blocks = (g.stride + mmf::kFernsThreads - 1) / mmf::kFernsThreads;
    const size_t px = (size_t)g.w * g.h, cap = (size_t)g.capacity, waves = (size_t)g.code_blocks * mmf::kFernsSearchWaves;
    auto device_side = [&]() -> int {
        MMF_HIP_TRY(fe->table.create((size_t)g.num * 6));
        MMF_HIP_TRY(fe->cur_image.create(px));
        MMF_HIP_TRY(fe->cur_vert.create(px));
        MMF_HIP_TRY(fe->cur_norm.create(px));
        MMF_HIP_TRY(fe->cur_codes.create((size_t)g.stride));
        MMF_HIP_TRY(fe->wave_good.create(waves));
        MMF_HIP_TRY(fe->db_codes.create(cap * g.stride));
        MMF_HIP_TRY(fe->db_good.create(cap));
        MMF_HIP_TRY(fe->db_times.create(cap));
        MMF_HIP_TRY(fe->db_poses.create(cap * 16));
        MMF_HIP_TRY(fe->db_image.create(cap * px));
        MMF_HIP_TRY(fe->db_vert.create(cap * px));
        MMF_HIP_TRY(fe->db_norm.create(cap * px));
        MMF_HIP_TRY(fe->counters.create(2));
        MMF_HIP_TRY(fe->co.create(cap));
        MMF_HIP_TRY(fe->both.create(cap));
        MMF_HIP_TRY(fe->dissim.create(cap));
        MMF_HIP_TRY(fe->record.create(1));
        MMF_HIP_TRY(fe->pin.create(1));
        // (the table is pageable host memory: the copy has left it when the call returns)
        MMF_HIP_TRY(hipMemcpyAsync(fe->table.get(), table, (size_t)g.num * 6 * sizeof(int), hipMemcpyHostToDevice, c->stream));
        MMF_HIP_TRY(hipMemsetAsync(fe->counters.get(), 0, 2 * sizeof(int), c->stream));
        // what a download may show before anything was written there
        MMF_HIP_TRY(hipMemsetAsync(fe->db_codes.get(), 0xff, cap * g.stride, c->stream));
        MMF_HIP_TRY(hipMemsetAsync(fe->db_good.get(), 0, cap * sizeof(int), c->stream));
        MMF_HIP_TRY(hipMemsetAsync(fe->db_times.get(), 0, cap * sizeof(int), c->stream));
        MMF_HIP_TRY(hipMemsetAsync(fe->co.get(), 0, cap * sizeof(int), c->stream));
        MMF_HIP_TRY(hipMemsetAsync(fe->both.get(), 0, cap * sizeof(int), c->stream));
        MMF_HIP_TRY(hipMemsetAsync(fe->dissim.get(), 0, cap * sizeof(float), c->stream));
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
        return MMF_OK;
    };
    if (int rc = device_side()) {
        const std::string keep = g_last_error;
        delete fe;
        return fail(rc, std::string(who) + ": " + keep);
    }
    *out = fe;
    return MMF_OK;
}

extern "C" int mmf_ferns_create(mmf_ctx* c, int width, int height, const mmf_ferns_config* cfg, const int* table, mmf_ferns** out) {
    return ferns_create_impl(c, width, height, cfg, table, out, "mmf_ferns_create");
}

// `st`: a further stream whose enqueued work may still use the buffers (the hook's lane), or nullptr
static void ferns_destroy_on(mmf_ferns* fe, hipStream_t st) {
    if (!fe) return;
    (void)hipSetDevice(fe->ctx->device);
    (void)hipStreamSynchronize(fe->ctx->stream);
    if (st) (void)hipStreamSynchronize(st);
    delete fe;
}
extern "C" void mmf_ferns_destroy(mmf_ferns* fe) { ferns_destroy_on(fe, nullptr); }

// on `st`, behind whatever the engine's last stream holds when that is `st` or has been joined by it
static int ferns_reset_on(mmf_ferns* fe, hipStream_t st) {
    MMF_HIP_TRY(hipMemsetAsync(fe->counters.get(), 0, 2 * sizeof(int), st));
    fe->processed = false;
    return MMF_OK;
}
extern "C" int mmf_ferns_reset(mmf_ferns* fe) {
    MMF_REQUIRE(fe != nullptr, "mmf_ferns_reset: null engine");
    MMF_HIP_TRY(hipSetDevice(fe->ctx->device));
    if (fe->last_stream && fe->last_stream != fe->ctx->stream) MMF_HIP_TRY(hipStreamSynchronize(fe->last_stream));
    return ferns_reset_on(fe, fe->ctx->stream);
}

extern "C" int mmf_ferns_set_threshold(mmf_ferns* fe, float threshold) {
    MMF_REQUIRE(fe != nullptr, "mmf_ferns_set_threshold: null engine");
    MMF_REQUIRE(threshold == threshold, "mmf_ferns_set_threshold: the threshold is NaN");
    fe->cfg.threshold = threshold;
    return MMF_OK;
}

// encode, search, select on `st`
static int ferns_process_on(mmf_ferns* fe, const void* image, const void* vert, const void* norm, const float* pose, int time, int flags,
                            hipStream_t st, const char* who) {
    using namespace mmf;
    MMF_REQUIRE(image != nullptr && vert != nullptr && norm != nullptr, std::string(who) + ": null image");
    MMF_REQUIRE(pose != nullptr, std::string(who) + ": null pose");
    MMF_REQUIRE(flags >= 1 && flags <= (MMF_FERNS_FIND | MMF_FERNS_ADD), std::string(who) + ": flags must be MMF_FERNS_FIND, MMF_FERNS_ADD or both");
    const FernsGeom& g = fe->geo;
    const FernsFrame in{static_cast<const uchar4*>(image), static_cast<const float4*>(vert), static_cast<const float4*>(norm)};
    FernsCall call;
    std::memcpy(call.pose, pose, sizeof(call.pose));
    call.time = time, call.flags = flags, call.min_time_gap = fe->cfg.min_time_gap;
    call.threshold = fe->cfg.threshold, call.min_similarity = fe->cfg.min_similarity;
    fe->last_stream = st;
    hipLaunchKernelGGL(ferns_encode_kernel, dim3((unsigned)(g.image_blocks + g.code_blocks)), dim3(kFernsThreads), 0, st, g, in,
                       (const int*)fe->table.get(), fe->cur());
    hipLaunchKernelGGL(ferns_search_kernel, dim3((unsigned)((g.capacity + kFernsSearchWaves - 1) / kFernsSearchWaves)), dim3(kFernsThreads),
                       (size_t)g.stride, st, g, (const uint8_t*)fe->cur_codes.get(), (const int*)fe->wave_good.get(), fe->db(), fe->co.get(),
                       fe->both.get(), fe->dissim.get());
    hipLaunchKernelGGL(ferns_select_kernel, dim3(1), dim3(kFernsSelectThreads), 0, st, g, fe->cur(), fe->db(), (const int*)fe->co.get(),
                       (const int*)fe->both.get(), (const float*)fe->dissim.get(), call, fe->record.get());
    fe->last_launches = 3;
    MMF_HIP_TRY(hipGetLastError());
    fe->processed = true;
    return MMF_OK;
}

extern "C" int mmf_ferns_process(mmf_ferns* fe, const void* image_rgba_dev, const void* vert_dev, const void* norm_dev, const float pose[16],
                                 int time, int flags) {
    MMF_REQUIRE(fe != nullptr, "mmf_ferns_process: null engine");
    MMF_HIP_TRY(hipSetDevice(fe->ctx->device));
    if (fe->last_stream && fe->last_stream != fe->ctx->stream) MMF_HIP_TRY(hipStreamSynchronize(fe->last_stream));
    return ferns_process_on(fe, image_rgba_dev, vert_dev, norm_dev, pose, time, flags, fe->ctx->stream, "mmf_ferns_process");
}

extern "C" int mmf_ferns_result(mmf_ferns* fe, mmf_ferns_result_t* out) {
    MMF_REQUIRE(fe != nullptr && out != nullptr, "mmf_ferns_result: null argument");
    if (!fe->processed) return fail(MMF_ERR_STATE, "mmf_ferns_result: no frame has been processed since creation or the last reset");
    MMF_HIP_TRY(hipSetDevice(fe->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(&fe->pin.get()->record, fe->record.get(), sizeof(mmf_ferns_result_t), hipMemcpyDeviceToHost, fe->stream()));
    MMF_HIP_TRY(hipStreamSynchronize(fe->stream()));
    *out = fe->pin.get()->record;
    return MMF_OK;
}

extern "C" int mmf_ferns_keyframe(mmf_ferns* fe, int id, const void** image_dev, const void** vert_dev, const void** norm_dev, float pose[16],
                                  int* time, int* good_codes) {
    MMF_REQUIRE(fe != nullptr, "mmf_ferns_keyframe: null engine");
    MMF_REQUIRE(id >= 0 && id < fe->geo.capacity, "mmf_ferns_keyframe: no such keyframe");
    MMF_HIP_TRY(hipSetDevice(fe->ctx->device));
    mmf_ferns::Pinned* p = fe->pin.get();
    hipStream_t st = fe->stream();
    MMF_HIP_TRY(hipMemcpyAsync(p->counters, fe->counters.get(), sizeof(p->counters), hipMemcpyDeviceToHost, st));
    MMF_HIP_TRY(hipMemcpyAsync(p->pose, fe->db_poses.get() + 16 * (size_t)id, sizeof(p->pose), hipMemcpyDeviceToHost, st));
    MMF_HIP_TRY(hipMemcpyAsync(&p->time, fe->db_times.get() + id, sizeof(int), hipMemcpyDeviceToHost, st));
    MMF_HIP_TRY(hipMemcpyAsync(&p->good, fe->db_good.get() + id, sizeof(int), hipMemcpyDeviceToHost, st));
    MMF_HIP_TRY(hipStreamSynchronize(st));
    MMF_REQUIRE(id < p->counters[0], "mmf_ferns_keyframe: keyframe " + std::to_string(id) + " is not stored (" + std::to_string(p->counters[0]) +
                                         " keyframes)");
    const size_t px = (size_t)fe->geo.w * fe->geo.h;
    if (image_dev) *image_dev = fe->db_image.get() + (size_t)id * px;
    if (vert_dev) *vert_dev = fe->db_vert.get() + (size_t)id * px;
    if (norm_dev) *norm_dev = fe->db_norm.get() + (size_t)id * px;
    if (pose) std::memcpy(pose, p->pose, sizeof(p->pose));
    if (time) *time = p->time;
    if (good_codes) *good_codes = p->good;
    return MMF_OK;
}

// for tests; synchronous on the stream of the last process call
extern "C" int mmf_ferns_download(mmf_ferns* fe, const char* name, void* host_dst, size_t bytes) {
    MMF_REQUIRE(fe != nullptr && name != nullptr && host_dst != nullptr, "mmf_ferns_download: null argument");
    const mmf::FernsGeom& g = fe->geo;
    const size_t px = (size_t)g.w * g.h, cap = (size_t)g.capacity;
    const std::string s(name);
    const void* src = nullptr;
    size_t want = 0, row = 0, pitch = 0;  // row != 0: rows of `row` bytes, `pitch` apart
    bool current = true;
    if (s == "image") src = fe->cur_image.get(), want = px * 4;
    else if (s == "vert") src = fe->cur_vert.get(), want = px * 16;
    else if (s == "norm") src = fe->cur_norm.get(), want = px * 16;
    else if (s == "codes") src = fe->cur_codes.get(), want = (size_t)g.num;
    else if (s == "co") src = fe->co.get(), want = cap * 4;
    else if (s == "dissim") src = fe->dissim.get(), want = cap * 4;
    else if (s == "db_codes") src = fe->db_codes.get(), want = cap * g.num, row = (size_t)g.num, pitch = (size_t)g.stride, current = false;
    else if (s == "db_times") src = fe->db_times.get(), want = cap * 4, current = false;
    else if (s == "db_good") src = fe->db_good.get(), want = cap * 4, current = false;
    MMF_REQUIRE(src != nullptr, "mmf_ferns_download: unknown array '" + s + "'");
    if (current && !fe->processed) return fail(MMF_ERR_STATE, "mmf_ferns_download: '" + s + "' has not been computed yet");
    MMF_REQUIRE(bytes == want, "mmf_ferns_download: '" + s + "' has " + std::to_string(want) + " bytes, the buffer " + std::to_string(bytes));
    MMF_HIP_TRY(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->stream();
    if (row != 0 && row != pitch)
        MMF_HIP_TRY(hipMemcpy2DAsync(host_dst, row, src, pitch, row, cap, hipMemcpyDeviceToHost, st));
    else
        MMF_HIP_TRY(hipMemcpyAsync(host_dst, src, want, hipMemcpyDeviceToHost, st));
    MMF_HIP_TRY(hipStreamSynchronize(st));
    return MMF_OK;
}

extern "C" int mmf_ferns_last_launches(mmf_ferns* fe) { return fe ? fe->last_launches : -1; }
