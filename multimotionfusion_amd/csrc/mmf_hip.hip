// mmf_hip.hip -- C ABI (include/mmf_hip.h) over the gfx950 tracking kernels.
// Built only for gfx950 with -ffp-contract=off (see multimotionfusion_amd/build.py).
#include "../../include/mmf_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <new>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "map_kernels.hpp"
#include "prep_batch.hpp"
#include "pose_algebra.hpp"
#include "track_kernels.hpp"
#include "tunables.hpp"
#include "gn_fused.hpp"

using namespace mmf;

// The enqueue side of a chain of dependent kernel launches: launches go out in call order on one stream, the first error
// is kept (`flush`).  (Rounds 2-3 and again round 5 could replay such a chain as a hipGraph -- one host call per chain, the
// arguments of the nodes that changed replaced.  With one model a graph launch reaches the GPU ~10 us later than the first
// kernel of a launch-by-launch chain; with eight models it takes the call's start from 330 to 80 us of the calling thread's
// time and the frame is no shorter: LABNOTES.md.)
// A timed launch (measurement mode 2, mmf_odom_enable_timing) records its dispatch's own start and end into `start` / `stop`.
struct TimedSlot {
    hipEvent_t start = nullptr, stop = nullptr;
};
struct Enqueuer {
    hipStream_t stream = nullptr;
    hipError_t err = hipSuccess;

    explicit Enqueuer(hipStream_t s) : stream(s) {}

    template <typename... KArgs, typename... Args>
    void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, Args&&... args) {
        launch(TimedSlot{}, kernel, grid, block, std::forward<Args>(args)...);
    }
    template <typename... KArgs, typename... Args>
    void launch(const TimedSlot& t, void (*kernel)(KArgs...), dim3 grid, dim3 block, Args&&... args) {
        if (t.start)
            hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, t.start, t.stop, 0, static_cast<KArgs>(args)...);
        else
            hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<KArgs>(args)...);
        const hipError_t e = hipGetLastError();
        if (err == hipSuccess) err = e;
    }
    hipError_t flush() const { return err; }  // everything launched so far is on the stream; the first error, if any
};

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define MMF_HIP_TRY(expr)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return fail(MMF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__) + " (" +  \
                                         __FILE__ + ":" + std::to_string(__LINE__) + ")");        \
    } while (0)

#define MMF_REQUIRE(cond, msg)                                  \
    do {                                                        \
        if (!(cond)) return fail(MMF_ERR_INVALID, (msg));       \
    } while (0)

// Waiting for a short dependent chain: hipStreamSynchronize / hipEventSynchronize park the thread and wake it ~20-30 us
// after the work is done (measured as idle gaps in the kernel trace); the frame has two such waits on its critical path.
// Poll first (the waits are a few hundred microseconds at most), park only when the work takes unusually long.
static hipError_t wait_stream(hipStream_t s) {
    for (int i = 0; i < 200000; ++i) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
    }
    return hipStreamSynchronize(s);
}
extern "C" int mmf_abi_version(void) { return MMF_ABI_VERSION; }
extern "C" const char* mmf_last_error(void) { return g_last_error.c_str(); }

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
constexpr int kMaxGrid = 2048;
constexpr int kMaxIcpGrid = 8192;  // the single-pass ICP producer needs one workgroup per BLOCK * PX pixels  // workgroups per reduction launch (grid-stride beyond)

struct CrfWs;
static void crf_ws_free(CrfWs* w);
struct MaskWs;
static void mask_ws_free(MaskWs* w);

struct mmf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float* partials_f = nullptr;    // kMaxGrid records: in-launch (ticket) reductions
    float* partials_icp = nullptr;  // kMaxGrid records: icp_kernel -> its consumer
    int2* partials_res = nullptr;   // kMaxGrid {count, sigma} records: rgb_residual_kernel -> its consumer
    unsigned* ticket = nullptr;
    OdomState* scratch_state = nullptr;  // for the stand-alone *Step entry points
    OdomState* host_state = nullptr;     // pinned staging
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void* match_ws = nullptr;  // descriptor matcher workspace: norms + arg-min keys, grown on demand
    size_t match_ws_rows = 0;
    void* slic_ws = nullptr;  // super-pixel resampling workspace (boxes, counts, sums), grown on demand
    size_t slic_ws_n = 0;
    void* slic_engine_ws = nullptr;  // super-pixel engine workspace (centres, counts, labels), grown on demand
    size_t slic_engine_cells = 0;
    struct CrfWs* crf_ws = nullptr;  // dense-CRF segmentation workspace (crf_kernels.hpp), grown on demand
    struct MaskWs* mask_ws = nullptr;  // label-image segmentation workspace (mask_kernels.hpp), created on first use
    char arch[64] = {0};
    int cu_count = 0;  // compute units of the device (the one-launch Gauss-Newton chain needs its grid resident at once)
};

static std::atomic<int> g_xcd_forced{-1};  // mmf_debug_set_xcd
extern "C" int mmf_ctx_create(int device, void* stream, int private_stream, mmf_ctx** out) {
    MMF_REQUIRE(out != nullptr, "mmf_ctx_create: out is null");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(MMF_ERR_NO_DEVICE, "mmf_ctx_create: no HIP device visible");
    MMF_REQUIRE(device >= 0 && device < count, "mmf_ctx_create: device index out of range");
    MMF_HIP_TRY(hipSetDevice(device));
    (void)tunables();  // the environment switches are read here, once
    mmf_ctx* c = new (std::nothrow) mmf_ctx();
    MMF_REQUIRE(c != nullptr, "mmf_ctx_create: out of host memory");
    c->device = device;
    hipDeviceProp_t prop;
    MMF_HIP_TRY(hipGetDeviceProperties(&prop, device));
    std::snprintf(c->arch, sizeof(c->arch), "%s", prop.gcnArchName);
    c->cu_count = prop.multiProcessorCount;
    if (std::strncmp(c->arch, "gfx950", 6) != 0) {
        std::string m = std::string("mmf_ctx_create: this library is built for gfx950 only, device is ") + c->arch;
        delete c;
        return fail(MMF_ERR_NO_DEVICE, m);
    }
    if (private_stream) {
        MMF_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    } else {
        c->stream = (hipStream_t)stream;
    }
    MMF_HIP_TRY(hipMalloc(&c->partials_f, sizeof(float) * kMaxGrid * kPartialStride));
    MMF_HIP_TRY(hipMalloc(&c->partials_icp, sizeof(float) * kMaxIcpGrid * kPartialStride));
    MMF_HIP_TRY(hipMalloc(&c->partials_res, sizeof(int2) * kMaxGrid));
    MMF_HIP_TRY(hipMalloc(&c->ticket, sizeof(unsigned) * kTicketWords));
    MMF_HIP_TRY(hipMemsetAsync(c->ticket, 0, sizeof(unsigned) * kTicketWords, c->stream));
    MMF_HIP_TRY(hipMalloc(&c->scratch_state, sizeof(OdomState)));
    MMF_HIP_TRY(hipMemsetAsync(c->scratch_state, 0, sizeof(OdomState), c->stream));
    MMF_HIP_TRY(hipHostMalloc(&c->host_state, sizeof(OdomState), hipHostMallocDefault));
    MMF_HIP_TRY(hipEventCreate(&c->ev0));
    MMF_HIP_TRY(hipEventCreate(&c->ev1));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    {  // (surfel_kernels.hpp: xcd_block)
        const int on = g_xcd_forced.load() < 0 ? (tunables().xcd_blocks ? 1 : 0) : g_xcd_forced.load();
        MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_xcd_blocks), &on, sizeof(on)));
    }
    *out = c;
    return MMF_OK;
}
// test / A-B hook: every XCD works on one contiguous eighth of a surfel pass's blocks (1, the default) or the blocks are dealt
// round-robin as the workgroups are (0); -1 = the default (MMF_XCD).  A device-wide word: set while no pass is running.
extern "C" unsigned mmf_debug_xcd_block(unsigned block, unsigned blocks) { return xcd_block_of(block, blocks); }  // (host: no device needed)
extern "C" int mmf_debug_set_xcd(int on) {
    g_xcd_forced.store(on < 0 ? -1 : (on ? 1 : 0));
    const int v = on < 0 ? (tunables().xcd_blocks ? 1 : 0) : (on ? 1 : 0);
    MMF_HIP_TRY(hipDeviceSynchronize());
    MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_xcd_blocks), &v, sizeof(v)));
    return MMF_OK;
}

extern "C" void mmf_ctx_destroy(mmf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->partials_f);
    (void)hipFree(c->partials_icp);
    (void)hipFree(c->partials_res);
    (void)hipFree(c->ticket);
    (void)hipFree(c->scratch_state);
    (void)hipHostFree(c->host_state);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    (void)hipFree(c->match_ws);
    (void)hipFree(c->slic_ws);
    (void)hipFree(c->slic_engine_ws);
    crf_ws_free(c->crf_ws);
    mask_ws_free(c->mask_ws);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int mmf_ctx_synchronize(mmf_ctx* c) {
    MMF_REQUIRE(c != nullptr, "mmf_ctx_synchronize: ctx is null");
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    return MMF_OK;
}

extern "C" void* mmf_ctx_stream(mmf_ctx* c) { return c ? (void*)c->stream : nullptr; }

extern "C" int mmf_ctx_device_name(mmf_ctx* c, char* buf, size_t buflen) {
    MMF_REQUIRE(c && buf && buflen > 0, "mmf_ctx_device_name: bad arguments");
    std::snprintf(buf, buflen, "%s", c->arch);
    return MMF_OK;
}

// ---------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------
static inline dim3 tile_grid(int cols, int rows) {
    return dim3((cols + kTileX - 1) / kTileX, (rows + kTileY - 1) / kTileY);
}
static inline dim3 tile_block() { return dim3(kTileX, kTileY); }

static inline int stride_elems(size_t step_bytes, int cols, size_t elem) {
    return step_bytes ? (int)(step_bytes / elem) : cols;
}

static inline int reduce_grid(int n, int per_block) {
    int g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > kMaxGrid) g = kMaxGrid;
    return g;
}

static inline LevelIntr level_intr(float fx, float fy, float cx, float cy, int level) {
    const int div = 1 << level;  // types.cuh:94-98
    return LevelIntr{fx / div, fy / div, cx / div, cy / div};
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// largest float x with sqrtf(x) <= t, and smallest x with sqrtf(x) >= t: sqrtf is monotonic and
// correctly rounded, so comparing squares against these is EXACTLY the reference's comparison of
// the norms (reduce.cu:301-306) -- see icp_rows_v
static float sq_max_le(float t) {
    float x = t * t;
    while (std::sqrt(std::nextafter(x, INFINITY)) <= t) x = std::nextafter(x, INFINITY);
    while (std::sqrt(x) > t) x = std::nextafter(x, -INFINITY);
    return x;
}
static float sq_min_ge(float t) {
    float x = t * t;
    while (std::sqrt(std::nextafter(x, -INFINITY)) >= t) x = std::nextafter(x, -INFINITY);
    while (std::sqrt(x) < t) x = std::nextafter(x, INFINITY);
    return x;
}
static void icp_args_derive(IcpArgs& a) {
    a.dist_sq_max = sq_max_le(a.dist_thres);
    a.sine_sq_min = sq_min_ge(a.angle_thres);
    // i / cols == umulhi(i, magic) as long as i * cols < 2^32; larger images divide (0 selects that)
    a.cols_magic = (long long)a.cols * a.rows * a.cols < (1ll << 32) ? (unsigned)((1ull << 32) / (unsigned)a.cols) + 1u : 0u;
}

// pixels per lane the vector loads allow for these maps (4, 2 or 1)
static int icp_max_px(const IcpArgs& a, int px) {
    auto ok = [&](int k) {
        const uintptr_t m = (uintptr_t)k * 4 - 1;
        return (a.cols % k == 0) && (a.vmap_curr.stride % k == 0) && (a.nmap_curr.stride % k == 0) &&
               ((uintptr_t)a.vmap_curr.base & m) == 0 && ((uintptr_t)a.nmap_curr.base & m) == 0 &&
               (!a.err_map || (((uintptr_t)a.err_map & m) == 0 && a.err_stride % k == 0));
    };
    while (px > 1 && !ok(px)) px /= 2;
    return px;
}
// can ONE pass of kMaxIcpGrid workgroups cover the image?  (larger ones: the multi-pass instantiation)
static bool icp2_fits(const IcpArgs& a, int block, int px) {
    const long long n = (long long)a.cols * a.rows;
    return n * a.cols < (1ll << 32) && (long long)kMaxIcpGrid * block * px >= n;
}

// Launches the ICP producer (icp_kernel2, gathering from a.prev_packed when it is set) on q and returns the number of partial
// records it writes.  Two pixels per lane where the maps allow, 256 lanes: every geometry of icp_kernel2 lands within 0.2 us
// at 640x480 on MI355X (the launch is bound by its two memory round trips and the dispatch floor, no longer by instruction
// issue), so one serves all levels.  Images too large for one pass of kMaxIcpGrid workgroups: those walk the image, one
// pixel per lane and pass.
template <int MODE>
static int launch_icp(Enqueuer& q, OdomState* st, IcpArgs a, float* partials) {
    icp_args_derive(a);
    const int px = icp_max_px(a, 2);
    const bool packed = a.prev_packed != nullptr;
    if (!icp2_fits(a, 256, px)) {
        q.launch(packed ? icp_kernel2<1, 1, 256, true, MODE, true> : icp_kernel2<1, 1, 256, false, MODE, true>,
                 dim3(kMaxIcpGrid), dim3(256), st, a, partials);
        return kMaxIcpGrid;
    }
    const int grid = (a.cols * a.rows + 256 * px - 1) / (256 * px);
    if (px == 2)
        q.launch(packed ? icp_kernel2<2, 1, 256, true, MODE> : icp_kernel2<2, 1, 256, false, MODE>, dim3(grid), dim3(256), st, a,
                 partials);
    else
        q.launch(packed ? icp_kernel2<1, 1, 256, true, MODE> : icp_kernel2<1, 1, 256, false, MODE>, dim3(grid), dim3(256), st, a,
                 partials);
    return grid;
}

static void unpack_se3_host(const float* tot, float* A, float* b) {  // reduce.cu:458-472
    int shift = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 7; ++j) {
            const float v = tot[shift++];
            if (j == 6)
                b[i] = v;
            else
                A[j * 6 + i] = A[i * 6 + j] = v;
        }
}

// ---------------------------------------------------------------------------------------------
// stand-alone device entry points (cudafuncs.cuh)
// ---------------------------------------------------------------------------------------------
extern "C" int mmf_icp_step(mmf_ctx* c, const float Rcurr[9], const float tcurr[3], const float* vmap_curr,
                            size_t vmap_curr_step, const float* nmap_curr, size_t nmap_curr_step,
                            const float Rprev_inv[9], const float tprev[3], const mmf_camera* intr,
                            const float* vmap_g_prev, size_t vmap_g_prev_step, const float* nmap_g_prev,
                            size_t nmap_g_prev_step, float dist_thres, float angle_thres, int cols, int rows,
                            float* A_host, float* b_host, float* residual_host, float* err_map_dev,
                            size_t err_map_step) {
    MMF_REQUIRE(c && Rcurr && tcurr && Rprev_inv && tprev && intr, "mmf_icp_step: null argument");
    MMF_REQUIRE(vmap_curr && nmap_curr && vmap_g_prev && nmap_g_prev, "mmf_icp_step: null map");
    MMF_REQUIRE(A_host && b_host && residual_host, "mmf_icp_step: null output");
    MMF_REQUIRE(cols > 0 && rows > 0 && (long long)cols * rows * 3 < (1ll << 31), "mmf_icp_step: bad size");
    MMF_HIP_TRY(hipSetDevice(c->device));
    OdomState* h = c->host_state;
    std::memcpy(h->Rcurr, Rcurr, sizeof(float) * 9);
    std::memcpy(h->tcurr, tcurr, sizeof(float) * 3);
    std::memcpy(h->Rprev_inv, Rprev_inv, sizeof(float) * 9);
    std::memcpy(h->tprev, tprev, sizeof(float) * 3);
    // Rprev .. tcurr are contiguous at the head of the struct
    MMF_HIP_TRY(hipMemcpyAsync(c->scratch_state, h, offsetof(OdomState, resultRt), hipMemcpyHostToDevice, c->stream));
    IcpArgs a;
    a.vmap_curr = MapView{vmap_curr, stride_elems(vmap_curr_step, cols, 4)};
    a.nmap_curr = MapView{nmap_curr, stride_elems(nmap_curr_step, cols, 4)};
    a.vmap_g_prev = MapView{vmap_g_prev, stride_elems(vmap_g_prev_step, cols, 4)};
    a.nmap_g_prev = MapView{nmap_g_prev, stride_elems(nmap_g_prev_step, cols, 4)};
    a.intr = LevelIntr{intr->fx, intr->fy, intr->cx, intr->cy};
    a.dist_thres = dist_thres;
    a.angle_thres = angle_thres;
    a.cols = cols;
    a.rows = rows;
    a.prev_packed = nullptr;
    a.err_map = err_map_dev;
    a.err_stride = stride_elems(err_map_step, cols, 4);
    Enqueuer q(c->stream);
    const int records = launch_icp<FINISH_RAW>(q, c->scratch_state, a, c->partials_icp);
    q.launch(icp_finish_kernel<FINISH_RAW>, dim3(1), dim3(256), c->scratch_state, c->partials_icp, (unsigned)records, a.intr);
    MMF_HIP_TRY(q.flush());
    float tot[32];
    MMF_HIP_TRY(hipMemcpyAsync(tot, c->scratch_state->out_f, sizeof(float) * 32, hipMemcpyDeviceToHost, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    unpack_se3_host(tot, A_host, b_host);
    residual_host[0] = tot[27];
    residual_host[1] = tot[28];
    return MMF_OK;
}

static RgbResidualArgs make_residual_args(float min_scale, const int16_t* dIdx, size_t dIdx_step, const int16_t* dIdy,
                                          size_t dIdy_step, const float* last_depth, size_t ld_step,
                                          const float* next_depth, size_t nd_step, const uint8_t* last_image,
                                          size_t li_step, const uint8_t* next_image, size_t ni_step,
                                          mmf_dataterm* corres, float max_depth_delta, int cols, int rows,
                                          float* err_map, size_t err_step) {
    RgbResidualArgs a;
    a.min_scale = min_scale;
    a.max_depth_delta = max_depth_delta;
    a.dIdx = dIdx;
    a.dIdy = dIdy;
    a.d_stride = stride_elems(dIdx_step, cols, 2);
    (void)dIdy_step;
    a.last_depth = last_depth;
    a.next_depth = next_depth;
    a.ld_stride = stride_elems(ld_step, cols, 4);
    a.nd_stride = stride_elems(nd_step, cols, 4);
    a.last_image = last_image;
    a.next_image = next_image;
    a.li_stride = stride_elems(li_step, cols, 1);
    a.ni_stride = stride_elems(ni_step, cols, 1);
    a.corres = corres;
    a.cols = cols;
    a.rows = rows;
    a.cols_magic = (unsigned)((1ull << 32) / (unsigned)cols) + 1u;
    a.err_map = err_map;
    a.err_stride = stride_elems(err_step, cols, 4);
    a.intr = LevelIntr{0, 0, 0, 0};
    a.extent = nullptr, a.extent_gen = 0u, a.extent_level = 0;
    return a;
}

// 4 pixels per lane needs whole 4-pixel groups per row and 16-byte aligned rows of every image
static bool residual_vec4_ok(const RgbResidualArgs& a) {
    auto al = [](const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; };
    return a.cols % 4 == 0 && a.ni_stride % 4 == 0 && a.d_stride % 4 == 0 && a.nd_stride % 4 == 0 &&
           al(a.next_image, 4) && al(a.dIdx, 8) && al(a.dIdy, 8) && al(a.next_depth, 16) &&
           (!a.err_map || (al(a.err_map, 16) && a.err_stride % 4 == 0)) && al(a.corres, 16) &&
           (long long)a.cols * a.rows * a.cols < (1ll << 32);  // index / cols by multiply-high
}

extern "C" int mmf_compute_rgb_residual(mmf_ctx* c, float min_scale, const int16_t* dIdx, size_t dIdx_step,
                                        const int16_t* dIdy, size_t dIdy_step, const float* last_depth,
                                        size_t last_depth_step, const float* next_depth, size_t next_depth_step,
                                        const uint8_t* last_image, size_t last_image_step, const uint8_t* next_image,
                                        size_t next_image_step, mmf_dataterm* corres_dev, float max_depth_delta,
                                        const float kt[3], const float krkinv[9], int cols, int rows,
                                        int* sigma_sum_host, int* count_host, float* err_map_dev,
                                        size_t err_map_step) {
    MMF_REQUIRE(c && dIdx && dIdy && last_depth && next_depth && last_image && next_image && corres_dev && kt &&
                    krkinv && sigma_sum_host && count_host,
                "mmf_compute_rgb_residual: null argument");
    MMF_REQUIRE(cols > 0 && rows > 0 && cols < 32768 && rows < 32768, "mmf_compute_rgb_residual: bad size");
    MMF_REQUIRE(dIdx_step == dIdy_step, "mmf_compute_rgb_residual: dIdx/dIdy steps differ");
    MMF_REQUIRE(aligned16(corres_dev), "mmf_compute_rgb_residual: corres must be 16-byte aligned");
    MMF_HIP_TRY(hipSetDevice(c->device));
    OdomState* h = c->host_state;
    std::memcpy(h->krkinv, krkinv, sizeof(float) * 9);
    std::memcpy(h->kt, kt, sizeof(float) * 3);
    MMF_HIP_TRY(hipMemcpyAsync(c->scratch_state->krkinv, h->krkinv, sizeof(float) * 12, hipMemcpyHostToDevice, c->stream));
    RgbResidualArgs a = make_residual_args(min_scale, dIdx, dIdx_step, dIdy, dIdy_step, last_depth, last_depth_step,
                                           next_depth, next_depth_step, last_image, last_image_step, next_image,
                                           next_image_step, corres_dev, max_depth_delta, cols, rows, err_map_dev,
                                           err_map_step);
    const bool vec4 = residual_vec4_ok(a);
    const int grid = reduce_grid(cols * rows, vec4 ? kBlock * 4 : kBlock);
    if (vec4)
        hipLaunchKernelGGL((rgb_residual_kernel<FINISH_RAW, 4>), dim3(grid), dim3(kBlock), 0, c->stream,
                           c->scratch_state, a, c->partials_res);
    else
        hipLaunchKernelGGL((rgb_residual_kernel<FINISH_RAW, 1>), dim3(grid), dim3(kBlock), 0, c->stream,
                           c->scratch_state, a, c->partials_res);
    MMF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(residual_finish_kernel, dim3(1), dim3(256), 0, c->stream, c->scratch_state, c->partials_res,
                       (unsigned)grid);
    MMF_HIP_TRY(hipGetLastError());
    int tot[2];
    MMF_HIP_TRY(hipMemcpyAsync(tot, c->scratch_state->out_i, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    *count_host = tot[0];
    *sigma_sum_host = tot[1];
    return MMF_OK;
}

extern "C" int mmf_rgb_step(mmf_ctx* c, const mmf_dataterm* corres_dev, float sigma, const float* cloud_dev, float fx,
                            float fy, const int16_t* dIdx, size_t dIdx_step, const int16_t* dIdy, size_t dIdy_step,
                            float sobel_scale, int cols, int rows, float* A_host, float* b_host) {
    MMF_REQUIRE(c && corres_dev && cloud_dev && dIdx && dIdy && A_host && b_host, "mmf_rgb_step: null argument");
    MMF_REQUIRE(cols > 0 && rows > 0, "mmf_rgb_step: bad size");
    MMF_REQUIRE(dIdx_step == dIdy_step, "mmf_rgb_step: dIdx/dIdy steps differ");
    MMF_REQUIRE(aligned16(corres_dev), "mmf_rgb_step: corres must be 16-byte aligned");
    MMF_HIP_TRY(hipSetDevice(c->device));
    c->host_state->sigmaVal = sigma;
    MMF_HIP_TRY(hipMemcpyAsync(&c->scratch_state->sigmaVal, &c->host_state->sigmaVal, sizeof(float),
                               hipMemcpyHostToDevice, c->stream));
    RgbStepArgs a;
    a.next_level = 0;
    a.final_step = 0;
    a.extent = nullptr, a.extent_gen = 0u, a.extent_level = 0;
    a.cols_magic = 0;
    a.residual_partials = nullptr;
    a.residual_records = 0;
    a.icp_partials = nullptr;
    a.icp_records = 0;
    a.corres = corres_dev;
    a.cloud = cloud_dev, a.cloud4 = nullptr;
    a.fx = fx;
    a.fy = fy;
    a.dIdx = dIdx;
    a.dIdy = dIdy;
    a.d_stride = stride_elems(dIdx_step, cols, 2);
    a.sobel_scale = sobel_scale;
    a.cols = cols;
    a.rows = rows;
    a.intr = LevelIntr{0, 0, 0, 0};
    if ((cols * rows) % 4 == 0) {
        const int grid = reduce_grid(cols * rows, kBlock * 4);
        hipLaunchKernelGGL((rgb_step_kernel<FINISH_RAW, 4>), dim3(grid), dim3(kBlock), 0, c->stream, c->scratch_state,
                           a, c->partials_f, c->ticket, BatchDelta{}, ChainGeom{});
    } else {
        const int grid = reduce_grid(cols * rows, kBlock);
        hipLaunchKernelGGL((rgb_step_kernel<FINISH_RAW, 1>), dim3(grid), dim3(kBlock), 0, c->stream, c->scratch_state,
                           a, c->partials_f, c->ticket, BatchDelta{}, ChainGeom{});
    }
    MMF_HIP_TRY(hipGetLastError());
    float tot[32];
    MMF_HIP_TRY(hipMemcpyAsync(tot, c->scratch_state->out_f, sizeof(float) * 32, hipMemcpyDeviceToHost, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    unpack_se3_host(tot, A_host, b_host);
    return MMF_OK;
}

extern "C" int mmf_so3_step(mmf_ctx* c, const uint8_t* last_image, size_t last_image_step, const uint8_t* next_image,
                            size_t next_image_step, const float image_basis[9], const float kinv[9],
                            const float krlr[9], int cols, int rows, float* A_host, float* b_host,
                            float* residual_host) {
    MMF_REQUIRE(c && last_image && next_image && image_basis && kinv && krlr && A_host && b_host && residual_host,
                "mmf_so3_step: null argument");
    MMF_REQUIRE(cols > 2 && rows > 2, "mmf_so3_step: bad size");
    MMF_HIP_TRY(hipSetDevice(c->device));
    OdomState* h = c->host_state;
    std::memcpy(h->imageBasis, image_basis, sizeof(float) * 9);
    std::memcpy(h->kinv, kinv, sizeof(float) * 9);
    std::memcpy(h->krlr, krlr, sizeof(float) * 9);
    MMF_HIP_TRY(hipMemcpyAsync(c->scratch_state->imageBasis, h->imageBasis, sizeof(float) * 27, hipMemcpyHostToDevice,
                               c->stream));
    So3Args a;
    a.last_image = last_image;
    a.next_image = next_image;
    a.l_stride = stride_elems(last_image_step, cols, 1);
    a.n_stride = stride_elems(next_image_step, cols, 1);
    a.cols = cols;
    a.rows = rows;
    a.cols_magic = (long long)cols * rows * cols < (1ll << 32) ? (unsigned)((1ull << 32) / (unsigned)cols) + 1u : 0u;
    a.intr = LevelIntr{0, 0, 0, 0};
    const int grid = reduce_grid(cols * rows, kBlock);
    hipLaunchKernelGGL((so3_kernel<FINISH_RAW>), dim3(grid), dim3(kBlock), 0, c->stream, c->scratch_state, a,
                       c->partials_f, c->ticket);
    MMF_HIP_TRY(hipGetLastError());
    float tot[32];
    MMF_HIP_TRY(hipMemcpyAsync(tot, c->scratch_state->out_f, sizeof(float) * 32, hipMemcpyDeviceToHost, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    int shift = 0;  // reduce.cu:1135-1149
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 4; ++j) {
            const float v = tot[shift++];
            if (j == 3)
                b_host[i] = v;
            else
                A_host[j * 3 + i] = A_host[i * 3 + j] = v;
        }
    residual_host[0] = tot[9];
    residual_host[1] = tot[10];
    return MMF_OK;
}

// ---- map / pyramid entry points ---------------------------------------------------------------
static int launch_create_vmap(mmf_ctx* c, LevelIntr in, const float* depth, int d_stride, int cols, int rows,
                              float* vmap, int v_stride, float cutoff) {
    hipLaunchKernelGGL(create_vmap_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, depth, d_stride, cols,
                       rows, vmap, v_stride, 1.f / in.fx, 1.f / in.fy, in.cx, in.cy, cutoff);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_create_vmap(mmf_ctx* c, const mmf_camera* intr, const float* depth, size_t depth_step, int cols,
                               int rows, float* vmap, size_t vmap_step, float depth_cutoff) {
    MMF_REQUIRE(c && intr && depth && vmap && cols > 0 && rows > 0, "mmf_create_vmap: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_create_vmap(c, LevelIntr{intr->fx, intr->fy, intr->cx, intr->cy}, depth,
                              stride_elems(depth_step, cols, 4), cols, rows, vmap, stride_elems(vmap_step, cols, 4),
                              depth_cutoff);
}

static int launch_create_nmap(mmf_ctx* c, const float* vmap, int v_stride, int cols, int rows, float* nmap,
                              int n_stride) {
    hipLaunchKernelGGL(create_nmap_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, rows, cols, vmap,
                       v_stride, nmap, n_stride);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_create_nmap(mmf_ctx* c, const float* vmap, size_t vmap_step, int cols, int rows, float* nmap,
                               size_t nmap_step) {
    MMF_REQUIRE(c && vmap && nmap && cols > 0 && rows > 0, "mmf_create_nmap: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_create_nmap(c, vmap, stride_elems(vmap_step, cols, 4), cols, rows, nmap,
                              stride_elems(nmap_step, cols, 4));
}

static int launch_transform(mmf_ctx* c, const float* vs, const float* ns, int s_stride, int cols, int rows,
                            const float R[9], const float t[3], float* vd, float* nd, int d_stride) {
    m33 Rm;
    std::memcpy(Rm.m, R, sizeof(float) * 9);
    hipLaunchKernelGGL(transform_maps_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, rows, cols, vs, ns,
                       s_stride, Rm, f3{t[0], t[1], t[2]}, vd, nd, d_stride);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_transform_maps(mmf_ctx* c, const float* vmap_src, const float* nmap_src, size_t src_step, int cols,
                                  int rows, const float R[9], const float t[3], float* vmap_dst, float* nmap_dst,
                                  size_t dst_step) {
    MMF_REQUIRE(c && vmap_src && nmap_src && R && t && vmap_dst && nmap_dst && cols > 0 && rows > 0,
                "mmf_transform_maps: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_transform(c, vmap_src, nmap_src, stride_elems(src_step, cols, 4), cols, rows, R, t, vmap_dst,
                            nmap_dst, stride_elems(dst_step, cols, 4));
}

static int launch_copy_maps(mmf_ctx* c, const float* v_rgba, const float* n_rgba, int cols, int rows, float* vd,
                            float* nd, int d_stride) {
    hipLaunchKernelGGL(copy_maps_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, rows, cols,
                       reinterpret_cast<const float4*>(v_rgba), reinterpret_cast<const float4*>(n_rgba), vd, nd,
                       d_stride);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_copy_maps(mmf_ctx* c, const float* vmap_rgba, const float* nmap_rgba, int cols, int rows,
                             float* vmap_dst, float* nmap_dst, size_t dst_step) {
    MMF_REQUIRE(c && vmap_rgba && nmap_rgba && vmap_dst && nmap_dst && cols > 0 && rows > 0,
                "mmf_copy_maps: bad argument");
    MMF_REQUIRE(aligned16(vmap_rgba) && aligned16(nmap_rgba), "mmf_copy_maps: RGBA images must be 16-byte aligned");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_copy_maps(c, vmap_rgba, nmap_rgba, cols, rows, vmap_dst, nmap_dst, stride_elems(dst_step, cols, 4));
}

template <bool NORMALIZE>
static int launch_resize(mmf_ctx* c, const float* in, int i_stride, int in_cols, int in_rows, float* out,
                         int o_stride) {
    const int dcols = in_cols / 2, drows = in_rows / 2;
    hipLaunchKernelGGL((resize_map_kernel<NORMALIZE>), tile_grid(dcols, drows), tile_block(), 0, c->stream, drows,
                       dcols, in_rows, in, i_stride, out, o_stride);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_resize_vmap(mmf_ctx* c, const float* in, size_t in_step, int in_cols, int in_rows, float* out,
                               size_t out_step) {
    MMF_REQUIRE(c && in && out && in_cols > 1 && in_rows > 1, "mmf_resize_vmap: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_resize<false>(c, in, stride_elems(in_step, in_cols, 4), in_cols, in_rows, out,
                                stride_elems(out_step, in_cols / 2, 4));
}

extern "C" int mmf_resize_nmap(mmf_ctx* c, const float* in, size_t in_step, int in_cols, int in_rows, float* out,
                               size_t out_step) {
    MMF_REQUIRE(c && in && out && in_cols > 1 && in_rows > 1, "mmf_resize_nmap: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_resize<true>(c, in, stride_elems(in_step, in_cols, 4), in_cols, in_rows, out,
                               stride_elems(out_step, in_cols / 2, 4));
}

static int launch_intensity(mmf_ctx* c, const uint8_t* img, int i_stride, int channels, int cols, int rows,
                            uint8_t* dst, int d_stride) {
    hipLaunchKernelGGL(image_to_intensity_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, img, i_stride,
                       channels, cols, rows, dst, d_stride);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_image_bgr_to_intensity(mmf_ctx* c, const uint8_t* img, size_t img_step, int channels, int cols,
                                          int rows, uint8_t* dst, size_t dst_step) {
    MMF_REQUIRE(c && img && dst && cols > 0 && rows > 0, "mmf_image_bgr_to_intensity: bad argument");
    MMF_REQUIRE(channels == 3 || channels == 4, "mmf_image_bgr_to_intensity: channels must be 3 or 4");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_intensity(c, img, img_step ? (int)img_step : cols * channels, channels, cols, rows, dst,
                            stride_elems(dst_step, cols, 1));
}

static int launch_vertices_to_depth(mmf_ctx* c, const float* vmap_rgba, int cols, int rows, float cutoff, float* dst,
                                    int d_stride) {
    hipLaunchKernelGGL(vertices_to_depth_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream,
                       reinterpret_cast<const float4*>(vmap_rgba), cols, rows, dst, d_stride, cutoff);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_vertices_to_depth(mmf_ctx* c, const float* vmap_rgba, int cols, int rows, float cutoff, float* dst,
                                     size_t dst_step) {
    MMF_REQUIRE(c && vmap_rgba && dst && cols > 0 && rows > 0, "mmf_vertices_to_depth: bad argument");
    MMF_REQUIRE(aligned16(vmap_rgba), "mmf_vertices_to_depth: RGBA image must be 16-byte aligned");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_vertices_to_depth(c, vmap_rgba, cols, rows, cutoff, dst, stride_elems(dst_step, cols, 4));
}

static int launch_project(mmf_ctx* c, const float* depth, int d_stride, int cols, int rows, LevelIntr in,
                          float* cloud, float* cloud4 = nullptr) {
    hipLaunchKernelGGL(project_points_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, depth, d_stride, cols,
                       rows, cloud, 1.0f / in.fx, 1.0f / in.fy, in.cx, in.cy, reinterpret_cast<float4*>(cloud4));
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_project_to_point_cloud(mmf_ctx* c, const float* depth, size_t depth_step, int cols, int rows,
                                          const mmf_camera* intr, int level, float* cloud) {
    MMF_REQUIRE(c && depth && intr && cloud && cols > 0 && rows > 0 && level >= 0 && level < 16,
                "mmf_project_to_point_cloud: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_project(c, depth, stride_elems(depth_step, cols, 4), cols, rows,
                          level_intr(intr->fx, intr->fy, intr->cx, intr->cy, level), cloud);
}

static int launch_pyrdown_f(mmf_ctx* c, const float* src, int s_stride, int scols, int srows, float* dst,
                            int d_stride) {
    const int dcols = scols / 2, drows = srows / 2;
    hipLaunchKernelGGL(pyrdown_gauss_f_kernel, tile_grid(dcols, drows), tile_block(), 0, c->stream, src, s_stride,
                       scols, srows, dst, d_stride, dcols, drows);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_pyr_down_gauss_f(mmf_ctx* c, const float* src, size_t src_step, int src_cols, int src_rows,
                                    float* dst, size_t dst_step) {
    MMF_REQUIRE(c && src && dst && src_cols > 1 && src_rows > 1, "mmf_pyr_down_gauss_f: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_pyrdown_f(c, src, stride_elems(src_step, src_cols, 4), src_cols, src_rows, dst,
                            stride_elems(dst_step, src_cols / 2, 4));
}

static int launch_pyrdown_u8(mmf_ctx* c, const uint8_t* src, int s_stride, int scols, int srows, uint8_t* dst,
                             int d_stride) {
    const int dcols = scols / 2, drows = srows / 2;
    hipLaunchKernelGGL(pyrdown_uchar_gauss_kernel, tile_grid(dcols, drows), tile_block(), 0, c->stream, src, s_stride,
                       scols, srows, dst, d_stride, dcols, drows);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_pyr_down_uchar_gauss(mmf_ctx* c, const uint8_t* src, size_t src_step, int src_cols, int src_rows,
                                        uint8_t* dst, size_t dst_step) {
    MMF_REQUIRE(c && src && dst && src_cols > 1 && src_rows > 1, "mmf_pyr_down_uchar_gauss: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_pyrdown_u8(c, src, stride_elems(src_step, src_cols, 1), src_cols, src_rows, dst,
                             stride_elems(dst_step, src_cols / 2, 1));
}

static int launch_derivative(mmf_ctx* c, const uint8_t* src, int s_stride, int cols, int rows, int16_t* dx,
                             int dx_stride, int16_t* dy, int dy_stride) {
    hipLaunchKernelGGL(derivative_kernel, tile_grid(cols, rows), tile_block(), 0, c->stream, src, s_stride, cols, rows,
                       dx, dx_stride, dy, dy_stride);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_compute_derivative_images(mmf_ctx* c, const uint8_t* src, size_t src_step, int cols, int rows,
                                             int16_t* dx, size_t dx_step, int16_t* dy, size_t dy_step) {
    MMF_REQUIRE(c && src && dx && dy && cols > 0 && rows > 0, "mmf_compute_derivative_images: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    return launch_derivative(c, src, stride_elems(src_step, cols, 1), cols, rows, dx, stride_elems(dx_step, cols, 2),
                             dy, stride_elems(dy_step, cols, 2));
}

// ---------------------------------------------------------------------------------------------
// RGBDOdometry object
// ---------------------------------------------------------------------------------------------
constexpr int kMaxTimedLaunches = 48;  // 19 iterations x (producer + step)

struct mmf_odom {
    mmf_ctx* ctx = nullptr;
    int width = 0, height = 0;
    float cx = 0, cy = 0, fx = 0, fy = 0;
    float dist_thres = 0, angle_thres = 0;
    float sobel_scale = 0.125f;         // RGBDOdometry.cpp:31-32
    float max_depth_delta_rgb = 0.07f;  // :33
    float max_depth_rgb = 6.0f;         // :34
    float min_grad[MMF_NUM_PYRS] = {5, 3, 1};  // :103-105

    // one slab of HBM; every buffer below points into it
    void* slab = nullptr;
    size_t slab_bytes = 0;
    float *vmaps_tmp = nullptr, *nmaps_tmp = nullptr;
    float *vmaps_g_prev[MMF_NUM_PYRS], *nmaps_g_prev[MMF_NUM_PYRS];
    float *vmaps_curr[MMF_NUM_PYRS], *nmaps_curr[MMF_NUM_PYRS];
    float *last_depth[MMF_NUM_PYRS], *next_depth[MMF_NUM_PYRS], *depth_pyr[MMF_NUM_PYRS];
    uint8_t *last_image[MMF_NUM_PYRS], *next_image[MMF_NUM_PYRS], *last_next_image[MMF_NUM_PYRS];
    int16_t *dIdx[MMF_NUM_PYRS], *dIdy[MMF_NUM_PYRS];
    float* cloud[MMF_NUM_PYRS];
    float* cloud4[MMF_NUM_PYRS];  // the same points as {X, Y, Z, 1/Z} (16-byte records: what gn_iter_kernel gathers)
    mmf_dataterm* corres[MMF_NUM_PYRS];
    float* prev_packed[MMF_NUM_PYRS];  // model vertex + normal, pixel interleaved 24-byte records (the ICP gather side)
    // reduction scratch of the Gauss-Newton loop and the two error images, inside the slab: every odometry object has
    // its own (concurrent chains on different streams, or one batched chain addressing model m at slab(m) - slab(0))
    float* gn_partials_f = nullptr;
    float* gn_partials_icp = nullptr;
    int2* gn_partials_res = nullptr;
    unsigned* gn_ticket = nullptr;
    float *icp_err = nullptr, *rgb_err = nullptr;  // Model::icpError / rgbError (R32F), written on the last level-0 iteration
    // extent.hpp: three boxes of four words (extent_of_level), noted by the model-side preparation's depth jobs when the owner asks for it (extent_gen != 0:
    // the number of the frame they were noted for), read by the two-launch chain's passes
    unsigned long long* extent = nullptr;
    unsigned extent_gen = 0;
    // prep_batch.hpp (PrepJob::rect_*): the box an object model's model-side preparation last found its prediction non-zero
    // in (device: two slots of four ints, the preparation's number & 1), and whether it describes the buffers (any
    // preparation of the whole frame leaves it unknown)
    int* prep_box = nullptr;
    unsigned prep_gen = 0;
    bool prep_box_known = false;
    unsigned sensor_gen = 0;     // number of the last sensor-side depth preparation (its smallest depth: extent words 18 / 19)
    float sensor_cutoff = 0.f;   // ... and the depth cut-off its vertex maps were made with
    // an OBJECT model (set by the orchestrator): the two-launch chain walks its images with a quarter of the workgroups
    // (track_kernels.hpp: ChainGeom), batched or alone
    bool sparse = false;
    // ... and the one-launch chain by its extents with a fraction of the workgroups (gn_fused.hpp: gn_iter_mixed_kernel), as
    // many as the box of its own depth needed in its LAST chain plus a quarter (OdomState::gn_need; 0: no chain yet)
    int gn_need[MMF_NUM_PYRS] = {0, 0, 0};
    int last_gn_fault = 0;          // OdomState::gn_fault of the last result picked up (odom_finish_tracking)
    GnTruncated* gn_truncated = nullptr;  // test hook (mmf_debug_gn_truncate): made by the first truncated chain
    bool walked_by_extent = false;  // the last chain enqueued walked this model by its extents (gn_iter_mixed_kernel)
    bool two_launch_once = false;  // the next chain this odometry leads is the two-launch chain (a frame tracked again)
    OdomState* state = nullptr;  // device
    OdomState* host_result = nullptr;  // pinned, device visible: odom_publish_kernel writes it, the host polls publish_seq
    OdomState* host_result_dev = nullptr;
    unsigned publish_seq = 0;          // sequence number of the last chain enqueued
    bool defer_publish = false;        // set by the orchestrator: the hand-over to the host + the fusion weight ride on the
    FrameRider rider;                  // frame's next resolve launch (frame_rider.hpp) instead of ending the chain
    bool have_tmp = false;  // vmaps_tmp filled by an initICP* call (ordering contract)
    // The reference COPIES its inputs at each init* call (RGBDOdometry.cpp:125,130; Model.cpp:359-388).
    // An owner that guarantees the images stay untouched until getIncrementalTransformation returns
    // (the native orchestrator: they live in its model / frame slabs) sets alias_inputs, and the three
    // device-to-device copies per frame (2 x 4.9 MB + 1.2 MB at 640x480) become pointer assignments.
    bool alias_inputs = false;
    const float *vtmp = nullptr, *ntmp = nullptr;  // what populateRGBDData / copyMaps read: own copy or alias
    const float* depth_l0 = nullptr;               // level 0 of the depth pyramid: own copy or alias
    // set by the batched model-side preparation (prep_collect_model): gradients and point clouds are already built, and next_depth is
    // last_depth (both come from the same prediction, RGBDOdometry.cpp:179 -- see odom_populate_rgbd)
    bool prep_batched = false;
    bool so3_prefetched = false;  // this frame's SO3 pre-alignment already ran (odom_prefetch_so3)
    const OdomState* so3_stage = nullptr;  // ... in this state (nullptr: in this odometry's own)
    // The gradient images are double buffered: the batched image-side preparation writes grad_w_*, the chain reads dIdx /
    // dIdy, and odom_adopt_gradients swaps the two when a prepared frame becomes the frame that is tracked -- so that the
    // NEXT frame's image side can be prepared while this frame's chain still reads its gradients.
    int16_t *grad_w_dx[MMF_NUM_PYRS], *grad_w_dy[MMF_NUM_PYRS];
    bool grad_pending = false;  // grad_w_* hold a prepared frame's gradients
    // The one-launch-per-iteration chain has a barrier inside every launch: its workgroups must all become resident.  Two
    // such launches from different streams can each hold part of the GPU and wait for the rest forever, so an owner that
    // keeps several chains in flight at once (the orchestrator without batching) clears this and gets the two-launch chain.
    bool exclusive_chain = true;
    // the beginning of the next tracking already ran, with these arguments, on the last launch of the preparation enqueued ahead
    // of it (track_kernels.hpp: prep_batch_begin_kernel); begin_spec_ok: the caller vouches that nothing touched the state since
    bool begin_spec_valid = false, begin_spec_ok = false;
    BeginArgs begin_spec;
    bool retry_so3_prefetched = false;  // what the last odom_enqueue_tracking consumed (a chain that gives up is enqueued again)
    const OdomState* retry_so3_stage = nullptr;
    bool pending_icp = false, pending_so3 = false;  // mode of the tracking call that is in flight (enqueue -> finish)
    hipStream_t track_stream = nullptr;             // the stream that call's chain runs on (the batch leader's)
    mmf_odom* result_of = nullptr;                  // the odometry (batch leader) whose chain publishes this one's result
    // measurement mode (mmf_odom_enable_timing): every producer / rgb_step launch of a tracking call carries its own
    // start / stop events (hipExtLaunchKernelGGL: the dispatch's own begin / end timestamps), the whole chain two more
    int timing = 0;  // 1: chain events only; 2: also every kernel of the chain
    hipEvent_t ev_kernel[2 * kMaxTimedLaunches] = {};
    int timed_kind[kMaxTimedLaunches] = {};  // level * 2 + (0 producer | 1 rgb_step)
    int n_timed = 0;
    hipEvent_t ev_chain[2] = {};
    mmf_odom_timing timing_acc;
    mmf_odom_stats stats;
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

extern "C" int mmf_odom_create(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy,
                               float dist_thresh, float angle_thresh, mmf_odom** out) {
    MMF_REQUIRE(c && out, "mmf_odom_create: null argument");
    MMF_REQUIRE(width >= 32 && height >= 32 && width % 4 == 0 && height % 4 == 0 && width < 32768 && height < 32768,
                "mmf_odom_create: width/height must be multiples of 4, >= 32");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_odom* o = new (std::nothrow) mmf_odom();
    MMF_REQUIRE(o != nullptr, "mmf_odom_create: out of host memory");
    o->ctx = c;
    o->width = width;
    o->height = height;
    o->cx = cx;
    o->cy = cy;
    o->fx = fx;
    o->fy = fy;
    o->dist_thres = dist_thresh;
    o->angle_thres = angle_thresh;
    std::memset(&o->stats, 0, sizeof(o->stats));
    std::memset(&o->timing_acc, 0, sizeof(o->timing_acc));
    o->stats.lastICPCount = o->stats.lastRGBCount = o->stats.lastSO3Count = (float)(width * height);  // :24-28

    // carve every pyramid buffer out of one allocation, each 256-byte aligned
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    const size_t n0 = (size_t)width * height;
    size_t o_vt = carve(4 * n0 * 4), o_nt = carve(4 * n0 * 4);
    size_t o_vgp[3], o_ngp[3], o_vc[3], o_nc[3], o_ld[3], o_nd[3], o_dp[3], o_li[3], o_ni[3], o_lni[3], o_dx[3],
        o_dy[3], o_dx2[3], o_dy2[3], o_cl[3], o_c4[3], o_co[3], o_pp[3];
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {
        const size_t n = (size_t)(width >> i) * (height >> i);
        o_vgp[i] = carve(3 * n * 4);
        o_ngp[i] = carve(3 * n * 4);
        o_vc[i] = carve(3 * n * 4);
        o_nc[i] = carve(3 * n * 4);
        o_ld[i] = carve(n * 4);
        o_nd[i] = carve(n * 4);
        o_dp[i] = carve(n * 4);
        o_li[i] = carve(n);
        o_ni[i] = carve(n);
        o_lni[i] = carve(n);
        o_dx[i] = carve(n * 2);
        o_dy[i] = carve(n * 2);
        o_dx2[i] = carve(n * 2);
        o_dy2[i] = carve(n * 2);
        o_cl[i] = carve(3 * n * 4);
        o_c4[i] = carve(4 * n * 4);
        o_co[i] = carve(n * sizeof(mmf_dataterm));
        o_pp[i] = carve(n * 6 * sizeof(float));
    }
    size_t o_state = carve(sizeof(OdomState));
    const size_t o_pf = carve(sizeof(float) * kMaxGrid * kPartialStride), o_pi = carve(sizeof(float) * kMaxIcpGrid * kPartialStride),
                 o_pr = carve(sizeof(int2) * kMaxGrid), o_tk = carve(sizeof(unsigned) * kTicketWords), o_ei = carve(n0 * 4),
                 o_er = carve(n0 * 4), o_ex = carve(kExtentWords * sizeof(unsigned long long) + 64);  // (+ prep_box)
    o->slab_bytes = off;
    hipError_t e = hipMalloc(&o->slab, o->slab_bytes);
    if (e != hipSuccess) {
        delete o;
        return fail(MMF_ERR_HIP, std::string("mmf_odom_create: hipMalloc: ") + hipGetErrorString(e));
    }
    MMF_HIP_TRY(hipMemsetAsync(o->slab, 0, o->slab_bytes, c->stream));
    char* base = static_cast<char*>(o->slab);
    o->vmaps_tmp = (float*)(base + o_vt);
    o->nmaps_tmp = (float*)(base + o_nt);
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {
        o->vmaps_g_prev[i] = (float*)(base + o_vgp[i]);
        o->nmaps_g_prev[i] = (float*)(base + o_ngp[i]);
        o->vmaps_curr[i] = (float*)(base + o_vc[i]);
        o->nmaps_curr[i] = (float*)(base + o_nc[i]);
        o->last_depth[i] = (float*)(base + o_ld[i]);
        o->next_depth[i] = (float*)(base + o_nd[i]);
        o->depth_pyr[i] = (float*)(base + o_dp[i]);
        o->last_image[i] = (uint8_t*)(base + o_li[i]);
        o->next_image[i] = (uint8_t*)(base + o_ni[i]);
        o->last_next_image[i] = (uint8_t*)(base + o_lni[i]);
        o->dIdx[i] = (int16_t*)(base + o_dx[i]);
        o->dIdy[i] = (int16_t*)(base + o_dy[i]);
        o->grad_w_dx[i] = (int16_t*)(base + o_dx2[i]);
        o->grad_w_dy[i] = (int16_t*)(base + o_dy2[i]);
        o->cloud[i] = (float*)(base + o_cl[i]);
        o->cloud4[i] = (float*)(base + o_c4[i]);
        o->corres[i] = (mmf_dataterm*)(base + o_co[i]);
        o->prev_packed[i] = (float*)(base + o_pp[i]);
    }
    o->state = (OdomState*)(base + o_state);
    o->gn_partials_f = (float*)(base + o_pf), o->gn_partials_icp = (float*)(base + o_pi);
    o->gn_partials_res = (int2*)(base + o_pr), o->gn_ticket = (unsigned*)(base + o_tk);
    o->icp_err = (float*)(base + o_ei), o->rgb_err = (float*)(base + o_er);
    o->extent = (unsigned long long*)(base + o_ex);
    o->prep_box = (int*)(base + o_ex + kExtentWords * sizeof(unsigned long long));
    MMF_HIP_TRY(hipHostMalloc(&o->host_result, sizeof(OdomState), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(o->host_result, 0, sizeof(OdomState));
    MMF_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&o->host_result_dev), o->host_result, 0));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    *out = o;
    return MMF_OK;
}

// The odometry of a model ANOTHER rank tracks (fusion_state.hpp: a shard rank's bookkeeping copies): the host
// struct only -- statistics as they arrive with the pose exchange -- no slab, no events, nothing a kernel could be given.
static int odom_create_bookkeeping(mmf_ctx* c, int width, int height, float cx, float cy, float fx, float fy, mmf_odom** out) {
    mmf_odom* o = new (std::nothrow) mmf_odom();
    MMF_REQUIRE(o != nullptr, "mmf_odom_create: out of host memory");
    o->ctx = c;
    o->width = width, o->height = height;
    o->cx = cx, o->cy = cy, o->fx = fx, o->fy = fy;
    std::memset(&o->stats, 0, sizeof(o->stats));
    std::memset(&o->timing_acc, 0, sizeof(o->timing_acc));
    o->stats.lastICPCount = o->stats.lastRGBCount = o->stats.lastSO3Count = (float)(width * height);
    *out = o;
    return MMF_OK;
}

extern "C" void mmf_odom_destroy(mmf_odom* o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    (void)hipStreamSynchronize(o->ctx->stream);
    (void)hipFree(o->slab);
    if (o->gn_truncated) (void)hipFree(o->gn_truncated);
    (void)hipHostFree(o->host_result);
    for (hipEvent_t e : o->ev_kernel)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : o->ev_chain)
        if (e) (void)hipEventDestroy(e);
    delete o;
}

extern "C" int mmf_odom_build_depth_pyramid(mmf_odom* o, const float* depth_l0, size_t step) {
    MMF_REQUIRE(o && depth_l0, "mmf_odom_build_depth_pyramid: null argument");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const size_t s = step ? step : (size_t)o->width * 4;
    if (o->alias_inputs && s == (size_t)o->width * 4) {
        o->depth_l0 = depth_l0;
    } else {
        MMF_HIP_TRY(hipMemcpy2DAsync(o->depth_pyr[0], (size_t)o->width * 4, depth_l0, s, (size_t)o->width * 4, o->height,
                                     hipMemcpyDeviceToDevice, c->stream));
        o->depth_l0 = o->depth_pyr[0];
    }
    for (int i = 1; i < MMF_NUM_PYRS; ++i) {  // Model.cpp:378-382
        int rc = launch_pyrdown_f(c, i == 1 ? o->depth_l0 : o->depth_pyr[i - 1], o->width >> (i - 1), o->width >> (i - 1),
                                  o->height >> (i - 1), o->depth_pyr[i], o->width >> i);
        if (rc) return rc;
    }
    return MMF_OK;
}

extern "C" int mmf_odom_init_icp(mmf_odom* o, const float* const depth_pyr[MMF_NUM_PYRS],
                                 const size_t steps[MMF_NUM_PYRS], float depth_cutoff) {
    MMF_REQUIRE(o != nullptr, "mmf_odom_init_icp: null odometry");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {  // RGBDOdometry.cpp:112-115
        const int cols = o->width >> i, rows = o->height >> i;
        const float* d = depth_pyr ? depth_pyr[i] : (i == 0 && o->depth_l0 ? o->depth_l0 : o->depth_pyr[i]);
        MMF_REQUIRE(d != nullptr, "mmf_odom_init_icp: null pyramid level");
        const int ds = (depth_pyr && steps && steps[i]) ? (int)(steps[i] / 4) : cols;
        int rc = launch_create_vmap(c, level_intr(o->fx, o->fy, o->cx, o->cy, i), d, ds, cols, rows, o->vmaps_curr[i],
                                    cols, depth_cutoff);
        if (rc) return rc;
        rc = launch_create_nmap(c, o->vmaps_curr[i], cols, cols, rows, o->nmaps_curr[i], cols);
        if (rc) return rc;
    }
    return MMF_OK;
}

static int odom_take_prediction(mmf_odom* o, const float* vert_rgba, const float* norm_rgba, float** vdst,
                                float** ndst) {
    mmf_ctx* c = o->ctx;
    o->prep_batched = false;
    const size_t bytes = (size_t)4 * o->width * o->height * sizeof(float);
    // the reference copies both textures into vmaps_tmp / nmaps_tmp (RGBDOdometry.cpp:125,130);
    // vmaps_tmp is read again by initRGB*/populateRGBDData (:179)
    if (o->alias_inputs) {
        o->vtmp = vert_rgba, o->ntmp = norm_rgba;
    } else {
        MMF_HIP_TRY(hipMemcpyAsync(o->vmaps_tmp, vert_rgba, bytes, hipMemcpyDeviceToDevice, c->stream));
        MMF_HIP_TRY(hipMemcpyAsync(o->nmaps_tmp, norm_rgba, bytes, hipMemcpyDeviceToDevice, c->stream));
        o->vtmp = o->vmaps_tmp, o->ntmp = o->nmaps_tmp;
    }
    o->have_tmp = true;
    int rc = launch_copy_maps(c, o->vtmp, o->ntmp, o->width, o->height, vdst[0], ndst[0], o->width);
    if (rc) return rc;
    for (int i = 1; i < MMF_NUM_PYRS; ++i) {
        rc = launch_resize<false>(c, vdst[i - 1], o->width >> (i - 1), o->width >> (i - 1), o->height >> (i - 1),
                                  vdst[i], o->width >> i);
        if (rc) return rc;
        rc = launch_resize<true>(c, ndst[i - 1], o->width >> (i - 1), o->width >> (i - 1), o->height >> (i - 1),
                                 ndst[i], o->width >> i);
        if (rc) return rc;
    }
    return MMF_OK;
}

extern "C" int mmf_odom_init_icp_from_prediction(mmf_odom* o, const float* vert_rgba, const float* norm_rgba,
                                                 float depth_cutoff) {
    (void)depth_cutoff;  // unused by the reference as well (RGBDOdometry.cpp:120-141)
    MMF_REQUIRE(o && vert_rgba && norm_rgba, "mmf_odom_init_icp_from_prediction: null argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    return odom_take_prediction(o, vert_rgba, norm_rgba, o->vmaps_curr, o->nmaps_curr);
}

extern "C" int mmf_odom_init_icp_model(mmf_odom* o, const float* vert_rgba, const float* norm_rgba,
                                       float depth_cutoff, const float pose[16]) {
    (void)depth_cutoff;  // unused by the reference as well (RGBDOdometry.cpp:143-175)
    MMF_REQUIRE(o && vert_rgba && norm_rgba && pose, "mmf_odom_init_icp_model: null argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    int rc = odom_take_prediction(o, vert_rgba, norm_rgba, o->vmaps_g_prev, o->nmaps_g_prev);
    if (rc) return rc;
    const float R[9] = {pose[0], pose[1], pose[2], pose[4], pose[5], pose[6], pose[8], pose[9], pose[10]};
    const float t[3] = {pose[3], pose[7], pose[11]};
    for (int i = 0; i < MMF_NUM_PYRS; ++i) {
        const int cols = o->width >> i, rows = o->height >> i;
        rc = launch_transform(o->ctx, o->vmaps_g_prev[i], o->nmaps_g_prev[i], cols, cols, rows, R, t,
                              o->vmaps_g_prev[i], o->nmaps_g_prev[i], cols);
        if (rc) return rc;
        const int n = cols * rows;
        hipLaunchKernelGGL(pack_prev_kernel, dim3((n + 255) / 256), dim3(256), 0, o->ctx->stream, o->vmaps_g_prev[i],
                           o->nmaps_g_prev[i], n, o->prev_packed[i]);
        MMF_HIP_TRY(hipGetLastError());
    }
    return MMF_OK;
}

// RGBDOdometry.cpp:177-194 (populateRGBDData); mask pyramids are never read and are omitted
static int odom_populate_rgbd(mmf_odom* o, const uint8_t* rgb, size_t step, int channels, float** depths,
                              uint8_t** images) {
    mmf_ctx* c = o->ctx;
    o->prep_batched = false;
    if (!o->have_tmp)
        return fail(MMF_ERR_STATE, "initRGB*/initRGBModel needs a preceding initICPModel / initICP(prediction): "
                                   "it reads vmaps_tmp (RGBDOdometry.cpp:197,202)");
    int rc = launch_vertices_to_depth(c, o->vtmp, o->width, o->height, o->max_depth_rgb, depths[0], o->width);
    if (rc) return rc;
    for (int i = 0; i + 1 < MMF_NUM_PYRS; ++i) {
        rc = launch_pyrdown_f(c, depths[i], o->width >> i, o->width >> i, o->height >> i, depths[i + 1],
                              o->width >> (i + 1));
        if (rc) return rc;
    }
    rc = launch_intensity(c, rgb, step ? (int)step : o->width * channels, channels, o->width, o->height, images[0],
                          o->width);
    if (rc) return rc;
    for (int i = 0; i + 1 < MMF_NUM_PYRS; ++i) {
        rc = launch_pyrdown_u8(c, images[i], o->width >> i, o->width >> i, o->height >> i, images[i + 1],
                               o->width >> (i + 1));
        if (rc) return rc;
    }
    return MMF_OK;
}

extern "C" int mmf_odom_init_rgb(mmf_odom* o, const uint8_t* rgb, size_t step, int channels) {
    MMF_REQUIRE(o && rgb && (channels == 3 || channels == 4), "mmf_odom_init_rgb: bad argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    return odom_populate_rgbd(o, rgb, step, channels, o->next_depth, o->next_image);
}

extern "C" int mmf_odom_init_rgb_model(mmf_odom* o, const uint8_t* rgb, size_t step, int channels) {
    MMF_REQUIRE(o && rgb && (channels == 3 || channels == 4), "mmf_odom_init_rgb_model: bad argument");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    return odom_populate_rgbd(o, rgb, step, channels, o->last_depth, o->last_image);
}

extern "C" int mmf_odom_init_first_rgb(mmf_odom* o, const uint8_t* rgb, size_t step, int channels) {
    MMF_REQUIRE(o && rgb && (channels == 3 || channels == 4), "mmf_odom_init_first_rgb: bad argument");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    int rc = launch_intensity(c, rgb, step ? (int)step : o->width * channels, channels, o->width, o->height,
                              o->last_next_image[0], o->width);
    if (rc) return rc;
    for (int i = 0; i + 1 < MMF_NUM_PYRS; ++i) {  // RGBDOdometry.cpp:212-214
        rc = launch_pyrdown_u8(c, o->last_next_image[i], o->width >> i, o->width >> i, o->height >> i,
                               o->last_next_image[i + 1], o->width >> (i + 1));
        if (rc) return rc;
    }
    return MMF_OK;
}

// ---- the whole per-frame preparation in four launches (prep_batch.hpp) -------------------------
static std::atomic<long> g_prep_big{-1};  // -1: MMF_PREP_BIG decides; 0: never; n > 0: that many pixels (mmf_debug_set_prep_big)
extern "C" int mmf_debug_set_prep_big(int n) {
    g_prep_big.store(n < 0 ? -1L : (long)n);
    return MMF_OK;
}
static size_t prep_big_job() {  // pixels from which a job's workgroups take four tiles each; MMF_PREP_BIG=0: never
    const long forced = g_prep_big.load();
    const long n = forced < 0 ? tunables().prep_big : forced;
    return n < 0 ? (size_t)200000 : (n > 0 ? (size_t)n : ~(size_t)0);
}
struct PrepBuilder {  // the jobs of one stage (possibly of several models); launched kMaxPrepJobs at a time
    std::vector<PrepJob> jobs;
    bool critical = false;  // PrepBatch::critical
    PrepJob& add(int op, int cols, int rows) {
        if (jobs.capacity() < 96) jobs.reserve(96);  // references handed out stay valid while a stage is being filled
        jobs.emplace_back();
        PrepJob& j = jobs.back();
        std::memset(&j, 0, sizeof(j));
        j.op = op;
        j.cols = cols, j.rows = rows;
        j.gx = (cols + kTileX - 1) / kTileX;
        j.reps = (size_t)cols * rows >= prep_big_job() ? 4 : 1;  // (PrepJob::reps)
        return j;
    }
    // rider: the beginning of the tracking these jobs prepare, on one more workgroup of the stage's LAST launch (BeginRider)
    template <int CAP>
    static int fill(PrepBatchT<CAP>& b, const std::vector<PrepJob>& jobs, size_t first, bool critical) {
        b.njobs = 0;
        b.critical = critical ? 1 : 0;
        int blocks = 0;
        for (size_t k = first; k < jobs.size() && b.njobs < CAP; ++k) {
            PrepJob& j = b.job[b.njobs++];
            j = jobs[k];
            j.first_block = blocks;
            blocks += j.rect_now ? j.rect_groups : j.gx * ((j.rows + kTileY * j.reps - 1) / (kTileY * j.reps));
        }
        return blocks;
    }
    int launch(Enqueuer& q, const BeginRider* rider = nullptr) {
        if (jobs.size() > (size_t)kMaxPrepJobs && !rider) {  // several models' jobs: the wide table (prep_batch.hpp)
            for (size_t first = 0; first < jobs.size(); first += kMaxPrepJobsWide) {
                PrepBatchWide b;
                const int blocks = fill(b, jobs, first, critical);
                q.launch(prep_batch_wide_kernel, dim3(blocks), tile_block(), b);
            }
            jobs.clear();
            return MMF_OK;
        }
        for (size_t first = 0; first < jobs.size(); first += kMaxPrepJobs) {
            PrepBatch b;
            const int blocks = fill(b, jobs, first, critical);
            if (rider && first + kMaxPrepJobs >= jobs.size()) {
                BeginRider r = *rider;
                r.prep_blocks = blocks;
                q.launch(prep_batch_begin_kernel, dim3(blocks + 1), tile_block(), b, r);
            } else {
                q.launch(prep_batch_kernel, dim3(blocks), tile_block(), b);
            }
        }
        jobs.clear();
        return MMF_OK;
    }
};
struct PrepStages {  // the four dependent launches of a frame's preparation
    PrepBuilder stage[4];
    void set_critical(bool on) {
        for (PrepBuilder& pb : stage) pb.critical = on;
    }
    int launch(Enqueuer& q, const BeginRider* rider = nullptr) {  // recorded; the caller flushes.  rider: on the last launch
        int last = -1;
        for (int k = 0; k < 4; ++k)
            if (!stage[k].jobs.empty()) last = k;
        for (int k = 0; k < 4; ++k)
            if (int rc = stage[k].launch(q, k == last ? rider : nullptr)) return rc;
        return MMF_OK;
    }
    int launch(hipStream_t stream, const BeginRider* rider = nullptr) {
        Enqueuer q(stream);
        if (int rc = launch(q, rider)) return rc;
        MMF_HIP_TRY(q.flush());
        return MMF_OK;
    }
    bool empty() const {
        for (const PrepBuilder& pb : stage)
            if (!pb.jobs.empty()) return false;
        return true;
    }
};

// Everything initICPModel + initRGBModel + generateCUDATextures/initICP + initRGB + the gradient and
// point-cloud passes of getIncrementalTransformation compute (RGBDOdometry.cpp:108-235, 332-334;
// Model.cpp:359-407), for inputs that stay untouched until tracking returns (the native orchestrator).
// The jobs split into those that depend only on the NEW sensor frame (filtered depth, RGB: vertex / normal maps, depth
// and intensity pyramids, gradients: prep_collect_sensor) and those that depend on the model's prediction and pose
// (prep_collect_model).  The orchestrator can run the first group for frame t+1 on a second stream while frame t is still
// being fused (mmf_fusion_prefetch_frame); PREP_ALL is both groups in the same four launches (prep_collect_all).
// Which stage a job goes to, and where in it, is fixed (prep_batch.hpp: the one arrangement): a stage's list of jobs decides
// which workgroup of the launch does what.
enum PrepSide { PREP_INPUT_IMAGE = 1, PREP_INPUT_DEPTH = 2, PREP_MODEL_SIDE = 4, PREP_ALL = 7 };

struct PrepSensorFrame {  // what the sensor side reads
    const float* depth_filtered = nullptr;  // the depth side's input
    float depth_cutoff = 0.f;
    const uint8_t* rgb = nullptr;  // the image side's input: interleaved, `channels` bytes per pixel
    int channels = 3;
};
struct PrepPrediction {  // what the model side reads: a model's prediction and the pose it is tracked from
    const float *vertex = nullptr, *normal = nullptr;  // RGBA32F
    const uint8_t* image = nullptr;
    int channels = 4;
    const float* pose = nullptr;      // row-major 4 x 4
    const float* depth_l0 = nullptr;  // the frame's filtered depth, which the model's chain reads as level 0 of the depth pyramid
    // optional device-side choice of the sources (PrepJob::sel): the alt_* images instead when *sel != 0 or, with sel_total
    // != 0, when fewer than sel_ratio of the sel_total thumbnail samples are covered
    const int* sel = nullptr;
    const float *alt_vertex = nullptr, *alt_normal = nullptr;
    const uint8_t* alt_image = nullptr;
    int sel_total = 0;
    float sel_ratio = 0.f;
    unsigned ext_gen = 0;  // != 0: the jobs that write the model's depth and vertex pyramids note the extent of what is valid (extent.hpp)
    // (device, level-0 pixels {x0, y0, x1, y1}; an OBJECT model prepared on its own only): where the prediction's images are
    // non-zero -- the jobs then cover the hull of that box and of the one the previous preparation saw (PrepJob::rect_*)
    const int* pred_box = nullptr;
};

static std::atomic<int> g_prep_rect{-1};  // -1: MMF_PREP_RECT decides (default on); 0 / 1: mmf_debug_set_prep_rect
extern "C" int mmf_debug_set_prep_rect(int on) {
    g_prep_rect.store(on < 0 ? -1 : (on ? 1 : 0));
    return MMF_OK;
}

static void prep_intr_f(PrepJob& j, const mmf_odom* o, int lvl) {  // f = {1/fx, 1/fy, cx, cy} of a level
    const LevelIntr in = level_intr(o->fx, o->fy, o->cx, o->cy, lvl);
    j.f[0] = 1.f / in.fx, j.f[1] = 1.f / in.fy, j.f[2] = in.cx, j.f[3] = in.cy;
}
static void prep_pose_f(PrepJob& j, const float pose[16]) {  // f = {R[9], t[3]}
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) j.f[3 * r + q] = pose[4 * r + q];
        j.f[9 + r] = pose[4 * r + 3];
    }
}
static PrepJob& prep_pyr_step(PrepBuilder& pb, const mmf_odom* o, int op, const void* src, void* dst, int lvl) {  // level lvl-1 -> lvl
    PrepJob& j = pb.add(op, o->width >> lvl, o->height >> lvl);
    j.src0 = src, j.dst0 = dst;
    j.scols = o->width >> (lvl - 1), j.srows = o->height >> (lvl - 1);
    return j;
}
// the fill-in images a model-side job reads instead of the prediction's when the device says so (PrepPrediction::sel)
static void prep_alt(PrepJob& j, const PrepPrediction& p, const void* alt0, const void* alt1 = nullptr) {
    j.sel = p.sel, j.alt0 = alt0, j.alt1 = alt1;
    if (p.sel && p.sel_total) j.sel_total = p.sel_total, j.sel_ratio = p.sel_ratio;  // *sel is a count (PrepJob::sel_total)
}

// depth side: stage k makes level k's vertex and normal maps and level k+1 of the depth pyramid -- three dependent launches
static void prep_depth_jobs(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr) {
    const float* depth[MMF_NUM_PYRS] = {fr.depth_filtered, o->depth_pyr[1], o->depth_pyr[2]};
    for (int lvl = 0; lvl < MMF_NUM_PYRS; ++lvl) {
        PrepBuilder& pb = stages.stage[lvl];
        if (lvl + 1 < MMF_NUM_PYRS) prep_pyr_step(pb, o, PREP_PYRDOWN_F, depth[lvl], o->depth_pyr[lvl + 1], lvl + 1);
        PrepJob& j = pb.add(PREP_VMAP_NMAP, o->width >> lvl, o->height >> lvl);
        j.src0 = depth[lvl], j.dst0 = o->vmaps_curr[lvl], j.dst1 = o->nmaps_curr[lvl];
        prep_intr_f(j, o, lvl);
        j.f[4] = fr.depth_cutoff;
        if (lvl == 0) {  // (extent.hpp: the sensor frame's smallest valid depth, for the object models' error-image launches)
            j.zmin = o->extent, j.zmin_gen = ++o->sensor_gen;
            o->sensor_cutoff = fr.depth_cutoff;
        }
    }
}
// image side: the intensity image in stage 0, then stage k+1 makes level k's gradients and level k+1 of the pyramid -- four
static void prep_image_jobs(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr) {
    PrepJob& in = stages.stage[0].add(PREP_INTENSITY, o->width, o->height);
    in.src0 = fr.rgb, in.dst0 = o->next_image[0], in.scols = o->width * fr.channels, in.channels = fr.channels;
    for (int lvl = 0; lvl < MMF_NUM_PYRS; ++lvl) {
        PrepBuilder& pb = stages.stage[lvl + 1];
        PrepJob& d = pb.add(PREP_DERIV, o->width >> lvl, o->height >> lvl);
        d.src0 = o->next_image[lvl], d.dst0 = o->grad_w_dx[lvl], d.dst1 = o->grad_w_dy[lvl];  // (odom_adopt_gradients)
        if (lvl + 1 < MMF_NUM_PYRS) prep_pyr_step(pb, o, PREP_PYRDOWN_U8, o->next_image[lvl], o->next_image[lvl + 1], lvl + 1);
    }
    o->grad_pending = true;
}
static void prep_collect_sensor(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr, int sides) {
    if (sides & PREP_INPUT_DEPTH) prep_depth_jobs(stages, o, fr);
    if (sides & PREP_INPUT_IMAGE) prep_image_jobs(stages, o, fr);
}

// Model side, two dependent launches (stages 1 and 2).  Level 1 of the camera-frame model maps (before the transform into
// the global frame) is the one thing a job stores for another: it lives behind level 0's place in the two 4*N-float staging
// images, which this path does not need as copies.
static float* prep_level1_of(float* staging, const mmf_odom* o) { return staging + 3 * (size_t)o->width * o->height; }
// ... what is made from a level's images: the packed records and the point records of levels 0 and 1, level 0's depth and
// intensity.  Nothing of the preparation reads level 0's, which come straight from the prediction: l0_stage is 2, beside the
// small jobs of levels 1 and 2, so that the first launch is the three quarter-size pyramid jobs alone (1: with a sensor side
// in the same launches)
static void prep_model_level_jobs(PrepStages& stages, mmf_odom* o, const PrepPrediction& p, int l0_stage) {
    const int W = o->width, H = o->height;
    {
        PrepBuilder& pb = stages.stage[l0_stage];
        PrepJob& t = pb.add(PREP_TEX_TP, W, H);
        t.src0 = p.vertex, t.src1 = p.normal, t.dst2 = o->prev_packed[0];
        prep_alt(t, p, p.alt_vertex, p.alt_normal);
        prep_pose_f(t, p.pose);
        if (p.ext_gen) t.aabb = o->extent, t.ext_gen = p.ext_gen;  // (extent.hpp: the pixel box and depth range of the valid vertices)
        PrepJob& c = pb.add(PREP_TEX_PROJECT, W, H);
        c.src0 = p.vertex, c.dst1 = o->cloud4[0], c.dst2 = o->last_depth[0];
        prep_alt(c, p, p.alt_vertex);
        prep_intr_f(c, o, 0);
        c.f[4] = o->max_depth_rgb;
        if (p.ext_gen) c.ext = o->extent, c.ext_gen = p.ext_gen;  // (the depth jobs: extent.hpp, extent_of_level)
        PrepJob& il = pb.add(PREP_INTENSITY, W, H);
        il.src0 = p.image, il.dst0 = o->last_image[0], il.scols = W * p.channels, il.channels = p.channels;
        prep_alt(il, p, p.alt_image);
    }
    {
        PrepBuilder& pb = stages.stage[2];
        PrepJob& t = pb.add(PREP_TRANSFORM_PACK, W >> 1, H >> 1);
        t.src0 = prep_level1_of(o->vmaps_tmp, o), t.src1 = prep_level1_of(o->nmaps_tmp, o), t.dst2 = o->prev_packed[1];
        prep_pose_f(t, p.pose);
        PrepJob& c = pb.add(PREP_PROJECT, W >> 1, H >> 1);
        c.src0 = o->last_depth[1], c.dst1 = o->cloud4[1];
        prep_intr_f(c, o, 1);
    }
}
// ... and the pyramid steps: level 1 from the prediction's images, level 2 -- with its records, in the same job -- from level 1
static void prep_model_pyramid_jobs(PrepStages& stages, mmf_odom* o, const PrepPrediction& p) {
    const int W = o->width, H = o->height;
    {
        PrepBuilder& pb = stages.stage[1];
        PrepJob& d = pb.add(PREP_TEX_PYR_F, W >> 1, H >> 1);
        d.src0 = p.vertex, d.scols = W, d.srows = H, d.dst0 = o->last_depth[1], d.f[0] = o->max_depth_rgb;
        prep_alt(d, p, p.alt_vertex);
        if (p.ext_gen) d.ext = o->extent + 4, d.ext_gen = p.ext_gen;
        PrepJob& u = pb.add(PREP_TEX_PYR_U8, W >> 1, H >> 1);
        u.src0 = p.image, u.scols = W, u.srows = H, u.channels = p.channels, u.dst0 = o->last_image[1];
        prep_alt(u, p, p.alt_image);
        PrepJob& r = pb.add(PREP_TEX_RESIZE, W >> 1, H >> 1);
        r.src0 = p.vertex, r.src1 = p.normal, r.scols = W, r.srows = H;
        r.dst0 = prep_level1_of(o->vmaps_tmp, o), r.dst1 = prep_level1_of(o->nmaps_tmp, o);
        prep_alt(r, p, p.alt_vertex, p.alt_normal);
    }
    {
        PrepBuilder& pb = stages.stage[2];
        prep_pyr_step(pb, o, PREP_PYRDOWN_U8, o->last_image[1], o->last_image[2], 2);
        PrepJob& t = prep_pyr_step(pb, o, PREP_RESIZE_TP, prep_level1_of(o->vmaps_tmp, o), nullptr, 2);
        t.src1 = prep_level1_of(o->nmaps_tmp, o), t.dst2 = o->prev_packed[2];
        prep_pose_f(t, p.pose);
        PrepJob& c = prep_pyr_step(pb, o, PREP_PYR_PROJECT, o->last_depth[1], nullptr, 2);
        c.dst1 = o->cloud4[2], c.dst2 = o->last_depth[2];
        prep_intr_f(c, o, 2);
        if (p.ext_gen) c.ext = o->extent + 8, c.ext_gen = p.ext_gen;
    }
}
// what the odometry remembers of a model-side preparation.  from (null: not boxed): the jobs of `stages` from these counts
// on are this preparation's, and they cover the prediction's box only (PrepPrediction::pred_box)
static void prep_model_done(PrepStages& stages, mmf_odom* o, const PrepPrediction& p, const size_t* from) {
    o->depth_l0 = p.depth_l0;
    o->vtmp = p.vertex, o->ntmp = p.normal;
    o->have_tmp = true;
    o->extent_gen = p.ext_gen;
    if (from) {
        const unsigned g = ++o->prep_gen;
        const int* prev = o->prep_box_known ? o->prep_box + 4 * ((g + 1u) & 1u) : nullptr;
        bool first = true;
        for (int k = 0; k < 4; ++k)
            for (size_t q = from[k]; q < stages.stage[k].jobs.size(); ++q) {
                PrepJob& j = stages.stage[k].jobs[q];
                int lvl = 0;
                while ((o->width >> lvl) > j.cols && lvl < MMF_NUM_PYRS - 1) ++lvl;
                j.rect_now = p.pred_box, j.rect_prev = prev;
                j.rect_level = lvl;
                j.rect_groups = lvl == 0 ? 48 : (lvl == 1 ? 32 : 16);
                j.rect_store = first ? o->prep_box + 4 * (g & 1u) : nullptr;
                first = false;
            }
    }
    o->prep_box_known = from != nullptr;
    o->prep_batched = true;
}
static void prep_collect_model(PrepStages& stages, mmf_odom* o, const PrepPrediction& p) {
    const bool rect_on = g_prep_rect.load() < 0 ? tunables().prep_rect : g_prep_rect.load() != 0;
    const bool boxed = p.pred_box != nullptr && p.sel == nullptr && rect_on && o->prep_box != nullptr;
    size_t from[4];
    for (int k = 0; k < 4; ++k) from[k] = stages.stage[k].jobs.size();
    prep_model_level_jobs(stages, o, p, 2);
    prep_model_pyramid_jobs(stages, o, p);
    prep_model_done(stages, o, p, boxed ? from : nullptr);
}
// One model and a sensor side not prepared ahead: both in the same four launches.  Within a stage: the depth side's jobs, what
// the model makes from a level's images, the image side's jobs, the model's pyramid steps.
static void prep_collect_all(PrepStages& stages, mmf_odom* o, const PrepSensorFrame& fr, const PrepPrediction& p) {
    prep_depth_jobs(stages, o, fr);
    prep_model_level_jobs(stages, o, p, 1);
    prep_image_jobs(stages, o, fr);
    prep_model_pyramid_jobs(stages, o, p);
    prep_model_done(stages, o, p, nullptr);
}
// the gradients the batched preparation wrote last become the ones the chain reads
static void odom_adopt_gradients(mmf_odom* o) {
    if (!o->grad_pending) return;
    o->grad_pending = false;
    for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(o->dIdx[i], o->grad_w_dx[i]), std::swap(o->dIdy[i], o->grad_w_dy[i]);
}

// one or both halves of a sensor frame's side, as launches of their own: recorded in q (the caller flushes) or on the context's stream
static int odom_prepare_sensor(mmf_odom* o, const PrepSensorFrame& fr, int sides, Enqueuer* q = nullptr) {
    PrepStages stages;
    prep_collect_sensor(stages, o, fr, sides);
    return q ? stages.launch(*q) : stages.launch(o->ctx->stream);
}

// Test entry: the batched preparation of n stand-alone odometries as ONE set of stages, filled the way the orchestrator fills
// them (fusion_orchestrator.hpp: fusion_collect_prep) -- host plumbing around the collectors above, no kernel of its own.
extern "C" int mmf_debug_odom_prepare(mmf_odom* const* odoms, const mmf_debug_prep_prediction* preds, int n, const float* depth_filtered,
                                      float depth_cutoff, const unsigned char* rgb, int rgb_channels, int sides) {
    MMF_REQUIRE(odoms && preds && n >= 1, "mmf_debug_odom_prepare: null argument, or no odometry");
    const bool sensor = depth_filtered != nullptr || rgb != nullptr;
    MMF_REQUIRE(!sensor || (sides & ~(PREP_INPUT_IMAGE | PREP_INPUT_DEPTH)) == 0, "mmf_debug_odom_prepare: sides is a mask of 1 (image) and 2 (depth)");
    MMF_REQUIRE(!sensor || (((sides & PREP_INPUT_DEPTH) == 0 || depth_filtered) && ((sides & PREP_INPUT_IMAGE) == 0 || rgb)),
                "mmf_debug_odom_prepare: a side is asked for without its input");
    MMF_REQUIRE(!sensor || (sides & PREP_INPUT_IMAGE) == 0 || rgb_channels == 3 || rgb_channels == 4, "mmf_debug_odom_prepare: rgb_channels must be 3 or 4");
    for (int k = 0; k < n; ++k) {
        const mmf_debug_prep_prediction& d = preds[k];
        MMF_REQUIRE(odoms[k] && odoms[k]->slab && odoms[k]->ctx == odoms[0]->ctx, "mmf_debug_odom_prepare: odometries of one context");
        MMF_REQUIRE(odoms[k]->width == odoms[0]->width && odoms[k]->height == odoms[0]->height, "mmf_debug_odom_prepare: odometries of one size");
        MMF_REQUIRE(d.vertex && d.normal && d.image && d.pose && (d.channels == 3 || d.channels == 4), "mmf_debug_odom_prepare: incomplete prediction");
        MMF_REQUIRE(!d.sel || (d.alt_vertex && d.alt_normal && d.alt_image && d.sel_total >= 0), "mmf_debug_odom_prepare: sel without the alt images");
    }
    mmf_ctx* c = odoms[0]->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    auto prediction = [&](int k) {
        const mmf_debug_prep_prediction& d = preds[k];
        PrepPrediction p;
        p.vertex = d.vertex, p.normal = d.normal, p.image = d.image, p.channels = d.channels, p.pose = d.pose;
        p.depth_l0 = depth_filtered;
        p.sel = d.sel, p.alt_vertex = d.alt_vertex, p.alt_normal = d.alt_normal, p.alt_image = d.alt_image;
        p.sel_total = d.sel_total, p.sel_ratio = d.sel_ratio;
        p.ext_gen = d.ext_gen, p.pred_box = d.pred_box;
        return p;
    };
    PrepSensorFrame fr;
    fr.depth_filtered = depth_filtered, fr.depth_cutoff = depth_cutoff, fr.rgb = rgb, fr.channels = rgb_channels;
    PrepStages stages;
    if (sensor && n == 1 && sides == (PREP_INPUT_IMAGE | PREP_INPUT_DEPTH)) {
        prep_collect_all(stages, odoms[0], fr, prediction(0));
    } else {
        if (sensor) prep_collect_sensor(stages, odoms[0], fr, sides);
        for (int k = 0; k < n; ++k) prep_collect_model(stages, odoms[k], prediction(k));
    }
    if (int rc = stages.launch(c->stream)) return rc;
    for (int k = 0; k < n; ++k) odom_adopt_gradients(odoms[k]);
    return MMF_OK;
}

static IcpArgs odom_icp_args(mmf_odom* o, int level, float* err_map) {
    const int cols = o->width >> level, rows = o->height >> level;
    IcpArgs a;
    a.vmap_curr = MapView{o->vmaps_curr[level], cols};
    a.nmap_curr = MapView{o->nmaps_curr[level], cols};
    a.vmap_g_prev = MapView{o->vmaps_g_prev[level], cols};
    a.nmap_g_prev = MapView{o->nmaps_g_prev[level], cols};
    a.intr = level_intr(o->fx, o->fy, o->cx, o->cy, level);
    a.dist_thres = o->dist_thres;
    a.angle_thres = o->angle_thres;
    a.cols = cols;
    a.rows = rows;
    a.prev_packed = o->prev_packed[level];
    a.err_map = err_map;
    a.err_stride = cols;
    icp_args_derive(a);
    return a;
}

// the ten launches of the SO3 pre-alignment (RGBDOdometry.cpp:239-310): last frame's image against this frame's
// at level 2 -- no model, no pose
static int odom_enqueue_so3(mmf_odom* o, Enqueuer& q, float* partials = nullptr, unsigned* ticket = nullptr, OdomState* state = nullptr) {
    if (!partials) partials = o->gn_partials_f, ticket = o->gn_ticket;
    if (!state) state = o->state;
    const int lvl = 2, cols = o->width >> lvl, rows = o->height >> lvl;
    So3Args a;
    a.last_image = o->last_next_image[lvl];
    a.next_image = o->next_image[lvl];
    a.l_stride = a.n_stride = cols;
    a.cols = cols;
    a.rows = rows;
    a.intr = level_intr(o->fx, o->fy, o->cx, o->cy, 2);
    a.cols_magic = (unsigned)((1ull << 32) / (unsigned)cols) + 1u;
    const int grid = reduce_grid(cols * rows, kBlock);
    for (int i = 0; i < 10; ++i) q.launch((so3_kernel<FINISH_GN>), dim3(grid), dim3(kBlock), state, a, partials, ticket);
    return MMF_OK;
}

// the SO3 pre-alignment of the NEXT frame ahead of its tracking, on `stream` (after that frame's intensity
// pyramid): its begin part, then the ten launches; getIncrementalTransformation then skips both
// `stage`: the state the pre-alignment runs in (its images are o's); the caller tells the consumer (mmf_odom::so3_stage)
static int odom_prefetch_so3(mmf_odom* o, Enqueuer& q, float* partials, unsigned* ticket, OdomState* stage) {
    q.launch(so3_begin_kernel, dim3(1), dim3(64), stage, level_intr(o->fx, o->fy, o->cx, o->cy, 2));
    return odom_enqueue_so3(o, q, partials, ticket, stage);
}

// RGBDOdometry::getIncrementalTransformation (RGBDOdometry.cpp:217-477), device resident:
// every kernel below is enqueued back to back on the context's stream; the data-dependent
// `break`s of the reference (:285-292, :376-378) become flags in the device state that make the
// remaining launches of that loop return immediately.
// first half: everything up to and including the copy of the result towards the host is enqueued on the
// context's stream, nothing waits.  The orchestrator enqueues the chains of all its models (one stream each)
// before it waits for the first result.
// The models one chain of launches tracks: o[0] leads (its stream, its launch arguments), the others ride at their
// slab offsets (BatchDelta).  All share the sensor-side images (fusion_orchestrator.hpp) and the configuration.
struct TrackBatch {
    int n = 1;
    mmf_odom* o[kMaxBatch];
    BatchDelta bd;
    BeginPoses poses;
};

// The tracking mode of one call, worked out once from the reference's five settings.
struct TrackMode {
    bool icp, rgb, rgb_only, so3;
    float icp_weight;
    int iterations[MMF_NUM_PYRS];  // Gauss-Newton iterations per level
    int first_iter_level;          // the coarsest level that runs iterations (the ones below it all do)
};
static TrackMode track_mode(int rgb_only, float icp_weight, int pyramid, int fast_odom, int so3) {
    TrackMode m;
    m.icp = !rgb_only && icp_weight > 0;  // :221-222
    m.rgb = rgb_only || icp_weight < 100;
    m.rgb_only = rgb_only != 0;
    m.so3 = so3 != 0;
    m.icp_weight = icp_weight;
    const int iterations[MMF_NUM_PYRS] = {fast_odom ? 3 : 10, pyramid ? 5 : 0, pyramid ? 4 : 0};  // :312-314
    std::copy(iterations, iterations + MMF_NUM_PYRS, m.iterations);
    m.first_iter_level = MMF_NUM_PYRS - 1;
    while (m.first_iter_level > 0 && !m.iterations[m.first_iter_level]) --m.first_iter_level;
    return m;
}

// The launch arguments of one pyramid level: the correspondence pass's and the ICP reduction's.  The error images are the
// caller's (the chains write them in the last level-0 iteration only, the planner checks the odometry's own).
struct LevelArgs {
    int cols, rows;
    LevelIntr in;
    RgbResidualArgs ra;
    IcpArgs ia;
};
static LevelArgs odom_level_args(mmf_odom* o, int i, float* rgb_err, float* icp_err) {
    LevelArgs l;
    l.cols = o->width >> i, l.rows = o->height >> i;
    l.in = level_intr(o->fx, o->fy, o->cx, o->cy, i);
    const float min_scale = (float)(std::pow((double)o->min_grad[i], 2.0) / std::pow((double)o->sobel_scale, 2.0));
    l.ra = make_residual_args(min_scale, o->dIdx[i], 0, o->dIdy[i], 0, o->last_depth[i], 0,
                              o->prep_batched ? o->last_depth[i] : o->next_depth[i], 0, o->last_image[i], 0, o->next_image[i],
                              0, o->corres[i], o->max_depth_delta_rgb, l.cols, l.rows, rgb_err, 0);
    l.ra.intr = l.in;
    l.ia = odom_icp_args(o, i, icp_err);
    return l;
}

// Launch geometry of gn_iter_kernel at a level of cols x rows pixels: a workgroup = the solver wave + the pixel waves.  The
// launch is a chain of latencies -- records, solve, two memory round trips, the count barrier -- and every workgroup waits at
// that barrier for the slowest one, so (measured on MI355X, tools/ab_libs.sh): at most one workgroup per CU (two on a CU
// reach the barrier 1.6 us after the others); exactly four pixel waves, one per SIMD, where that fits (a fifth doubles up on
// one SIMD and is the long pole of every arithmetic phase: what 640x480 suffered with four pixels per lane, 300 lanes in 256
// workgroups); as few pixels per lane as those two allow (a lane's serial arithmetic is on the critical path).  Five pixels
// per lane exist for 640x480: 240 workgroups x 256 lanes x 5.
// MMF_GN_PX="p0,p1,p2" forces the pixels per lane of a level, MMF_GN_GROUPS the workgroup limit (tuning aids).
struct GnGeometry {
    int px, lanes, threads, groups;
};
// mixed: a launch that also carries object models walked by their extents (gn_iter_mixed_kernel).  Its register count allows
// three waves per SIMD, and the GPU places a second 5-wave workgroup on a CU only with four (measured: tools/gn_mixed_probe.py
// -- the object models' workgroups started when the camera model's had finished); workgroups of FOUR waves (the solver wave
// + three pixel waves, 192 pixel lanes) take one wave slot per SIMD and three of them share a CU.  (256 lanes measured slower
// at 2, 4 and 8 models: LABNOTES.md.)
constexpr int kGnMixedLanes = 192;
static_assert(kGnMixedLanes % 64 == 0 && kGnMixedLanes <= kGnSparseLanes,
              "the sparse walk keeps a workgroup's correspondences in LDS, sized for kGnSparseLanes lanes");
static bool gn_geometry(int level, int cols, int rows, GnGeometry* out, bool mixed = false) {
    if (mixed) {
        GnGeometry base;
        if (!gn_geometry(level, cols, rows, &base, false) || base.lanes != kBlock) return false;
        const int groups = (cols * rows / base.px + kGnMixedLanes - 1) / kGnMixedLanes;
        if (groups > kGnMaxGroups) return false;
        *out = GnGeometry{base.px, kGnMixedLanes, kGnMixedLanes + 64, groups};
        return true;
    }
    const int* forced = tunables().gn_px;
    const int max_groups = tunables().gn_groups;
    const int n = cols * rows;
    const int want = (level >= 0 && level < 3) ? forced[level] : 0;
    // a lane's pixels lie in one row; the window words are 4-byte aligned columns
    auto allowed = [&](int px) { return cols % px == 0 && cols % 4 == 0 && (!(want == 1 || want == 2 || want == 4 || want == 5) || px == want); };
    static const int kPx[4] = {1, 2, 4, 5};
    for (int k = 0; k < 4; ++k) {  // four pixel waves per workgroup (three, 192 lanes: no different, tools/ab_env.sh)
        const int px = kPx[k];
        const int groups = (n / px + kBlock - 1) / kBlock;
        if (!allowed(px) || groups > max_groups || groups > kGnMaxGroups) continue;
        *out = GnGeometry{px, kBlock, kBlock + 64, groups};
        return true;
    }
    for (int k = 3; k >= 0; --k) {  // larger workgroups, as few of them as the limit asks for
        const int px = kPx[k];
        if (!allowed(px)) continue;
        const int total = n / px;
        const int lanes = std::max(kBlock, (total + max_groups - 1) / max_groups);
        const int groups = (total + lanes - 1) / lanes;
        if (lanes > 64 * (kGnMaxWaves - 1) || groups > kGnMaxGroups) continue;
        *out = GnGeometry{px, lanes, (lanes + 63) / 64 * 64 + 64, groups};
        return true;
    }
    return false;
}
// calls f(std::integral_constant<int, PX>) for the pixels per lane of a Gauss-Newton launch (1, 2, 4 or 5: gn_geometry)
template <typename F>
static auto with_gn_px(int px, F&& f) {
    switch (px) {
        case 5: return f(std::integral_constant<int, 5>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 1>{});
    }
}
// How the chain of one call runs: one launch per iteration (gn_iter_kernel) or two (producer + rgb_step), and how the one-launch
// chain walks the models of a batch (gn_fused.hpp: GnBatchGeom).  Made by odom_plan_chain, the only place that decides it.
struct GnChainPlan {
    bool one_launch = false;
    bool mixed = false;  // object models walked by their extents ride the launch (gn_iter_mixed_kernel)
    unsigned sparse_mask = 0, ext_gen = 0;
    GnGeometry geo[MMF_NUM_PYRS] = {};
    int groups[MMF_NUM_PYRS][kMaxBatch] = {};  // workgroups of model m at level l
};
// workgroups of an OBJECT model per launch of the one-launch chain at pyramid level l (a property of the model, batched or
// alone: its float sums keep their order): its photometric box must fit them in ONE pass (32 x 1280 pixels at 640x480 level 0,
// a box of 200 x 200), its ICP rectangle takes as many passes as it needs
static std::atomic<int> g_sparse_groups{0};  // test hook (mmf_debug_set_sparse_groups): that many at every level instead
// need: the lanes the model's box took in its last chain (0: unknown -- 32 / 24 / 16 workgroups, a box of 200 x 200 at 640x480);
// lanes: pixel lanes of a workgroup.  Returns dense_groups when the model is better walked like the camera model.
static int gn_sparse_groups(int level, int dense_groups, int need, int lanes) {
    static const int k[MMF_NUM_PYRS] = {32, 24, 16};
    const int forced = g_sparse_groups.load();
    if (forced > 0) return std::min(dense_groups, forced);
    int want = k[level < MMF_NUM_PYRS ? level : MMF_NUM_PYRS - 1];
    if (need > 0) want = std::max(8, (need + need / 4 + lanes - 1) / lanes + 1);
    return want * 4 >= dense_groups * 3 ? dense_groups : want;
}
extern "C" int mmf_debug_set_sparse_groups(int n) {
    g_sparse_groups.store(n > 0 ? n : 0);
    return MMF_OK;
}
static std::atomic<bool> g_gn_latched_off{false};
static std::atomic<int> g_track_cull{-1};  // -1: tunables().track_cull; 0 / 1: mmf_debug_set_track_cull
extern "C" int mmf_debug_set_track_cull(int mode) {
    g_track_cull.store(mode < 0 ? -1 : (mode ? 1 : 0));
    return MMF_OK;
}
static std::atomic<int> g_gn_force_fault{0};
static std::atomic<int> g_sparse_check{0};
// test hooks of the object models' walk in the one-launch chain (gn_fused.hpp: gn_sparse_icp_box): checking mode on / off, and the
// number of correspondences the last chain of an odometry accepted outside the rectangle it would have walked (must be 0)
extern "C" int mmf_debug_set_sparse_check(int on) {
    g_sparse_check.store(on ? 1 : 0);
    return MMF_OK;
}
extern "C" int mmf_debug_odom_sparse_outside(mmf_odom* o, unsigned* outside, int* walked_by_extent, int rect[9]) {
    if (!o || !o->host_result) return fail(MMF_ERR_INVALID, "mmf_debug_odom_sparse_outside: null argument");
    if (outside) *outside = o->host_result->gn_dbg_outside;
    if (walked_by_extent) *walked_by_extent = o->walked_by_extent ? 1 : 0;
    if (rect) {
        std::memcpy(rect, o->host_result->gn_dbg_rect, sizeof(int) * 6);
        std::memcpy(rect + 6, o->gn_need, sizeof(int) * 3);
    }
    return MMF_OK;
}
static std::atomic<int> g_gn_recoveries{0};
// odom_finish_tracking: the one-launch chain gave up; track again (odom_retrack_prepare).  A private sentinel, outside the
// public mmf_status range (include/mmf_hip.h: 0 and small negatives): it never leaves the library (gn_retry_twice).
constexpr int kGnRetry = 0x6e726574;
static int gn_retry_twice() { return fail(MMF_ERR_STATE, "odometry: tracking gave up twice (the two-launch chain reported a fault)"); }

static bool odom_sparse_on() { return (g_track_cull.load() < 0 ? tunables().track_cull : g_track_cull.load()) != 0; }
static void odom_begin_rider_used();
// what odom_begin_kernel is told (RGBDOdometry.cpp:221-228, 237, 252-255, 316-328); every byte defined (the blocks are compared)
static BeginArgs odom_begin_args(const mmf_odom* o, const float trans[3], const float rot[9], const TrackMode& tm,
                                 bool so3_prefetched, const OdomState* so3_stage, bool one_launch) {
    BeginArgs b;
    std::memset(&b, 0, sizeof(b));
    std::memcpy(b.trans, trans, sizeof(b.trans));
    std::memcpy(b.rot, rot, sizeof(b.rot));
    b.rgb_only = tm.rgb_only ? 1 : 0;
    b.icp = tm.icp ? 1 : 0;
    b.rgb = tm.rgb ? 1 : 0;
    b.so3 = tm.so3 ? 1 : 0;
    b.icp_weight = tm.icp_weight;
    b.so3_intr = level_intr(o->fx, o->fy, o->cx, o->cy, 2);
    b.so3_prefetched = (tm.so3 && so3_prefetched) ? 1 : 0;
    b.so3_stage = b.so3_prefetched ? so3_stage : nullptr;
    // nothing runs between the beginning and the first level's begin unless the SO3 loop does: one launch
    b.fold_level_begin = (!tm.so3 || so3_prefetched) ? 1 : 0;
    // the one-launch chain has no per-level begin: its first launch reads what this one prepares
    b.first_intr = level_intr(o->fx, o->fy, o->cx, o->cy, one_launch ? tm.first_iter_level : MMF_NUM_PYRS - 1);
    return b;
}

// can several models ride one chain (every level on the fused producer path)?  Same tests as the two-launch chain.
static bool odom_batchable(mmf_odom* o, const TrackMode& tm) {
    if (!tm.icp || !tm.rgb || tm.rgb_only || !o->prep_batched) return false;
    for (int i = 0; i <= tm.first_iter_level; ++i) {
        const LevelArgs l = odom_level_args(o, i, nullptr, nullptr);
        if (!residual_vec4_ok(l.ra) || !icp2_fits(l.ia, kBlock, std::min(2, icp_max_px(l.ia, 2)))) return false;
    }
    return true;
}

// can the chain run as one launch per iteration (gn_iter_kernel)?  Both terms on, four pixels per lane at every level,
// every level's grid small enough to be resident at once (the count barrier inside the launch).  MMF_GN_FUSED=0 keeps the
// two-launch chain (A/B runs, and the test that compares the two).
static std::atomic<int> g_gn_fused{-1};  // -1: MMF_GN_FUSED decides (default on); 0 / 1: mmf_debug_set_gn_fused
extern "C" int mmf_debug_set_gn_fused(int on) {
    g_gn_fused.store(on < 0 ? -1 : (on ? 1 : 0));
    if (on) g_gn_latched_off.store(false);  // (a test that asks for the one-launch chain again gets it)
    return MMF_OK;
}
// test hook: the next n one-launch chains of this process give up at their third launch (the count barrier of that launch
// polls zero times), as if a workgroup had never arrived: exercises the recovery below without another process on the GPU
extern "C" int mmf_debug_force_gn_fault(int n) {
    g_gn_force_fault.store(n < 0 ? 0 : n);
    return MMF_OK;
}
// test hook: the next one-launch chain of this process runs n launches of gn_iter_kernel at pyramid level first_level and
// nothing else, then ends (gn_truncated_final_kernel) and leaves its last launch's sums and the pose its last solve made in
// a buffer of the odometry's (GnTruncated; read by mmf_debug_gn_truncated).  A call that cannot take the one-launch chain while this is armed fails.
static std::atomic<int> g_gn_truncate{0};  // n << 8 | first_level
extern "C" int mmf_debug_gn_truncate(int n, int first_level) {
    if (n < 0 || n > 64 || first_level < 0 || first_level >= MMF_NUM_PYRS) return fail(MMF_ERR_INVALID, "mmf_debug_gn_truncate: bad argument");
    g_gn_truncate.store(n ? (n << 8 | first_level) : 0);
    return MMF_OK;
}
extern "C" int mmf_debug_gn_truncated(mmf_odom* o, double totals[58], unsigned count_sumsq[2], double rt[12], float pose[24]) {
    MMF_REQUIRE(o && o->gn_truncated && totals && count_sumsq && rt && pose, "mmf_debug_gn_truncated: null argument, or no truncated chain ran");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    MMF_HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    GnTruncated h;
    MMF_HIP_TRY(hipMemcpy(&h, o->gn_truncated, sizeof(h), hipMemcpyDeviceToHost));
    std::memcpy(totals, h.tot, sizeof(h.tot));
    std::memcpy(count_sumsq, h.cnt, sizeof(h.cnt));
    std::memcpy(rt, h.rt, sizeof(h.rt));
    std::memcpy(pose, h.pose, sizeof(h.pose));
    return MMF_OK;
}
// how often a one-launch chain gave up and its frame was tracked again on the two-launch chain, and whether the one-launch
// chain is still in use (it is latched off by the first such event: whatever kept its workgroups from being resident
// together -- another process on this GPU -- is likely still there)
extern "C" int mmf_gn_chain_status(int* recoveries, int* one_launch_chain_in_use) {
    if (recoveries) *recoveries = g_gn_recoveries.load();
    if (one_launch_chain_in_use) *one_launch_chain_in_use = g_gn_latched_off.load() ? 0 : 1;
    return MMF_OK;
}
// the smaller occupancy of a launch shape's two variants (with and without the error images) bounds the chain
template <typename K>
static int gn_occupancy(K with_err, K without_err, int threads) {
    int nb = 0, nb2 = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, with_err, threads, 0);
    const hipError_t e2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb2, without_err, threads, 0);
    if (e != hipSuccess || e2 != hipSuccess) return (void)hipGetLastError(), 0;
    return std::min(nb, nb2);
}
// How many workgroups of gn_iter_kernel<px, .> (mixed: gn_iter_mixed_kernel) with `threads` threads the device holds at once:
// the occupancy the runtime reports for the kernel (registers, LDS) x the compute units.  The launch spins on its own
// workgroups (count barrier), so a grid beyond this could only time out; such sizes, partitioned or smaller devices take the
// two-launch chain.
static long long gn_resident_groups(mmf_ctx* c, int px, bool mixed, int threads) {
    static std::mutex mu;
    static std::map<std::tuple<int, bool, int>, int> per_cu;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(px, mixed, threads);
    auto it = per_cu.find(key);
    if (it == per_cu.end()) {
        const int nb = with_gn_px(px, [&](auto PX) {
            constexpr int P = decltype(PX)::value;
            return mixed ? gn_occupancy(gn_iter_mixed_kernel<P, true>, gn_iter_mixed_kernel<P, false>, threads)
                         : gn_occupancy(gn_iter_kernel<P, true>, gn_iter_kernel<P, false>, threads);
        });
        it = per_cu.emplace(key, nb).first;
    }
    return (long long)it->second * c->cu_count;
}
// The chain's plan for o (batch: the models riding with it, o first).  sparse_on: object models may be walked by their extents.
static GnChainPlan odom_plan_chain(mmf_odom* o, const TrackMode& tm, const TrackBatch* batch, bool sparse_on) {
    const int models = batch ? batch->n : 1;
    const int forced = g_gn_fused.load();
    const bool enabled = (forced < 0 ? tunables().gn_fused : forced != 0) && o->exclusive_chain && !g_gn_latched_off.load();
    // (more than MMF_GN_FUSED_MAX models: the batched two-launch chain)
    if (!enabled || !tm.icp || !tm.rgb || tm.rgb_only || models > tunables().gn_fused_max) return GnChainPlan();
    // the models walked by their extents: object models whose preparation noted extents for THIS frame (one number for all)
    GnChainPlan pl;
    for (int m = 0; m < models && sparse_on; ++m) {
        const mmf_odom* om = batch ? batch->o[m] : o;
        if (!om->sparse || om->extent_gen == 0) continue;
        if (pl.ext_gen == 0) pl.ext_gen = om->extent_gen;
        if (om->extent_gen == pl.ext_gen) pl.sparse_mask |= 1u << m;
    }
    pl.mixed = pl.sparse_mask != 0;
    for (int i = 0; i <= tm.first_iter_level; ++i) {
        const LevelArgs l = odom_level_args(o, i, o->rgb_err, o->icp_err);
        if (!residual_vec4_ok(l.ra) || icp_max_px(l.ia, 4) != 4 || !l.ia.prev_packed) return GnChainPlan();
        GnGeometry& geo = pl.geo[i];
        if (!gn_geometry(i, l.cols, l.rows, &geo, pl.mixed)) return GnChainPlan();
        // the count barrier inside the launch needs every workgroup of it resident at once
        long long total = 0;
        for (int m = 0; m < models; ++m) {
            const mmf_odom* om = batch ? batch->o[m] : o;
            pl.groups[i][m] = ((pl.sparse_mask >> m) & 1u) ? gn_sparse_groups(i, geo.groups, om->gn_need[i], geo.lanes) : geo.groups;
            total += pl.groups[i][m];
        }
        if (total > gn_resident_groups(o->ctx, geo.px, pl.mixed, geo.threads)) return GnChainPlan();
    }
    pl.one_launch = true;
    return pl;
}

// The models one call tracks and what both forms of the chain need to know about them, worked out once.
// Object models (extent.hpp): in the two-launch chain (track_kernels.hpp: ChainGeom) their passes skip what lies outside
// the model's own depth when the preparation noted its extents for this frame, and they walk their images with a
// quarter of the workgroups; in the one-launch chain (gn_fused.hpp: gn_iter_mixed_kernel) they walk their extents with a
// fraction of the workgroups, which is what lets ALL models of a frame be resident in one launch.
// MMF_TRACK_CULL=0 / mmf_debug_set_track_cull(0): every model like the first.
struct ChainCall {
    mmf_odom* o;  // the leader
    const TrackBatch* batch;
    TrackMode tm;
    unsigned ny;  // models
    BatchDelta bd;
    BeginPoses poses;
    float *icp_err, *rgb_err;  // the error images the last level-0 iteration writes (null: none)
    bool sparse_on, lead_sparse, foll_sparse;
    unsigned cull_gen;     // the extents the two-launch chain's passes skip by (0: none)
    bool two_launch_once;  // (odom_retrack_prepare: this frame is being tracked again)
    bool so3_ran_here;     // the SO3 loop runs in the chain, in the leader's state: shared with the others at the first level begin

    mmf_odom* model(unsigned m) const { return batch ? batch->o[m] : o; }
};
static ChainCall odom_chain_call(mmf_odom* o, const TrackMode& tm, const TrackBatch* batch, float* icp_err, float* rgb_err) {
    ChainCall x;
    x.o = o, x.batch = batch, x.tm = tm;
    x.ny = batch ? (unsigned)batch->n : 1u;
    std::memset(&x.bd, 0, sizeof(x.bd));
    std::memset(&x.poses, 0, sizeof(x.poses));
    if (batch) x.bd = batch->bd, x.poses = batch->poses;
    x.icp_err = icp_err, x.rgb_err = rgb_err;
    x.two_launch_once = false;
    for (unsigned m = 0; m < x.ny; ++m) {
        x.two_launch_once = x.two_launch_once || x.model(m)->two_launch_once;
        x.model(m)->two_launch_once = false;
    }
    x.sparse_on = odom_sparse_on();
    x.lead_sparse = x.sparse_on && o->sparse;
    x.foll_sparse = x.sparse_on && batch && x.ny > 1;
    unsigned foll_gen = x.foll_sparse ? batch->o[1]->extent_gen : 0u;
    for (unsigned m = 1; m < x.ny && x.foll_sparse; ++m) {
        x.foll_sparse = batch->o[m]->sparse;
        if (batch->o[m]->extent_gen != foll_gen) foll_gen = 0u;
    }
    if (!x.foll_sparse) foll_gen = 0u;
    // (the kernels drop the first model's extent in a batch; a sparse model tracked alone keeps its own)
    x.cull_gen = x.ny > 1 ? foll_gen : (x.lead_sparse ? o->extent_gen : 0u);
    x.so3_ran_here = tm.so3 && !o->so3_prefetched;
    return x;
}

// measurement mode 2: the next event pair of o's chain for a launch of `kind` (level * 2 + 0 producer | 1 rgb_step)
static TimedSlot odom_timed_slot(mmf_odom* o, int kind) {
    if (o->timing < 2 || o->n_timed >= kMaxTimedLaunches) return TimedSlot{};
    const int k = o->n_timed++;
    o->timed_kind[k] = kind;
    return TimedSlot{o->ev_kernel[2 * k], o->ev_kernel[2 * k + 1]};
}

// What a chain leaves to odom_chain_publish.
struct ChainTail {
    bool end_folded = false;     // odom_end ran in the finishing lane of the frame's last rgb_step (or in gn_final_kernel)
    bool final_pending = false;  // the one-launch chain's last solve (final_args) shares a launch with the hand-over
    GnIterArgs final_args;
};

// begin: the derivatives (unless the batched preparation wrote them), odom_begin_kernel (unless it rode the preparation:
// odom_begin_rider), the SO3 loop (:239-310)
static int odom_chain_begin(const ChainCall& x, const float trans[3], const float rot[9], bool one_launch, Enqueuer& q) {
    mmf_odom* o = x.o;
    mmf_ctx* c = o->ctx;
    if (x.tm.rgb && !o->prep_batched)
        for (int i = 0; i < MMF_NUM_PYRS; ++i) {  // :230-235
            int rc = launch_derivative(c, o->next_image[i], o->width >> i, o->width >> i, o->height >> i, o->dIdx[i],
                                       o->width >> i, o->dIdy[i], o->width >> i);
            if (rc) return rc;
        }
    const BeginArgs b = odom_begin_args(o, trans, rot, x.tm, o->so3_prefetched, o->so3_stage, one_launch);
    o->n_timed = 0;
    if (o->timing) MMF_HIP_TRY(hipEventRecord(o->ev_chain[0], c->stream));
    // from here to the last step: kernels only, enqueued one by one in call order (Enqueuer keeps the first error)
    // (the beginning may have run already, on the last launch of the preparation enqueued ahead of this frame: odom_begin_rider)
    const bool begun = o->begin_spec_valid && o->begin_spec_ok && !x.batch && std::memcmp(&b, &o->begin_spec, sizeof(b)) == 0;
    o->begin_spec_valid = o->begin_spec_ok = false;
    if (!begun)
        q.launch(odom_begin_kernel, dim3(x.ny), dim3(64), o->state, b, x.bd, x.poses);
    else
        odom_begin_rider_used();
    o->retry_so3_prefetched = o->so3_prefetched, o->retry_so3_stage = o->so3_stage;  // (odom_retrack_prepare)
    if (x.so3_ran_here) {
        int rc = odom_enqueue_so3(o, q);
        if (rc) return rc;
    }
    o->so3_prefetched = false;
    o->so3_stage = nullptr;
    return MMF_OK;
}

// both terms on and every level fits: ONE launch per iteration (gn_fused.hpp) instead of producer + step, at the plan's
// geometry.  (More than three models: the batched two-launch chain is as fast (four) or faster -- 8 models 1.40 ms against
// 1.60 -- because a model's workgroups hold their CUs at the count barrier while the next models' wait for a place.)
static int odom_one_launch_chain(const ChainCall& x, const GnChainPlan& plan, Enqueuer& q, ChainTail* tail, bool truncated = false) {
    mmf_odom* o = x.o;
    GnIterArgs a;
    std::memset(&a, 0, sizeof(a));
    a.poll_sleep = tunables().gn_sleep;
    a.max_polls = kGnMaxPolls;
    a.check_sparse = g_sparse_check.load();
    bool force_fault = false;
    for (int n = g_gn_force_fault.load(); n > 0 && !force_fault;) force_fault = g_gn_force_fault.compare_exchange_weak(n, n - 1);
    int it = 0;
    for (int i = x.tm.first_iter_level; i >= 0; --i) {
        const LevelArgs l = odom_level_args(o, i, nullptr, nullptr);
        LevelArgs last = l;  // the last level-0 iteration also writes the error images
        last.ra.err_map = x.rgb_err, last.ia.err_map = x.icp_err;
        if (!o->prep_batched) {  // :332-334
            MMF_HIP_TRY(q.flush());
            int rc = launch_project(o->ctx, o->last_depth[i], l.cols, l.cols, l.rows, l.in, o->cloud[i], o->cloud4[i]);
            if (rc) return rc;
        }
        if (i == x.tm.first_iter_level && x.so3_ran_here)  // the SO3 loop ran in between: seed resultRt from its result now
            q.launch(gn_level_begin_kernel, dim3(x.ny), dim3(64), o->state, 1, l.in, x.bd, 1);
        const GnGeometry& geo = plan.geo[i];
        a.lanes = geo.lanes;
        a.cloud4 = reinterpret_cast<const float4*>(o->cloud4[i]);
        a.fx = l.in.fx, a.fy = l.in.fy, a.sobel_scale = o->sobel_scale;
        a.intr = l.in;
        a.ifx = 1.0 / (double)l.in.fx, a.ify = 1.0 / (double)l.in.fy;
        // object models walked by their extents: one one-dimensional grid, a geometry per model (GnBatchGeom)
        GnBatchGeom gg;
        std::memset(&gg, 0, sizeof(gg));
        if (plan.mixed) {
            for (unsigned m = 0; m < (unsigned)kMaxBatch; ++m) gg.start[m + 1] = gg.start[m] + (m < x.ny ? plan.groups[i][m] : 0);
            gg.sparse_mask = plan.sparse_mask, gg.ext_gen = plan.ext_gen, gg.level = i, gg.extent = o->extent;
            gg.sensor = o->extent, gg.sensor_gen = o->sensor_gen, gg.sensor_cutoff = o->sensor_cutoff;
            gg.rotate = gg.start[1];  // the object models' workgroups first (the first model of a batch is the camera model)
        }
        for (int j = 0; j < x.tm.iterations[i]; ++j) {
            const bool last_l0 = (i == 0 && j == x.tm.iterations[i] - 1);
            a.ra = last_l0 ? last.ra : l.ra;
            a.ia = last_l0 ? last.ia : l.ia;
            a.it = it;
            a.max_polls = (it == 2 && force_fault) ? 0 : kGnMaxPolls;
            const bool err = last_l0 && (x.icp_err || x.rgb_err);
            const TimedSlot slot = odom_timed_slot(o, i * 2);
            with_gn_px(geo.px, [&](auto PX) {
                constexpr int P = decltype(PX)::value;
                if (plan.mixed)
                    q.launch(slot, err ? gn_iter_mixed_kernel<P, true> : gn_iter_mixed_kernel<P, false>, dim3(gg.start[kMaxBatch]),
                             dim3(geo.threads), o->state, a, x.bd, gg);
                else
                    q.launch(slot, err ? gn_iter_kernel<P, true> : gn_iter_kernel<P, false>, dim3(geo.groups, x.ny), dim3(geo.threads),
                             o->state, a, x.bd);
            });
            ++it;
        }
    }
    if (truncated) {  // (mmf_debug_gn_truncate) no solve behind the last launch: its sums and the pose it ran with, then the frame's end
        tail->end_folded = true;
        a.it = it;
        a.intr = level_intr(o->fx, o->fy, o->cx, o->cy, x.tm.first_iter_level);  // the level the launches ran at (the loop went on to level 0)
        a.ifx = 1.0 / (double)a.intr.fx, a.ify = 1.0 / (double)a.intr.fy;
        q.launch(gn_truncated_final_kernel, dim3(1), dim3(64), o->state, a, o->gn_truncated);
        return MMF_OK;
    }
    // the last solve + RGBDOdometry.cpp:464-467: one workgroup per model
    a.it = it;
    a.intr = level_intr(o->fx, o->fy, o->cx, o->cy, 0);
    a.ifx = 1.0 / (double)a.intr.fx, a.ify = 1.0 / (double)a.intr.fy;
    tail->end_folded = true;
    // the chain's last solve shares a launch with the hand-over of the result to the host (odom_chain_publish), unless the
    // chain is being timed as such (its closing event lies between the two)
    if (o->timing)
        q.launch(gn_final_kernel, dim3(x.ny), dim3(kBlock), o->state, a, x.bd);
    else
        tail->final_pending = true, tail->final_args = a;
    return MMF_OK;
}

// producer (ICP reduction + correspondence pass, or the two apart) + rgb_step per iteration
static int odom_two_launch_chain(const ChainCall& x, Enqueuer& q, ChainTail* tail) {
    mmf_odom* o = x.o;
    const TrackMode& tm = x.tm;
    auto quarter = [](int full) { return std::max(std::min(full, 32), (full + 3) / 4); };
    bool begin_folded = !x.so3_ran_here;  // this level's gn_level_begin already ran (in odom_begin_kernel, or in the
                                          // last rgb_step of the level before)
    for (int i = MMF_NUM_PYRS - 1; i >= 0; --i) {
        const bool first_level = i == MMF_NUM_PYRS - 1;
        const int cols = o->width >> i, rows = o->height >> i;
        const LevelIntr in = level_intr(o->fx, o->fy, o->cx, o->cy, i);
        if (tm.rgb && !o->prep_batched) {  // :332-334
            MMF_HIP_TRY(q.flush());
            int rc = launch_project(o->ctx, o->last_depth[i], cols, cols, rows, in, o->cloud[i], o->cloud4[i]);
            if (rc) return rc;
        }
        if (!begin_folded)
            q.launch(gn_level_begin_kernel, dim3(x.ny), dim3(64), o->state, first_level ? 1 : 0, in, x.bd,
                     (first_level && x.so3_ran_here) ? 1 : 0);
        begin_folded = false;
        if (!tm.iterations[i]) continue;

        LevelArgs l = odom_level_args(o, i, nullptr, nullptr);
        l.ra.extent = x.cull_gen ? o->extent : nullptr, l.ra.extent_gen = x.cull_gen, l.ra.extent_level = i;
        LevelArgs last = l;  // the last level-0 iteration also writes the error images
        last.ra.err_map = x.rgb_err, last.ia.err_map = x.icp_err;
        RgbStepArgs step;  // :418-423, then :425-460 in the finishing workgroup
        step.residual_partials = o->gn_partials_res;
        step.icp_partials = o->gn_partials_icp;
        step.corres = o->corres[i];
        step.cloud = nullptr, step.cloud4 = reinterpret_cast<const float4*>(o->cloud4[i]);
        step.fx = in.fx;
        step.fy = in.fy;
        step.dIdx = o->dIdx[i];
        step.dIdy = o->dIdy[i];
        step.d_stride = cols;
        step.sobel_scale = o->sobel_scale;
        step.cols = cols;
        step.rows = rows;
        step.cols_magic = l.ra.cols_magic;
        step.extent = l.ra.extent, step.extent_gen = l.ra.extent_gen, step.extent_level = l.ra.extent_level;

        for (int j = 0; j < tm.iterations[i]; ++j) {
            const bool last_l0 = (i == 0 && j == tm.iterations[i] - 1);
            const RgbResidualArgs& ra = last_l0 ? last.ra : l.ra;
            const IcpArgs& ia = last_l0 ? last.ia : l.ia;
            const bool res_vec4 = tm.rgb && residual_vec4_ok(ra);
            int res_records = tm.rgb ? reduce_grid(cols * rows, res_vec4 ? kBlock * 4 : kBlock) : 0, icp_records = 0;
            const int ipx = tm.icp ? std::min(2, icp_max_px(ia, 2)) : 1;
            ChainGeom geom;
            std::memset(&geom, 0, sizeof(geom));
            const bool fuse_producers = tm.rgb && tm.icp && res_vec4 && icp2_fits(ia, kBlock, ipx);
            if (fuse_producers) {  // ICP reduction + correspondence pass side by side in one launch
                icp_records = (cols * rows + kBlock * ipx - 1) / (kBlock * ipx);
                if (x.lead_sparse)  // (every model of this launch, then)
                    res_records = quarter(res_records);
                else if (x.foll_sparse)
                    geom.res_f = (unsigned)quarter(res_records);
                q.launch(odom_timed_slot(o, i * 2), ipx == 2 ? track_producer_kernel<2, true> : track_producer_kernel<1, true>,
                         dim3(icp_records + res_records, x.ny), dim3(kBlock), o->state, ia, (unsigned)icp_records, ra,
                         o->gn_partials_icp, o->gn_partials_res, x.bd, geom);
            } else {
                MMF_REQUIRE(x.ny == 1, "odom_enqueue_tracking: this level cannot be batched");
                if (tm.rgb)
                    q.launch(res_vec4 ? rgb_residual_kernel<FINISH_GN, 4> : rgb_residual_kernel<FINISH_GN, 1>, dim3(res_records),
                             dim3(kBlock), o->state, ra, o->gn_partials_res);
                if (tm.icp) {  // :403-410
                    icp_records = launch_icp<FINISH_GN>(q, o->state, ia, o->gn_partials_icp);
                    if (!tm.rgb)  // ICP-only tracking: one workgroup sums the records, solves, updates the pose
                        q.launch(icp_finish_kernel<FINISH_GN>, dim3(1), dim3(256), o->state, o->gn_partials_icp,
                                 (unsigned)icp_records, in);
                }
            }
            if (!tm.rgb) continue;
            RgbStepArgs a = step;
            a.residual_records = (unsigned)res_records;
            a.icp_records = (unsigned)icp_records;
            a.intr = in;
            // the last step of a level also does the next level's gn_level_begin (one launch less per
            // level).  Not with rgbOnly: its divergence `break` skips the finishing lane.
            a.next_level = 0;
            a.final_step = (last_l0 && !tm.rgb_only) ? 1 : 0;  // odom_end in the finishing lane (which rgbOnly's `break` skips)
            tail->end_folded = a.final_step != 0;
            if (j == tm.iterations[i] - 1 && i > 0 && tm.iterations[i - 1] > 0 && !tm.rgb_only) {
                a.next_level = 1;
                a.intr = level_intr(o->fx, o->fy, o->cx, o->cy, i - 1);  // only read by the finishing lane's rgb_prepare
                begin_folded = true;
            }
            int grid = reduce_grid(cols * rows, kBlock * 4);  // width, height are multiples of 4
            if (fuse_producers && x.lead_sparse)
                grid = quarter(grid);
            else if (fuse_producers && x.foll_sparse)
                geom.step_f = (unsigned)quarter(grid);
            // (the 4-pixel correspondence pass wrote compact records)
            q.launch(odom_timed_slot(o, i * 2 + 1), res_vec4 ? rgb_step_kernel<FINISH_GN, 4, true> : rgb_step_kernel<FINISH_GN, 4, false>,
                     dim3(grid, x.ny), dim3(kBlock), o->state, a, o->gn_partials_f, o->gn_ticket, x.bd, geom);
        }
    }
    return MMF_OK;
}

// publish: the end kernel, every model's result towards the host on the chain's stream, the image ring
static int odom_chain_publish(const ChainCall& x, Enqueuer& q, const ChainTail& tail) {
    mmf_odom* o = x.o;
    if (!tail.end_folded) q.launch(odom_end_kernel, dim3(x.ny), dim3(64), o->state, x.bd);
    MMF_HIP_TRY(q.flush());
    if (o->timing) MMF_HIP_TRY(hipEventRecord(o->ev_chain[1], o->ctx->stream));
    PublishTargets to;
    std::memset(&to, 0, sizeof(to));
    const unsigned seq = ++o->publish_seq;
    for (unsigned m = 0; m < x.ny; ++m) {
        mmf_odom* om = x.model(m);
        to.host[m] = om->host_result_dev;
        om->publish_seq = seq;
        // a follower of a batch takes the LEADER's counter: whatever its own earlier chains left in the pinned flag, it is not
        // this chain's number before this chain has written it
        om->host_result->publish_seq = ~seq;
        om->pending_icp = x.tm.icp, om->pending_so3 = x.tm.so3;
        om->track_stream = o->ctx->stream;
        om->result_of = o;
        if (om != o) om->so3_prefetched = false;
        // the image ring (:469-473).  Host bookkeeping only -- the launches above hold their pointers by value -- and
        // done here rather than when the result is picked up, so that the next frame's sensor-side preparation can be
        // enqueued while this chain runs
        if (x.tm.so3)
            for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(om->last_next_image[i], om->next_image[i]);
    }
    o->rider = FrameRider();
    if (tail.final_pending && o->defer_publish && x.ny == 1) {
        q.launch(gn_final_kernel, dim3(x.ny), dim3(kBlock), o->state, tail.final_args, x.bd);
        o->rider.st = o->state, o->rider.host = o->host_result_dev, o->rider.seq = seq;
    } else if (tail.final_pending) {
        q.launch(gn_final_publish_kernel, dim3(x.ny), dim3(kBlock), o->state, tail.final_args, x.bd, to, seq);
    } else {
        q.launch(odom_publish_kernel, dim3(x.ny), dim3(128), o->state, to, seq, x.bd);
    }
    MMF_HIP_TRY(q.flush());
    return MMF_OK;
}

static int odom_enqueue_tracking(mmf_odom* o, const float trans[3], const float rot[9], const TrackMode& tm, float* icp_err_dev,
                                 float* rgb_err_dev, const TrackBatch* batch = nullptr) {
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
#ifdef MMF_STAMPS  // (diagnostic builds: MMF_DBG_NO_ERR=1 leaves the error images out, so that a chain's last launch is an ordinary one)
    if (std::getenv("MMF_DBG_NO_ERR")) icp_err_dev = rgb_err_dev = nullptr;
#endif
    MMF_REQUIRE(!batch || batch->n == 1 || odom_batchable(o, tm), "odom_enqueue_tracking: not batchable");
    TrackMode tmx = tm;
    const int truncate = g_gn_truncate.exchange(0);
    if (truncate) {  // (mmf_debug_gn_truncate) n launches at one level
        for (int i = 0; i < MMF_NUM_PYRS; ++i) tmx.iterations[i] = 0;
        tmx.first_iter_level = truncate & 0xFF;
        tmx.iterations[tmx.first_iter_level] = truncate >> 8;
    }
    const ChainCall x = odom_chain_call(o, tmx, batch, icp_err_dev, rgb_err_dev);
    const GnChainPlan plan = x.two_launch_once ? GnChainPlan() : odom_plan_chain(o, tmx, batch, x.sparse_on);
    MMF_REQUIRE(!truncate || (plan.one_launch && x.ny == 1), "odom_enqueue_tracking: a truncated chain needs the one-launch chain of one model");
    if (truncate && !o->gn_truncated) {
        MMF_HIP_TRY(hipMalloc(&o->gn_truncated, sizeof(GnTruncated)));
        MMF_HIP_TRY(hipMemset(o->gn_truncated, 0, sizeof(GnTruncated)));
    }
    for (unsigned m = 0; m < x.ny; ++m) x.model(m)->walked_by_extent = plan.one_launch && ((plan.sparse_mask >> m) & 1u) != 0;
    Enqueuer q(o->ctx->stream);
    ChainTail tail;
    int rc = odom_chain_begin(x, trans, rot, plan.one_launch, q);
    if (rc == MMF_OK) rc = plan.one_launch ? odom_one_launch_chain(x, plan, q, &tail, truncate != 0) : odom_two_launch_chain(x, q, &tail);
    return rc == MMF_OK ? odom_chain_publish(x, q, tail) : rc;
}

// The beginning of the NEXT tracking of one model, to ride the last launch of the preparation that is being enqueued ahead of
// it (track_kernels.hpp: prep_batch_begin_kernel): `pose` = where that tracking will start (the model's pose now), so3_stage =
// the staged pre-alignment of that frame (null: none, the tracking runs it itself).  odom_enqueue_tracking skips its own
// odom_begin_kernel when it is about to pass these very arguments and the caller says the state was left alone (begin_spec_ok).
static std::atomic<int> g_begin_rider{-1};      // -1: MMF_BEGIN_RIDER decides (default on); 0 / 1: mmf_debug_set_begin_rider
static std::atomic<int> g_begin_riders_used{0};  // chains that found their beginning done (mmf_debug_begin_rider_count)
extern "C" int mmf_debug_set_begin_rider(int on) {
    g_begin_rider.store(on < 0 ? -1 : (on ? 1 : 0));
    return MMF_OK;
}
extern "C" int mmf_debug_begin_rider_count(void) { return g_begin_riders_used.load(); }
static void odom_begin_rider_used() { g_begin_riders_used.fetch_add(1); }
static bool odom_begin_rider(mmf_odom* o, const float pose[16], const TrackMode& tm, const OdomState* so3_stage, BeginRider* out) {
    o->begin_spec_valid = o->begin_spec_ok = false;
    const int forced = g_begin_rider.load();
    if (!(forced < 0 ? tunables().begin_rider : forced != 0) || o->two_launch_once) return false;
    const bool one_launch = odom_plan_chain(o, tm, nullptr, odom_sparse_on()).one_launch;
    const float trans[3] = {pose[3], pose[7], pose[11]};
    const float rot[9] = {pose[0], pose[1], pose[2], pose[4], pose[5], pose[6], pose[8], pose[9], pose[10]};
    std::memset(out, 0, sizeof(*out));
    out->st = o->state;
    out->a = odom_begin_args(o, trans, rot, tm, so3_stage != nullptr, so3_stage, one_launch);
    o->begin_spec = out->a;
    o->begin_spec_valid = true;
    return true;
}

// second half: wait for the stream, hand the result out
static int odom_finish_tracking(mmf_odom* o, float trans[3], float rot[9]) {
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    // the chain it rode on publishes into this odometry's pinned state and then stores the sequence number
    if (o->result_of) {
        const volatile unsigned* flag = &o->host_result->publish_seq;
        bool seen = false;
        const auto t_poll = std::chrono::steady_clock::now();
        while (!seen) {  // a few seconds of polling at most, then the stream says why
            for (int i = 0; i < 4096 && !seen; ++i) seen = *flag == o->publish_seq;
            if (seen || std::chrono::steady_clock::now() - t_poll > std::chrono::seconds(5)) break;
        }
        if (!seen) {
            MMF_HIP_TRY(hipStreamSynchronize(o->track_stream));
            MMF_REQUIRE(*flag == o->publish_seq, "odometry: the tracking result did not reach the host");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        MMF_HIP_TRY(wait_stream(c->stream));
    }
    o->track_stream = nullptr, o->result_of = nullptr;
    const bool icp = o->pending_icp, so3 = o->pending_so3;
    if (o->timing) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, o->ev_chain[0], o->ev_chain[1]) == hipSuccess) {
            o->timing_acc.chain_us_sum += ms * 1e3;
            o->timing_acc.chains += 1;
        }
        for (int k = 0; k < o->n_timed; ++k)
            if (hipEventElapsedTime(&ms, o->ev_kernel[2 * k], o->ev_kernel[2 * k + 1]) == hipSuccess) {
                const int lvl = o->timed_kind[k] >> 1, step = o->timed_kind[k] & 1;
                double* sum = step ? o->timing_acc.rgb_step_us_sum : o->timing_acc.producer_us_sum;
                double* mn = step ? o->timing_acc.rgb_step_us_min : o->timing_acc.producer_us_min;
                int* n = step ? o->timing_acc.rgb_step_launches : o->timing_acc.producer_launches;
                sum[lvl] += ms * 1e3;
                if (n[lvl] == 0 || ms * 1e3 < mn[lvl]) mn[lvl] = ms * 1e3;
                n[lvl] += 1;
            }
        o->n_timed = 0;
    }

    const OdomState* r = o->host_result;
    if (o->walked_by_extent) std::memcpy(o->gn_need, r->gn_need, sizeof(o->gn_need));  // (valid also when the chain gave up)
    if (r->gn_fault) {  // the one-launch chain gave up: nothing of its result is valid
        o->last_gn_fault = r->gn_fault;
        return kGnRetry;
    }
    o->last_gn_fault = 0;
    std::memcpy(trans, r->trans_out, sizeof(float) * 3);
    std::memcpy(rot, r->rot_out, sizeof(float) * 9);
    // members the reference leaves untouched in a given mode keep their previous values
    if (icp) {
        o->stats.lastICPError = r->st.lastICPError;
        o->stats.lastICPCount = r->st.lastICPCount;
    }
    o->stats.lastRGBError = r->st.lastRGBError;
    o->stats.lastRGBCount = r->st.lastRGBCount;
    if (so3) {
        o->stats.lastSO3Error = r->st.lastSO3Error;
        o->stats.lastSO3Count = r->st.lastSO3Count;
    }
    if (r->st.iterations_run > 0) {
        std::memcpy(o->stats.lastA, r->st.lastA, sizeof(double) * 36);
        std::memcpy(o->stats.lastb, r->st.lastb, sizeof(double) * 6);
    }
    o->stats.iterations_run = r->st.iterations_run;
    o->stats.so3_iterations_run = r->st.so3_iterations_run;
    return MMF_OK;
}

// A one-launch chain gave up (odom_finish_tracking returned kGnRetry for a model it tracked): the process stops using that
// chain, and every odometry the chain drove is put back to where odom_enqueue_tracking found it -- the image ring (:469-473)
// and the prefetched SO3 pre-alignment it consumed -- so that the same call can be enqueued again and take the two-launch
// chain from the pose the frame started with.  RGBDOdometry.cpp:464-467: the call returns a pose or reverts, it never aborts.
static void odom_retrack_prepare(mmf_odom* const* odoms, int n, int so3) {
    // An object model whose extent did not fit its workgroups (kGnFaultExtent) says nothing about the GPU: this frame is tracked
    // again on the two-launch chain, the model's next chain is sized by what the box needed (odom_finish_tracking has taken
    // OdomState::gn_need over), and the one-launch chain stays in use.
    bool extent_only = true;
    for (int k = 0; k < n; ++k) {
        const int fault = odoms[k]->host_result ? odoms[k]->host_result->gn_fault : 0;
        if (fault != 0 && fault != kGnFaultExtent) extent_only = false;
    }
    if (!extent_only) g_gn_latched_off.store(true);
    g_gn_recoveries.fetch_add(1);
    for (int k = 0; k < n; ++k) {
        mmf_odom* o = odoms[k];
        o->two_launch_once = true;
        if (so3)
            for (int i = 0; i < MMF_NUM_PYRS; ++i) std::swap(o->last_next_image[i], o->next_image[i]);
        o->so3_prefetched = odoms[0]->retry_so3_prefetched, o->so3_stage = odoms[0]->retry_so3_stage;
        o->track_stream = nullptr, o->result_of = nullptr;
    }
}

extern "C" int mmf_odom_get_incremental_transformation(mmf_odom* o, float trans[3], float rot[9], int rgb_only,
                                                       float icp_weight, int pyramid, int fast_odom, int so3,
                                                       float* icp_err_dev, float* rgb_err_dev) {
    MMF_REQUIRE(o && trans && rot, "mmf_odom_get_incremental_transformation: null argument");
    const float trans0[3] = {trans[0], trans[1], trans[2]};
    float rot0[9];
    std::memcpy(rot0, rot, sizeof(rot0));
    const TrackMode tm = track_mode(rgb_only, icp_weight, pyramid, fast_odom, so3);
    int rc = odom_enqueue_tracking(o, trans, rot, tm, icp_err_dev, rgb_err_dev);
    if (rc) return rc;
    rc = odom_finish_tracking(o, trans, rot);
    if (rc != kGnRetry) return rc;
    odom_retrack_prepare(&o, 1, so3);
    rc = odom_enqueue_tracking(o, trans0, rot0, tm, icp_err_dev, rgb_err_dev);
    if (rc) return rc;
    rc = odom_finish_tracking(o, trans, rot);
    return rc == kGnRetry ? gn_retry_twice() : rc;
}

// measurement mode: per-launch durations of the Gauss-Newton kernels from the dispatches' own timestamps
extern "C" int mmf_odom_enable_timing(mmf_odom* o, int on) {
    MMF_REQUIRE(o != nullptr, "mmf_odom_enable_timing: null odometry");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    if (on && !o->ev_chain[0]) {
        for (hipEvent_t& e : o->ev_kernel) MMF_HIP_TRY(hipEventCreate(&e));
        for (hipEvent_t& e : o->ev_chain) MMF_HIP_TRY(hipEventCreate(&e));
    }
    o->timing = on < 0 ? 0 : (on > 2 ? 2 : on);
    std::memset(&o->timing_acc, 0, sizeof(o->timing_acc));
    return MMF_OK;
}
extern "C" int mmf_odom_get_timing(mmf_odom* o, mmf_odom_timing* out) {
    MMF_REQUIRE(o && out, "mmf_odom_get_timing: null argument");
    *out = o->timing_acc;
    return MMF_OK;
}

extern "C" int mmf_odom_get_stats(mmf_odom* o, mmf_odom_stats* out) {
    MMF_REQUIRE(o && out, "mmf_odom_get_stats: null argument");
    *out = o->stats;
    return MMF_OK;
}

// RGBDOdometry.cpp:479 -- lastA.lu().inverse(); Gauss-Jordan with partial pivoting on the host
extern "C" int mmf_odom_get_covariance(mmf_odom* o, double cov[36]) {
    MMF_REQUIRE(o && cov, "mmf_odom_get_covariance: null argument");
    double a[6][12];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            a[i][j] = o->stats.lastA[i * 6 + j];
            a[i][6 + j] = (i == j) ? 1.0 : 0.0;
        }
    for (int col = 0; col < 6; ++col) {
        int piv = col;
        for (int r = col + 1; r < 6; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (piv != col)
            for (int k = 0; k < 12; ++k) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 12; ++k) a[col][k] /= d;
        for (int r = 0; r < 6; ++r)
            if (r != col) {
                const double f = a[r][col];
                for (int k = 0; k < 12; ++k) a[r][k] -= f * a[col][k];
            }
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) cov[i * 6 + j] = a[i][6 + j];
    return MMF_OK;
}

extern "C" int mmf_odom_buffer(mmf_odom* o, const char* name, int level, void** dev_ptr, size_t* bytes) {
    MMF_REQUIRE(o && name && dev_ptr && bytes && level >= 0 && level < MMF_NUM_PYRS, "mmf_odom_buffer: bad argument");
    const size_t n = (size_t)(o->width >> level) * (o->height >> level);
    const std::string s(name);
    void* p = nullptr;
    size_t b = 0;
    if (s == "vmaps_curr") p = o->vmaps_curr[level], b = 3 * n * 4;
    else if (s == "nmaps_curr") p = o->nmaps_curr[level], b = 3 * n * 4;
    else if (s == "vmaps_g_prev") p = o->vmaps_g_prev[level], b = 3 * n * 4;
    else if (s == "nmaps_g_prev") p = o->nmaps_g_prev[level], b = 3 * n * 4;
    else if (s == "last_depth") p = o->last_depth[level], b = n * 4;
    else if (s == "next_depth") p = o->next_depth[level], b = n * 4;
    else if (s == "depth_pyr") p = o->depth_pyr[level], b = n * 4;
    else if (s == "cloud") p = o->cloud[level], b = 3 * n * 4;
    else if (s == "cloud4") p = o->cloud4[level], b = 4 * n * 4;         // {X, Y, Z, 1/Z} per pixel
    else if (s == "prev_packed") p = o->prev_packed[level], b = 6 * n * 4;  // {vertex, normal} per pixel
    else if (s == "last_image") p = o->last_image[level], b = n;
    else if (s == "next_image") p = o->next_image[level], b = n;
    else if (s == "last_next_image") p = o->last_next_image[level], b = n;
    else if (s == "dIdx") p = o->dIdx[level], b = n * 2;
    else if (s == "dIdy") p = o->dIdy[level], b = n * 2;
    else if (s == "corres") p = o->corres[level], b = n * sizeof(mmf_dataterm);
    else if (s == "icp_error") p = o->icp_err, b = (size_t)o->width * o->height * 4;  // Model::icpError / rgbError (R32F, full size;
    else if (s == "rgb_error") p = o->rgb_err, b = (size_t)o->width * o->height * 4;  // `level` is ignored)
    else if (s == "extent") p = o->extent, b = kExtentWords * sizeof(unsigned long long);  // extent.hpp's words (tests; `level` is ignored)
    else if (s == "prep_box") p = o->prep_box, b = 8 * sizeof(int);                        // PrepJob::rect_store's two slots
    else return fail(MMF_ERR_INVALID, "mmf_odom_buffer: unknown buffer name '" + s + "'");
    *dev_ptr = p;
    *bytes = b;
    return MMF_OK;
}

extern "C" int mmf_odom_download(mmf_odom* o, const char* name, int level, void* host_dst, size_t host_bytes) {
    MMF_REQUIRE(host_dst != nullptr, "mmf_odom_download: null destination");
    void* p = nullptr;
    size_t b = 0;
    int rc = mmf_odom_buffer(o, name, level, &p, &b);
    if (rc) return rc;
    MMF_REQUIRE(b == host_bytes, "mmf_odom_download: size mismatch");
    MMF_HIP_TRY(hipSetDevice(o->ctx->device));
    MMF_HIP_TRY(hipMemcpyAsync(host_dst, p, b, hipMemcpyDeviceToHost, o->ctx->stream));
    MMF_HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    return MMF_OK;
}

extern "C" int mmf_odom_time_icp_kernel(mmf_odom* o, int level, int reps, int variant, float* mean_us_out) {
    MMF_REQUIRE(o && mean_us_out && level >= 0 && level < MMF_NUM_PYRS && reps > 0, "mmf_odom_time_icp_kernel: bad argument");
    MMF_REQUIRE(variant == 0, "mmf_odom_time_icp_kernel: variant must be 0 (the shipped launch geometry)");
    mmf_ctx* c = o->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const IcpArgs a = odom_icp_args(o, level, nullptr);
    Enqueuer q(c->stream);
    // the state's pose fields are whatever the last getIncrementalTransformation left (or zero);
    // FINISH_RAW only writes out_f
    for (int w = 0; w < 3; ++w) launch_icp<FINISH_RAW>(q, o->state, a, c->partials_icp);
    MMF_HIP_TRY(q.flush());
    MMF_HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; ++r) launch_icp<FINISH_RAW>(q, o->state, a, c->partials_icp);
    MMF_HIP_TRY(q.flush());
    MMF_HIP_TRY(hipEventRecord(c->ev1, c->stream));
    MMF_HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    MMF_HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_us_out = ms * 1000.0f / reps;
    return MMF_OK;
}

// =============================================================================================
// Surfel model (Core/Model/Model.{h,cpp} + Core/Model/ModelProjection.{h,cpp}), pure HIP
// =============================================================================================
#include "surfel_kernels.hpp"
#include "pass_rect.hpp"

#include "model_host.hpp"

// =============================================================================================
// Keypoint descriptor matching (Core/Utils/PointTracker.cpp:100-114) on the f32 matrix cores
// =============================================================================================
#include "match_kernels.hpp"

extern "C" int mmf_match_descriptors(mmf_ctx* c, const float* query, int nq, const float* train, int nt, int dim,
                                     float max_distance, int* train_idx, float* distance) {
    MMF_REQUIRE(c && (query || nq == 0) && (train || nt == 0) && (train_idx || nq == 0) && (distance || nq == 0),
                "mmf_match_descriptors: null argument");
    MMF_REQUIRE(nq >= 0 && nt >= 0 && dim > 0 && dim % 8 == 0, "mmf_match_descriptors: dim must be a positive multiple of 8");
    MMF_REQUIRE(((uintptr_t)query & 15u) == 0 && ((uintptr_t)train & 15u) == 0, "mmf_match_descriptors: 16-byte aligned rows");
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (nq == 0) return MMF_OK;
    // workspace: [qn | tn] floats, then [row keys | col keys]
    const size_t rows = (size_t)nq + (size_t)nt;
    if (rows > c->match_ws_rows) {
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(c->match_ws);
        c->match_ws = nullptr;
        c->match_ws_rows = 0;
        const size_t cap = rows + rows / 2 + 256;
        MMF_HIP_TRY(hipMalloc(&c->match_ws, cap * (sizeof(float) + sizeof(unsigned long long))));
        c->match_ws_rows = cap;
    }
    unsigned long long* keys = static_cast<unsigned long long*>(c->match_ws);
    float* norms = reinterpret_cast<float*>(keys + c->match_ws_rows);
    unsigned long long *row_best = keys, *col_best = keys + nq;
    float *qn = norms, *tn = norms + nq;
    if (nt == 0)  // nothing to match against: every query stays unmatched
        hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, keys, rows, kNoMatchKey);
    if (nt > 0) {  // the norms kernel also resets the arg-min keys
        hipLaunchKernelGGL(row_norms_kernel, dim3((nq + 31) / 32 + (nt + 31) / 32), dim3(64), 0, c->stream, query, nq, train, nt,
                           dim, qn, tn, row_best, col_best, kNoMatchKey);
        if (dim % kMatchSlab == 0)  // 64 x 64 workgroup tiles with LDS-shared operands
            hipLaunchKernelGGL(match_tile64_kernel, dim3((nt + 63) / 64, (nq + 63) / 64), dim3(256), 0, c->stream, query, train,
                               qn, tn, nq, nt, dim, row_best, col_best);
        else
            hipLaunchKernelGGL(match_tile_kernel, dim3((nt + 31) / 32, (nq + 31) / 32), dim3(64), 0, c->stream, query, train, qn,
                               tn, nq, nt, dim, row_best, col_best);
    }
    hipLaunchKernelGGL(match_cross_check_kernel, dim3((nq + 255) / 256), dim3(256), 0, c->stream, row_best, col_best, nq,
                       max_distance, train_idx, distance);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// =============================================================================================
// RigidRANSAC (Core/Utils/RigidRANSAC.{h,cpp}): host code, see rigid_ransac.hpp; batches of
// independent problems on the device, see ransac_kernels.hpp
// =============================================================================================
#include <functional>

#include "ransac_kernels.hpp"

struct mmf_ransac {
    mmf::RigidRANSAC impl;
    mmf_ransac(int it, float thr, float frac) : impl(it, thr, frac) {}
};

static void isometry_to_4x4(const mmf::Isometry3f& T, float out[16]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[r * 4 + c] = T.R[r * 3 + c];
        out[r * 4 + 3] = T.t[r];
    }
    out[12] = out[13] = out[14] = 0.f;
    out[15] = 1.f;
}

extern "C" int mmf_rigid_fit(const float* p0, const float* p1, int n, const unsigned char* mask, float T[16]) {
    MMF_REQUIRE(p0 && p1 && T && n > 0, "mmf_rigid_fit: bad argument");
    isometry_to_4x4(mmf::rigid_fit(p0, p1, n, mask), T);
    return MMF_OK;
}

extern "C" int mmf_rigid_apply(const float T[16], const float* p0, const float* p1, int n, float* distance) {
    MMF_REQUIRE(T && p0 && p1 && distance && n >= 0, "mmf_rigid_apply: bad argument");
    mmf::Isometry3f I;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) I.R[r * 3 + c] = T[r * 4 + c];
        I.t[r] = T[r * 4 + 3];
    }
    mmf::rigid_apply(I, p0, p1, n, distance);
    return MMF_OK;
}

extern "C" int mmf_ransac_create(int iterations, float inlier_threshold, float inlier_fraction, mmf_ransac** out) {
    MMF_REQUIRE(out && iterations >= 0, "mmf_ransac_create: bad argument");
    *out = new (std::nothrow) mmf_ransac(iterations, inlier_threshold, inlier_fraction);
    MMF_REQUIRE(*out != nullptr, "mmf_ransac_create: out of host memory");
    return MMF_OK;
}

extern "C" void mmf_ransac_destroy(mmf_ransac* r) { delete r; }

extern "C" int mmf_ransac_estimate(mmf_ransac* r, const float* p0, const float* p1, int n, const unsigned char* mask,
                                   float T[16], float* error, unsigned char* inlier, int* has_inlier) {
    MMF_REQUIRE(r && p0 && p1 && T && error, "mmf_ransac_estimate: null argument");
    MMF_REQUIRE(n >= 3, "mmf_ransac_estimate: needs at least 3 correspondences (RigidRANSAC.cpp:133)");
    const mmf::RigidRANSAC::Result res = r->impl.estimate(p0, p1, n, mask);
    isometry_to_4x4(res.transformation, T);
    *error = res.error;
    if (has_inlier) *has_inlier = res.inlier.empty() ? 0 : 1;
    if (inlier)
        for (int i = 0; i < n; ++i) inlier[i] = res.inlier.empty() ? 0 : res.inlier[i];
    return MMF_OK;
}

// test hooks of the shared core (host code, no device): the restated hash beside std::hash<float>, and one problem
// through table + hash + sort + core as the device verifier runs it
extern "C" int mmf_debug_hash_float(const float* x, int n, unsigned long long* restated, unsigned long long* libstdcxx) {
    MMF_REQUIRE(x && restated && libstdcxx && n >= 0, "mmf_debug_hash_float: bad argument");
    for (int i = 0; i < n; ++i) {
        restated[i] = mmf::ransac_core::hash_float_bits(mmf::ransac_core::float_bits(x[i]));
        libstdcxx[i] = (unsigned long long)std::hash<float>()(x[i]);
    }
    return MMF_OK;
}

static bool ransac_config_ok(const mmf_ransac_config* cfg) {
    return cfg && cfg->iterations >= 1 && cfg->iterations <= mmf::kRansacMaxIterations;
}

extern "C" int mmf_debug_ransac_core_host(const mmf_ransac_config* cfg, const float* p0, const float* p1, int n, float T[16],
                                          float* error, unsigned char* inlier, int* has_inlier) {
    MMF_REQUIRE(ransac_config_ok(cfg) && p0 && p1 && T && error, "mmf_debug_ransac_core_host: bad argument");
    MMF_REQUIRE(n >= 3 && n <= 65535, "mmf_debug_ransac_core_host: needs 3 .. 65535 correspondences");
    std::vector<unsigned short> triples(3 * (size_t)cfg->iterations);
    mmf::ransac_triples(cfg->iterations, n, triples.data());
    mmf::Isometry3f I;
    const int count = mmf::ransac_core_host({cfg->iterations, cfg->inlier_threshold, cfg->inlier_fraction}, triples.data(), p0, p1, n,
                                            &I, error, inlier);
    isometry_to_4x4(I, T);
    if (has_inlier) *has_inlier = count > 0 ? 1 : 0;
    return MMF_OK;
}

extern "C" int mmf_debug_rounded_ops(mmf_ctx* c, int op, const void* a_dev, const void* b_dev, size_t n, void* out_dev) {
    MMF_REQUIRE(c && a_dev && out_dev && n > 0 && op >= 0 && op <= 5, "mmf_debug_rounded_ops: bad argument");
    MMF_REQUIRE(b_dev || op == 0 || op == 2 || op == 3, "mmf_debug_rounded_ops: the operation takes two arguments");
    MMF_HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(mmf::ransac_ops_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, op, a_dev, b_dev, n, out_dev);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// ---- mmf_ransac_batch: ragged batches of independent problems, one wave each (ransac_kernels.hpp) --------------------
struct mmf_ransac_batch {
    mmf_ctx* ctx = nullptr;
    mmf::RigidRANSAC::Config cfg{10, 0.03f, 0.8f};
    int max_points = 0;
    std::vector<unsigned short> table;  // the host core of an oversized problem reads it too
    unsigned short* table_dev = nullptr;
    int *off_pin = nullptr, *off_dev = nullptr;  // offsets on their way to the device
    size_t off_cap = 0;
    mmf_ransac_result* res_pin = nullptr;  // host memory the device writes
    size_t res_cap = 0;
    unsigned char* inl_pin = nullptr;
    size_t inl_cap = 0;
    int last_launches = 0;

    mmf::RansacDeviceConfig device_config() const {
        return mmf::RansacDeviceConfig{cfg.iterations, cfg.inlier_threshold, cfg.inlier_fraction, max_points, (max_points + 63) / 64 * 64, table_dev};
    }
};

extern "C" void mmf_ransac_batch_destroy(mmf_ransac_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    (void)hipFree(b->table_dev);
    (void)hipFree(b->off_dev);
    if (b->off_pin) (void)hipHostFree(b->off_pin);
    if (b->res_pin) (void)hipHostFree(b->res_pin);
    if (b->inl_pin) (void)hipHostFree(b->inl_pin);
    delete b;
}

// pinned buffers for n problems of `total` rows (every earlier estimate has been awaited)
static int ransac_batch_reserve(mmf_ransac_batch* b, size_t n, size_t total) {
    if (n + 1 > b->off_cap) {
        if (b->off_pin) (void)hipHostFree(b->off_pin);
        (void)hipFree(b->off_dev);
        b->off_pin = nullptr, b->off_dev = nullptr, b->off_cap = 0;
        const size_t cap = (n + 1) * 2;
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->off_pin), cap * sizeof(int), hipHostMallocDefault));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b->off_dev), cap * sizeof(int)));
        b->off_cap = cap;
    }
    if (n > b->res_cap) {
        if (b->res_pin) (void)hipHostFree(b->res_pin);
        b->res_pin = nullptr, b->res_cap = 0;
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->res_pin), n * 2 * sizeof(mmf_ransac_result), hipHostMallocMapped | hipHostMallocCoherent));
        b->res_cap = n * 2;
    }
    if (total + 1 > b->inl_cap) {
        if (b->inl_pin) (void)hipHostFree(b->inl_pin);
        b->inl_pin = nullptr, b->inl_cap = 0;
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->inl_pin), (total + 1) * 2, hipHostMallocMapped | hipHostMallocCoherent));
        b->inl_cap = (total + 1) * 2;
    }
    return MMF_OK;
}

extern "C" int mmf_ransac_batch_create(mmf_ctx* c, const mmf_ransac_config* cfg, int max_points, mmf_ransac_batch** out) {
    MMF_REQUIRE(c && out, "mmf_ransac_batch_create: null argument");
    MMF_REQUIRE(ransac_config_ok(cfg), "mmf_ransac_batch_create: 1 <= iterations <= 32");
    MMF_REQUIRE(max_points >= 3 && max_points <= mmf::kRansacMaxPoints, "mmf_ransac_batch_create: 3 <= max_points <= 1024");
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_ransac_batch* b = new (std::nothrow) mmf_ransac_batch();
    MMF_REQUIRE(b != nullptr, "mmf_ransac_batch_create: out of host memory");
    b->ctx = c;
    b->cfg = {cfg->iterations, cfg->inlier_threshold, cfg->inlier_fraction};
    b->max_points = max_points;
    b->table = mmf::ransac_triple_table(cfg->iterations, max_points);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->table_dev), b->table.size() * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMemcpyAsync(b->table_dev, b->table.data(), b->table.size() * sizeof(unsigned short), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int rc = MMF_OK;
    if (e == hipSuccess) rc = ransac_batch_reserve(b, 64, 64 * 64);
    if (e != hipSuccess || rc != MMF_OK) {
        mmf_ransac_batch_destroy(b);
        if (rc != MMF_OK) return rc;
        MMF_HIP_TRY(e);
    }
    *out = b;
    return MMF_OK;
}

extern "C" int mmf_ransac_batch_max_points(mmf_ransac_batch* b) { return b ? b->max_points : -1; }
extern "C" int mmf_ransac_batch_last_launches(mmf_ransac_batch* b) { return b ? b->last_launches : -1; }

// p0 / p1 = DEVICE [offsets[n]][3]; offsets = HOST [n + 1], offsets[0] = 0, ascending; results = HOST [n]; inlier (optional) =
// HOST [offsets[n]] over each problem's hash-sorted rows.  One launch, one wait.
extern "C" int mmf_ransac_batch_estimate(mmf_ransac_batch* b, const float* p0_dev, const float* p1_dev, const int* offsets,
                                         int n_problems, mmf_ransac_result* results, unsigned char* inlier) {
    MMF_REQUIRE(b && offsets && n_problems >= 0 && (results || n_problems == 0), "mmf_ransac_batch_estimate: bad argument");
    b->last_launches = 0;
    MMF_REQUIRE(offsets[0] == 0, "mmf_ransac_batch_estimate: offsets start at 0");
    for (int p = 0; p < n_problems; ++p) MMF_REQUIRE(offsets[p + 1] >= offsets[p], "mmf_ransac_batch_estimate: offsets must ascend");
    const size_t total = (size_t)offsets[n_problems];
    MMF_REQUIRE(total == 0 || (p0_dev && p1_dev), "mmf_ransac_batch_estimate: null points");
    if (n_problems == 0) return MMF_OK;
    MMF_HIP_TRY(hipSetDevice(b->ctx->device));
    int rc = ransac_batch_reserve(b, (size_t)n_problems, total);
    if (rc) return rc;
    hipStream_t st = b->ctx->stream;
    std::memcpy(b->off_pin, offsets, ((size_t)n_problems + 1) * sizeof(int));
    MMF_HIP_TRY(hipMemcpyAsync(b->off_dev, b->off_pin, ((size_t)n_problems + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    const mmf::RansacDeviceConfig dc = b->device_config();
    hipLaunchKernelGGL(mmf::ransac_batch_kernel, dim3((unsigned)n_problems), dim3(64), mmf::ransac_lds_bytes(dc.cap, false), st, p0_dev,
                       p1_dev, (const int*)b->off_dev, dc, b->res_pin, b->inl_pin);
    MMF_HIP_TRY(hipGetLastError());
    b->last_launches = 1;
    MMF_HIP_TRY(wait_stream(st));
    std::memcpy(results, b->res_pin, (size_t)n_problems * sizeof(mmf_ransac_result));
    if (inlier && total) std::memcpy(inlier, b->inl_pin, total);
    return MMF_OK;
}

// ---------------------------------------------------------------------------------------------
// Keypoint redetection: the view store and Model::getBestMatch (Core/Model/Model.cpp:781-874)
// ---------------------------------------------------------------------------------------------
#include "redetect_host.hpp"

// ---------------------------------------------------------------------------------------------
// Keypoint tracks on the device: tracker::PointTracker and the per-model track sets
// (Core/Utils/PointTracker.cpp:27-226; Core/Model/Model.cpp:630-640, 739-775)
// ---------------------------------------------------------------------------------------------
#include "tracker_host.hpp"

// ---------------------------------------------------------------------------------------------
// SuperPoint keypoint network (Core/MultiMotionFusion.cpp:78,233)
// ---------------------------------------------------------------------------------------------
#include "superpoint_host.hpp"

// ---------------------------------------------------------------------------------------------
// Super-pixel resampling for the segmentation (Core/Segmentation/Slic.h:48-146)
// ---------------------------------------------------------------------------------------------
#include "slic_kernels.hpp"

struct SlicWs {
    mmf::SlicBox* box;
    int *counts, *dcounts, *rgb_sums;
    float* sums;
};

static int slic_workspace(mmf_ctx* c, int n, SlicWs* ws) {
    if ((size_t)n > c->slic_ws_n) {
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(c->slic_ws);
        c->slic_ws = nullptr, c->slic_ws_n = 0;
        const size_t cap = (size_t)n + n / 2 + 64;
        MMF_HIP_TRY(hipMalloc(&c->slic_ws, cap * (sizeof(mmf::SlicBox) + 6 * sizeof(int))));
        c->slic_ws_n = cap;
    }
    const size_t cap = c->slic_ws_n;
    ws->box = static_cast<mmf::SlicBox*>(c->slic_ws);
    ws->counts = reinterpret_cast<int*>(ws->box + cap);
    ws->dcounts = ws->counts + cap;
    ws->rgb_sums = ws->dcounts + cap;
    ws->sums = reinterpret_cast<float*>(ws->rgb_sums + 3 * cap);
    return MMF_OK;
}

static int slic_check(const int* labels, int width, int height, int spixel_size, const char* who) {
    if (!labels || width <= 0 || height <= 0) return fail(MMF_ERR_INVALID, std::string(who) + ": bad label image");
    // Slic::Slic asserts spixelSize in (10, 256) (Slic.cpp:23)
    if (!(spixel_size > 10 && spixel_size < 256) || width / spixel_size < 1 || height / spixel_size < 1)
        return fail(MMF_ERR_INVALID, std::string(who) + ": super-pixel size must be in (10, 256) and fit the image");
    return MMF_OK;
}

extern "C" int mmf_slic_downsample(mmf_ctx* c, const int* labels, int width, int height, int spixel_size, const float* image,
                                   int channels, int channel, int thresholded, float min_threshold, float* out,
                                   int* counts_out) {
    MMF_REQUIRE(c && image && out, "mmf_slic_downsample: null argument");
    MMF_REQUIRE(channels >= 1 && channel >= 0 && channel < channels, "mmf_slic_downsample: bad channel");
    if (int rc = slic_check(labels, width, height, spixel_size, "mmf_slic_downsample")) return rc;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int spx = width / spixel_size, spy = height / spixel_size, n = spx * spy, npix = width * height;
    SlicWs ws;
    if (int rc = slic_workspace(c, n, &ws)) return rc;
    using namespace mmf;
    hipLaunchKernelGGL(slic_reset_kernel, grid1d(n), dim3(256), 0, c->stream, n, ws.box, ws.counts, ws.rgb_sums);
    hipLaunchKernelGGL(slic_census_kernel, grid1d(npix), dim3(256), 0, c->stream, labels, width, height, n, ws.box, ws.counts,
                       (const uint8_t*)nullptr, 0, ws.rgb_sums);
    hipLaunchKernelGGL(slic_sum_kernel, dim3((n + 3) / 4), dim3(256), 0, c->stream, labels, width, n, image, channels, channel,
                       thresholded ? 1 : 0, min_threshold, ws.box, ws.sums, ws.dcounts);
    hipLaunchKernelGGL(slic_finish_kernel, grid1d(n), dim3(256), 0, c->stream, labels, width, height, spixel_size, spx, spy,
                       ws.counts, thresholded ? ws.dcounts : ws.counts, ws.sums, out);
    MMF_HIP_TRY(hipGetLastError());
    if (counts_out) MMF_HIP_TRY(hipMemcpyAsync(counts_out, ws.counts, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    return MMF_OK;
}

extern "C" int mmf_slic_downsample_rgb(mmf_ctx* c, const int* labels, int width, int height, int spixel_size,
                                       const uint8_t* rgb, int channels, uint8_t* out) {
    MMF_REQUIRE(c && rgb && out, "mmf_slic_downsample_rgb: null argument");
    MMF_REQUIRE(channels == 3 || channels == 4, "mmf_slic_downsample_rgb: 3 or 4 channels");
    if (int rc = slic_check(labels, width, height, spixel_size, "mmf_slic_downsample_rgb")) return rc;
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int spx = width / spixel_size, spy = height / spixel_size, n = spx * spy, npix = width * height;
    SlicWs ws;
    if (int rc = slic_workspace(c, n, &ws)) return rc;
    using namespace mmf;
    hipLaunchKernelGGL(slic_reset_kernel, grid1d(n), dim3(256), 0, c->stream, n, ws.box, ws.counts, ws.rgb_sums);
    hipLaunchKernelGGL(slic_census_kernel, grid1d(npix), dim3(256), 0, c->stream, labels, width, height, n, ws.box, ws.counts,
                       rgb, channels, ws.rgb_sums);
    hipLaunchKernelGGL(slic_finish_rgb_kernel, grid1d(n), dim3(256), 0, c->stream, labels, width, height, spixel_size, spx, spy,
                       ws.counts, ws.rgb_sums, out);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

extern "C" int mmf_slic_upsample_u8(mmf_ctx* c, const int* labels, int width, int height, const uint8_t* map, int nspix,
                                    uint8_t* out) {
    MMF_REQUIRE(c && labels && map && out && width > 0 && height > 0 && nspix > 0, "mmf_slic_upsample_u8: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    const int npix = width * height;
    hipLaunchKernelGGL(mmf::slic_upsample_u8_kernel, grid1d(npix), dim3(256), 0, c->stream, labels, npix, nspix, map, out);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// ---- the super-pixel engine (slic_engine_kernels.hpp) -----------------------------------------------------
#include "slic_engine_kernels.hpp"

// centres [cells][8] float, counts [cells] int, labels [pixels] int in one allocation (a context's, or a fusion's own:
// the fusion runs the engine on a stream of its own)
struct SlicEngineWs {
    void* mem = nullptr;
    size_t cells = 0, pixels = 0;
    float* centres() const { return static_cast<float*>(mem); }
    int* counts() const { return reinterpret_cast<int*>(centres() + cells * mmf::kSlicCentreStride); }
    int* labels() const { return counts() + ((cells + 3) & ~(size_t)3); }  // (16-byte aligned: one store per four labels)
};

// `quiet`: the stream whose enqueued work may still use the old allocation
static int slic_engine_workspace(SlicEngineWs* ws, size_t cells, size_t pixels, hipStream_t quiet) {
    if (cells <= ws->cells && pixels <= ws->pixels) return MMF_OK;
    cells = std::max(cells, ws->cells), pixels = std::max(pixels, ws->pixels);
    MMF_HIP_TRY(hipStreamSynchronize(quiet));
    (void)hipFree(ws->mem);
    ws->mem = nullptr, ws->cells = ws->pixels = 0;
    const size_t bytes = cells * mmf::kSlicCentreStride * sizeof(float) + ((cells + 3) & ~(size_t)3) * sizeof(int) + pixels * sizeof(int);
    MMF_HIP_TRY(hipMalloc(&ws->mem, bytes));
    ws->cells = cells, ws->pixels = pixels;
    return MMF_OK;
}

// S in (10, 256) and dividing both sides: gSLICr's map is ceil(W/S) x ceil(H/S) while Slic.h sizes everything by
// (W/S) (H/S) -- on a ragged image the reference indexes past its own arrays
static int slic_engine_check(int width, int height, int spixel_size, const char* who) {
    if (width <= 0 || height <= 0 || !(spixel_size > 10 && spixel_size < 256))
        return fail(MMF_ERR_INVALID, std::string(who) + ": super-pixel size must be in (10, 256)");
    if (width % spixel_size != 0 || height % spixel_size != 0 || (long long)width * height > (long long)INT_MAX / 4)
        return fail(MMF_ERR_INVALID, std::string(who) + ": the super-pixel size must divide the image's width and height (" +
                                         std::to_string(width) + " x " + std::to_string(height) + ", S = " + std::to_string(spixel_size) + ")");
    return MMF_OK;
}

// initialise; iterations x (associate, update); associate -- 2 + 2 * iterations launches on `st` (+ 1 for centres_out);
// labels_out == nullptr: the workspace's label image (the fusion's)
static int slic_engine_enqueue(const SlicEngineWs& ws, hipStream_t st, const uint8_t* rgb, int W, int H, int S, int iterations,
                               const float* centres_in, int* labels_out, float* centres_out, int* counts_out) {
    using namespace mmf;
    SlicEngineGeom g;
    g.W = W, g.H = H, g.S = S, g.mx = W / S, g.my = H / S;
    const float t = 1.0f / (1.4242f * (float)S), u = 5.0f / (1.7321f * 128.0f);
    g.nxy = t * t, g.nc = u * u;
    const int n = g.mx * g.my;
    int* labels = labels_out ? labels_out : ws.labels();
    const int vec = (reinterpret_cast<uintptr_t>(rgb) % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 16 == 0) ? 1 : 0;
    const dim3 agrid = grid1d(((size_t)W * H + 3) / 4);
    hipLaunchKernelGGL(slic_engine_init_kernel, grid1d(n), dim3(256), 0, st, g, rgb, centres_in, ws.centres(), ws.counts());
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(slic_engine_associate_kernel, agrid, dim3(256), 0, st, g, rgb, (const float*)ws.centres(), labels, vec);
        hipLaunchKernelGGL(slic_engine_update_kernel, dim3(n), dim3(256), 0, st, g, rgb, (const int*)labels, ws.centres(), ws.counts());
    }
    hipLaunchKernelGGL(slic_engine_associate_kernel, agrid, dim3(256), 0, st, g, rgb, (const float*)ws.centres(), labels, vec);
    if (centres_out) hipLaunchKernelGGL(slic_engine_export_kernel, grid1d(n), dim3(256), 0, st, n, (const float*)ws.centres(), centres_out);
    MMF_HIP_TRY(hipGetLastError());
    if (counts_out) MMF_HIP_TRY(hipMemcpyAsync(counts_out, ws.counts(), (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    return MMF_OK;
}

extern "C" int mmf_slic_segment(mmf_ctx* c, const uint8_t* rgb, int width, int height, int spixel_size, int iterations,
                                const float* centres_in, int* labels_out, float* centres_out, int* counts_out) {
    MMF_REQUIRE(c && rgb && labels_out, "mmf_slic_segment: null argument");
    MMF_REQUIRE(iterations >= 0 && iterations <= 1000, "mmf_slic_segment: iterations must be in [0, 1000]");
    if (int rc = slic_engine_check(width, height, spixel_size, "mmf_slic_segment")) return rc;
    MMF_HIP_TRY(hipSetDevice(c->device));
    SlicEngineWs ws;
    ws.mem = c->slic_engine_ws, ws.cells = c->slic_engine_cells, ws.pixels = 0;
    const int rc = slic_engine_workspace(&ws, (size_t)(width / spixel_size) * (height / spixel_size), 0, c->stream);
    c->slic_engine_ws = ws.mem, c->slic_engine_cells = ws.cells;
    if (rc) return rc;
    return slic_engine_enqueue(ws, c->stream, rgb, width, height, spixel_size, iterations, centres_in, labels_out, centres_out, counts_out);
}

// ---- dense-CRF motion segmentation (crf_kernels.hpp; Segmentation.cpp:159-740) ---------------------------------------
#include "crf_kernels.hpp"

struct CrfWs {
    size_t cells = 0;        // capacity in super-pixels (every per-cell buffer holds kCrfMaxLabels rows where it has labels)
    size_t partial_n = 0;    // floats of `partial`
    float *low_depth = nullptr, *maps = nullptr, *U = nullptr, *feat = nullptr, *Q = nullptr, *xs = nullptr, *xa = nullptr;
    float *Ds = nullptr, *Da = nullptr, *ones = nullptr, *partial = nullptr;
    int *cstat = nullptr, *cid = nullptr, *flabel = nullptr;
    uint8_t *raw_map = nullptr, *map = nullptr;
    mmf::CrfSummary* sum_dev = nullptr;
    mmf::CrfSummary* sum_host = nullptr;  // pinned
    int* grid = nullptr;  // B3 labels
    size_t grid_cap = 0;
    int grid_w = 0, grid_h = 0, grid_s = 0;
    bool valid = false;  // a segmentation ran (mmf_crf_last)
    int cells_x = 0, cells_y = 0;
};

static void crf_ws_free(CrfWs* w) {
    if (!w) return;
    for (void* p : {(void*)w->low_depth, (void*)w->maps, (void*)w->U, (void*)w->feat, (void*)w->Q, (void*)w->xs, (void*)w->xa,
                    (void*)w->Ds, (void*)w->Da, (void*)w->ones, (void*)w->partial, (void*)w->cstat, (void*)w->cid,
                    (void*)w->flabel, (void*)w->raw_map, (void*)w->map, (void*)w->sum_dev, (void*)w->grid})
        (void)hipFree(p);
    (void)hipHostFree(w->sum_host);
    delete w;
}

static int crf_workspace(mmf_ctx* c, size_t n, size_t partial_n, CrfWs** out) {
    if (!c->crf_ws) {
        c->crf_ws = new (std::nothrow) CrfWs();
        MMF_REQUIRE(c->crf_ws != nullptr, "mmf_crf: out of host memory");
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->crf_ws->sum_dev), sizeof(mmf::CrfSummary)));
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->crf_ws->sum_host), sizeof(mmf::CrfSummary), hipHostMallocDefault));
    }
    CrfWs* w = c->crf_ws;
    if (n > w->cells) {
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
        for (void** p : {(void**)&w->low_depth, (void**)&w->maps, (void**)&w->U, (void**)&w->feat, (void**)&w->Q, (void**)&w->xs,
                         (void**)&w->xa, (void**)&w->Ds, (void**)&w->Da, (void**)&w->ones, (void**)&w->cstat, (void**)&w->cid,
                         (void**)&w->flabel, (void**)&w->raw_map, (void**)&w->map}) {
            (void)hipFree(*p);
            *p = nullptr;
        }
        w->cells = 0, w->valid = false;
        const size_t L = mmf::kCrfMaxLabels;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->low_depth), n * sizeof(float)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->maps), 2 * L * n * sizeof(float)));
        for (float** p : {&w->U, &w->Q, &w->xs, &w->xa}) MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), L * n * sizeof(float)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->feat), 8 * n * sizeof(float)));
        for (float** p : {&w->Ds, &w->Da, &w->ones}) MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), n * sizeof(float)));
        MMF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w->ones), 0x3f800000, n, c->stream));  // 1.0f
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->cstat), 6 * n * sizeof(int)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->cid), n * sizeof(int)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->flabel), n * sizeof(int)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->raw_map), n));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->map), n));
        w->cells = n;
    }
    if (partial_n > w->partial_n) {
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(w->partial);
        w->partial = nullptr, w->partial_n = 0;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->partial), partial_n * sizeof(float)));
        w->partial_n = partial_n;
    }
    *out = w;
    return MMF_OK;
}

extern "C" int mmf_crf_default_config(mmf_crf_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_crf_default_config: null argument");
    // GUI/Tools/GUI.h:211-226, pushed by GUI/MainController.cpp:658-670 before any segmentation runs
    // (the Segmentation.h:140-159 member defaults 1/30, 1/0.4, 1/8, 40, 40, 5, 0.01, 40, 10, 0.07 / 0.4 never reach a frame)
    cfg->sigma_rgb = 10.f, cfg->sigma_depth = 0.9f, cfg->sigma_pos = 1.8f;
    cfg->weight_appearance = 7.f, cfg->weight_smoothness = 2.f;
    cfg->threshold_new = 5.5f, cfg->unary_weight_error = 75.f, cfg->unary_k_error = 0.0375f;
    cfg->iterations = 10;
    cfg->min_rel_size_new = 0.005f, cfg->max_rel_size_new = 0.4f;
    cfg->spixel_size = 16;  // SegmentationConfiguration::sp_size (Segmentation.h:79)
    cfg->model_spawn_offset = 22;
    cfg->inhibit_new = 0;
    return MMF_OK;
}

static int crf_check_config(const mmf_crf_config* cfg, const char* who) {
    MMF_REQUIRE(cfg != nullptr, std::string(who) + ": null configuration");
    if (!(cfg->sigma_rgb > 0.f && cfg->sigma_depth > 0.f && cfg->sigma_pos > 0.f) || cfg->iterations < 0 ||
        cfg->model_spawn_offset < 0 || !(cfg->spixel_size > 10 && cfg->spixel_size < 256))
        return fail(MMF_ERR_INVALID, std::string(who) + ": bad CRF configuration (sigmas > 0, iterations >= 0, spixel_size in (10, 256))");
    return MMF_OK;
}

// stages 2-14 on the context's stream, from the stage-1 maps in w->low_depth and `maps`; the summary is copied to pinned
// memory behind them (the caller synchronises)
static int crf_enqueue(mmf_ctx* c, CrfWs* w, const mmf_crf_config* cfg, const int* labels, int W, int H, const uint8_t* rgb,
                       const float* maps, const unsigned* ids, int M, unsigned next_id, int allow_new, uint8_t* mask_out) {
    using namespace mmf;
    const int S = cfg->spixel_size, spx = W / S, spy = H / S, N = spx * spy, L = M + (allow_new ? 1 : 0);
    hipStream_t st = c->stream;
    CrfParams p;
    p.scale_rgb = 1.0f / cfg->sigma_rgb, p.scale_depth = 1.0f / cfg->sigma_depth, p.scale_pos = 1.0f / cfg->sigma_pos;
    p.w_app = cfg->weight_appearance, p.w_smooth = cfg->weight_smoothness;
    p.thr_new = cfg->threshold_new, p.w_err = cfg->unary_weight_error, p.k_err = cfg->unary_k_error;
    p.min_rel = cfg->min_rel_size_new, p.max_rel = cfg->max_rel_size_new;
    hipLaunchKernelGGL(crf_prep_kernel, dim3(1), dim3(1024), 0, st, w->low_depth, maps, rgb, N, spx, M, allow_new, p, w->U, w->feat,
                       w->sum_dev);
    const int nsplit = (N + kCrfTJ - 1) / kCrfTJ;
    const dim3 pgrid((N + kCrfTI - 1) / kCrfTI, nsplit), cgrid((N + 255) / 256);
    auto pair = [&](int Lp, const float* xs, const float* xa) {
        if (Lp <= 1) hipLaunchKernelGGL(crf_pair_kernel<1>, pgrid, dim3(256), 0, st, w->feat, N, Lp, xs, xa, w->partial);
        else if (Lp <= 2) hipLaunchKernelGGL(crf_pair_kernel<2>, pgrid, dim3(256), 0, st, w->feat, N, Lp, xs, xa, w->partial);
        else if (Lp <= 4) hipLaunchKernelGGL(crf_pair_kernel<4>, pgrid, dim3(256), 0, st, w->feat, N, Lp, xs, xa, w->partial);
        else if (Lp <= 8) hipLaunchKernelGGL(crf_pair_kernel<8>, pgrid, dim3(256), 0, st, w->feat, N, Lp, xs, xa, w->partial);
        else if (Lp <= 16) hipLaunchKernelGGL(crf_pair_kernel<16>, pgrid, dim3(256), 0, st, w->feat, N, Lp, xs, xa, w->partial);
        else hipLaunchKernelGGL(crf_pair_kernel<32>, pgrid, dim3(256), 0, st, w->feat, N, Lp, xs, xa, w->partial);
    };
    auto softmax = [&](int mode, const float* part) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, cgrid, dim3(256), 0, st, mode, N, L, nsplit, part, (const float*)w->U, p.w_smooth, p.w_app, w->Ds,
                               w->Da, w->Q, w->xs, w->xa, (const CrfSummary*)w->sum_dev);
        };
        if (L <= 2) go(crf_softmax_kernel<2>);
        else if (L <= 4) go(crf_softmax_kernel<4>);
        else if (L <= 8) go(crf_softmax_kernel<8>);
        else if (L <= 16) go(crf_softmax_kernel<16>);
        else go(crf_softmax_kernel<32>);
    };
    const int iters = cfg->iterations;
    if (iters > 0) pair(1, w->ones, w->ones);
    softmax(0, iters > 0 ? (const float*)w->partial : nullptr);
    for (int it = 0; it < iters; ++it) {
        pair(L, w->xs, w->xa);
        softmax(1, w->partial);
    }
    CrfPostArgs a;
    a.Q = w->Q, a.low_depth = w->low_depth;
    a.N = N, a.spx = spx, a.spy = spy, a.W = W, a.H = H, a.S = S, a.L = L, a.M = M, a.allow_new = allow_new ? 1 : 0;
    a.next_id = next_id;
    for (int l = 0; l < kCrfMaxLabels; ++l) a.ids[l] = l < M ? ids[l] : (l == M ? next_id : 255u);
    a.min_rel = p.min_rel, a.max_rel = p.max_rel;
    a.cstat = w->cstat, a.cid = w->cid, a.flabel = w->flabel, a.raw_map = w->raw_map, a.map = w->map, a.sum = w->sum_dev;
    const size_t lds = (size_t)N * sizeof(int) + (((size_t)N + 3) & ~(size_t)3);
    MMF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(crf_post_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(crf_post_kernel, dim3(1), dim3(1024), lds, st, a);
    hipLaunchKernelGGL(slic_upsample_u8_kernel, grid1d((size_t)W * H), dim3(256), 0, st, labels, W * H, N, (const uint8_t*)w->map, mask_out);
    MMF_HIP_TRY(hipGetLastError());
    MMF_HIP_TRY(hipMemcpyAsync(w->sum_host, w->sum_dev, sizeof(CrfSummary), hipMemcpyDeviceToHost, st));
    w->valid = true, w->cells_x = spx, w->cells_y = spy;
    return MMF_OK;
}

// checks shared by the stand-alone call and the fusion; *labels_out = the label image to use (the grid when labels is NULL)
static int crf_begin(mmf_ctx* c, const mmf_crf_config* cfg, const int* labels, int W, int H, const unsigned* ids, int M,
                     unsigned next_id, int allow_new, const char* who, CrfWs** ws, const int** labels_out) {
    if (int rc = crf_check_config(cfg, who)) return rc;
    const int S = cfg->spixel_size;
    MMF_REQUIRE(W > 0 && H > 0 && W / S >= 1 && H / S >= 1, std::string(who) + ": the image is smaller than one super-pixel");
    const int N = (W / S) * (H / S), L = M + (allow_new ? 1 : 0);
    MMF_REQUIRE(M >= 1 && L <= mmf::kCrfMaxLabels, std::string(who) + ": 1 to 32 labels (models + the new one)");
    MMF_REQUIRE(N <= mmf::kCrfMaxCells, std::string(who) + ": at most 16384 super-pixels");
    for (int i = 0; i < M; ++i) {
        MMF_REQUIRE(ids[i] < 255u, std::string(who) + ": model ids must be below 255");
        for (int j = 0; j < i; ++j) MMF_REQUIRE(ids[i] != ids[j], std::string(who) + ": duplicate model id");
        MMF_REQUIRE(!allow_new || ids[i] != next_id, std::string(who) + ": the new label's id is a model's");
    }
    MMF_REQUIRE(!allow_new || next_id < 255u, std::string(who) + ": the new label's id must be below 255");
    const size_t nsplit = (size_t)(N + mmf::kCrfTJ - 1) / mmf::kCrfTJ;
    CrfWs* w = nullptr;
    if (int rc = crf_workspace(c, (size_t)N, nsplit * 2 * (size_t)std::max(L, 1) * (size_t)N, &w)) return rc;
    if (!labels) {  // B3
        if (w->grid_w != W || w->grid_h != H || w->grid_s != S) {
            if ((size_t)W * H > w->grid_cap) {
                MMF_HIP_TRY(hipStreamSynchronize(c->stream));
                (void)hipFree(w->grid);
                w->grid = nullptr, w->grid_cap = 0;
                MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->grid), (size_t)W * H * sizeof(int)));
                w->grid_cap = (size_t)W * H;
            }
            hipLaunchKernelGGL(mmf::crf_grid_labels_kernel, grid1d((size_t)W * H), dim3(256), 0, c->stream, W, H, S, W / S, H / S, w->grid);
            MMF_HIP_TRY(hipGetLastError());
            w->grid_w = W, w->grid_h = H, w->grid_s = S;
        }
        labels = w->grid;
    }
    *ws = w, *labels_out = labels;
    return MMF_OK;
}

static void crf_models_out(const mmf::CrfSummary& s, mmf_segmentation_model* models_out, int* n_models_out, int* has_new_label) {
    if (models_out)
        for (int i = 0; i < s.n_models_out; ++i) models_out[i] = s.models[i];
    if (n_models_out) *n_models_out = s.n_models_out;
    if (has_new_label) *has_new_label = s.has_new_label;
}

extern "C" int mmf_crf_segment(mmf_ctx* c, const mmf_crf_config* cfg, const int* labels, int width, int height, const uint8_t* rgb,
                               const float* depth, const float* low_maps, const unsigned* ids, int n_models, unsigned next_id,
                               int allow_new, uint8_t* mask_out, mmf_segmentation_model* models_out, int* n_models_out,
                               int* has_new_label) {
    MMF_REQUIRE(c && rgb && depth && low_maps && ids && mask_out, "mmf_crf_segment: null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    CrfWs* w = nullptr;
    const int* lab = nullptr;
    if (int rc = crf_begin(c, cfg, labels, width, height, ids, n_models, next_id, allow_new, "mmf_crf_segment", &w, &lab)) return rc;
    // stage 1 of the depth (:178); the models' maps come in
    if (int rc = mmf_slic_downsample(c, lab, width, height, cfg->spixel_size, depth, 1, 0, 1, 0.02f, w->low_depth, nullptr)) return rc;
    if (int rc = crf_enqueue(c, w, cfg, lab, width, height, rgb, low_maps, ids, n_models, next_id, allow_new, mask_out)) return rc;
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    crf_models_out(*w->sum_host, models_out, n_models_out, has_new_label);
    return MMF_OK;
}

extern "C" int mmf_crf_last(mmf_ctx* c, mmf_crf_info* info, mmf_segmentation_model* models, int capacity, float* unaries, float* q,
                            uint8_t* raw_map, uint8_t* map) {
    MMF_REQUIRE(c != nullptr, "mmf_crf_last: null context");
    CrfWs* w = c->crf_ws;
    MMF_REQUIRE(w && w->valid, "mmf_crf_last: no segmentation has run on this context");
    MMF_HIP_TRY(hipSetDevice(c->device));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    const mmf::CrfSummary& s = *w->sum_host;
    const size_t N = (size_t)s.n_cells, L = (size_t)s.n_labels;
    if (info) {
        info->n_cells = s.n_cells, info->cells_x = w->cells_x, info->cells_y = w->cells_y;
        info->n_labels = s.n_labels, info->n_models = s.n_models_out;
        info->allow_new = s.allow_new, info->has_new_label = s.has_new_label, info->range_invalid = s.range_invalid;
        info->n_components = s.n_components, info->range = s.range;
    }
    if (models)
        for (int i = 0; i < s.n_models_out && i < capacity; ++i) models[i] = s.models[i];
    if (unaries) MMF_HIP_TRY(hipMemcpyAsync(unaries, w->U, L * N * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (q) MMF_HIP_TRY(hipMemcpyAsync(q, w->Q, L * N * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (raw_map) MMF_HIP_TRY(hipMemcpyAsync(raw_map, w->raw_map, N, hipMemcpyDeviceToDevice, c->stream));
    if (map) MMF_HIP_TRY(hipMemcpyAsync(map, w->map, N, hipMemcpyDeviceToDevice, c->stream));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    return MMF_OK;
}

// ---- segmentation from a frame's given label image (mask_kernels.hpp; Segmentation.cpp:89-147) ----------------------------
#include "mask_kernels.hpp"

struct MaskWs {
    double* slab = nullptr;  // [2][rows][256]: the workgroups' float64 partial sums of pass 1 and pass 2
    size_t rows = 0;
    unsigned *cnt = nullptr, *first = nullptr;  // [256] pixels / smallest pixel index per label (zero / ~0 between calls)
    mmf::MaskPlan* plan = nullptr;
    mmf::MaskSummary* sum_dev = nullptr;
    mmf::MaskSummary* sum_host = nullptr;  // pinned
};

static void mask_ws_free(MaskWs* w) {
    if (!w) return;
    for (void* p : {(void*)w->slab, (void*)w->cnt, (void*)w->first, (void*)w->plan, (void*)w->sum_dev}) (void)hipFree(p);
    (void)hipHostFree(w->sum_host);
    delete w;
}

static int mask_workspace(mmf_ctx* c, size_t rows, MaskWs** out) {
    if (!c->mask_ws) {
        c->mask_ws = new (std::nothrow) MaskWs();
        MMF_REQUIRE(c->mask_ws != nullptr, "mmf_mask: out of host memory");
        MaskWs* w = c->mask_ws;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->cnt), 256 * sizeof(unsigned)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->first), 256 * sizeof(unsigned)));
        MMF_HIP_TRY(hipMemsetAsync(w->cnt, 0, 256 * sizeof(unsigned), c->stream));
        MMF_HIP_TRY(hipMemsetAsync(w->first, 0xff, 256 * sizeof(unsigned), c->stream));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->plan), sizeof(mmf::MaskPlan)));
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->sum_dev), sizeof(mmf::MaskSummary)));
        MMF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w->sum_host), sizeof(mmf::MaskSummary), hipHostMallocDefault));
    }
    MaskWs* w = c->mask_ws;
    if (rows > w->rows) {
        MMF_HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(w->slab);
        w->slab = nullptr, w->rows = 0;
        MMF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->slab), 2 * rows * 256 * sizeof(double)));
        w->rows = rows;
    }
    *out = w;
    return MMF_OK;
}

// checks shared by the stand-alone call and the fusion, then the four launches and the summary's copy on the context's stream.
// labels / depth / mask_out: DEVICE; ids / mapping: HOST.  The result is in ws->sum_host once the stream has drained.
static int mask_enqueue(mmf_ctx* c, int W, int H, const uint8_t* labels, const float* depth, const unsigned* ids, int M,
                        unsigned next_id, int allow_new, const uint8_t* mapping, uint8_t* mask_out, const char* who, MaskWs** ws) {
    using namespace mmf;
    MMF_REQUIRE(W > 0 && H > 0 && (long long)W * H < (1ll << 31), std::string(who) + ": bad image size");
    MMF_REQUIRE(M >= 1 && M <= 255, std::string(who) + ": 1 to 255 models");
    MMF_REQUIRE(ids[0] == 0u, std::string(who) + ": the first model of the list is the global one (id 0)");
    MMF_REQUIRE(next_id <= 255u, std::string(who) + ": the new label's id must fit the id image (<= 255)");
    for (int i = 0; i < M; ++i) {
        MMF_REQUIRE(ids[i] <= 255u, std::string(who) + ": model ids must fit the id image (<= 255)");
        for (int j = 0; j < i; ++j) MMF_REQUIRE(ids[i] != ids[j], std::string(who) + ": duplicate model id");
        MMF_REQUIRE(!allow_new || ids[i] != next_id, std::string(who) + ": the new label's id is a model's");
    }
    const size_t n = (size_t)W * H;
    MMF_REQUIRE(labels + n <= mask_out || mask_out + n <= labels, std::string(who) + ": mask_out overlaps the label image");
    const size_t rows = (n + kMaskTile - 1) / kMaskTile;
    MaskWs* w = nullptr;
    if (int rc = mask_workspace(c, rows, &w)) return rc;
    MaskArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = (int)n, a.n_models = M, a.allow_new = allow_new ? 1 : 0, a.next_id = next_id;
    for (int i = 0; i < M; ++i) a.ids[i] = (uint8_t)ids[i];
    std::memcpy(a.mapping, mapping, 256);
    hipStream_t st = c->stream;
    double *slab1 = w->slab, *slab2 = w->slab + rows * 256;
    const bool vec = reinterpret_cast<uintptr_t>(labels) % 4 == 0 && reinterpret_cast<uintptr_t>(mask_out) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(depth) % 16 == 0;
    const dim3 grid((unsigned)rows), block(kMaskThreads);
    if (vec)
        hipLaunchKernelGGL((mask_bins_kernel<1, true>), grid, block, 0, st, labels, depth, a.n, (const MaskPlan*)nullptr, (uint8_t*)nullptr,
                           slab1, w->cnt, w->first);
    else
        hipLaunchKernelGGL((mask_bins_kernel<1, false>), grid, block, 0, st, labels, depth, a.n, (const MaskPlan*)nullptr, (uint8_t*)nullptr,
                           slab1, w->cnt, w->first);
    hipLaunchKernelGGL(mask_decide_kernel, dim3(1), dim3(256), 0, st, a, (const double*)slab1, (int)rows, (const unsigned*)w->cnt,
                       (const unsigned*)w->first, w->plan);
    if (vec)
        hipLaunchKernelGGL((mask_bins_kernel<2, true>), grid, block, 0, st, labels, depth, a.n, (const MaskPlan*)w->plan, mask_out, slab2,
                           (unsigned*)nullptr, (unsigned*)nullptr);
    else
        hipLaunchKernelGGL((mask_bins_kernel<2, false>), grid, block, 0, st, labels, depth, a.n, (const MaskPlan*)w->plan, mask_out, slab2,
                           (unsigned*)nullptr, (unsigned*)nullptr);
    hipLaunchKernelGGL(mask_finish_kernel, dim3(1), dim3(256), 0, st, a, (const double*)slab2, (int)rows, (const MaskPlan*)w->plan, w->cnt,
                       w->first, w->sum_dev);
    if (const hipError_t e = hipGetLastError()) {
        // a launch was refused: whatever went out before it may have left counts in the integer bins that only the finish
        // launch clears, so they are re-armed here, behind that work, for the next call on this context
        (void)hipMemsetAsync(w->cnt, 0, 256 * sizeof(unsigned), st);
        (void)hipMemsetAsync(w->first, 0xff, 256 * sizeof(unsigned), st);
        return fail(MMF_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    MMF_HIP_TRY(hipMemcpyAsync(w->sum_host, w->sum_dev, sizeof(MaskSummary), hipMemcpyDeviceToHost, st));
    *ws = w;
    return MMF_OK;
}

extern "C" int mmf_mask_default_config(mmf_mask_config* cfg) {
    MMF_REQUIRE(cfg != nullptr, "mmf_mask_default_config: cfg is null");
    cfg->model_spawn_offset = 22;  // (as mmf_crf_default_config: what the GUI pushes into setModelSpawnOffset)
    cfg->inhibit_new = 0;
    return MMF_OK;
}

extern "C" int mmf_mask_segment(mmf_ctx* c, int width, int height, const uint8_t* labels, const float* depth, const unsigned* ids,
                                int n_models, unsigned next_id, int allow_new, uint8_t mapping[256], uint8_t* mask_out,
                                mmf_segmentation_model* models_out, int* n_models_out, int* has_new_label, int* new_label) {
    MMF_REQUIRE(c && labels && depth && ids && mapping && mask_out, "mmf_mask_segment: null argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    MaskWs* w = nullptr;
    if (int rc = mask_enqueue(c, width, height, labels, depth, ids, n_models, next_id, allow_new, mapping, mask_out, "mmf_mask_segment", &w))
        return rc;
    MMF_HIP_TRY(hipStreamSynchronize(c->stream));
    const mmf::MaskSummary& s = *w->sum_host;
    std::memcpy(mapping, s.mapping, 256);
    if (models_out)
        for (int i = 0; i < s.n_models_out; ++i) models_out[i] = s.models[i];
    if (n_models_out) *n_models_out = s.n_models_out;
    if (has_new_label) *has_new_label = s.has_new_label;
    if (new_label) *new_label = s.new_label;
    return MMF_OK;
}

// the two exponentials of the surfel path as the gfx950 build evaluates them -- mmf_expf (include/mmf_math.h: surfel
// confidence, SuperPoint softmax, scalar bilateral filter) and the packed expf_nonpositive2 of the two-pixel bilateral
// filter -- on caller-supplied arguments, so that a test can hold BOTH against a float64 exp instead of against the
// oracle that shares their source
__global__ void debug_expf_kernel(const float* __restrict__ x, int n, float* __restrict__ out_mmf, float* __restrict__ out_pk) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i >= n) return;
    const float a = x[i], b = i + 1 < n ? x[i + 1] : 0.f;
    out_mmf[i] = mmf_expf(a);
    if (i + 1 < n) out_mmf[i + 1] = mmf_expf(b);
    const v2fs arg[1] = {v2fs{a, b}};
    v2fs e[1];
    expf_nonpositive2<1>(arg, e);
    out_pk[i] = e[0].x;
    if (i + 1 < n) out_pk[i + 1] = e[0].y;
}
extern "C" int mmf_debug_expf(mmf_ctx* c, const float* x_dev, int n, float* out_mmf_dev, float* out_packed_dev) {
    MMF_REQUIRE(c && x_dev && out_mmf_dev && out_packed_dev && n > 0, "mmf_debug_expf: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(debug_expf_kernel, grid1d(((size_t)n + 1) / 2), dim3(256), 0, c->stream, x_dev, n, out_mmf_dev, out_packed_dev);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

// the one-launch chain's wave-parallel solve and pose update (gn_fused.hpp: gn_solve_rows) on n caller-supplied systems, so that
// a test can hold it against float64 outside the 19 iterations it otherwise hides in.  Device pointers: sys = n x {A[36], b[6]},
// rt = n x 16 doubles, prev = n x {Rprev[9], tprev[3]} floats; rt_out = n x 12 doubles, pose_out = n x 24 floats.
extern "C" int mmf_debug_gn_solve(mmf_ctx* c, const double* sys_dev, const double* rt_dev, const float* prev_dev, float fx, float fy,
                                  float cx, float cy, int n, double* rt_out_dev, float* pose_out_dev) {
    MMF_REQUIRE(c && sys_dev && rt_dev && prev_dev && rt_out_dev && pose_out_dev && n > 0, "mmf_debug_gn_solve: bad argument");
    MMF_HIP_TRY(hipSetDevice(c->device));
    const LevelIntr in{fx, fy, cx, cy};
    hipLaunchKernelGGL(gn_solve_debug_kernel, dim3(1), dim3(64), 0, c->stream, sys_dev, rt_dev, prev_dev, in, n, rt_out_dev, pose_out_dev);
    MMF_HIP_TRY(hipGetLastError());
    return MMF_OK;
}

#ifdef MMF_STAMPS
// diagnostic builds only (tools/rgb_step_probe.py): phase-stamp buffer of the instrumented kernels
extern "C" int mmf_debug_set_stamps(void* dev_buf) {
    unsigned long long* p = static_cast<unsigned long long*>(dev_buf);
    MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_mmf_dbg), &p, sizeof(p)));
    MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_mmf_dbg_solve), &p, sizeof(p)));
    return MMF_OK;
}
#endif

// ---- dense optical flow after Farneback (flow_kernels.hpp, flow_host.hpp; Segmentation.cpp:779-804) ----
#include "flow_kernels.hpp"
#include "flow_host.hpp"

// ---- the inference of the flow CRF (flowcrf_kernels.hpp, flowcrf_host.hpp; Segmentation.cpp:819-1263) ----
#include "flowcrf_kernels.hpp"
#include "flowcrf_host.hpp"

// ---- the blob stage of the flow_crf segmentation (flowseg_kernels.hpp, flowseg_host.hpp; Segmentation.cpp:1270-1324) ----
#include "flowseg_kernels.hpp"
#include "flowseg_host.hpp"

// =============================================================================================
// Orchestrator: MultiMotionFusion::processFrame / predict (Core/MultiMotionFusion.cpp:207-854, 863-875)
// =============================================================================================
#include "stream_lane.hpp"
#include "fusion_state.hpp"
#include "fusion_hooks.hpp"
#include "fusion_keypoints.hpp"
#include "fusion_ingest.hpp"
#include "fusion_orchestrator.hpp"

// =============================================================================================
// Per-rigid-body shard across GPUs: frame broadcast + pose all-gather over RCCL
// =============================================================================================
#include "shard_rccl.hpp"
