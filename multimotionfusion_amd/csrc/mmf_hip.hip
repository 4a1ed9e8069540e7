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

// MMF_HIP_TRY(expr, cleanup): `cleanup` runs before the return -- a create function past its `new` hands the half-built
// object to its destroy function
#define MMF_HIP_TRY(expr, ...)                                                                    \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            __VA_ARGS__;                                                                          \
            return fail(MMF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__) + " (" +  \
                                         __FILE__ + ":" + std::to_string(__LINE__) + ")");        \
        }                                                                                         \
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

static Override g_xcd_forced;  // mmf_debug_set_xcd; else MMF_XCD
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
    // from here on a failure unmakes what is there (mmf_ctx_destroy takes a half-built context)
    c->device = device;
    hipDeviceProp_t prop;
    MMF_HIP_TRY(hipGetDeviceProperties(&prop, device), mmf_ctx_destroy(c));
    std::snprintf(c->arch, sizeof(c->arch), "%s", prop.gcnArchName);
    c->cu_count = prop.multiProcessorCount;
    if (std::strncmp(c->arch, "gfx950", 6) != 0) {
        std::string m = std::string("mmf_ctx_create: this library is built for gfx950 only, device is ") + c->arch;
        mmf_ctx_destroy(c);
        return fail(MMF_ERR_NO_DEVICE, m);
    }
    if (private_stream) {
        MMF_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), mmf_ctx_destroy(c));
        c->own_stream = true;
    } else {
        c->stream = (hipStream_t)stream;
    }
    MMF_HIP_TRY(hipMalloc(&c->partials_f, sizeof(float) * kMaxGrid * kPartialStride), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipMalloc(&c->partials_icp, sizeof(float) * kMaxIcpGrid * kPartialStride), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipMalloc(&c->partials_res, sizeof(int2) * kMaxGrid), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipMalloc(&c->ticket, sizeof(unsigned) * kTicketWords), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipMemsetAsync(c->ticket, 0, sizeof(unsigned) * kTicketWords, c->stream), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipMalloc(&c->scratch_state, sizeof(OdomState)), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipMemsetAsync(c->scratch_state, 0, sizeof(OdomState), c->stream), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipHostMalloc(&c->host_state, sizeof(OdomState), hipHostMallocDefault), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipEventCreate(&c->ev0), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipEventCreate(&c->ev1), mmf_ctx_destroy(c));
    MMF_HIP_TRY(hipStreamSynchronize(c->stream), mmf_ctx_destroy(c));
    {  // (surfel_kernels.hpp: xcd_block)
        const int on = (int)g_xcd_forced.get(tunables().xcd_blocks ? 1 : 0);
        MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_xcd_blocks), &on, sizeof(on)), mmf_ctx_destroy(c));
    }
    *out = c;
    return MMF_OK;
}
// test / A-B hook: every XCD works on one contiguous eighth of a surfel pass's blocks (1, the default) or the blocks are dealt
// round-robin as the workgroups are (0); -1 = the default (MMF_XCD).  A device-wide word: set while no pass is running.
extern "C" unsigned mmf_debug_xcd_block(unsigned block, unsigned blocks) { return xcd_block_of(block, blocks); }  // (host: no device needed)
extern "C" int mmf_debug_set_xcd(int on) {
    override_flag(g_xcd_forced, on);
    const int v = (int)g_xcd_forced.get(tunables().xcd_blocks ? 1 : 0);
    MMF_HIP_TRY(hipDeviceSynchronize());
    MMF_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_xcd_blocks), &v, sizeof(v)));
    return MMF_OK;
}

// Safe on a half-built context (mmf_ctx_create's failure paths): null pointers free nothing, a stream that was not made is not ours.
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
// RGBDOdometry: the object, the batched preparation, the Gauss-Newton chain
// ---------------------------------------------------------------------------------------------
#include "odom_host.hpp"
#include "prep_host.hpp"
#include "chain_host.hpp"

// =============================================================================================
// Surfel model (Core/Model/Model.{h,cpp} + Core/Model/ModelProjection.{h,cpp}), pure HIP
// =============================================================================================
#include "surfel_kernels.hpp"
#include "pass_rect.hpp"

#include "model_host.hpp"
#include "export_host.hpp"
#include "import_host.hpp"

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
#include "stream_lane.hpp"
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

// ---- the fern keyframe database (ferns_kernels.hpp, ferns_host.hpp; Core/Ferns.cpp) ----
#include "ferns_kernels.hpp"
#include "ferns_host.hpp"

// =============================================================================================
// Orchestrator: MultiMotionFusion::processFrame / predict (Core/MultiMotionFusion.cpp:207-854, 863-875)
// =============================================================================================
#include "fusion_state.hpp"
#include "fusion_hooks.hpp"
#include "fusion_keypoints.hpp"
#include "fusion_ingest.hpp"
#include "fusion_orchestrator.hpp"
#include "modeldb_host.hpp"

// =============================================================================================
// Per-rigid-body shard across GPUs: frame broadcast + pose all-gather over RCCL
// =============================================================================================
#include "shard_rccl.hpp"
