// FlowCrf (multimotionfusion_amd/cpp/FlowCrf.h) on a 64 x 48 frame, one model (id 7) and the new label (id 9): a rectangle
// without depth (in the frame and in the model's prediction) that moves by (2, 1) flow pixels over a still, valid background.
//   1. no tracks: every unary is log 2, the labels tie inside the rectangle (the first one wins) and the model's projection
//      probability 1 wins outside: the id image is 7 everywhere;
//   2. outlier tracks inside the rectangle (8 pixels in 33 ms against the model's still frame): their cells become 9, the
//      background stays 7; the large image is the small one scaled up by four; 35 launches at 10 iterations.
// Build: see tests/test_gpu_flowcrf_cpp.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multimotionfusion_amd/cpp/FlowCrf.h"

static const int W = 64, H = 48, w = 16, h = 12;
static const int RX0 = 4, RX1 = 12, RY0 = 3, RY1 = 9;  // the rectangle, in cells

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main() {
    mmf::Context& ctx = mmf::default_context();
    const float fx = 64.f, fy = 64.f, cx = 31.5f, cy = 23.5f, Z = 1.5f;
    std::vector<float> depth((size_t)W * H, Z), vert((size_t)W * H * 4, 0.f), flow((size_t)w * h * 2, 0.f), motion((size_t)w * h, 0.f);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const bool in = x / 4 >= RX0 && x / 4 < RX1 && y / 4 >= RY0 && y / 4 < RY1;
            if (in) depth[(size_t)y * W + x] = 0.f;
            vert[((size_t)y * W + x) * 4 + 2] = depth[(size_t)y * W + x];
        }
    for (int y = RY0; y < RY1; ++y)
        for (int x = RX0; x < RX1; ++x) {
            flow[2 * ((size_t)y * w + x)] = 2.f, flow[2 * ((size_t)y * w + x) + 1] = 1.f;
            motion[(size_t)y * w + x] = (2.236068f - 0.2f) / 4.8f;
        }
    DeviceArray<float> d_depth, d_vert, d_flow, d_motion;
    d_depth.upload(depth), d_vert.upload(vert), d_flow.upload(flow), d_motion.upload(motion);

    // outlier tracks on a grid inside the rectangle: the end pixel, the start 8 pixels to its left
    std::vector<int> xy_cur, xy_prev, ok;
    std::vector<float> co_cur, co_prev;
    std::vector<long long> ts_cur, ts_prev;
    std::vector<int> cells;
    for (int py = 4 * RY0 + 2; py < 4 * RY1; py += 8)
        for (int px = 4 * RX0 + 10; px < 4 * RX1; px += 8) {
            xy_cur.push_back(px), xy_cur.push_back(py), xy_prev.push_back(px - 8), xy_prev.push_back(py);
            co_cur.push_back((px - cx) / fx * Z), co_cur.push_back((py - cy) / fy * Z), co_cur.push_back(Z);
            co_prev.push_back((px - 8 - cx) / fx * Z), co_prev.push_back((py - cy) / fy * Z), co_prev.push_back(Z);
            ts_prev.push_back(1000000000LL), ts_cur.push_back(1033000000LL), ok.push_back(1);
            cells.push_back((int)std::nearbyint(0.25 * py) * w + (int)std::nearbyint(0.25 * px));  // half to even
        }
    const int n = (int)ok.size();
    CHECK(n >= 6);
    DeviceArray<int> d_xy_cur, d_xy_prev, d_ok;
    DeviceArray<float> d_co_cur, d_co_prev;
    DeviceArray<long long> d_ts_cur, d_ts_prev;
    d_xy_cur.upload(xy_cur), d_xy_prev.upload(xy_prev), d_ok.upload(ok), d_co_cur.upload(co_cur), d_co_prev.upload(co_prev);
    d_ts_cur.upload(ts_cur), d_ts_prev.upload(ts_prev);

    FlowCrf crf(ctx, W, H, fx, fy, cx, cy, 2, 64);
    CHECK(crf.isValid() && crf.crfWidth() == w && crf.crfHeight() == h);
    const unsigned char ids[1] = {7};
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float* vertex[1] = {d_vert.ptr()};
    mmf_flowcrf_input in;
    std::memset(&in, 0, sizeof(in));
    in.n_models = 1, in.allow_new = 1, in.new_id = 9, in.ids = ids, in.T_start = eye, in.T_end = eye, in.vertex = vertex;
    in.depth = d_depth.ptr(), in.flow = d_flow.ptr(), in.motion = d_motion.ptr();

    crf.infer(in, static_cast<mmf_tracker*>(nullptr));
    std::vector<unsigned char> seg = crf.downloadSegmentation();
    for (unsigned char v : seg) CHECK(v == 7);
    CHECK(crf.lastLaunches() == 35);

    mmf_flowcrf_tracks tr;
    tr.xy_cur = d_xy_cur.ptr(), tr.co_cur = d_co_cur.ptr(), tr.ts_cur = d_ts_cur.ptr(), tr.ok_cur = d_ok.ptr();
    tr.xy_prev = d_xy_prev.ptr(), tr.co_prev = d_co_prev.ptr(), tr.ts_prev = d_ts_prev.ptr(), tr.ok_prev = d_ok.ptr(), tr.count = n;
    crf.infer(in, &tr);
    seg = crf.downloadSegmentation();
    for (int c : cells) CHECK(seg[(size_t)c] == 9);
    int nine = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const bool in_rect = x >= RX0 && x < RX1 && y >= RY0 && y < RY1;
            if (!in_rect) CHECK(seg[(size_t)y * w + x] == 7);
            nine += seg[(size_t)y * w + x] == 9;
        }
    CHECK(nine >= n);
    CHECK(crf.lastLaunches() == 35);
    int L = 0;
    CHECK(crf.getProbabilities(&L) != nullptr && L == 2);
    std::vector<unsigned char> full((size_t)W * H);
    mmf::hip_check(hipMemcpy(full.data(), crf.getSegmentationFull(), full.size(), hipMemcpyDeviceToHost), "hipMemcpy");
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) CHECK(full[(size_t)y * W + x] == seg[(size_t)(y / 4) * w + x / 4]);
    std::printf("flowcrf engine check: ok (%d tracks, %d cells of the new label)\n", n, nine);
    return 0;
}
