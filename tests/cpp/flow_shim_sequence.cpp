// MultiMotionFusion::setOpticalFlow / getLastFlow (multimotionfusion_amd/cpp/MultiMotionFusion.h) over three frames: the
// field the shim hands out is, bit for bit, what the C ABI's engine (mmf_flow_compute) computes on the same frame pair; the
// first frame has none; the moving box carries more motion than the static wall.
// Build: see tests/test_gpu_flow_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"
#include "../../multimotionfusion_amd/cpp/cudafuncs.h"

static const int W = 320, H = 240;
static const float FX = 264.f, FY = 264.f, CX = 160.f, CY = 120.f;

struct Frame {
    std::vector<uint8_t> rgb;
    std::vector<float> depth;
    std::vector<uint8_t> box;
};

// wall at z = 2.5 m, a 0.5 m box face at z = 1.6 m sliding sideways by box_shift; static camera
static Frame render(float box_shift) {
    Frame f;
    f.rgb.resize((size_t)W * H * 3), f.depth.resize((size_t)W * H), f.box.resize((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float dx = (x - CX) / FX, dy = (y - CY) / FY;
            float z = 2.5f + 0.15f * std::sin(3.f * dx * 2.5f) * std::cos(2.f * dy * 2.5f);
            float px = dx * z, py = dy * z;
            const float bx = dx * 1.6f - box_shift, by = dy * 1.6f;
            bool box = false;
            if (std::fabs(bx) < 0.25f && std::fabs(by) < 0.2f) z = 1.6f + 0.1f * bx + 0.05f * by, px = bx, py = by, box = true;
            const float v = 0.5f + 0.2f * std::sin(9.f * px + (box ? 1.f : 0.f)) * std::sin(7.f * py) + 0.2f * std::sin(4.f * px + 3.f * py);
            const size_t i = (size_t)y * W + x;
            f.depth[i] = z, f.box[i] = box;
            f.rgb[3 * i] = (uint8_t)(40 + 180 * v), f.rgb[3 * i + 1] = (uint8_t)(30 + 170 * v), f.rgb[3 * i + 2] = (uint8_t)(50 + 150 * (1 - v));
        }
    return f;
}

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

static bool same_bits(const std::vector<float>& a, const float* dev, size_t n) {
    std::vector<float> b(n);
    if (hipMemcpy(b.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return false;
    return a.size() == n && std::memcmp(a.data(), b.data(), n * sizeof(float)) == 0;
}

int main() {
    mmf::Context ctx(0);
    mmf_fusion_config cfg;
    mmf_fusion_default_config(&cfg);
    cfg.conf_global_init = 1.f;
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, CX, CY, FX, FY, &cfg);
    CHECK(!mmf->getLastFlow().valid);  // off: nothing to hand out
    mmf->setOpticalFlow(true);
    CHECK(mmf->frontEndSettings().at("opticalFlow") == 1.f);
    mmf_flow_config fc;
    CHECK(mmf_flow_default_config(&fc) == MMF_OK);
    mmf_flow* engine = nullptr;
    CHECK(mmf_flow_create(ctx.get(), W, H, &fc, &engine) == MMF_OK);
    std::vector<Frame> frames;
    for (int i = 0; i < 3; ++i) frames.push_back(render(0.05f * i));
    DeviceArray<unsigned char> prev_rgb, next_rgb;
    for (int i = 0; i < 3; ++i) {
        FrameData frame;
        frame.timestamp = 1000 + 33 * i, frame.rgb = frames[(size_t)i].rgb.data(), frame.depth = frames[(size_t)i].depth.data();
        if (mmf->processFrame(frame)) return 2;
        const MultiMotionFusion::OpticalFlow got = mmf->getLastFlow();
        if (i == 0) {
            CHECK(!got.valid);
            continue;
        }
        CHECK(got.valid && got.width == W / 4 && got.height == H / 4);
        prev_rgb.upload(frames[(size_t)i - 1].rgb), next_rgb.upload(frames[(size_t)i].rgb);
        CHECK(mmf_flow_compute(engine, prev_rgb.ptr(), next_rgb.ptr()) == MMF_OK);
        CHECK(mmf_ctx_synchronize(ctx.get()) == MMF_OK);
        const float *flow = nullptr, *magnitude = nullptr, *motion = nullptr;
        int w = 0, h = 0;
        CHECK(mmf_flow_result(engine, &flow, &magnitude, &motion, &w, &h) == MMF_OK && w == got.width && h == got.height);
        const size_t px = (size_t)w * h;
        CHECK(same_bits(got.flow, flow, 2 * px) && same_bits(got.magnitude, magnitude, px) && same_bits(got.motion, motion, px));
        // the box slides to the right (0.05 m at 1.6 m: ~8 frame pixels, ~2 flow-image pixels); the wall stands still
        double in = 0, out = 0, in_x = 0;
        size_t n_in = 0, n_out = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t k = (size_t)y * w + x;
                if (frames[(size_t)i - 1].box[(size_t)(4 * y + 2) * W + 4 * x + 2])
                    in += got.motion[k], in_x += got.flow[2 * k], ++n_in;
                else
                    out += got.motion[k], ++n_out;
            }
        std::printf("frame %d: mean motion inside the box %.4f (flow.x %.3f), outside %.4f\n", i, in / n_in, in_x / n_in, out / n_out);
        CHECK(n_in > 0 && n_out > 0 && in / n_in > out / n_out && in_x / n_in > 0.5);
    }
    mmf->setOpticalFlow(false);
    CHECK(!mmf->getLastFlow().valid && mmf->frontEndSettings().at("opticalFlow") == 0.f);
    mmf_flow_destroy(engine);
    delete mmf;
    std::printf("flow shim sequence: ok\n");
    return 0;
}
