// MultiMotionFusion::setFlowInference / getLastFlowInference (multimotionfusion_amd/cpp/MultiMotionFusion.h) over three frames
// of one model: the setter needs the optical-flow hook (MMF_ERR_STATE without it); the first frame has no result, every later
// one an id image of the frame's size / 4 that holds the one model's id everywhere, and its copy scaled up by 4; the poses are
// the same bits as without the hook; switching the optical flow off takes the inference with it.
// Build: see tests/test_gpu_flowcrf_shim.py.  Exit code 0 = every check passed.
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
};

// a wall at z = 2.5 m with a 0.5 m box face at z = 1.6 m sliding sideways by box_shift; static camera
static Frame render(float box_shift) {
    Frame f;
    f.rgb.resize((size_t)W * H * 3), f.depth.resize((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float dx = (x - CX) / FX, dy = (y - CY) / FY;
            float z = 2.5f + 0.15f * std::sin(3.f * dx * 2.5f) * std::cos(2.f * dy * 2.5f);
            float px = dx * z, py = dy * z;
            const float bx = dx * 1.6f - box_shift, by = dy * 1.6f;
            if (std::fabs(bx) < 0.25f && std::fabs(by) < 0.2f) z = 1.6f + 0.1f * bx + 0.05f * by, px = bx, py = by;
            const float v = 0.5f + 0.2f * std::sin(9.f * px) * std::sin(7.f * py) + 0.2f * std::sin(4.f * px + 3.f * py);
            const size_t i = (size_t)y * W + x;
            f.depth[i] = z;
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

// three frames; the pose behind each into `poses`
static int run(mmf::Context& ctx, const std::vector<Frame>& frames, bool hook, std::vector<float>* poses) {
    mmf_fusion_config cfg;
    mmf_fusion_default_config(&cfg);
    cfg.conf_global_init = 1.f;
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, CX, CY, FX, FY, &cfg);
    CHECK(!mmf->getLastFlowInference().valid);  // off: nothing to hand out
    mmf_flowcrf_config fc;
    CHECK(mmf_flowcrf_default_config(&fc) == MMF_OK);
    CHECK(mmf_fusion_set_flow_inference(mmf->handle(), &fc) == MMF_ERR_STATE);  // the optical-flow hook is off
    mmf->setOpticalFlow(true);
    if (hook) {
        mmf->setFlowInference(true);
        CHECK(mmf->frontEndSettings().at("flowInference") == 1.f);
    }
    for (size_t i = 0; i < frames.size(); ++i) {
        FrameData frame;
        frame.timestamp = 1000 + 33 * (long long)i, frame.rgb = const_cast<uint8_t*>(frames[i].rgb.data()), frame.depth = const_cast<float*>(frames[i].depth.data());
        if (mmf->processFrame(frame)) return 2;
        float pose[16];
        mmf->getCurrPose(pose);
        poses->insert(poses->end(), pose, pose + 16);
        const MultiMotionFusion::FlowInference got = mmf->getLastFlowInference();
        if (!hook || i == 0) {
            CHECK(!got.valid);
            continue;
        }
        CHECK(got.valid && got.width == W / 4 && got.height == H / 4 && got.labels == 1);
        CHECK(got.ids.size() == (size_t)(W / 4) * (H / 4) && got.ids_full.size() == (size_t)W * H);
        for (unsigned char v : got.ids) CHECK(v == 0);
        for (unsigned char v : got.ids_full) CHECK(v == 0);
    }
    if (hook) {
        mmf->setOpticalFlow(true);  // replaces the flow engine: the inference stays on, with nothing to hand out yet
        CHECK(mmf->frontEndSettings().at("flowInference") == 1.f && !mmf->getLastFlowInference().valid);
        int on = 1;
        CHECK(mmf_fusion_last_flow_inference(mmf->handle(), nullptr, nullptr, nullptr, nullptr, nullptr, &on) == MMF_OK && on == 0);
        mmf->setOpticalFlow(false);
        CHECK(!mmf->getLastFlowInference().valid && mmf->frontEndSettings().at("flowInference") == 0.f);
        int has = 1;
        CHECK(mmf_fusion_last_flow_inference(mmf->handle(), nullptr, nullptr, nullptr, nullptr, nullptr, &has) == MMF_ERR_STATE);
    }
    delete mmf;
    return 0;
}

int main() {
    mmf::Context ctx(0);
    std::vector<Frame> frames;
    for (int i = 0; i < 3; ++i) frames.push_back(render(0.05f * i));
    std::vector<float> off, on;
    if (int rc = run(ctx, frames, false, &off)) return rc;
    if (int rc = run(ctx, frames, true, &on)) return rc;
    CHECK(off.size() == 48 && on.size() == 48 && std::memcmp(off.data(), on.data(), 48 * sizeof(float)) == 0);
    std::printf("flowcrf shim sequence: ok\n");
    return 0;
}
