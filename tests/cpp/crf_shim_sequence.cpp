// processFrame(FrameData) through the C++ shim on frames WITHOUT an id image, multiple models enabled, segmentation mode ""
// (the default): the built-in dense CRF segments each frame and spawns the box that moves in front of the wall.  The
// spawn setters of the GUI block (GUI/MainController.cpp:658-670) reach it through the shim.
// Build: see tests/test_gpu_crf_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

static const int W = 320, H = 240;
static const float FX = 264.f, FY = 264.f, CX = 160.f, CY = 120.f;

struct Frame {
    std::vector<uint8_t> rgb;
    std::vector<float> depth;
};

// wall at z = 2.5 m, a 0.5 m box face at z = 1.6 m sliding sideways by box_shift; static camera
static Frame render(float box_shift) {
    Frame f;
    f.rgb.resize((size_t)W * H * 3), f.depth.resize((size_t)W * H);
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

int main() {
    mmf::Context ctx(0);
    mmf_fusion_config cfg;
    mmf_fusion_default_config(&cfg);
    cfg.conf_global_init = 1.f;
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, CX, CY, FX, FY, &cfg);
    mmf->setEnableMultipleModels(true);
    mmf->setModelSpawnOffset(2);
    mmf->setNewModelMinRelativeSize(0.005f);
    mmf->setNewModelMaxRelativeSize(0.4f);
    int spawned_at = -1;
    for (int i = 0; i < 8; ++i) {
        const Frame fr = render(0.08f * i);
        FrameData frame;
        frame.timestamp = 1000 + 33 * i, frame.rgb = fr.rgb.data(), frame.depth = fr.depth.data();
        if (mmf->processFrame(frame)) return 2;
        if (spawned_at < 0 && mmf->getModels().size() > 1) spawned_at = i;
    }
    std::printf("spawned at frame %d, %zu models\n", spawned_at, mmf->getModels().size());
    CHECK(spawned_at >= 2);  // not before the spawn offset is reached
    CHECK(mmf->frontEndSettings().at("modelSpawnOffset") == 2.f);
    delete mmf;
    std::printf("crf shim sequence: ok\n");
    return 0;
}
