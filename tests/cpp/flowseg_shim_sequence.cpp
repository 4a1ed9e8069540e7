// SegmentationConfiguration::mode == "flow_crf" through the reference's own constructor of MultiMotionFusion
// (multimotionfusion_amd/cpp/MultiMotionFusion.h) over three frames, and the stand-alone engine (cpp/FlowSegmentation.h).
// The mode switches on the optical flow, the inference and the blob stage: a maskless multi-model frame no longer ends in the
// missing-segmentation error; the first frame has nothing to hand out, every later one the camera model's entry with the
// area of the whole image.  The engine: a 2 x 2 block has area 1 (16 super-pixels' worth), a ring is filled.
// Build: see tests/test_gpu_flowseg_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multimotionfusion_amd/cpp/FlowSegmentation.h"
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

static int sequence(const std::vector<Frame>& frames, const char* mode) {
    const bool flow_crf = std::strcmp(mode, "flow_crf") == 0;
    OdometryConfig odom_cfg;
    SegmentationConfiguration segm_cfg;
    segm_cfg.mode = mode;
    MultiMotionFusion mmf(200, 35000, 5e-05f, 1e-05f, /*closeLoops*/ false, false, false, 115, /*confGlobal*/ 1.f, /*confObject*/ 0.01f,
                          /*depthCut*/ 15.f, /*icpWeight*/ 10.f, false, 0.3095f, true, false, /*modelSpawnOffset*/ 2, Model::MatchingType::Drost,
                          std::string(), false, std::string(), odom_cfg, segm_cfg);
    mmf.setEnableMultipleModels(true);
    CHECK(mmf.frontEndSettings().at("opticalFlow") == (flow_crf ? 1.f : 0.f));
    CHECK(!mmf.getLastFlowSegmentation().valid);  // no frame yet
    for (size_t i = 0; i < frames.size(); ++i) {
        FrameData frame;
        frame.timestamp = 1000 + 33 * (long long)i, frame.rgb = const_cast<uint8_t*>(frames[i].rgb.data()), frame.depth = const_cast<float*>(frames[i].depth.data());
        if (mmf.processFrame(frame)) return 2;
        const MultiMotionFusion::FlowSegmentation got = mmf.getLastFlowSegmentation();
        if (!flow_crf || i == 0) {
            CHECK(!got.valid);
            continue;
        }
        CHECK(got.valid && got.has_result);
        // modelSpawnOffset 2: the new label may appear from the second segmented frame on (MultiMotionFusion.cpp:148, :410)
        CHECK(got.summary.allow_new == (i >= 2 ? 1 : 0));
        CHECK(got.summary.n_entries >= 1 && got.summary.models[0].id == 0 && got.summary.models[0].avg_confidence == 0.4f);
        // no tracks: the camera's label everywhere -- one blob, the polygon through the outermost cell centres
        if (!got.summary.has_new_label) {
            CHECK(got.summary.area2[0] == 2 * (W / 4 - 1) * (H / 4 - 1) && got.summary.first_cell[0] == 0);
            CHECK(got.summary.models[0].super_pixel_count == 16u * (unsigned)((W / 4 - 1) * (H / 4 - 1)));
            CHECK(got.summary.models[0].depth_mean > 1.5f && got.summary.models[0].depth_mean < 2.7f && got.summary.models[0].depth_std > 0.f);
        }
    }
    if (flow_crf) {
        CHECK(mmf.getModels().size() >= 1);
        mmf.setFlowInference(false);  // takes the mode with it
        CHECK(!mmf.getLastFlowSegmentation().valid);
        int has = 0;
        CHECK(mmf_fusion_last_flow_segmentation(mmf.handle(), nullptr, &has) == MMF_ERR_STATE);
    }
    return 0;
}

static int engine(mmf::Context& ctx) {
    const int w = 8, h = 6;
    FlowSegmentation fs(ctx, 4 * w, 4 * h, 4);
    CHECK(fs.isValid() && fs.crfWidth() == w && fs.crfHeight() == h);
    std::vector<unsigned char> ids((size_t)w * h, 0);
    ids[1 * w + 1] = ids[1 * w + 2] = ids[2 * w + 1] = ids[2 * w + 2] = 5;                    // a 2 x 2 block: area 1
    for (int y = 1; y <= 3; ++y)
        for (int x = 4; x <= 6; ++x) ids[(size_t)y * w + x] = (x == 5 && y == 2) ? 0 : 9;  // a 3 x 3 ring: area 4, centre filled
    std::vector<float> depth((size_t)16 * w * h, 1.5f);
    unsigned char* d_ids = nullptr;
    float* d_depth = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&d_ids), ids.size()) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_depth), depth.size() * 4) == hipSuccess);
    CHECK(hipMemcpy(d_ids, ids.data(), ids.size(), hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(d_depth, depth.data(), depth.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
    fs.run(d_ids, d_depth, {0, 5}, true, 9);
    const FlowSegmentation::Result r = fs.result();
    CHECK(r.segm && r.full && fs.lastLaunches() == 8);
    CHECK(r.summary.allow_new == 1 && r.summary.new_cells == 9 && r.summary.has_new_label == 1 && r.summary.n_entries == 3);  // 9 / 48 > 0.05
    CHECK(r.summary.area2[1] == 2 && r.summary.first_cell[1] == 1 * w + 1 && r.summary.models[1].super_pixel_count == 16u);
    CHECK(r.summary.area2[2] == 8 && r.summary.models[2].id == 9 && r.summary.models[2].super_pixel_count == 64u);
    CHECK(r.summary.models[2].depth_mean == 1.5f && r.summary.models[2].depth_std == 0.f);
    const std::vector<unsigned char> segm = fs.downloadSegmentation();
    CHECK(segm[2 * w + 5] == 9 && segm[1 * w + 1] == 5 && segm[0] == 0);
    (void)hipFree(d_ids), (void)hipFree(d_depth);
    return 0;
}

int main() {
    Resolution::setResolution(W, H);
    Intrinsics::setIntrinics(FX, FY, CX, CY);
    std::vector<Frame> frames;
    for (int i = 0; i < 3; ++i) frames.push_back(render(0.05f * i));
    if (int rc = engine(MultiMotionFusion::defaultContext())) return rc;
    if (int rc = sequence(frames, "flow_crf")) return rc;
    std::printf("flowseg shim sequence: ok\n");
    return 0;
}
