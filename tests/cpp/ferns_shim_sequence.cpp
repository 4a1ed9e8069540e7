// The C++ shim on the fern keyframe database (multimotionfusion_amd/cpp/Ferns.h, MultiMotionFusion::setFernDatabase):
//   1. class Ferns on hand-made fill-in images: addFrame keeps a new view and refuses a repeated one, findCandidate finds the
//      keyframe a view repeats once it is old enough, its similarity is blockHDAware of the two rows of codes, frame(id) hands
//      out what was stored, a full database drops;
//   2. MultiMotionFusion::setFernDatabase(true) over four frames: every frame's record equals the C ABI's engine fed the
//      camera model's fill-in images, pose and tick; setFernThresh reaches the engine; getFerns() shows the keyframes.
// Build: see tests/test_gpu_ferns_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multimotionfusion_amd/cpp/Ferns.h"
#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"
#include "../../multimotionfusion_amd/cpp/cudafuncs.h"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

// fill-in images of a w x h frame: blocks of 8 x 8 pixels with a colour and a depth of their own, `phase` shifts the pattern
struct Images {
    DeviceArray<unsigned char> image;
    DeviceArray<float> vert, norm;
    Images(int w, int h, int phase) {
        std::vector<unsigned char> rgba((size_t)w * h * 4);
        std::vector<float> v((size_t)w * h * 4), n((size_t)w * h * 4);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                const unsigned b = (unsigned)((y / 8) * 131 + (x / 8) * 31 + phase * 977) * 2654435761u;
                rgba[4 * i] = (unsigned char)(b >> 8), rgba[4 * i + 1] = (unsigned char)(b >> 16), rgba[4 * i + 2] = (unsigned char)(b >> 24);
                rgba[4 * i + 3] = 255;
                v[4 * i] = 0.01f * x, v[4 * i + 1] = 0.01f * y, v[4 * i + 2] = (b & 15u) == 0u ? 0.f : 0.5f + (float)(b & 255u) / 40.f, v[4 * i + 3] = 1.f;
                n[4 * i] = 0.f, n[4 * i + 1] = 0.f, n[4 * i + 2] = -1.f, n[4 * i + 3] = (float)phase;
            }
        image.upload(rgba), vert.upload(v), norm.upload(n);
    }
};

static int standalone(mmf::Context& ctx) {
    const int W = 64, H = 48;
    Ferns ferns(ctx, W, H, 200, 15000, 115.f, {}, 5, 2);
    CHECK(ferns.width == 8 && ferns.height == 6 && ferns.num == 200 && ferns.frames() == 0 && ferns.lastClosest == -1);
    Images a(W, H, 0), b(W, H, 1), c(W, H, 2);
    GPUTexture ai(a.image.ptr(), W, H, GPUTexture::RGBA8), av(a.vert.ptr(), W, H, GPUTexture::RGBA32F), an(a.norm.ptr(), W, H, GPUTexture::RGBA32F);
    GPUTexture bi(b.image.ptr(), W, H, GPUTexture::RGBA8), bv(b.vert.ptr(), W, H, GPUTexture::RGBA32F), bn(b.norm.ptr(), W, H, GPUTexture::RGBA32F);
    GPUTexture ci(c.image.ptr(), W, H, GPUTexture::RGBA8), cv(c.vert.ptr(), W, H, GPUTexture::RGBA32F), cn(c.norm.ptr(), W, H, GPUTexture::RGBA32F);
    float pose[16] = {1, 0, 0, 0.5f, 0, 1, 0, -2.f, 0, 0, 1, 3.f, 0, 0, 0, 1};
    CHECK(ferns.addFrame(&ai, &av, &an, pose, 10, 0.3095f) && ferns.frames() == 1);
    const std::vector<uint8_t> codes_a = ferns.lastCodes();
    CHECK(!ferns.addFrame(&ai, &av, &an, pose, 11, 0.3095f) && ferns.frames() == 1);  // the same view: dissimilarity 0
    CHECK(ferns.lastResult().add_minimum == 0.f && ferns.lastResult().good_codes > 100);
    CHECK(ferns.addFrame(&bi, &bv, &bn, pose, 12, 0.3095f) && ferns.frames() == 2);
    // find: keyframe 0 is the view itself, but only once it is more than 300 ticks old
    Ferns::Candidate none = ferns.findCandidate(&av, &an, &ai, 310);
    CHECK(none.id == -1 && !none.candidate && ferns.lastClosest == -1);
    Ferns::Candidate hit = ferns.findCandidate(&av, &an, &ai, 311);
    CHECK(hit.id == 0 && hit.candidate && hit.dissim == 0.f && hit.similarity == 1.f && hit.srcTime == 10 && ferns.lastClosest == 0);
    CHECK(std::memcmp(hit.pose, pose, sizeof(pose)) == 0);
    // a view the database has not seen: the closest keyframe is one of the two, its similarity blockHDAware of the rows
    Ferns::Candidate far = ferns.findCandidate(&cv, &cn, &ci, 1000);
    CHECK(far.id == 0 || far.id == 1);
    std::vector<uint8_t> db((size_t)2 * 200);
    CHECK(mmf_ferns_download(ferns.handle(), "db_codes", db.data(), db.size()) == MMF_OK);
    CHECK(std::memcmp(db.data(), codes_a.data(), 200) == 0);
    const std::vector<uint8_t> row(db.begin() + 200 * far.id, db.begin() + 200 * (far.id + 1));
    const float sim = Ferns::blockHDAware(ferns.lastCodes(), row);
    CHECK(std::memcmp(&sim, &far.similarity, sizeof(float)) == 0 && far.candidate == (sim > 0.3f));
    // what was stored
    const Ferns::Frame f0 = ferns.frame(0);
    CHECK(f0.id == 0 && f0.srcTime == 10 && f0.goodCodes > 100);
    CHECK(std::memcmp(f0.pose, pose, sizeof(pose)) == 0 && f0.initRgb && f0.initVerts && f0.initNorms);
    std::vector<float> small((size_t)8 * 6 * 4);
    CHECK(hipMemcpy(small.data(), f0.initVerts, small.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(small[0] == 0.01f * 4 && small[1] == 0.01f * 4);  // small pixel (0, 0) is the frame's texel (4, 4)
    // capacity 2: the third new view is dropped and counted
    CHECK(!ferns.addFrame(&ci, &cv, &cn, pose, 2000, 0.3095f) && ferns.frames() == 2 && ferns.dropped() == 1);
    ferns.reset();
    CHECK(ferns.frames() == 0 && ferns.addFrame(&ci, &cv, &cn, pose, 1, 0.3095f) && ferns.dropped() == 0);
    return 0;
}

static const int W = 160, H = 120;
static const float FX = 132.f, FY = 132.f, CX = 80.f, CY = 60.f;

// a wall with relief at 2.5 m seen by a camera that has moved sideways by `shift` metres
static void render(float shift, std::vector<uint8_t>& rgb, std::vector<float>& depth) {
    rgb.resize((size_t)W * H * 3), depth.resize((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float dx = (x - CX) / FX, dy = (y - CY) / FY;
            const float px = dx * 2.5f + shift, py = dy * 2.5f;
            const float z = 2.5f + 0.15f * std::sin(3.f * px) * std::cos(2.f * py);
            const float v = 0.5f + 0.2f * std::sin(9.f * px) * std::sin(7.f * py) + 0.2f * std::sin(4.f * px + 3.f * py);
            const size_t i = (size_t)y * W + x;
            depth[i] = z;
            rgb[3 * i] = (uint8_t)(40 + 180 * v), rgb[3 * i + 1] = (uint8_t)(30 + 170 * v), rgb[3 * i + 2] = (uint8_t)(50 + 150 * (1 - v));
        }
}

static bool same_record(const mmf_ferns_result_t& a, const mmf_ferns_result_t& b) {
    return a.added == b.added && a.dropped_total == b.dropped_total && a.count == b.count && a.good_codes == b.good_codes &&
           std::memcmp(&a.add_minimum, &b.add_minimum, 4) == 0 && a.closest == b.closest && std::memcmp(&a.closest_dissim, &b.closest_dissim, 4) == 0 &&
           a.candidate == b.candidate && a.closest_time == b.closest_time && std::memcmp(a.closest_pose, b.closest_pose, sizeof(a.closest_pose)) == 0 &&
           (std::memcmp(&a.closest_similarity, &b.closest_similarity, 4) == 0 || (a.closest_similarity != a.closest_similarity && b.closest_similarity != b.closest_similarity));
}

static int hook(mmf::Context& ctx) {
    mmf_fusion_config cfg;
    mmf_fusion_default_config(&cfg);
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, CX, CY, FX, FY, &cfg);
    CHECK(!mmf->getLastFernResult().valid && !mmf->getLost());
    mmf->setFernThresh(0.3095f);
    mmf->setFernDatabase(true);
    CHECK(mmf->frontEndSettings().at("fernDatabase") == 1.f && !mmf->getLastFernResult().valid && mmf->getFerns().frames() == 0);
    // the engine the hook's is compared with: the same configuration and table (seed 0)
    mmf_ferns_config fc;
    CHECK(mmf_ferns_default_config(&fc) == MMF_OK);
    fc.max_depth_mm = (int)(cfg.depth_cutoff * 1000.f);
    CHECK(mmf->getFerns().maxDepth == fc.max_depth_mm && mmf->getFerns().num == fc.num);
    std::vector<int> table((size_t)fc.num * 6);
    CHECK(mmf_ferns_make_table(0, fc.num, W / 8, H / 8, fc.max_depth_mm, table.data()) == MMF_OK);
    mmf_ferns* engine = nullptr;
    CHECK(mmf_ferns_create(ctx.get(), W, H, &fc, table.data(), &engine) == MMF_OK);
    std::vector<uint8_t> rgb;
    std::vector<float> depth;
    for (int i = 0; i < 4; ++i) {
        render(0.004f * i, rgb, depth);
        FrameData frame;
        frame.timestamp = 1000 + 33 * i, frame.rgb = rgb.data(), frame.depth = depth.data();
        const int tick = mmf->getTick();
        if (i == 3) {  // from here on every frame is kept
            mmf->setFernThresh(-1.f);
            CHECK(mmf_ferns_set_threshold(engine, -1.f) == MMF_OK);
        }
        if (mmf->processFrame(frame)) return 2;
        const MultiMotionFusion::FernResult got = mmf->getLastFernResult();
        CHECK(got.valid);
        ModelPointer cam = mmf->getBackgroundModel();
        GPUTexture image = cam->getFillInImageTexture(), vert = cam->getFillInVertexTexture(), norm = cam->getFillInNormalTexture();
        float pose[16];
        mmf->getCurrPose(pose);
        CHECK(mmf_ferns_process(engine, image.data(), vert.data(), norm.data(), pose, tick, MMF_FERNS_FIND | MMF_FERNS_ADD) == MMF_OK);
        mmf_ferns_result_t want;
        CHECK(mmf_ferns_result(engine, &want) == MMF_OK);
        std::printf("frame %d: tick %d good %d added %d count %d minimum %g closest %d\n", i, tick, got.record.good_codes, got.record.added,
                    got.record.count, (double)got.record.add_minimum, got.record.closest);
        CHECK(same_record(got.record, want));
        // the camera has hardly moved: the first frame is the keyframe, the next two resemble it; the fourth is kept by the threshold
        CHECK(got.record.added == (i == 0 || i == 3 ? 1 : 0) && got.record.good_codes > 250);
        CHECK(mmf->getFerns().frames() == got.record.count);
    }
    CHECK(mmf->getFerns().frames() == 2);
    const Ferns::Frame f0 = mmf->getFerns().frame(0), f1 = mmf->getFerns().frame(1);
    CHECK(f0.srcTime == 1 && f1.srcTime == 4 && f0.initVerts != nullptr && f0.goodCodes > 250);
    mmf->setFernDatabase(false);
    CHECK(!mmf->getLastFernResult().valid && mmf->frontEndSettings().at("fernDatabase") == 0.f && !mmf->getLost());
    mmf_ferns_destroy(engine);
    delete mmf;
    return 0;
}

int main() {
    mmf::Context ctx(0);
    if (int rc = standalone(ctx)) return rc;
    if (int rc = hook(ctx)) return rc;
    std::printf("ferns shim sequence: ok\n");
    return 0;
}
