// Back-dating through the C++ shims: MultiMotionFusion::setTrackBackdating / getLastBackdatedPoses (cpp/MultiMotionFusion.h)
// over processFrame(FrameData) with a keypoint predictor, and tracker::PointTracker::backdate (cpp/PointTracker.h) on the same
// table afterwards.  The frames, their id images and the SuperPoint weights come from files the test writes (argv[1]: per
// frame rgb u8 x 3, depth f32, mask u8; argv[2]: the 12 {weight, bias} arrays as float32; argv[3..10]: width, height, frames,
// the frame that brings the new label, cx, cy, fx, fy).  Every entry is printed with its floats as bit patterns, and
// tests/test_gpu_backdate_shim.py compares the lines with the Python mirror's run.
// Build: see tests/test_gpu_backdate_shim.py.  Exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

static unsigned bits(float v) {
    unsigned u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

static void print_entries(const char* what, int frame, int model, const std::vector<mmf_backdated_pose>& e) {
    std::printf("%s %d model %d entries %zu\n", what, frame, model, e.size());
    for (const mmf_backdated_pose& p : e) {
        std::printf("entry %d %lld %d %d %d %d %d %08x %d", p.stamp, p.timestamp, p.from, p.both, p.nvalid, p.status, p.host_estimated,
                    bits(p.error), p.n_inliers);
        for (float v : p.T) std::printf(" %08x", bits(v));
        for (float v : p.pose) std::printf(" %08x", bits(v));
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    CHECK(argc == 11);
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]), SPAWN = std::atoi(argv[6]);
    CHECK(W > 0 && H > 0 && N > 0);
    const size_t npix = (size_t)W * H;
    std::vector<std::vector<uint8_t>> rgb((size_t)N), mask((size_t)N);
    std::vector<std::vector<float>> depth((size_t)N);
    FILE* fp = std::fopen(argv[1], "rb");
    CHECK(fp != nullptr);
    for (int i = 0; i < N; ++i) {
        rgb[i].resize(npix * 3), depth[i].resize(npix), mask[i].resize(npix);
        CHECK(std::fread(rgb[i].data(), 1, npix * 3, fp) == npix * 3);
        CHECK(std::fread(depth[i].data(), sizeof(float), npix, fp) == npix);
        CHECK(std::fread(mask[i].data(), 1, npix, fp) == npix);
    }
    std::fclose(fp);
    static const size_t wsize[12] = {64 * 9, 64 * 64 * 9, 64 * 64 * 9, 64 * 64 * 9, 128 * 64 * 9, 128 * 128 * 9,
                                     128 * 128 * 9, 128 * 128 * 9, 256 * 128 * 9, 65 * 256, 256 * 128 * 9, 256 * 256};
    static const size_t bsize[12] = {64, 64, 64, 64, 128, 128, 128, 128, 256, 65, 256, 256};
    std::vector<std::vector<float>> store;
    fp = std::fopen(argv[2], "rb");
    CHECK(fp != nullptr);
    for (int l = 0; l < 12; ++l)
        for (size_t n : {wsize[l], bsize[l]}) {
            store.emplace_back(n);
            CHECK(std::fread(store.back().data(), sizeof(float), n, fp) == n);
        }
    std::fclose(fp);
    std::vector<const float*> weights;
    for (auto& v : store) weights.push_back(v.data());
    const float cx = (float)std::atof(argv[7]), cy = (float)std::atof(argv[8]), fx = (float)std::atof(argv[9]), fy = (float)std::atof(argv[10]);

    mmf::Context ctx(0);
    SuperPoint kp(ctx, weights.data(), W, H, 1024);
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, cx, cy, fx, fy);
    mmf->setEnableMultipleModels(true);
    mmf->setEnableRedetection(true);
    mmf->setKeypointPredictor(&kp, 4096, 1024);
    mmf->getTracker()->setViewLog(8);
    int model = 0;
    CHECK(mmf->getLastBackdatedPoses(&model).empty() && model == -1);
    mmf->setTrackBackdating(4);
    for (int i = 0; i < N; ++i) {
        FrameData frame;
        frame.timestamp = 1000 + 33000000LL * i, frame.rgb = rgb[i].data(), frame.depth = depth[i].data();
        if (i > 0) frame.mask = mask[i].data(), frame.hasNewLabel = i == SPAWN;
        if (mmf->processFrame(frame)) return 2;
        const std::vector<mmf_backdated_pose> e = mmf->getLastBackdatedPoses(&model);
        print_entries("frame", i, model, e);
        CHECK((i == SPAWN) == (model == 1) && (i == SPAWN || e.empty()));
    }
    // the tracker's own call on the table the last frame left: label 1 with the reference's history, label 0 with a longer one
    const mmf_ransac_config cfg = {10, 0.03f, 0.6f};
    mmf_ransac_batch* batch = nullptr;
    CHECK(mmf_ransac_batch_create(ctx.get(), &cfg, 1024, &batch) == MMF_OK);
    print_entries("tracker", 2, 1, mmf->getTracker()->backdate(1, batch));
    print_entries("tracker", 3, 0, mmf->getTracker()->backdate(0, batch, 3));
    mmf_ransac_batch_destroy(batch);
    mmf->setTrackBackdating(0);
    delete mmf;
    std::printf("backdate shim sequence: ok\n");
    return 0;
}
