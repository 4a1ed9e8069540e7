// The keypoint front end through the C++ shims: tracker::PointTracker (cpp/PointTracker.h) on its own, then
// MultiMotionFusion::processFrame(FrameData) with setKeypointPredictor / setOdomInit("kp") / setOdomRefine(true)
// (cpp/MultiMotionFusion.h; MultiMotionFusion.cpp:223-248, 312-335).  The frames and the SuperPoint weights come from files the
// test writes (argv[1]: per frame rgb u8 x 3, depth f32; argv[2]: the 12 {weight, bias} arrays as float32; argv[3..9]: width,
// height, frames, cx, cy, fx, fy).  Per frame the pose, the tracks and the track transformation are printed with nine
// significant digits, and tests/test_gpu_tracker_shim.py compares them with the Python mirror's run.
// Build: see tests/test_gpu_tracker_shim.py.  Exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 10);
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
    CHECK(W > 0 && H > 0 && N > 0);
    const size_t npix = (size_t)W * H;
    std::vector<std::vector<uint8_t>> rgb((size_t)N);
    std::vector<std::vector<float>> depth((size_t)N);
    FILE* fp = std::fopen(argv[1], "rb");
    CHECK(fp != nullptr);
    for (int i = 0; i < N; ++i) {
        rgb[i].resize(npix * 3), depth[i].resize(npix);
        CHECK(std::fread(rgb[i].data(), 1, npix * 3, fp) == npix * 3);
        CHECK(std::fread(depth[i].data(), sizeof(float), npix, fp) == npix);
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
    const float cx = (float)std::atof(argv[6]), cy = (float)std::atof(argv[7]), fx = (float)std::atof(argv[8]), fy = (float)std::atof(argv[9]);

    mmf::Context ctx(0);
    SuperPoint kp(ctx, weights.data(), W, H, 1024);
    {  // the tracker on its own: two frames of the same four keypoints on a plane that comes 10 cm closer
        tracker::PointTracker pt(ctx, W, H, fx, fy, cx, cy, 64, 16);
        float* plane = nullptr;
        CHECK(hipMalloc(reinterpret_cast<void**>(&plane), npix * sizeof(float)) == hipSuccess);
        std::vector<float> host(npix, 2.0f);
        const std::vector<double> coordinates = {0.25, 0.25, 0.75, 0.25, 0.25, 0.75, 0.75, 0.75};
        std::vector<double> descriptors(4 * 256, 0.0);
        for (int k = 0; k < 4; ++k) descriptors[(size_t)k * 256 + (size_t)k] = 1.0;
        for (int i = 0; i < 2; ++i) {
            ctx.synchronize();
            for (float& z : host) z = 2.0f - 0.1f * (float)i;
            CHECK(hipMemcpy(plane, host.data(), npix * sizeof(float), hipMemcpyHostToDevice) == hipSuccess);
            pt.addKeypoints(coordinates, descriptors, 1000 + i, plane);
            pt.prune(30, 0);
        }
        CHECK(pt.numTracks() == 4 && pt.length() == 2 && pt.dropped() == 0);
        CHECK(pt.getLastTrackTransform(0).inlier.empty());  // no model holds the tracks yet
        std::vector<int> xy;
        std::vector<float> coordinate, descriptor;
        CHECK(pt.getVisible(xy, coordinate, descriptor) == 4 && xy[0] == W / 4 && xy[1] == H / 4 && coordinate[2] == 1.9f);
        ctx.synchronize();
        (void)hipFree(plane);
    }

    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, cx, cy, fx, fy);
    mmf->setKeypointPredictor(&kp, 4096, 1024);
    mmf->setOdomInit("kp");
    mmf->setOdomRefine(true);
    CHECK(mmf->frontEndSettings().at("odomInitKp") == 1.f && mmf->frontEndSettings().at("hasKeypointPredictor") == 1.f);
    for (int i = 0; i < N; ++i) {
        FrameData frame;
        frame.timestamp = 1000 + 33000000LL * i, frame.rgb = rgb[i].data(), frame.depth = depth[i].data();
        if (mmf->processFrame(frame)) return 2;
        float pose[16];
        mmf->getCurrPose(pose);
        std::printf("frame %d tracks %zu length %zu pose", i, mmf->getTracker()->numTracks(), mmf->getTracker()->length());
        for (float v : pose) std::printf(" %.9g", (double)v);
        std::printf("\n");
        const std::vector<float> T = mmf->getLastTrackTransforms();
        CHECK(T.size() == (i == 0 ? 0u : 16u));
        if (i > 0) {
            std::printf("transform %d", i);
            for (float v : T) std::printf(" %.9g", (double)v);
            std::printf("\n");
        }
        CHECK(mmf->getTick() == i + 2);
    }
    const RigidRANSAC::Result last = mmf->getTracker()->getLastTrackTransform(0);  // every track joined model 0
    std::printf("last");
    for (float v : last.transformation) std::printf(" %.9g", (double)v);
    std::printf("\n");
    mmf->setKeypointPredictor(nullptr);  // detached: the next frame is an ordinary one
    FrameData frame;
    frame.timestamp = 1000 + 33000000LL * N, frame.rgb = rgb[(size_t)N - 1].data(), frame.depth = depth[(size_t)N - 1].data();
    const size_t before = mmf->getTracker()->numTracks();
    if (mmf->processFrame(frame)) return 2;
    CHECK(mmf->getTracker()->numTracks() == before && mmf->getLastTrackTransforms().empty());
    delete mmf;
    std::printf("tracker shim sequence: ok\n");
    return 0;
}
