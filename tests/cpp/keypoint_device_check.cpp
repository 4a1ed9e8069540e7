// The keypoint front end of cpp/MultiMotionFusion.h inside the library call (setKeypointFrontEndOnDevice(true)) against the
// caller-driven one (false): the same frames through two MultiMotionFusion objects with setKeypointPredictor /
// setOdomInit("kp") / setOdomRefine(true).  argv as tests/cpp/tracker_shim_sequence.cpp: [1] per frame rgb u8 x 3, depth f32;
// [2] the 12 {weight, bias} arrays as float32; [3..9] width, height, frames, cx, cy, fx, fy.  Prints per frame both track
// counts and whether the poses are the same bits, then "poses agree: 0|1" and "tracks agree: 0|1".
// Build: see tests/test_gpu_keypoint_device.py.  Exit code 0 = the program ran through.
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
    std::vector<float> poses[2];
    std::vector<size_t> tracks[2];
    for (int on = 0; on < 2; ++on) {
        SuperPoint kp(ctx, weights.data(), W, H, 1024);
        MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, cx, cy, fx, fy);
        mmf->setKeypointPredictor(&kp, 4096, 1024);
        mmf->setOdomInit("kp");
        mmf->setOdomRefine(true);
        mmf->setKeypointFrontEndOnDevice(on != 0);
        CHECK(mmf->frontEndSettings().at("keypointFrontEndOnDevice") == (float)on);
        for (int i = 0; i < N; ++i) {
            FrameData frame;
            frame.timestamp = 1000 + 33000000LL * i, frame.rgb = rgb[i].data(), frame.depth = depth[i].data();
            if (mmf->processFrame(frame)) return 2;
            float pose[16];
            mmf->getCurrPose(pose);
            poses[on].insert(poses[on].end(), pose, pose + 16);
            tracks[on].push_back(mmf->getTracker()->numTracks());
            CHECK(mmf->getLastTrackTransforms().size() == (i == 0 ? 0u : 16u));
            CHECK(mmf->getTick() == i + 2);
        }
        delete mmf;
    }
    bool same_poses = true, same_tracks = true;
    for (int i = 0; i < N; ++i) {
        const bool p = std::memcmp(&poses[0][(size_t)i * 16], &poses[1][(size_t)i * 16], 16 * sizeof(float)) == 0;
        std::printf("frame %d tracks %zu %zu pose bits %s\n", i, tracks[0][i], tracks[1][i], p ? "equal" : "DIFFER");
        same_poses = same_poses && p;
        same_tracks = same_tracks && tracks[0][i] == tracks[1][i] && tracks[0][i] > 0;
    }
    std::printf("poses agree: %d\ntracks agree: %d\n", same_poses ? 1 : 0, same_tracks ? 1 : 0);
    return 0;
}
