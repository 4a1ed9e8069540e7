// Keypoint redetection through the C++ shim: setEnableRedetection forwards to the library, Model::store /
// Model::getBestMatch / Model::activate drive the view store.  A rigid set of 40 keypoints with unit descriptors is stored
// as 5 views (every fourth keypoint missing in turn), then seen again moved by a known rigid motion among distractors:
// getBestMatch must find it (error < 0.01, more than 5 inliers), recover the motion, and refuse unrelated descriptors.
// Build: see tests/test_gpu_redetect_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

static const int W = 320, H = 240, K = 40, D = 256;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

static std::vector<float> unit_rows(std::mt19937& rng, int n) {
    std::normal_distribution<float> g(0.f, 1.f);
    std::vector<float> d((size_t)n * D);
    for (int i = 0; i < n; ++i) {
        double s = 0;
        for (int k = 0; k < D; ++k) d[(size_t)i * D + k] = g(rng), s += (double)d[(size_t)i * D + k] * d[(size_t)i * D + k];
        for (int k = 0; k < D; ++k) d[(size_t)i * D + k] = (float)(d[(size_t)i * D + k] / std::sqrt(s));
    }
    return d;
}

int main() {
    mmf::Context ctx(0);
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, 160.f, 120.f, 264.f, 264.f, nullptr);
    mmf->setEnableMultipleModels(true);
    mmf->setEnableRedetection(true);
    CHECK(mmf->frontEndSettings().at("enableRedetection") == 1.f);
    ModelPointer model = mmf->getModels().front();  // (any model of the fusion reaches the fusion's view store)
    CHECK(mmf->getInactiveModels().empty());

    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(-0.15f, 0.15f);
    std::vector<float> pts((size_t)K * 3), desc = unit_rows(rng, K);
    for (int i = 0; i < K; ++i) pts[3 * i] = u(rng), pts[3 * i + 1] = u(rng), pts[3 * i + 2] = 1.5f + u(rng);
    // 5 views; view v lacks the keypoints i with i % 4 == v % 4; one empty view in the middle
    std::vector<int> counts;
    std::vector<float> vdesc, vcoord;
    for (int v = 0; v < 6; ++v) {
        int n = 0;
        for (int i = 0; i < K && v != 3; ++i) {
            if (i % 4 == v % 4) continue;
            vdesc.insert(vdesc.end(), desc.begin() + (size_t)i * D, desc.begin() + (size_t)(i + 1) * D);
            vcoord.insert(vcoord.end(), pts.begin() + 3 * i, pts.begin() + 3 * i + 3);
            ++n;
        }
        counts.push_back(n);
    }
    CHECK(model->store((int)counts.size(), counts.data(), vdesc.data(), vcoord.data()));
    CHECK(!model->store((int)counts.size(), counts.data(), vdesc.data(), vcoord.data()));  // stored before: skipped

    // the object again: rotated by 0.3 rad about y, shifted, 30 of its keypoints + 8 distractors
    const float c = std::cos(0.3f), s = std::sin(0.3f), t[3] = {0.2f, -0.1f, 0.3f};
    std::vector<float> qdesc, qcoord;
    for (int i = 0; i < 30; ++i) {
        qdesc.insert(qdesc.end(), desc.begin() + (size_t)i * D, desc.begin() + (size_t)(i + 1) * D);
        const float* p = &pts[3 * i];
        qcoord.push_back(c * p[0] + s * p[2] + t[0]), qcoord.push_back(p[1] + t[1]), qcoord.push_back(-s * p[0] + c * p[2] + t[2]);
    }
    const std::vector<float> noise = unit_rows(rng, 8);
    qdesc.insert(qdesc.end(), noise.begin(), noise.end());
    for (int i = 0; i < 8 * 3; ++i) qcoord.push_back(2.f + u(rng));
    const RigidRANSAC::Config cfg{10, 0.03f, 0.8f};
    const Model::BestMatch best = model->getBestMatch(qdesc.data(), qcoord.data(), 38, cfg);
    std::printf("best view %d error %g inliers %zu\n", best.view, best.error, best.inlier.size());
    CHECK(best.view >= 0 && best.view != 3 && best.error < 0.01f);
    int inliers = 0;
    for (unsigned char b : best.inlier) inliers += b;
    CHECK(inliers > 5);
    // query ~ T train: T is the motion
    const float* T = best.transformation;
    CHECK(std::fabs(T[0] - c) < 1e-3f && std::fabs(T[2] - s) < 1e-3f && std::fabs(T[8] + s) < 1e-3f);
    CHECK(std::fabs(T[3] - t[0]) < 2e-3f && std::fabs(T[7] - t[1]) < 2e-3f && std::fabs(T[11] - t[2]) < 2e-3f);
    // unrelated descriptors: no view reaches three matches that agree on a motion
    const std::vector<float> other = unit_rows(rng, 38);
    const Model::BestMatch none = model->getBestMatch(other.data(), qcoord.data(), 38, cfg);
    CHECK(!(none.error < 0.01f));
    // Model::activate: pose = lastPose = the inverse of the transformation
    float pose[16] = {c, 0, -s, 0, 0, 1, 0, 0, s, 0, c, 0, 0, 0, 0, 1}, got[16];
    model->activate(pose, 1234);
    model->getPose(got);
    for (int i = 0; i < 16; ++i) CHECK(got[i] == pose[i] && model->getLastPose()[i] == pose[i]);
    // a frame with redetection on and nothing to search: no keypoints, no inactive models
    std::vector<uint8_t> rgb((size_t)W * H * 3, 90);
    std::vector<float> depth((size_t)W * H, 2.f);
    FrameData frame;
    frame.timestamp = 1000, frame.rgb = rgb.data(), frame.depth = depth.data();
    CHECK(!mmf->processFrame(frame));
    CHECK(mmf->getLastRedetections().empty());
    delete mmf;
    std::printf("redetect shim sequence: ok\n");
    return 0;
}
