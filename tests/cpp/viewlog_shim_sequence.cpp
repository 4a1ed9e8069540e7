// The models' keypoint views through the C++ shims: tracker::PointTracker::setViewLog / frame / modelViews
// (cpp/PointTracker.h), Model::storeDevice and MultiMotionFusion::getLastStoredViews (cpp/MultiMotionFusion.h).  Twelve
// keypoints on a plane are added three times while the plane comes closer, every track joins model 0, the model's views of
// the three frames are built on the device with the identity as pose and go into the fusion's view store without passing
// through the host; the keypoints of the second frame, moved by a known rigid motion, must then be found in view 1.
// Build: see tests/test_gpu_viewlog_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

static const int W = 320, H = 240, K = 12, D = 256;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main() {
    const float cx = 160.f, cy = 120.f, fx = 264.f, fy = 264.f;
    mmf::Context ctx(0);
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, cx, cy, fx, fy, nullptr);
    mmf->setEnableMultipleModels(true);
    mmf->setEnableRedetection(true);
    CHECK(mmf->getLastStoredViews().empty());
    ModelPointer model = mmf->getModels().front();  // (any model of the fusion reaches the fusion's view store)

    tracker::PointTracker pt(ctx, W, H, fx, fy, cx, cy, 64, 16);
    CHECK(pt.frame() == 0);
    pt.setViewLog(4);
    const size_t npix = (size_t)W * H;
    float* plane = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&plane), npix * sizeof(float)) == hipSuccess);
    std::vector<float> host(npix);
    std::vector<double> coordinates, descriptors((size_t)K * D, 0.0);
    for (int k = 0; k < K; ++k) {  // a 4 x 3 grid with a bend in it: no three of the points' depths make the set planar
        coordinates.push_back(0.2 + 0.2 * (k % 4)), coordinates.push_back(0.25 + 0.25 * (k / 4));
        descriptors[(size_t)k * D + (size_t)k] = 1.0;
    }
    for (int i = 0; i < 3; ++i) {
        ctx.synchronize();
        for (size_t p = 0; p < npix; ++p) host[p] = 2.0f - 0.1f * (float)i + 0.002f * (float)(p % W) + 0.0005f * (float)((p / W) % 7);
        CHECK(hipMemcpy(plane, host.data(), npix * sizeof(float), hipMemcpyHostToDevice) == hipSuccess);
        pt.addKeypoints(coordinates, descriptors, 1000 + i, plane);
        pt.prune(30, 0);
        CHECK(pt.frame() == i + 1);
    }
    CHECK(pt.numTracks() == (size_t)K && pt.length() == 3);
    pt.associateAll({0});

    const std::vector<int> frames = {1, 2, 3, 9};  // (9: not in the log)
    std::vector<float> poses;
    for (size_t v = 0; v < frames.size(); ++v)
        for (int e = 0; e < 16; ++e) poses.push_back(e % 5 == 0 ? 1.f : 0.f);
    const tracker::PointTracker::ModelViews views = pt.modelViews(0, frames, poses);
    CHECK(views.missing == 1 && views.counts.size() == 4);
    CHECK(views.counts[0] == K && views.counts[1] == K && views.counts[2] == K && views.counts[3] == 0);
    CHECK(pt.modelViews(5, frames, poses).counts[0] == 0);  // a model without tracks
    const tracker::PointTracker::ModelViews again = pt.modelViews(0, frames, poses);
    std::vector<float> coord((size_t)3 * K * 3);
    CHECK(hipMemcpy(coord.data(), again.coordinate, coord.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess);
    // the identity leaves the camera-frame coordinates: keypoint 0 of frame 2 at pixel (64, 60), depth from the plane
    const float z = 2.0f - 0.1f + 0.002f * 64.f + 0.0005f * (float)(60 % 7);
    CHECK(coord[(size_t)K * 3 + 2] == z && std::fabs(coord[(size_t)K * 3] - z * (64.f - cx) / fx) < 1e-6f);
    CHECK(model->storeDevice((int)again.counts.size(), again.counts.data(), again.descriptor, again.coordinate));
    CHECK(!model->storeDevice((int)again.counts.size(), again.counts.data(), again.descriptor, again.coordinate));  // stored before

    // frame 2's keypoints again, rotated by 0.3 rad about y and shifted
    const float c = std::cos(0.3f), s = std::sin(0.3f), t[3] = {0.2f, -0.1f, 0.3f};
    std::vector<float> qdesc((size_t)K * D, 0.f), qcoord;
    for (int k = 0; k < K; ++k) {
        qdesc[(size_t)k * D + (size_t)k] = 1.f;
        const float* p = &coord[(size_t)(K + k) * 3];
        qcoord.push_back(c * p[0] + s * p[2] + t[0]), qcoord.push_back(p[1] + t[1]), qcoord.push_back(-s * p[0] + c * p[2] + t[2]);
    }
    const Model::BestMatch best = model->getBestMatch(qdesc.data(), qcoord.data(), K, RigidRANSAC::Config{10, 0.03f, 0.8f});
    std::printf("best view %d error %g\n", best.view, best.error);
    CHECK(best.view == 1 && best.error < 1e-4f);
    const float* T = best.transformation;
    CHECK(std::fabs(T[0] - c) < 1e-3f && std::fabs(T[2] - s) < 1e-3f && std::fabs(T[3] - t[0]) < 2e-3f && std::fabs(T[11] - t[2]) < 2e-3f);
    ctx.synchronize();
    (void)hipFree(plane);
    delete mmf;
    std::printf("viewlog shim sequence: ok\n");
    return 0;
}
