// The Slic shim (multimotionfusion_amd/cpp/Slic.h) as Segmentation.cpp:173-178, 218-221, 683 uses the reference's class --
// setInputImage, processFrame, downsample / downsampleThresholded / upsample on the engine's labels -- and processFrame
// through the MultiMotionFusion shim on maskless multi-model frames with setSuperpixelEngine(true): no label image from
// outside, the moving box is spawned.
// Build: see tests/test_gpu_slic_shim.py.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"
#include "../../multimotionfusion_amd/cpp/Slic.h"

static const int W = 320, H = 240, S = 16;
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

static int slic_class(mmf::Context& ctx) {
    const Frame fr = render(0.16f);
    DeviceArray<unsigned char> rgb;
    DeviceArray<float> depth;
    rgb.upload(fr.rgb), depth.upload(fr.depth);
    Slic slic(ctx, W, H, S);
    CHECK(!slic.isValid());
    slic.setInputImage(rgb.ptr());
    CHECK(slic.isValid());
    slic.processFrame();
    const std::vector<int> labels = slic.downloadResult();
    const int n = (W / S) * (H / S);
    CHECK((int)slic.getSpixelNum() == n && (int)labels.size() == W * H);
    std::vector<int> counts((size_t)n, 0);
    int off_grid = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int l = labels[(size_t)y * W + x];
            CHECK(l >= 0 && l < n);
            // the 3 x 3 neighbourhood of the pixel's cell
            CHECK(std::abs(l % (W / S) - x / S) <= 1 && std::abs(l / (W / S) - y / S) <= 1);
            counts[(size_t)l]++;
            off_grid += l != (y / S) * (W / S) + x / S;
        }
    CHECK(off_grid > 0);
    for (int k = 0; k < n; ++k) CHECK(slic.getSuperpixelSize((unsigned)k) == (unsigned)counts[(size_t)k]);
    // lowDepth = downsampleThresholded<float>(depth, 0.02): the mean of a label's depths (all of them are > 0.02 here)
    std::vector<float> low;
    slic.downsampleThresholded<float>(depth.ptr(), 0.02f).download(low);
    std::vector<double> sum((size_t)n, 0.0);
    for (size_t i = 0; i < labels.size(); ++i) sum[(size_t)labels[i]] += fr.depth[i];
    for (int k = 0; k < n; ++k)
        if (counts[(size_t)k] > 0) CHECK(std::fabs(low[(size_t)k] - sum[(size_t)k] / counts[(size_t)k]) <= 1e-4 * low[(size_t)k]);
    std::vector<float> low2;
    slic.downsample<float>(depth.ptr()).download(low2);
    for (int k = 0; k < n; ++k)
        if (counts[(size_t)k] > 0) CHECK(low2[(size_t)k] == low[(size_t)k]);
    std::vector<unsigned char> low_rgb;
    slic.downsample().download(low_rgb);
    CHECK((int)low_rgb.size() == 3 * n);
    // upsample<unsigned char>(map): full[i] = map[labels[i]]
    std::vector<unsigned char> map((size_t)n), full;
    for (int k = 0; k < n; ++k) map[(size_t)k] = (unsigned char)(k % 251);
    DeviceArray<unsigned char> map_dev;
    map_dev.upload(map);
    slic.upsample<unsigned char>(map_dev.ptr()).download(full);
    for (size_t i = 0; i < labels.size(); ++i) CHECK(full[i] == map[(size_t)labels[i]]);
    std::printf("Slic: %d super-pixels, %d of %d pixels off the grid\n", n, off_grid, W * H);
    return 0;
}

int main() {
    mmf::Context ctx(0);
    if (int rc = slic_class(ctx)) return rc;
    mmf_fusion_config cfg;
    mmf_fusion_default_config(&cfg);
    cfg.conf_global_init = 1.f;
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, CX, CY, FX, FY, &cfg);
    mmf->setEnableMultipleModels(true);
    mmf->setModelSpawnOffset(2);
    mmf->setNewModelMinRelativeSize(0.005f);
    mmf->setNewModelMaxRelativeSize(0.4f);
    mmf->setSuperpixelEngine(true);
    int spawned_at = -1;
    DeviceArray<int> used((size_t)W * H);
    for (int i = 0; i < 8; ++i) {
        const Frame fr = render(0.08f * i);
        FrameData frame;
        frame.timestamp = 1000 + 33 * i, frame.rgb = fr.rgb.data(), frame.depth = fr.depth.data();
        if (mmf->processFrame(frame)) return 2;
        if (spawned_at < 0 && mmf->getModels().size() > 1) spawned_at = i;
        if (i == 0) continue;
        // the labels the segmentation used are the engine's of this frame: the Slic class on the same image gives them
        CHECK(mmf_fusion_last_superpixels(mmf->handle(), used.ptr()) == MMF_OK);
        std::vector<int> a;
        used.download(a);
        DeviceArray<unsigned char> rgb;
        rgb.upload(fr.rgb);
        Slic slic(ctx, W, H, S);
        slic.setInputImage(rgb.ptr());
        slic.processFrame(false);
        CHECK(a == slic.downloadResult());
    }
    std::printf("spawned at frame %d, %zu models\n", spawned_at, mmf->getModels().size());
    CHECK(spawned_at >= 2);  // not before the spawn offset is reached
    CHECK(mmf->frontEndSettings().at("superpixelEngine") == 1.f);
    delete mmf;
    std::printf("slic shim sequence: ok\n");
    return 0;
}
