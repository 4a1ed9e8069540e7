// processFrame(FrameData) through the C++ shim with setMaskSegmentation(true): FrameData::mask carries the frame's RAW labels,
// as the reference's log readers deliver them, and the shim's processFrame maps them, spawns the models and computes the model
// data (Segmentation.cpp:89-147).  The frames come from a file the test writes (argv[1]: per frame rgb u8 x 3, depth f32,
// labels u8; argv[2..8]: width, height, frames, cx, cy, fx, fy); per frame the model ids, confidence thresholds and poses are printed with
// nine significant digits (a float32 survives that), and tests/test_gpu_mask_shim.py compares them with the Python mirror's run.
// Build: see tests/test_gpu_mask_shim.py.  Exit code 0 = every check passed.
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
    CHECK(argc == 9);
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), N = std::atoi(argv[4]);
    CHECK(W > 0 && H > 0 && N > 0);
    const size_t npix = (size_t)W * H;
    std::vector<std::vector<uint8_t>> rgb((size_t)N), labels((size_t)N);
    std::vector<std::vector<float>> depth((size_t)N);
    FILE* fp = std::fopen(argv[1], "rb");
    CHECK(fp != nullptr);
    for (int i = 0; i < N; ++i) {
        rgb[i].resize(npix * 3), depth[i].resize(npix), labels[i].resize(npix);
        CHECK(std::fread(rgb[i].data(), 1, npix * 3, fp) == npix * 3);
        CHECK(std::fread(depth[i].data(), sizeof(float), npix, fp) == npix);
        CHECK(std::fread(labels[i].data(), 1, npix, fp) == npix);
    }
    std::fclose(fp);

    mmf::Context ctx(0);
    mmf_fusion_config cfg;
    mmf_fusion_default_config(&cfg);
    cfg.preallocated_models = 2;
    const float cx = (float)std::atof(argv[5]), cy = (float)std::atof(argv[6]), fx = (float)std::atof(argv[7]), fy = (float)std::atof(argv[8]);
    MultiMotionFusion* mmf = new MultiMotionFusion(ctx, W, H, cx, cy, fx, fy, &cfg);
    mmf->setEnableMultipleModels(true);
    mmf->setMaskSegmentation(true);
    mmf->setModelSpawnOffset(1);  // (pushed into the mask configuration while the mode is on)
    for (int i = 0; i < N; ++i) {
        FrameData frame;
        frame.timestamp = 1000 + i, frame.rgb = rgb[i].data(), frame.depth = depth[i].data(), frame.mask = labels[i].data();
        frame.hasNewLabel = (i % 2) == 0;  // ignored with the mode on
        if (mmf->processFrame(frame)) return 2;
        for (const ModelPointer& m : mmf->getModels()) {
            float pose[16];
            m->getPose(pose);
            std::printf("frame %d model %u conf %.9g pose", i, m->getID(), (double)m->getConfidenceThreshold());
            for (float v : pose) std::printf(" %.9g", (double)v);
            std::printf("\n");
        }
    }
    const std::vector<uint8_t> table = mmf->getMaskMapping();
    std::printf("table");
    for (int l = 0; l < 256; ++l)
        if (table[(size_t)l]) std::printf(" %d:%d", l, (int)table[(size_t)l]);
    std::printf("\n");
    CHECK(mmf->getModels().size() == 3);
    CHECK(mmf->frontEndSettings().at("maskSegmentation") == 1.f);
    // inhibitModels reaches the mask configuration too: a fresh label is recorded and spawns nothing
    mmf->setSetInhibit(true);
    std::vector<uint8_t> more(labels[(size_t)N - 1]);
    for (size_t p = 0; p < 40; ++p) more[p] = 99;
    FrameData frame;
    frame.timestamp = 1000 + N, frame.rgb = rgb[(size_t)N - 1].data(), frame.depth = depth[(size_t)N - 1].data(), frame.mask = more.data();
    if (mmf->processFrame(frame)) return 2;
    CHECK(mmf->getModels().size() == 3);
    CHECK(mmf->getMaskMapping()[99] == 3);
    delete mmf;
    std::printf("mask shim sequence: ok\n");
    return 0;
}
