// Restoring dense surfels through the C++ shim: Model::importCloud followed by an export gives the records back byte for
// byte, Model::setTimestamps moves the timestamps and nothing else, and MultiMotionFusion::setRestoreDense(true) makes
// loadModels() give the restored model the records of its cloud.ply (without it: none, as before).
// Build: see tests/test_gpu_modeldb_restore_shim.py; the argument is a scratch directory.  Exit code 0 = every check passed.
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <random>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

namespace fs = std::filesystem;
static const int W = 320, H = 240, D = 256, REC = 31;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const fs::path root(argv[1]);
    const std::string dir = (root / "shim").string() + "/";
    Resolution::setResolution(W, H);
    Intrinsics::setIntrinics(264.f, 264.f, 160.f, 120.f);
    OdometryConfig odom_cfg;
    SegmentationConfiguration segm_cfg;
    MultiMotionFusion mmf(200, 35000, 5e-05f, 1e-05f, /*closeLoops*/ false, false, false, 115, /*confGlobal*/ 10.f, /*confObject*/ 0.01f,
                          /*depthCut*/ 15.f, /*icpWeight*/ 10.f, false, 0.3095f, true, false, 20, Model::MatchingType::Drost, dir, false,
                          std::string(), odom_cfg, segm_cfg);
    mmf.setEnableMultipleModels(true);
    mmf.setEnableRedetection(true);
    ModelPointer global = mmf.getModels().front();

    // 300 records: finite, no -0.0 in the positions, no zero normal component -- the set on which import then export is the identity
    std::mt19937 rng(9);
    std::uniform_real_distribution<float> u(0.25f, 1.f);
    const unsigned n = 300;
    std::vector<unsigned char> records((size_t)n * REC);
    for (unsigned i = 0; i < n; ++i) {
        unsigned char* r = &records[(size_t)i * REC];
        for (int k : {0, 4, 8, 15, 19, 23, 27}) {
            const float v = (rng() & 1u) ? u(rng) : -u(rng);
            std::memcpy(r + k, &v, 4);
        }
        for (int k = 12; k < 15; ++k) r[k] = (unsigned char)(rng() & 255u);
    }
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    global->importCloud(records.data(), n, nullptr, 11.f, 5);
    CHECK(global->lastCount() == n && mmf_model_import_last_launches(global->handle()) == 1);
    std::vector<unsigned char> back((size_t)n * REC);
    unsigned got = 0;
    CHECK(mmf_model_export_cloud(global->handle(), identity, 10.f, back.data(), n, &got) == MMF_OK && got == n);
    CHECK(back == records);
    global->setTimestamps(300);
    for (const auto& s : global->downloadMap()) {
        float v[12];
        std::memcpy(v, &s, sizeof(v));
        CHECK(v[3] == 11.f && v[5] == 0.f && v[6] == 5.f && v[7] == 300.f);
    }

    // the camera model's database entry, copied to model-3, is what loadModels restores as an object model
    const std::vector<int> counts = {3, 0, 40};
    std::vector<float> desc((size_t)43 * D), coord((size_t)43 * 3);
    for (float& v : desc) v = u(rng);
    for (float& v : coord) v = u(rng);
    CHECK(global->store((int)counts.size(), counts.data(), desc.data(), coord.data()));
    mmf.savePly();
    fs::create_directories(fs::path(dir) / "model_db" / "model-3");
    for (const char* name : {"tracks.ply", "cloud.ply"})
        fs::copy_file(fs::path(dir) / "model_db" / "model-0" / name, fs::path(dir) / "model_db" / "model-3" / name);
    CHECK(mmf.loadModels() == 1);  // setRestoreDense defaults to false: no dense surfels, as before
    CHECK(mmf.getInactiveModels().size() == 1 && mmf.getInactiveModels().back()->lastCount() == 0);
    mmf.setRestoreDense(true);
    CHECK(mmf.loadModels() == 1);
    CHECK(mmf.getInactiveModels().size() == 2 && mmf.getInactiveModels().front()->lastCount() == 0);
    ModelPointer restored = mmf.getInactiveModels().back();
    CHECK(restored->getID() == 2 && restored->lastCount() == n);
    mmf_dense_restore info[2];
    int n_info = 0;
    CHECK(mmf_fusion_last_dense_restores(mmf.handle(), info, 2, &n_info) == MMF_OK && n_info == 1);
    CHECK(info[0].model_id == 2 && info[0].surfels == n && info[0].status == MMF_DENSE_RESTORED);
    // its surfels: the file's records (the camera model's pose is the identity: the file holds `records`), stable for the model
    got = 0;
    CHECK(mmf_model_export_cloud(restored->handle(), identity, mmf_model_confidence_threshold(restored->handle()), back.data(), n, &got) == MMF_OK);
    CHECK(got == n && back == records);
    // ... and Model::importPly of the same file
    restored->importPly(dir + "model_db/model-3/cloud.ply", nullptr, 3.f, 7);
    CHECK(restored->lastCount() == n);
    std::printf("modeldb restore shim sequence: ok\n");
    return 0;
}
