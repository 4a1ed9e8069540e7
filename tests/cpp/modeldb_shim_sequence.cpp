// The model database through the C++ shim: MultiMotionFusion::savePly() into the constructor's exportDirectory,
// Model::exportModelPLY(export_dir, global_pose) and MultiMotionFusion::loadModels(), their files compared byte for byte with
// the C ABI's (mmf_fusion_save_models, mmf_model_export_ply).  The camera model gets a 300-surfel map and three keypoint views;
// its database entry, copied to model-3, is what loadModels restores as an inactive object model.
// Build: see tests/test_gpu_modeldb_shim.py; the argument is a scratch directory.  Exit code 0 = every check passed.
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <random>
#include <vector>

#include "../../multimotionfusion_amd/cpp/MultiMotionFusion.h"

namespace fs = std::filesystem;
static const int W = 320, H = 240, D = 256;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

static std::vector<char> slurp(const fs::path& p) {
    std::ifstream in(p, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const fs::path root(argv[1]);
    const std::string shim_dir = (root / "shim").string() + "/", abi_dir = (root / "abi").string() + "/", model_dir = (root / "model").string() + "/";
    fs::create_directories(model_dir);
    Resolution::setResolution(W, H);
    Intrinsics::setIntrinics(264.f, 264.f, 160.f, 120.f);
    OdometryConfig odom_cfg;
    SegmentationConfiguration segm_cfg;
    MultiMotionFusion mmf(200, 35000, 5e-05f, 1e-05f, /*closeLoops*/ false, false, false, 115, /*confGlobal*/ 10.f, /*confObject*/ 0.01f,
                          /*depthCut*/ 15.f, /*icpWeight*/ 10.f, false, 0.3095f, true, false, 20, Model::MatchingType::Drost, shim_dir, false,
                          std::string(), odom_cfg, segm_cfg);
    mmf.setEnableMultipleModels(true);
    mmf.setEnableRedetection(true);
    ModelPointer global = mmf.getModels().front();

    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    const unsigned n = 300;
    std::vector<float> map((size_t)n * 12);
    for (unsigned i = 0; i < n; ++i) {
        float* s = &map[(size_t)i * 12];
        for (int k = 0; k < 12; ++k) s[k] = u(rng);
        s[3] = i % 3 == 0 ? 5.f : 20.f;  // every third surfel is below the camera model's threshold of 10
        s[4] = (float)(rng() & 0xFFFFFFu);
    }
    CHECK(mmf_model_upload_map(global->handle(), map.data(), n) == MMF_OK);
    const float pose[16] = {1, 0, 0, 0.5f, 0, 1, 0, -0.25f, 0, 0, 1, 2.f, 0, 0, 0, 1};  // exact: pose * pose^-1 has one answer
    global->overridePose(pose);
    const std::vector<int> counts = {3, 0, 40};
    std::vector<float> desc((size_t)43 * D), coord((size_t)43 * 3);
    for (float& v : desc) v = u(rng);
    for (float& v : coord) v = u(rng);
    CHECK(global->store((int)counts.size(), counts.data(), desc.data(), coord.data()));

    mmf.savePly();
    CHECK(mmf_fusion_save_models(mmf.handle(), abi_dir.c_str()) == MMF_OK);
    for (const char* name : {"cloud-0.ply", "model_db/model-0/cloud.ply", "model_db/model-0/tracks.ply"}) {
        const std::vector<char> a = slurp(fs::path(shim_dir) / name), b = slurp(fs::path(abi_dir) / name);
        CHECK(!a.empty() && a == b);
    }
    const std::vector<char> cloud = slurp(fs::path(abi_dir) / "cloud-0.ply");
    const std::string expect = "ply\nformat binary_little_endian 1.0\nelement vertex 200\n";
    CHECK(cloud.size() > expect.size() && std::string(cloud.begin(), cloud.begin() + (long)expect.size()) == expect);
    global->exportModelPLY(model_dir, pose);  // global pose * pose^-1 = identity, as savePly gives the camera model
    CHECK(slurp(fs::path(model_dir) / "cloud-0.ply") == cloud);
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(mmf_model_export_ply(global->handle(), (model_dir + "abi.ply").c_str(), identity) == MMF_OK);
    CHECK(slurp(fs::path(model_dir) / "abi.ply") == cloud);

    // -restore: the entry of an object model (loadModels looks at model-1 .. model-255)
    CHECK(mmf.loadModels() == 0 && mmf.getInactiveModels().empty());
    fs::create_directories(fs::path(shim_dir) / "model_db" / "model-3");
    fs::copy_file(fs::path(shim_dir) / "model_db" / "model-0" / "tracks.ply", fs::path(shim_dir) / "model_db" / "model-3" / "tracks.ply");
    CHECK(mmf.loadModels() == 1);
    CHECK(mmf.getInactiveModels().size() == 1 && mmf.getInactiveModels().front()->getID() == 1 && mmf.getModels().size() == 1);
    int rows = -1, model = -1;
    CHECK(mmf_viewstore_num_views(mmf_fusion_viewstore(mmf.handle())) == 6);
    CHECK(mmf_viewstore_view(mmf_fusion_viewstore(mmf.handle()), 5, &model, nullptr, &rows) == MMF_OK && model == 1 && rows == 40);
    std::printf("modeldb shim sequence: ok\n");
    return 0;
}
