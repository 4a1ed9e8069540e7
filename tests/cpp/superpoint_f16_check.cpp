// cpp/SuperPoint.h with Precision::F16 against the C ABI: one image through SuperPoint(ctx, weights, w, h, n, SuperPoint::F16)
// ::getFeatures and through mmf_superpoint_create_ex(..., MMF_SP_F16) + mmf_superpoint_get_features; a default-constructed
// object must report F32.  argv: [1] image u8 x 3; [2] the 12 {weight, bias} arrays as float32; [3] width; [4] height.
// Prints "precision: f16", "keypoints: n" and "shim agrees: 0|1".  Build: see tests/test_gpu_superpoint_f16_shim.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../multimotionfusion_amd/cpp/SuperPoint.h"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 5);
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
    CHECK(W > 0 && H > 0);
    const size_t npix = (size_t)W * H;
    std::vector<uint8_t> rgb(npix * 3);
    FILE* fp = std::fopen(argv[1], "rb");
    CHECK(fp != nullptr);
    CHECK(std::fread(rgb.data(), 1, rgb.size(), fp) == rgb.size());
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

    mmf::Context ctx(0);
    unsigned char* image = nullptr;
    CHECK(hipMalloc((void**)&image, rgb.size()) == hipSuccess);
    CHECK(hipMemcpy(image, rgb.data(), rgb.size(), hipMemcpyHostToDevice) == hipSuccess);
    const int max_kp = 1024;
    {
        SuperPoint plain(ctx, weights.data(), W, H, max_kp);
        CHECK(plain.precision() == SuperPoint::F32);
    }
    SuperPoint kp(ctx, weights.data(), W, H, max_kp, SuperPoint::F16);
    CHECK(kp.precision() == SuperPoint::F16);
    CHECK(mmf_superpoint_precision(kp.handle()) == MMF_SP_F16);
    std::printf("precision: f16\n");
    std::vector<double> coordinates, descriptors;
    std::tie(coordinates, descriptors) = kp.getFeatures(image, W, H, 3);
    const size_t n = coordinates.size() / 2;
    std::printf("keypoints: %zu\n", n);
    CHECK(descriptors.size() == n * 256);

    mmf_superpoint* raw = nullptr;
    CHECK(mmf_superpoint_create_ex(ctx.get(), weights.data(), W, H, max_kp, MMF_SP_F16, &raw) == 0);
    std::vector<int> xy((size_t)max_kp * 2);
    std::vector<float> conf((size_t)max_kp), desc((size_t)max_kp * 256);
    int m = 0;
    CHECK(mmf_superpoint_get_features(raw, image, W, H, 3, 0.015f, 4, 4, xy.data(), conf.data(), desc.data(), &m) == 0);
    bool same = (size_t)m == n;
    for (size_t k = 0; same && k < n; ++k)
        same = coordinates[2 * k] == (double)xy[2 * k] / (double)W && coordinates[2 * k + 1] == (double)xy[2 * k + 1] / (double)H;
    for (size_t k = 0; same && k < n * 256; ++k) same = descriptors[k] == (double)desc[k];
    std::printf("shim agrees: %d\n", same ? 1 : 0);
    mmf_superpoint_destroy(raw);
    CHECK(mmf_superpoint_create_ex(ctx.get(), weights.data(), W, H, max_kp, 2, &raw) != 0);  // no such precision
    (void)hipFree(image);
    return 0;
}
