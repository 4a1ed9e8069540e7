// Host code only: the RANSAC core shared with the device verifier (csrc/rigid_ransac.hpp) against a fresh RigidRANSAC per
// problem, over the sizes and kinds of tests/ransac_cases.py.  Built with -fsanitize=address,undefined by
// tests/test_ransac_core.py and run directly; prints "ok <problems> <with inliers>" or the first difference.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../multimotionfusion_amd/csrc/rigid_ransac.hpp"

namespace {

std::mt19937 rng(12345);
float uni(float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }

void make(int kind, int n, std::vector<float>& p0, std::vector<float>& p1) {
    p0.assign(3 * (size_t)n, 0.f), p1.assign(3 * (size_t)n, 0.f);
    const float ang = uni(-3.f, 3.f), c = std::cos(ang), s = std::sin(ang);
    const float R[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, t[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
    const float dir[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)}, dir2[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
    const float fixed[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
    for (int i = 0; i < n; ++i) {
        float q[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
        const float a = uni(-1, 1), b = uni(-1, 1);
        for (int k = 0; k < 3; ++k) {
            if (kind == 5) q[k] = fixed[k];                   // coincident
            if (kind == 6) q[k] = a * dir[k];                 // collinear
            if (kind == 7) q[k] = a * dir[k] + b * dir2[k];   // coplanar
        }
        for (int k = 0; k < 3; ++k) p1[3 * i + k] = q[k];
        if (kind == 8) q[2] = -q[2];  // mirrored
        for (int r = 0; r < 3; ++r) p0[3 * i + r] = R[3 * r] * q[0] + R[3 * r + 1] * q[1] + R[3 * r + 2] * q[2] + t[r] + uni(-0.0005f, 0.0005f);
        const bool outlier = kind == 2 || (kind == 1 && uni(0, 1) < 0.3f);
        if (outlier)
            for (int k = 0; k < 3; ++k) p0[3 * i + k] = uni(-2, 2);
        if (kind == 3 && (i & 1))  // duplicated rows
            for (int k = 0; k < 3; ++k) p0[3 * i + k] = p0[3 * (i - 1) + k], p1[3 * i + k] = p1[3 * (i - 1) + k];
        if (kind == 4) {  // components that are +-0.0
            if (i % 2 == 0) p0[3 * i] = 0.f;
            if (i % 3 == 0) p1[3 * i + 1] = -0.f;
        }
    }
}

}  // namespace

int main() {
    const int sizes[] = {3, 4, 5, 6, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 700, 1023, 1024};
    const mmf::RigidRANSAC::Config cfg{10, 0.03f, 0.8f};
    const std::vector<unsigned short> table = mmf::ransac_triple_table(cfg.iterations, 1024);
    int problems = 0, with = 0;
    std::vector<float> p0, p1;
    for (int rep = 0; rep < 2; ++rep)
        for (int n : sizes)
            for (int kind = 0; kind < 9; ++kind) {
                make(kind, n, p0, p1);
                mmf::RigidRANSAC fresh(cfg);
                const mmf::RigidRANSAC::Result ref = fresh.estimate(p0.data(), p1.data(), n);
                mmf::Isometry3f T;
                float error;
                std::vector<unsigned char> inlier(n);
                const int count = mmf::ransac_core_host(cfg, table.data() + 3 * (size_t)(n - 3) * cfg.iterations, p0.data(), p1.data(), n, &T,
                                                        &error, inlier.data());
                bool same = std::memcmp(T.R, ref.transformation.R, sizeof(T.R)) == 0 && std::memcmp(T.t, ref.transformation.t, sizeof(T.t)) == 0 &&
                            std::memcmp(&error, &ref.error, sizeof(float)) == 0 && (count > 0) == !ref.inlier.empty();
                if (same && count > 0) same = std::memcmp(inlier.data(), ref.inlier.data(), (size_t)n) == 0;
                if (!same) {
                    std::printf("differs: kind %d n %d error %g / %g\n", kind, n, (double)error, (double)ref.error);
                    return 1;
                }
                ++problems, with += count > 0 ? 1 : 0;
            }
    std::printf("ok %d %d\n", problems, with);
    return 0;
}
