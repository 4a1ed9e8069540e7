// rigid_ransac.hpp -- host-side restatement of Core/Utils/RigidRANSAC.{h,cpp} (keypoint-based pose
// initialisation: Model::getLastTrackTransform, Model.cpp:739-779, called from MultiMotionFusion.cpp:322
// ahead of the dense tracker).  Plain C++ without Eigen; N is a few dozen to a few hundred keypoints, so the class
// stays on the host like the reference's.
//
// Kept from the reference: the hash-sorted correspondence order (RigidRANSAC.cpp:10-58, std::hash<float> of
// libstdc++), std::shuffle on a std::default_random_engine that lives in the object (so successive
// estimate() calls continue its sequence), the candidate test `Ninliers > max(rint(fraction * N), 3)`, the
// refit on the inliers and the mean inlier error as the score.  fit() is the least-squares rigid transform
// T_01 with p0 ~ R p1 + t (Umeyama 1991 / Kabsch): R = U diag(1, 1, det U det V) V^T of the 3x3 correlation
// matrix; the 3x3 SVD is a Jacobi eigen-decomposition of A^T A in double (Eigen::JacobiSVD<Matrix3f> in the
// reference: same rotation up to float rounding wherever it is unique).
//
// The arithmetic -- jacobi_eigen_sym3, svd3, det3, rigid_fit, rigid_apply and the steps of estimate() (ransac_core) -- is
// MMF_HD: compiled for the host here and for the device by ransac_kernels.hpp, one source for both, no std:: algorithm on
// that path.  With -ffp-contract=off and correctly rounded sqrt and division the two sides agree bit for bit
// (DESIGN.md B6 (4)).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMF_HD __host__ __device__
#define MMF_UNROLL _Pragma("unroll")
#else
#define MMF_HD
#define MMF_UNROLL
#endif

namespace mmf {

struct Isometry3f {  // row-major 3x3 rotation + translation: x -> R x + t
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    float t[3] = {0, 0, 0};
};

namespace ransac_detail {

MMF_HD inline void jacobi_eigen_sym3(double S[9], double V[9]) {  // S symmetric -> eigenvalues on its diagonal, S = V D V^T
    for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double off = S[1] * S[1] + S[2] * S[2] + S[5] * S[5];
        if (off < 1e-300) break;
        MMF_UNROLL  // (compile-time 3x3 indices: the matrices stay in registers on the device)
        for (int p = 0; p < 2; ++p)
            MMF_UNROLL
            for (int q = p + 1; q < 3; ++q) {
                const double apq = S[p * 3 + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (S[q * 3 + q] - S[p * 3 + p]) / (2.0 * apq);
                const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 3; ++k) {  // S <- J^T S J, V <- V J
                    const double skp = S[k * 3 + p], skq = S[k * 3 + q];
                    S[k * 3 + p] = c * skp - s * skq;
                    S[k * 3 + q] = s * skp + c * skq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double spk = S[p * 3 + k], sqk = S[q * 3 + k];
                    S[p * 3 + k] = c * spk - s * sqk;
                    S[q * 3 + k] = s * spk + c * sqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k * 3 + p], vkq = V[k * 3 + q];
                    V[k * 3 + p] = c * vkp - s * vkq;
                    V[k * 3 + q] = s * vkp + c * vkq;
                }
            }
    }
}

MMF_HD inline double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

MMF_HD inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}
MMF_HD inline void normalise3(double* a) {
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (n > 0) a[0] /= n, a[1] /= n, a[2] /= n;
}
MMF_HD inline void swap_eig(double& ea, double* va, double& eb, double* vb) {
    const double e = ea;
    ea = eb, eb = e;
    for (int r = 0; r < 3; ++r) {
        const double v = va[r];
        va[r] = vb[r], vb[r] = v;
    }
}

// A = U diag(s) V^T with s descending, U and V orthogonal (full SVD of a 3x3)
MMF_HD inline void svd3(const double A[9], double U[9], double s[3], double V[9]) {
    double AtA[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) AtA[r * 3 + c] = A[0 * 3 + r] * A[0 * 3 + c] + A[1 * 3 + r] * A[1 * 3 + c] + A[2 * 3 + r] * A[2 * 3 + c];
    double Vt[9];
    jacobi_eigen_sym3(AtA, Vt);
    // eigenvalues descending, each with its eigenvector: the stable three-element insertion that std::sort of libstdc++
    // performs on three elements (ties -- and unordered values -- keep the result of the std::sort this replaces)
    double e0 = AtA[0], e1 = AtA[4], e2 = AtA[8];
    double v0[3] = {Vt[0], Vt[3], Vt[6]}, v1[3] = {Vt[1], Vt[4], Vt[7]}, v2[3] = {Vt[2], Vt[5], Vt[8]};
    if (e1 > e0) swap_eig(e0, v0, e1, v1);
    if (e2 > e0) {  // (2, 0, 1)
        swap_eig(e1, v1, e2, v2);
        swap_eig(e0, v0, e1, v1);
    } else if (e2 > e1) {
        swap_eig(e1, v1, e2, v2);
    }
    const double ev[3] = {e0, e1, e2};
    for (int c = 0; c < 3; ++c) s[c] = std::sqrt(0.0 < ev[c] ? ev[c] : 0.0);
    for (int r = 0; r < 3; ++r) V[r * 3 + 0] = v0[r], V[r * 3 + 1] = v1[r], V[r * 3 + 2] = v2[r];
    // U columns: A v_c / s_c; rank-deficient columns completed to an orthonormal basis
    double u[3][3];
    int good = 0;
    const double floor0 = s[0] < 1e-300 ? 1e-300 : s[0];
    for (int c = 0; c < 3; ++c) {
        double col[3] = {0, 0, 0};
        for (int r = 0; r < 3; ++r) col[r] = A[r * 3 + 0] * V[0 * 3 + c] + A[r * 3 + 1] * V[1 * 3 + c] + A[r * 3 + 2] * V[2 * 3 + c];
        if (s[c] > 1e-12 * floor0) {
            for (int r = 0; r < 3; ++r) u[c][r] = col[r] / s[c];
            good = c + 1;
        }
    }
    if (good == 0) u[0][0] = 1, u[0][1] = 0, u[0][2] = 0, good = 1;
    if (good == 1) {  // any unit vector orthogonal to u0
        const double* a = u[0];
        const int k = std::fabs(a[0]) < std::fabs(a[1]) ? (std::fabs(a[0]) < std::fabs(a[2]) ? 0 : 2) : (std::fabs(a[1]) < std::fabs(a[2]) ? 1 : 2);
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        cross3(a, e, u[1]);
        normalise3(u[1]);
        good = 2;
    }
    if (good == 2) {
        cross3(u[0], u[1], u[2]);
        normalise3(u[2]);
    }
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) U[r * 3 + c] = u[c][r];
}

}  // namespace ransac_detail

// row selections of a fit: every row, the rows a byte mask flags, the rows whose bit is set in 64-bit words
struct SelAll {
    MMF_HD bool operator()(int) const { return true; }
};
struct SelBytes {
    const unsigned char* mask;
    MMF_HD bool operator()(int i) const { return mask[i] != 0; }
};
struct SelBits {  // bit (i & 63) of words[(i >> 6) * stride]
    const unsigned long long* words;
    int stride;
    MMF_HD bool operator()(int i) const { return (words[(size_t)(i >> 6) * stride] >> (i & 63)) & 1ull; }
};

// RigidRANSAC.cpp:73-120: least-squares T_01 over the selected rows, summed in ascending row order
template <class Sel>
MMF_HD inline Isometry3f rigid_fit_sel(const float* p0, const float* p1, int n, Sel sel) {
    using namespace ransac_detail;
    double m0[3] = {0, 0, 0}, m1[3] = {0, 0, 0};
    int cnt = 0;
    for (int i = 0; i < n; ++i)
        if (sel(i)) {
            for (int k = 0; k < 3; ++k) m0[k] += p0[3 * i + k], m1[k] += p1[3 * i + k];
            ++cnt;
        }
    Isometry3f T;
    if (cnt == 0) return T;
    for (int k = 0; k < 3; ++k) m0[k] /= cnt, m1[k] /= cnt;
    double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // A[r][c] = sum_i (p0_i - m0)[r] (p1_i - m1)[c]
    for (int i = 0; i < n; ++i)
        if (sel(i))
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) A[r * 3 + c] += (p0[3 * i + r] - m0[r]) * (p1[3 * i + c] - m1[c]);
    double U[9], s[3], V[9];
    svd3(A, U, s, V);
    const double d = det3(U) * det3(V);  // guarantee det R = +1 (RigidRANSAC.cpp:111)
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = U[r * 3 + 0] * V[c * 3 + 0] + U[r * 3 + 1] * V[c * 3 + 1] + d * U[r * 3 + 2] * V[c * 3 + 2];
    for (int k = 0; k < 9; ++k) T.R[k] = (float)R[k];
    for (int r = 0; r < 3; ++r) T.t[r] = (float)(m0[r] - (R[r * 3 + 0] * m1[0] + R[r * 3 + 1] * m1[1] + R[r * 3 + 2] * m1[2]));
    return T;
}

// the rows selected by mask (all rows when mask is null)
inline Isometry3f rigid_fit(const float* p0, const float* p1, int n, const unsigned char* mask = nullptr) {
    return mask ? rigid_fit_sel(p0, p1, n, SelBytes{mask}) : rigid_fit_sel(p0, p1, n, SelAll{});
}

// RigidRANSAC.cpp:122-126: the distance || p0 - T p1 || of one row
MMF_HD inline float rigid_distance(const Isometry3f& T, const float* p0, const float* p1) {
    float d2 = 0;
    for (int r = 0; r < 3; ++r) {
        const float x = T.R[r * 3 + 0] * p1[0] + T.R[r * 3 + 1] * p1[1] + T.R[r * 3 + 2] * p1[2] + T.t[r];
        const float e = p0[r] - x;
        d2 += e * e;
    }
    return std::sqrt(d2);
}

inline void rigid_apply(const Isometry3f& T, const float* p0, const float* p1, int n, float* dist) {
    for (int i = 0; i < n; ++i) dist[i] = rigid_distance(T, p0 + 3 * i, p1 + 3 * i);
}

// ---- the steps of estimate(), shared by RigidRANSAC, ransac_core_host and the device verifier (ransac_kernels.hpp) ------------
namespace ransac_core {

// std::hash<float> of libstdc++ on 64-bit restated: 0 for +-0, else _Hash_bytes (MurmurHash64A-style) of the value's four
// bytes with the seed 0xc70f6907
MMF_HD inline unsigned long long hash_float_bits(unsigned b) {
    if ((b & 0x7fffffffu) == 0u) return 0ull;
    const unsigned long long mul = 0xc6a4a7935bd1e995ull;
    unsigned long long h = 0xc70f6907ull ^ (4ull * mul);
    h ^= (unsigned long long)b;
    h *= mul;
    h = (h ^ (h >> 47)) * mul;
    h ^= h >> 47;
    return h;
}
MMF_HD inline unsigned float_bits(float v) {
    union {
        float f;
        unsigned u;
    } x;
    x.f = v;
    return x.u;
}
MMF_HD inline unsigned long long hash3(const float* v) {  // RigidRANSAC.cpp:10-22
    unsigned long long seed = 0;
    for (int i = 0; i < 3; ++i) seed ^= hash_float_bits(float_bits(v[i])) + 0xBADEAFFEull + (seed << 6) + (seed >> 2);
    return seed;
}
// the sort key of one correspondence (RigidRANSAC.cpp:36-47); rows are ordered by (key, original index) ascending
MMF_HD inline unsigned long long hash_row(const float* p0, const float* p1) {
    unsigned long long seed = 0;
    seed ^= hash3(p0) + 0xCAFED00Dull + (seed << 6) + (seed >> 2);
    seed ^= hash3(p1) + 0xCAFED00Dull + (seed << 6) + (seed >> 2);
    return seed;
}

// a hypothesis becomes a candidate with more inliers than this (RigidRANSAC.cpp:163)
MMF_HD inline int candidate_floor(float inlier_fraction, int N) {
    const int f = (int)rintf(inlier_fraction * N);
    return f > 3 ? f : 3;
}

// the fit to three rows, added in ascending row order like the masked loop of rigid_fit
MMF_HD inline Isometry3f fit_triple(const float* p0s, const float* p1s, int a, int b, int c) {
    int t;
    if (b < a) t = a, a = b, b = t;
    if (c < b) t = b, b = c, c = t;
    if (b < a) t = a, a = b, b = t;
    const int rows[3] = {a, b, c};
    float q0[9], q1[9];
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) q0[3 * j + k] = p0s[3 * rows[j] + k], q1[3 * j + k] = p1s[3 * rows[j] + k];
    return rigid_fit_sel(q0, q1, 3, SelAll{});
}

// the refit on a candidate's inliers and its score, the mean inlier distance: both sequential in row order
template <class Sel>
MMF_HD inline Isometry3f refit_score(const float* p0s, const float* p1s, int N, Sel inlier, int Ninliers, float* error) {
    const Isometry3f Tall = rigid_fit_sel(p0s, p1s, N, inlier);
    float sum = 0;
    for (int i = 0; i < N; ++i) {
        const float d = rigid_distance(Tall, p0s + 3 * i, p1s + 3 * i);
        sum += inlier(i) ? d : 0.f;
    }
    *error = sum / Ninliers;
    return Tall;
}

}  // namespace ransac_core

class RigidRANSAC {
   public:
    struct Config {
        int iterations;
        float inlier_threshold;
        float inlier_fraction;
    };
    struct Result {
        Isometry3f transformation;
        float error = std::numeric_limits<float>::infinity();
        std::vector<unsigned char> inlier;  // over the HASH-SORTED rows, like the reference's (empty: no model beat the initial fit)
    };

    RigidRANSAC(int iterations, float inlier_threshold, float inlier_fraction) : cfg{iterations, inlier_threshold, inlier_fraction} {}
    explicit RigidRANSAC(const Config& config) : cfg(config) {}

    // RigidRANSAC.cpp:128-180; needs n >= 3 (and >= 3 masked rows when a mask is given)
    Result estimate(const float* p0, const float* p1, int N, const unsigned char* mask = nullptr) {
        Result result;
        std::vector<float> p0s(3 * (size_t)N), p1s(3 * (size_t)N);
        sort_by_hash(p0, p1, N, p0s.data(), p1s.data());
        result.transformation = rigid_fit(p0s.data(), p1s.data(), N, mask);
        std::vector<float> distance(N);
        std::vector<unsigned char> weights(N), inliers(N);
        const int Nparams = 3;
        for (int it = 0; it < cfg.iterations; ++it) {
            std::vector<std::ptrdiff_t> idx(N);
            for (int i = 0; i < N; ++i) idx[i] = i;
            std::shuffle(idx.begin(), idx.end(), generator);
            std::fill(weights.begin(), weights.end(), 0);
            int chosen = 0;
            for (size_t i = 0; i < idx.size() && chosen < Nparams; ++i) {
                const std::ptrdiff_t id = idx[i];
                const unsigned char w = mask ? mask[id] : 1;
                chosen += (w && !weights[id]) ? 1 : 0;
                weights[id] = w;
            }
            if (chosen < Nparams) break;  // the reference asserts here
            const Isometry3f transform = rigid_fit(p0s.data(), p1s.data(), N, weights.data());
            rigid_apply(transform, p0s.data(), p1s.data(), N, distance.data());
            int Ninliers = 0;
            for (int i = 0; i < N; ++i) {
                inliers[i] = (distance[i] < cfg.inlier_threshold) && (!mask || mask[i]);
                Ninliers += inliers[i];
            }
            if (Ninliers > ransac_core::candidate_floor(cfg.inlier_fraction, N)) {
                float error;
                const Isometry3f Tall = ransac_core::refit_score(p0s.data(), p1s.data(), N, SelBytes{inliers.data()}, Ninliers, &error);
                if (error < result.error) {
                    result.error = error;
                    result.transformation = Tall;
                    result.inlier = inliers;
                }
            }
        }
        return result;
    }

    // RigidRANSAC.cpp:10-58: correspondences ordered by a hash of their six floats, ties by their index
    static void sort_by_hash(const float* p0, const float* p1, int N, float* p0s, float* p1s) {
        std::vector<std::pair<unsigned long long, std::size_t>> hash(N);
        for (int i = 0; i < N; ++i) hash[i] = {ransac_core::hash_row(p0 + 3 * i, p1 + 3 * i), (std::size_t)i};
        std::sort(hash.begin(), hash.end());
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < 3; ++k) {
                p0s[3 * i + k] = p0[3 * hash[i].second + k];
                p1s[3 * i + k] = p1[3 * hash[i].second + k];
            }
    }

   private:
    std::default_random_engine generator;
    const Config cfg;
};

// ---- the per-problem rule of the device verifier, on the host ---------------------------------------------
// A FRESH engine per problem and no mask: the rows hypothesis `it` is fitted to are the first three entries of the shuffled
// index vector, a function of (N, it) alone.  ransac_triples writes them for one N (out[iterations][3]), with the class's own
// std::shuffle on its own engine type; the table holds them for 3 <= N <= max_points, entry (N, it) at
// 3 * ((N - 3) * iterations + it).
inline void ransac_triples(int iterations, int N, unsigned short* out) {
    std::default_random_engine generator;
    std::vector<std::ptrdiff_t> idx(N);
    for (int it = 0; it < iterations; ++it) {
        for (int i = 0; i < N; ++i) idx[i] = i;
        std::shuffle(idx.begin(), idx.end(), generator);
        for (int k = 0; k < 3; ++k) out[3 * it + k] = (unsigned short)idx[k];
    }
}
inline std::vector<unsigned short> ransac_triple_table(int iterations, int max_points) {
    std::vector<unsigned short> table((size_t)3 * (size_t)iterations * (size_t)(max_points - 2));
    for (int N = 3; N <= max_points; ++N) ransac_triples(iterations, N, table.data() + 3 * (size_t)(N - 3) * iterations);
    return table;
}

// estimate(p0, p1, N) of a fresh RigidRANSAC(cfg) from the table and the shared steps, in the order the device verifier
// takes them: sort, hypotheses, inlier words, refits, scan.  triples = the table's rows of this N ([iterations][3]); inlier
// (optional, N bytes) is over the hash-sorted rows.
// Returns the number of inliers of the winning hypothesis, 0 when none was accepted (error +inf, T = the all-points fit).
inline int ransac_core_host(const RigidRANSAC::Config& cfg, const unsigned short* triples, const float* p0, const float* p1, int N,
                            Isometry3f* T, float* error, unsigned char* inlier) {
    using namespace ransac_core;
    std::vector<float> p0s(3 * (size_t)N), p1s(3 * (size_t)N);
    RigidRANSAC::sort_by_hash(p0, p1, N, p0s.data(), p1s.data());
    const int words = (N + 63) / 64;
    std::vector<unsigned long long> bits((size_t)words * cfg.iterations, 0ull);
    std::vector<int> count(cfg.iterations, 0);
    for (int it = 0; it < cfg.iterations; ++it) {
        const unsigned short* tr = triples + 3 * it;
        const Isometry3f Th = fit_triple(p0s.data(), p1s.data(), tr[0], tr[1], tr[2]);
        for (int i = 0; i < N; ++i)
            if (rigid_distance(Th, p0s.data() + 3 * i, p1s.data() + 3 * i) < cfg.inlier_threshold) {
                bits[(size_t)(i >> 6) * cfg.iterations + it] |= 1ull << (i & 63);
                ++count[it];
            }
    }
    *T = rigid_fit_sel(p0s.data(), p1s.data(), N, SelAll{});
    *error = std::numeric_limits<float>::infinity();
    int best = -1;
    for (int it = 0; it < cfg.iterations; ++it) {
        if (!(count[it] > candidate_floor(cfg.inlier_fraction, N))) continue;
        float e;
        const Isometry3f Tall = refit_score(p0s.data(), p1s.data(), N, SelBits{bits.data() + it, cfg.iterations}, count[it], &e);
        if (e < *error) *error = e, *T = Tall, best = it;
    }
    if (inlier)
        for (int i = 0; i < N; ++i) inlier[i] = best < 0 ? 0 : (unsigned char)SelBits{bits.data() + best, cfg.iterations}(i);
    return best < 0 ? 0 : count[best];
}

}  // namespace mmf
