// FPFH + Fast Global Registration (fgr.hip; include/mloam_hip.h section (f13)): the arithmetic that exists ONCE -- for the kernels (__host__ __device__), for the
// host tail of mlh_fgr_register (the tuple test, OptimizePairwise, GetOutputTrans: bounded by 3 tuple_max_cnt correspondences), for the device tail of
// mlh_fgr_register_device (the same trial, the same per-correspondence term and solve, and the plan that cuts the tuple test into independent trials) and for the
// tests' CPU restatement (tests/host/fgr_ref.cpp) -- and the option validation. A header of its own so that a stand-alone host program can run it under a sanitizer
// (tests/host/fgr_host_main.cpp; tests/host/fgr_tail_main.cpp replays the device plan).
// Restated from mloam_loop/ThirdParty/FastGlobalRegistration/app.cpp, with its lines: NormalizePoints' per-point arithmetic (324-390), the tuple test (242-307),
// OptimizePairwise (392-505), TransformPoints (507-517), GetOutputTrans (519-534).
// Restated FROM MEMORY of PCL 1.8.0 and FLANN 1.8 -- neither library's source is available to this project, so none of this could be checked against it:
//   pcl::computeMeanAndCovarianceMatrix (common/centroid.hpp): nine un-centred sums xx xy xz yy yz zz x y z, divided by the count, covariance = E[ab] - E[a] E[b];
//   pcl::computeRoots / computeRoots2 / eigen33 (common/eigen.hpp): scale by the largest absolute coefficient (1 when that is <= the smallest normal number),
//     c0 c1 c2 of the characteristic polynomial, |c0| < epsilon -> the quadratic, else the trigonometric closed form, roots sorted, a non-positive smallest root ->
//     the quadratic; the eigenvector of the smallest root from the largest of the three row cross products of (A - lambda I);
//   pcl::solvePlaneParameters (features/feature.hpp): curvature = |lambda / trace|, 0 when the trace is 0;  pcl::flipNormalTowardsViewpoint: flip when
//     (vp - p) . n < 0;  NormalEstimation::computeFeature: fewer than 3 neighbours -> NaN;
//   pcl::computePairFeatures (features/pfh_tools.hpp) and FPFHEstimation::computePointSPFHSignature / weightPointSPFHSignature (features/fpfh.hpp): d_pi_ =
//     1.0f / (2.0f * float(M_PI)); the bin index computed in double from the float feature; hist_incr = 100.0f / float(k - 1); weight = 1.0f / d2;
//     block scale = float(100.0 / sum) when the sum is non-zero;
//   flann::L2<float>::operator() (algorithms/dist.h): groups of four differences, result += d0 d0 + d1 d1 + d2 d2 + d3 d3, then the tail one by one;
//     flann::RadiusResultSet::addPoint: dist < radius (strict).
// CHOSEN, as everywhere in this library: sums of three or four f32 terms (dot products, squared norms, matrix-vector rows) run left to right; Eigen's own reduction
// order is not restated. Translation units that include this header are compiled with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/mloam_hip.h"

#if defined(__HIPCC__)
#define MLH_FGR_HD __host__ __device__ inline
#else
#define MLH_FGR_HD inline
#endif
// the pieces of one tuple-test trial: left to the inliner's judgement, the host's sequential loop over them came out 15 % slower than the loop written out
#define MLH_FGR_HD_FORCE __attribute__((always_inline)) MLH_FGR_HD

namespace mlh {

constexpr int FGR_BINS = 11, FGR_DIM = 33;
constexpr int FGR_MIN_CORRES = 10;           // app.cpp:412

// the argument at fault, or nullptr
inline const char *fgr_opts_fault(const mlh_fgr_opts &o)
{
    const auto radius = [](float v) { return std::isfinite(v) && v > 0.f && v <= 1e3f; };
    if (!radius(o.normal_radius)) return "normal_radius";
    if (!radius(o.fpfh_radius)) return "fpfh_radius";
    if (!std::isfinite(o.div_factor) || !(o.div_factor > 1.0)) return "div_factor";
    if (o.use_absolute_scale != 0 && o.use_absolute_scale != 1) return "use_absolute_scale";
    if (!std::isfinite(o.max_corr_dist) || !(o.max_corr_dist > 0.0)) return "max_corr_dist";
    if (o.iteration_number < 0 || o.iteration_number > 10000) return "iteration_number";
    if (!std::isfinite(o.tuple_scale) || !(o.tuple_scale > 0.f) || o.tuple_scale > 1.f) return "tuple_scale";
    if (o.tuple_max_cnt < 1 || o.tuple_max_cnt > 1000000) return "tuple_max_cnt";
    if (std::isnan(o.global_registration_threshold)) return "global_registration_threshold";
    return nullptr;
}

inline void fgr_opts_defaults(mlh_fgr_opts &o)      // mloam_loop/config/config_loop_realvehicle.yaml
{
    o = mlh_fgr_opts();
    o.normal_radius = 1.0f; o.fpfh_radius = 1.5f;
    o.div_factor = 1.4; o.use_absolute_scale = 1; o.max_corr_dist = 0.025; o.iteration_number = 64;
    o.tuple_scale = 0.95f; o.tuple_max_cnt = 1000;
    o.global_registration_threshold = 2.0;
    o.seed = 1;
}

// ---------------------------------------------------------------- radius search
// FLANN's L2 over three coordinates; a neighbour counts when this is strictly below r * r (the f32 product)
MLH_FGR_HD float fgr_sqdist3(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---------------------------------------------------------------- normals (T = float: the library; T = double: the tests' measure of the f32 error)
template <typename T> MLH_FGR_HD void fgr_roots2(T b, T c, T roots[3])
{
    roots[0] = T(0);
    T d = b * b - T(4) * c;
    if (d < T(0)) d = T(0);
    const T sd = std::sqrt(d);
    roots[2] = T(0.5) * (b + sd);
    roots[1] = T(0.5) * (b - sd);
}

// m: the upper triangle {00, 01, 02, 11, 12, 22}
template <typename T> MLH_FGR_HD void fgr_compute_roots(const T m[6], T roots[3])
{
    const T m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[3], m12 = m[4], m22 = m[5];
    const T c0 = m00 * m11 * m22 + T(2) * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
    const T c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
    const T c2 = m00 + m11 + m22;
    if (std::fabs(c0) < std::numeric_limits<T>::epsilon()) { fgr_roots2(c2, c1, roots); return; }
    const T s_inv3 = T(1.0 / 3.0), s_sqrt3 = std::sqrt(T(3));
    const T c2_over_3 = c2 * s_inv3;
    T a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > T(0)) a_over_3 = T(0);
    const T half_b = T(0.5) * (c0 + c2_over_3 * (T(2) * c2_over_3 * c2_over_3 - c1));
    T q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > T(0)) q = T(0);
    const T rho = std::sqrt(-a_over_3);
    const T theta = std::atan2(std::sqrt(-q), half_b) * s_inv3;
    const T cos_theta = std::cos(theta), sin_theta = std::sin(theta);
    roots[0] = c2_over_3 + T(2) * rho * cos_theta;
    roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    if (roots[0] >= roots[1]) { const T t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
    if (roots[1] >= roots[2]) {
        const T t = roots[1]; roots[1] = roots[2]; roots[2] = t;
        if (roots[0] >= roots[1]) { const T u = roots[0]; roots[0] = roots[1]; roots[1] = u; }
    }
    if (roots[0] <= T(0)) fgr_roots2(c2, c1, roots);
}

// evals: the three roots scaled back, ascending; evec: the unit eigenvector of evals[0]
template <typename T> MLH_FGR_HD void fgr_eigen33(const T m[6], T evals[3], T evec[3])
{
    T scale = T(0);
    for (int i = 0; i < 6; ++i) { const T a = std::fabs(m[i]); if (a > scale) scale = a; }
    if (scale <= std::numeric_limits<T>::min()) scale = T(1);
    T s[6];
    for (int i = 0; i < 6; ++i) s[i] = m[i] / scale;
    T roots[3];
    fgr_compute_roots(s, roots);
    for (int i = 0; i < 3; ++i) evals[i] = roots[i] * scale;
    const T r0[3] = {s[0] - roots[0], s[1], s[2]}, r1[3] = {s[1], s[3] - roots[0], s[4]}, r2[3] = {s[2], s[4], s[5] - roots[0]};
    const T v1[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    const T v2[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
    const T v3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    const T l1 = (v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2], l2 = (v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2], l3 = (v3[0] * v3[0] + v3[1] * v3[1]) + v3[2] * v3[2];
    const T *v = v3;
    T l = l3;
    if (l1 >= l2 && l1 >= l3) { v = v1; l = l1; }
    else if (l2 >= l1 && l2 >= l3) { v = v2; l = l2; }
    const T n = std::sqrt(l);
    for (int i = 0; i < 3; ++i) evec[i] = v[i] / n;
}

// accu: the nine sums xx xy xz yy yz zz x y z over `count` neighbours of the point p. out: {nx, ny, nz, curvature}. evals (may be null) <- the three eigenvalues,
// cos_flip (may be null) <- (0 - p) . n before the flip.
template <typename T> MLH_FGR_HD void fgr_normal_from_sums(const T accu_in[9], int count, const T p[3], T out[4], T *evals_out, T *cos_flip)
{
    if (count < 3) {
        const T nan = std::numeric_limits<T>::quiet_NaN();
        out[0] = out[1] = out[2] = out[3] = nan;
        if (evals_out) evals_out[0] = evals_out[1] = evals_out[2] = nan;
        if (cos_flip) *cos_flip = nan;
        return;
    }
    T a[9];
    for (int i = 0; i < 9; ++i) a[i] = accu_in[i] / T(count);
    const T cov[6] = {a[0] - a[6] * a[6], a[1] - a[6] * a[7], a[2] - a[6] * a[8], a[3] - a[7] * a[7], a[4] - a[7] * a[8], a[5] - a[8] * a[8]};
    T evals[3], n[3];
    fgr_eigen33(cov, evals, n);
    const T eig_sum = cov[0] + cov[3] + cov[5];
    out[3] = eig_sum != T(0) ? std::fabs(evals[0] / eig_sum) : T(0);
    const T vx = T(0) - p[0], vy = T(0) - p[1], vz = T(0) - p[2];
    const T c = (vx * n[0] + vy * n[1]) + vz * n[2];
    if (c < T(0)) { n[0] *= T(-1); n[1] *= T(-1); n[2] *= T(-1); }
    out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
    if (evals_out) { evals_out[0] = evals[0]; evals_out[1] = evals[1]; evals_out[2] = evals[2]; }
    if (cos_flip) *cos_flip = c;
}

// ---------------------------------------------------------------- SPFH
// computePairFeatures(p1, n1, p2, n2): false when the pair is skipped. a1, a2 (may be null) <- the two cosines the swap is decided on.
template <typename T> MLH_FGR_HD bool fgr_pair_features(const T p1[3], const T n1_in[3], const T p2[3], const T n2_in[3], T &f1, T &f2, T &f3, T *a1 = nullptr, T *a2 = nullptr)
{
    T dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const T f4 = std::sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]);
    f1 = f2 = f3 = T(0);
    if (f4 == T(0)) return false;
    T n1[3] = {n1_in[0], n1_in[1], n1_in[2]}, n2[3] = {n2_in[0], n2_in[1], n2_in[2]};
    const T angle1 = ((n1[0] * dp[0] + n1[1] * dp[1]) + n1[2] * dp[2]) / f4;
    const T angle2 = ((n2[0] * dp[0] + n2[1] * dp[1]) + n2[2] * dp[2]) / f4;
    if (a1) *a1 = angle1;
    if (a2) *a2 = angle2;
    if (std::acos(std::fabs(angle1)) > std::acos(std::fabs(angle2))) {
        for (int i = 0; i < 3; ++i) { n1[i] = n2_in[i]; n2[i] = n1_in[i]; dp[i] *= T(-1); }
        f3 = -angle2;
    } else
        f3 = angle1;
    T v[3] = {dp[1] * n1[2] - dp[2] * n1[1], dp[2] * n1[0] - dp[0] * n1[2], dp[0] * n1[1] - dp[1] * n1[0]};
    const T v_norm = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (v_norm == T(0)) { f3 = T(0); return false; }
    for (int i = 0; i < 3; ++i) v[i] /= v_norm;
    const T w[3] = {n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]};
    f2 = (v[0] * n2[0] + v[1] * n2[1]) + v[2] * n2[2];
    f1 = std::atan2((w[0] * n2[0] + w[1] * n2[1]) + w[2] * n2[2], (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2]);
    return true;
}

// where a feature falls in its [0, 1] bin range, in f64 on the f32 feature as PCL writes it: f1 -> (f1 + M_PI) * d_pi_, f2 / f3 -> (f + 1.0) * 0.5
MLH_FGR_HD double fgr_unit_f1(float f1)
{
    const float d_pi = 1.0f / (2.0f * 3.14159265358979323846f);
    return (double(f1) + 3.14159265358979323846) * double(d_pi);
}
MLH_FGR_HD double fgr_unit_f23(float f) { return (double(f) + 1.0) * 0.5; }
// floor(11 u) clamped to [0, 10]; NaN: bin 0 (x86 converts floor(NaN) to INT_MIN, which the clamp raises to 0)
MLH_FGR_HD int fgr_bin(double u)
{
    const double h = std::floor(double(FGR_BINS) * u);
    if (!(h >= 0.0)) return 0;
    if (h >= double(FGR_BINS)) return FGR_BINS - 1;
    return int(h);
}
// the f32 bin value of an integer count: `count` sequential additions of hist_incr = 100.0f / float(k - 1) (k: the point's neighbours, itself included)
MLH_FGR_HD float fgr_spfh_value(int count, int k)
{
    const float incr = 100.0f / float(k - 1);
    float v = 0.f;
    for (int c = 0; c < count; ++c) v += incr;
    return v;
}
// weightPointSPFHSignature's block scale
MLH_FGR_HD float fgr_block_scale(float sum) { return sum != 0.f ? float(100.0 / double(sum)) : sum; }

// ---------------------------------------------------------------- matching
MLH_FGR_HD float fgr_l2_33(const float *a, const float *b)
{
    float result = 0.f;
    for (int g = 0; g < 32; g += 4) {
        const float d0 = a[g] - b[g], d1 = a[g + 1] - b[g + 1], d2 = a[g + 2] - b[g + 2], d3 = a[g + 3] - b[g + 3];
        result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    const float d = a[32] - b[32];
    result += d * d;
    return result;
}
MLH_FGR_HD bool fgr_row_finite(const float *a)
{
    bool ok = true;
    for (int i = 0; i < FGR_DIM; ++i) ok = ok && (fabsf(a[i]) <= 3.402823466e38f);      // false for NaN and for infinities
    return ok;
}

// ---------------------------------------------------------------- the tail: the host's (fgr_host_tail) and what the device's kernels share with it
// one mutual pair after the un-swap: i indexes cloud 0 (model), j cloud 1 (data); p, q their NORMALISED points
struct FgrPair { int32_t i, j; float p[3], q[3]; };
static_assert(sizeof(FgrPair) == 32, "the pinned pair record");

// the tuple test's generator (DEPARTURE from srand(time(NULL)) / rand()): xorshift64*, 31 bits per draw like rand()
struct FgrRng {
    uint64_t s;
    MLH_FGR_HD explicit FgrRng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull) { if (s == 0) s = 0x2545F4914F6CDD1Dull; }
    MLH_FGR_HD uint32_t next()
    {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return uint32_t((s * 0x2545F4914F6CDD1Dull) >> 33);
    }
};

// The state update of next() is a linear map A over GF(2)^64 (three xor-shifts), so the state in front of draw k is A^k s0: a product of the A^(2^b) of k's set
// bits. The table: FGR_RNG_POWERS matrices of 64 words, word i of matrix b = A^(2^b) applied to bit i. Built once on the host (fgr_rng_table()) and handed to the
// device once per context; 2^FGR_RNG_POWERS draws are more than 3 x 100 x any pair count an int32 holds.
constexpr int FGR_RNG_POWERS = 44;
constexpr int FGR_RNG_TABLE_WORDS = FGR_RNG_POWERS * 64;

MLH_FGR_HD uint64_t fgr_gf2_apply(const uint64_t *m, uint64_t v)
{
    uint64_t r = 0;
    for (int i = 0; i < 64; ++i) r ^= ((v >> i) & 1ull) ? m[i] : 0ull;
    return r;
}
inline void fgr_rng_table_build(uint64_t *table)
{
    for (int i = 0; i < 64; ++i) {
        uint64_t s = 1ull << i;
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        table[i] = s;
    }
    for (int b = 1; b < FGR_RNG_POWERS; ++b)
        for (int i = 0; i < 64; ++i) table[b * 64 + i] = fgr_gf2_apply(table + (b - 1) * 64, table[(b - 1) * 64 + i]);
}
inline const uint64_t *fgr_rng_table()
{
    static const std::vector<uint64_t> t = [] { std::vector<uint64_t> v; v.resize(FGR_RNG_TABLE_WORDS); fgr_rng_table_build(v.data()); return v; }();
    return t.data();
}
// the generator as it stands in front of draw k (k < 2^FGR_RNG_POWERS) of the sequence FgrRng(seed) starts
MLH_FGR_HD FgrRng fgr_rng_at(const uint64_t *table, uint64_t seed, uint64_t k)
{
    FgrRng r(seed);
    for (int b = 0; b < FGR_RNG_POWERS; ++b)
        if ((k >> b) & 1ull) r.s = fgr_gf2_apply(table + b * 64, r.s);
    return r;
}
inline FgrRng fgr_rng_at(uint64_t seed, uint64_t k) { return fgr_rng_at(fgr_rng_table(), seed, k); }

MLH_FGR_HD_FORCE float fgr_dist3(const float a[3], const float b[3])
{
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// One trial of the tuple test (app.cpp:256-291): three draws of rng (fgr_trial_draw: the emit pass repeats them alone for a trial it knows to be accepted),
// r[] <- the three pair indices; true when the three side lengths of the two triangles agree
// within `scale`. ncorr > 0. The only text of this arithmetic: fgr_tuple_test below, the device's count and emit kernels and the tests' replay call it.
MLH_FGR_HD_FORCE void fgr_trial_draw(int ncorr, FgrRng &rng, int r[3])
{
    const int r0 = int(rng.next() % uint32_t(ncorr)), r1 = int(rng.next() % uint32_t(ncorr)), r2 = int(rng.next() % uint32_t(ncorr));
    r[0] = r0; r[1] = r1; r[2] = r2;
}
MLH_FGR_HD_FORCE bool fgr_trial_accepts(const FgrPair *pairs, int ncorr, bool swapped, float scale, FgrRng &rng, int r[3])
{
    fgr_trial_draw(ncorr, rng, r);
    const int r0 = r[0], r1 = r[1], r2 = r[2];
    const FgrPair &c0 = pairs[size_t(r0)], &c1 = pairs[size_t(r1)], &c2 = pairs[size_t(r2)];
    const float *i0 = swapped ? c0.q : c0.p, *i1 = swapped ? c1.q : c1.p, *i2 = swapped ? c2.q : c2.p;
    const float *j0 = swapped ? c0.p : c0.q, *j1 = swapped ? c1.p : c1.q, *j2 = swapped ? c2.p : c2.q;
    const float li0 = fgr_dist3(i0, i1), li1 = fgr_dist3(i1, i2), li2 = fgr_dist3(i2, i0);
    const float lj0 = fgr_dist3(j0, j1), lj1 = fgr_dist3(j1, j2), lj2 = fgr_dist3(j2, j0);
    return (li0 * scale < lj0) && (lj0 < li0 / scale) && (li1 * scale < lj1) && (lj1 < li1 / scale) && (li2 * scale < lj2) && (lj2 < li2 / scale);
}

// app.cpp:242-307 on the cross-checked pairs. swapped: cloud 1 was `i` (the li side). corres <- 3 entries per accepted tuple (indices into pairs); returns the
// tuples accepted; *trials <- the trials run.
inline int fgr_tuple_test(const std::vector<FgrPair> &pairs, bool swapped, float tuple_scale, int tuple_max_cnt, uint64_t seed, std::vector<int32_t> &corres, int *trials)
{
    corres.clear();
    const int ncorr = int(pairs.size());
    const long long number_of_trial = (long long)ncorr * 100;
    FgrRng rng(seed);
    const float scale = tuple_scale;
    const FgrPair *const recs = pairs.data();     // (read once: the loop's stores into corres could alias the vector's own words)
    int cnt = 0;
    long long t = 0;
    for (t = 0; t < number_of_trial; ++t) {
        int r[3];
        if (fgr_trial_accepts(recs, ncorr, swapped, scale, rng, r)) {
            corres.push_back(r[0]); corres.push_back(r[1]); corres.push_back(r[2]);
            ++cnt;
        }
        if (cnt >= tuple_max_cnt) break;        // (the reference leaves the loop before the counter's increment: trials = t, as its printout had it)
    }
    if (trials) *trials = int(t);
    return cnt;
}

// ---- the same test as a plan of independent trials (fgr.hip: fgr_tuple_count_kernel / _scan_kernel / _emit_kernel; tests/host/fgr_tail_main.cpp replays it).
// Trial t uses draws 3 t .. 3 t + 2 whatever earlier trials decided, so the trials are cut into segments of FGR_TT_RUN x FGR_TT_TPB consecutive trials, one per
// workgroup, and every thread owns a run of FGR_TT_RUN consecutive trials of its segment: it jumps to draw 3 t_first (fgr_rng_at) and steps on from there. The
// accepted trials' ranks in trial order are: the segment's base (the exclusive prefix of the segments' counts) + the accepted trials of the segment's threads
// before this one + those of this thread's run before this trial. The result of the sequential loop above is the trials of rank < tuple_max_cnt.
constexpr int FGR_TT_RUN = 16, FGR_TT_TPB = 256;
constexpr long long FGR_TT_SEGMENT = (long long)FGR_TT_RUN * FGR_TT_TPB;
MLH_FGR_HD long long fgr_tt_total_trials(int ncorr) { return ncorr > 0 ? (long long)ncorr * 100 : 0; }
MLH_FGR_HD int fgr_tt_segments(int ncorr) { return int((fgr_tt_total_trials(ncorr) + FGR_TT_SEGMENT - 1) / FGR_TT_SEGMENT); }
// the run of `thread` of `segment`: [*begin, *end) (empty behind the last trial)
MLH_FGR_HD void fgr_tt_run(long long total_trials, int segment, int thread, long long *begin, long long *end)
{
    const long long b = (long long)segment * FGR_TT_SEGMENT + (long long)thread * FGR_TT_RUN;
    const long long e = b + FGR_TT_RUN;
    *begin = b < total_trials ? b : total_trials;
    *end = e < total_trials ? e : total_trials;
}
// bit i of the result: trial begin + i is accepted. Never draws -- and so never divides by ncorr -- when the run is empty.
MLH_FGR_HD uint32_t fgr_tt_run_mask(const uint64_t *table, const FgrPair *pairs, int ncorr, bool swapped, float scale, uint64_t seed, long long begin, long long end)
{
    static_assert(FGR_TT_RUN <= 32, "a run's accepted trials are one 32-bit mask");
    if (begin >= end) return 0u;
    FgrRng rng = fgr_rng_at(table, seed, uint64_t(begin) * 3ull);
    uint32_t mask = 0u;
    for (long long t = begin; t < end; ++t) {
        int r[3];
        if (fgr_trial_accepts(pairs, ncorr, swapped, scale, rng, r)) mask |= 1u << int(t - begin);
    }
    return mask;
}
// a segment recomputes its trials in the emit pass only when some of its accepted trials are kept
MLH_FGR_HD bool fgr_tt_segment_emits(int base, int count, int tuple_max_cnt) { return count > 0 && base < tuple_max_cnt; }
MLH_FGR_HD bool fgr_tt_rank_kept(int rank, int tuple_max_cnt) { return rank < tuple_max_cnt; }
// the trial that is written as n_trials by the emit pass: the one whose acceptance made the count reach the cap
MLH_FGR_HD bool fgr_tt_rank_is_last(int rank, int tuple_max_cnt) { return rank == tuple_max_cnt - 1; }
MLH_FGR_HD int fgr_tt_tuples(long long total_accepted, int tuple_max_cnt) { return total_accepted < (long long)tuple_max_cnt ? int(total_accepted) : tuple_max_cnt; }
// n_trials when the cap is never reached (0 for ncorr = 0); otherwise the emit pass's trial index stands
MLH_FGR_HD bool fgr_tt_cap_reached(long long total_accepted, int tuple_max_cnt) { return total_accepted >= (long long)tuple_max_cnt; }

struct FgrTail {
    float trans[16];                 // TransOutput_, row-major
    double final_cost, final_cost_normalize;
    bool optimised;                  // false: fewer than FGR_MIN_CORRES correspondences, nothing ran
};

// 4 x 4 f32 row-major product, sums left to right
MLH_FGR_HD void fgr_mat4_mul(const float A[16], const float B[16], float C[16])
{
    float t[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            t[r * 4 + c] = ((A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c]) + A[r * 4 + 3] * B[12 + c];
    for (int i = 0; i < 16; ++i) C[i] = t[i];
}

// -JTJ.llt().solve(JTr): CHOSEN a plain (unblocked, lower) Cholesky and two triangular solves
MLH_FGR_HD void fgr_llt_solve6(const double A[36], const double b[6], double x[6])
{
    double L[36] = {0};
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        const double ljj = std::sqrt(d);
        L[j * 6 + j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i * 6 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = s / ljj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k]; y[i] = s / L[i * 6 + i]; }
    for (int i = 5; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k]; x[i] = s / L[i * 6 + i]; }
}

// AngleAxisd(rz, Z) * AngleAxisd(ry, Y) * AngleAxisd(rx, X): Eigen multiplies angle-axes as quaternions, then toRotationMatrix()
MLH_FGR_HD void fgr_zyx_rotation(double rx, double ry, double rz, double R[9])
{
    const auto qmul = [](const double a[4], const double b[4], double o[4]) {      // (x, y, z, w)
        o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
        o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
        o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
        o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    };
    const double qz[4] = {0, 0, std::sin(0.5 * rz), std::cos(0.5 * rz)}, qy[4] = {0, std::sin(0.5 * ry), 0, std::cos(0.5 * ry)}, qx[4] = {std::sin(0.5 * rx), 0, 0, std::cos(0.5 * rx)};
    double qzy[4], q[4];
    qmul(qz, qy, qzy);
    qmul(qzy, qx, q);
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// ---- one iteration of OptimizePairwise, in the pieces fgr_optimize_pairwise below and fgr.hip's fgr_optimize_kernel share
// the sums of one iteration: the upper triangle of JTJ row by row ((0,0) (0,1) .. (5,5): 21), JTr (6), r2
constexpr int FGR_OPT_SUMS = 28, FGR_OPT_JTR = 21, FGR_OPT_R2 = 27;
MLH_FGR_HD constexpr int fgr_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }      // i <= j
// the device keeps the working copy of q in registers up to this many correspondences (FGR_OPT_QREG per thread of one workgroup of FGR_OPT_TPB) and in an HBM
// buffer beyond; the default tuple_max_cnt = 1000 gives 3000
constexpr int FGR_OPT_TPB = 256, FGR_OPT_QREG = 12;
constexpr int FGR_OPT_REG_MAX = 3072;
static_assert(FGR_OPT_REG_MAX == FGR_OPT_TPB * FGR_OPT_QREG, "the register-resident limit");

// the schedule of `par` in front of iteration itr (app.cpp:420-423)
MLH_FGR_HD double fgr_par_step(double par, int itr, double max_corr_dist, double div_factor)
{
    return (itr % 4 == 0 && par > max_corr_dist) ? par / div_factor : par;
}

// one correspondence's term of app.cpp:436-476 added to the sums: rpq = p - q, the line-process weight s = (par / (rpq . rpq + par))^2 (temp in f32), the three
// rows  J(1) = -q2, J(2) = q1, J(3) = -1 | J(2) = -q0, J(0) = q2, J(4) = -1 | J(0) = -q1, J(1) = q0, J(5) = -1  and the r2 contribution. Every sum receives its
// terms in the order the reference's loops give them (row by row); JTJ is symmetric to the bit (a product commutes), so its upper triangle is the whole of it.
MLH_FGR_HD void fgr_pairwise_accumulate(const float p[3], const float qq[3], double par, double acc[FGR_OPT_SUMS])
{
    const float rpq[3] = {p[0] - qq[0], p[1] - qq[1], p[2] - qq[2]};
    const float dot = (rpq[0] * rpq[0] + rpq[1] * rpq[1]) + rpq[2] * rpq[2];
    const float temp = float(par / (double(dot) + par));
    const double s = double(temp * temp);
    const int idx[3][3] = {{1, 2, 3}, {2, 0, 4}, {0, 1, 5}};
    const double val[3][3] = {{-double(qq[2]), double(qq[1]), -1.0}, {-double(qq[0]), double(qq[2]), -1.0}, {-double(qq[1]), double(qq[0]), -1.0}};
    for (int row = 0; row < 3; ++row) {
        const double r = double(rpq[row]);
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b)
                if (idx[row][a] <= idx[row][b]) acc[fgr_tri(idx[row][a], idx[row][b])] += (val[row][a] * val[row][b]) * s;
            acc[FGR_OPT_JTR + idx[row][a]] += (val[row][a] * r) * s;
        }
        acc[FGR_OPT_R2] += r * r * s;
    }
    acc[FGR_OPT_R2] += (par * (1.0 - std::sqrt(s)) * (1.0 - std::sqrt(s)));
}

// the sums -> delta (app.cpp:478-497): result = -JTJ.llt().solve(JTr), the Z Y X rotation, the f32 4 x 4
MLH_FGR_HD void fgr_pairwise_delta(const double acc[FGR_OPT_SUMS], float delta[16])
{
    double JTJ[36], JTr[6], x[6];
    for (int i = 0; i < 6; ++i) {
        for (int j = i; j < 6; ++j) JTJ[i * 6 + j] = JTJ[j * 6 + i] = acc[fgr_tri(i, j)];
        JTr[i] = acc[FGR_OPT_JTR + i];
    }
    fgr_llt_solve6(JTJ, JTr, x);
    for (int i = 0; i < 6; ++i) x[i] = -x[i];
    double R[9];
    fgr_zyx_rotation(x[0], x[1], x[2], R);
    const float d[16] = {float(R[0]), float(R[1]), float(R[2]), float(x[3]), float(R[3]), float(R[4]), float(R[5]), float(x[4]),
                         float(R[6]), float(R[7]), float(R[8]), float(x[5]), 0.f, 0.f, 0.f, 1.f};
    for (int i = 0; i < 16; ++i) delta[i] = d[i];
}

// TransformPoints on one point: temp = R * p + t
MLH_FGR_HD void fgr_transform_point(const float delta[16], float qq[3])
{
    const float a = qq[0], b = qq[1], d = qq[2];
    qq[0] = ((delta[0] * a + delta[1] * b) + delta[2] * d) + delta[3];
    qq[1] = ((delta[4] * a + delta[5] * b) + delta[6] * d) + delta[7];
    qq[2] = ((delta[8] * a + delta[9] * b) + delta[10] * d) + delta[11];
}

// OptimizePairwise(decrease_mu_ = true), app.cpp:392-505, over the correspondences corres[c] -> pairs[corres[c]] (p: pointcloud_[0], q: pcj_copy). Every
// correspondence keeps its own copy of q: TransformPoints moves every point of pcj_copy by the same delta, so copies of one point stay equal.
inline FgrTail fgr_optimize_pairwise(const std::vector<FgrPair> &pairs, const std::vector<int32_t> &corres, double start_scale, double div_factor, double max_corr_dist,
                                     int iteration_number)
{
    FgrTail out;
    for (int i = 0; i < 16; ++i) out.trans[i] = (i % 5 == 0) ? 1.f : 0.f;
    out.final_cost = out.final_cost_normalize = std::numeric_limits<double>::quiet_NaN();
    out.optimised = false;
    const size_t n = corres.size();
    if (n < size_t(FGR_MIN_CORRES)) return out;
    out.optimised = true;
    double par = start_scale;
    std::vector<float> q(3 * n);
    for (size_t c = 0; c < n; ++c) for (int d = 0; d < 3; ++d) q[3 * c + size_t(d)] = pairs[size_t(corres[c])].q[d];
    float trans[16];
    for (int i = 0; i < 16; ++i) trans[i] = out.trans[i];
    for (int itr = 0; itr < iteration_number; ++itr) {
        par = fgr_par_step(par, itr, max_corr_dist, div_factor);
        double acc[FGR_OPT_SUMS] = {0};
        for (size_t c = 0; c < n; ++c) fgr_pairwise_accumulate(pairs[size_t(corres[c])].p, &q[3 * c], par, acc);
        float delta[16];
        fgr_pairwise_delta(acc, delta);
        fgr_mat4_mul(delta, trans, trans);
        for (size_t c = 0; c < n; ++c) fgr_transform_point(delta, &q[3 * c]);
        out.final_cost = acc[FGR_OPT_R2];
        out.final_cost_normalize = acc[FGR_OPT_R2] / double(n);
    }
    for (int i = 0; i < 16; ++i) out.trans[i] = trans[i];      // TransOutput_ = trans * Identity
    return out;
}

// GetOutputTrans, app.cpp:519-534: R kept, t = -R * Means[1] + t * GlobalScale + Means[0], f32, then widened
inline void fgr_output_trans(const float trans[16], const float mean0[3], const float mean1[3], float global_scale, double T[16])
{
    float o[16] = {0};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = trans[r * 4 + c];
        const float rm = (-trans[r * 4] * mean1[0] + -trans[r * 4 + 1] * mean1[1]) + -trans[r * 4 + 2] * mean1[2];
        o[r * 4 + 3] = (rm + trans[r * 4 + 3] * global_scale) + mean0[r];
    }
    o[15] = 1.f;
    for (int i = 0; i < 16; ++i) T[i] = double(o[i]);
}

// the whole tail of mlh_fgr_register on the fetched pairs
inline void fgr_host_tail(const std::vector<FgrPair> &pairs, bool swapped, const float mean0[3], const float mean1[3], float global_scale, float start_scale,
                          const mlh_fgr_opts &o, mlh_fgr_result &res)
{
    std::vector<int32_t> corres;
    int trials = 0;
    const int tuples = fgr_tuple_test(pairs, swapped, o.tuple_scale, o.tuple_max_cnt, o.seed, corres, &trials);
    const FgrTail t = fgr_optimize_pairwise(pairs, corres, double(start_scale), o.div_factor, o.max_corr_dist, o.iteration_number);
    fgr_output_trans(t.trans, mean0, mean1, global_scale, res.T_relative);
    res.final_cost = t.final_cost;
    res.final_cost_normalize = t.final_cost_normalize;
    res.accepted = (t.optimised && t.final_cost_normalize <= o.global_registration_threshold) ? 1 : 0;
    res.swapped = swapped ? 1 : 0;
    res.n_mutual = int32_t(pairs.size()); res.n_tuples = tuples; res.n_corres = int32_t(corres.size()); res.n_trials = trials;
    res.global_scale = double(global_scale); res.start_scale = double(start_scale);
    for (int d = 0; d < 3; ++d) { res.means[d] = double(mean0[d]); res.means[3 + d] = double(mean1[d]); }
}

}  // namespace mlh
