// A stand-alone CPU restatement of LoopRegistration::performGlobalRegistration (mloam_loop/src/loop_registration.cpp:18-101: pcl::NormalEstimation,
// pcl::FPFHEstimationOMP, fgr::CApp) for the tests of section (f13), as loopreg_ref.cpp is for (f12). Plain g++, called through ctypes (tests/fgr_cases.py).
// The per-pair, per-bin, eigen33 and distance arithmetic and the tail (tuple test, OptimizePairwise, GetOutputTrans) come from m-loam_amd/csrc/fgr_host.hpp, the
// one place they exist (what that header restates from memory of PCL 1.8.0 / FLANN is listed there). What is written HERE is the part the device does differently:
//   the radius search is brute force; the neighbours of a point are visited in ascending (squared distance, index) order, the order PCL's sorted search results
//   have, and every f32 sum runs in that order; NormalizePoints sums the points sequentially as app.cpp:340-345 does; the nearest-row search is a plain loop.
// Every stage accepts the previous stage's output from outside (normals, SPFH counts, features), so that a stage can be compared on exactly known inputs.
// Flags, all computed in f64: per point the number of FRAGILE pair features -- a feature within 1e-5 (in [0, 1] bin-range units) of an interior bin edge, or all
// three of a pair whose swap decision | |angle1| - |angle2| | is below 2e-6 without being exactly 0 (acosf near pi / 2 resolves 1.2e-7: two libms can order two
// cosines that close differently) --; per normal whether |cos| of the flip test is below 1e-5 |p| and whether the relative
// eigen-gap (l1 - l0) / trace is below 1e-3.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "fgr_host.hpp"

using namespace mlh;

namespace {

struct Nbr { float d2; int idx; };

// neighbours of point i with d2 < r * r, ascending (d2, index)
std::vector<Nbr> neighbours(const float *pts4, int n, int i, float radius)
{
    const float r2 = radius * radius;
    std::vector<Nbr> out;
    for (int j = 0; j < n; ++j) {
        const float d2 = fgr_sqdist3(pts4[4 * i], pts4[4 * i + 1], pts4[4 * i + 2], pts4[4 * j], pts4[4 * j + 1], pts4[4 * j + 2]);
        if (d2 < r2) out.push_back(Nbr{d2, j});
    }
    std::sort(out.begin(), out.end(), [](const Nbr &a, const Nbr &b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.idx < b.idx); });
    return out;
}

template <typename T> void normal_of(const float *pts4, const std::vector<Nbr> &nb, int i, T out[4], T evals[3], T *cos_flip)
{
    T a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (const Nbr &q : nb) {
        const T x = T(pts4[4 * q.idx]), y = T(pts4[4 * q.idx + 1]), z = T(pts4[4 * q.idx + 2]);
        a[0] += x * x; a[1] += x * y; a[2] += x * z; a[3] += y * y; a[4] += y * z; a[5] += z * z; a[6] += x; a[7] += y; a[8] += z;
    }
    const T p[3] = {T(pts4[4 * i]), T(pts4[4 * i + 1]), T(pts4[4 * i + 2])};
    fgr_normal_from_sums<T>(a, int(nb.size()), p, out, evals, cos_flip);
}

double edge_distance(double u)
{
    double best = 1.0;
    for (int k = 1; k < FGR_BINS; ++k) best = std::min(best, std::fabs(u - double(k) / FGR_BINS));
    return best;
}

void features_of(const float *pts4, int n, float normal_radius, float fpfh_radius, const float *normals_in, const int32_t *counts_in, const int32_t *k_in, const float *feat_in,
                 std::vector<float> &feat);

}  // namespace

extern "C" {

// normals4 [n x 4] f32; normals64 [n x 4] the same code in f64 over the same neighbour sets (may be null); flag_flip / flag_gap [n]; k [n] (each may be null)
void fr_normals(const float *pts4, int n, float radius, float *normals4, double *normals64, uint8_t *flag_flip, uint8_t *flag_gap, int32_t *k)
{
    for (int i = 0; i < n; ++i) {
        const std::vector<Nbr> nb = neighbours(pts4, n, i, radius);
        float o[4], ev[3], cf;
        normal_of<float>(pts4, nb, i, o, ev, &cf);
        std::memcpy(normals4 + 4 * i, o, sizeof(o));
        double od[4], evd[3], cfd;
        normal_of<double>(pts4, nb, i, od, evd, &cfd);
        if (normals64) std::memcpy(normals64 + 4 * i, od, sizeof(od));
        const double pn = std::sqrt(double(pts4[4 * i]) * pts4[4 * i] + double(pts4[4 * i + 1]) * pts4[4 * i + 1] + double(pts4[4 * i + 2]) * pts4[4 * i + 2]);
        const double trace = evd[0] + evd[1] + evd[2];
        if (flag_flip) flag_flip[i] = (nb.size() >= 3 && std::fabs(cfd) < 1e-5 * pn) ? 1 : 0;
        if (flag_gap) flag_gap[i] = (nb.size() >= 3 && !((evd[1] - evd[0]) / trace >= 1e-3)) ? 1 : 0;
        if (k) k[i] = int32_t(nb.size());
    }
}

// counts [n x 33], k [n], fragile [n] (the number of fragile pair features of the point; may be null)
void fr_spfh(const float *pts4, int n, const float *normals4, float radius, int32_t *counts, int32_t *k, int32_t *fragile)
{
    for (int i = 0; i < n; ++i) {
        const std::vector<Nbr> nb = neighbours(pts4, n, i, radius);
        int32_t *h = counts + size_t(i) * FGR_DIM;
        std::fill(h, h + FGR_DIM, 0);
        int frag = 0;
        const float p1[3] = {pts4[4 * i], pts4[4 * i + 1], pts4[4 * i + 2]}, n1[3] = {normals4[4 * i], normals4[4 * i + 1], normals4[4 * i + 2]};
        const double p1d[3] = {p1[0], p1[1], p1[2]}, n1d[3] = {n1[0], n1[1], n1[2]};
        for (const Nbr &q : nb) {
            if (q.idx == i) continue;
            const float p2[3] = {pts4[4 * q.idx], pts4[4 * q.idx + 1], pts4[4 * q.idx + 2]}, n2[3] = {normals4[4 * q.idx], normals4[4 * q.idx + 1], normals4[4 * q.idx + 2]};
            float f1, f2, f3;
            if (!fgr_pair_features<float>(p1, n1, p2, n2, f1, f2, f3)) continue;
            ++h[fgr_bin(fgr_unit_f1(f1))];
            ++h[FGR_BINS + fgr_bin(fgr_unit_f23(f2))];
            ++h[2 * FGR_BINS + fgr_bin(fgr_unit_f23(f3))];
            const double p2d[3] = {p2[0], p2[1], p2[2]}, n2d[3] = {n2[0], n2[1], n2[2]};
            double g1, g2, g3, a1 = 0, a2 = 0;
            if (!fgr_pair_features<double>(p1d, n1d, p2d, n2d, g1, g2, g3, &a1, &a2)) { frag += 3; continue; }
            if (std::isnan(g1) || std::isnan(g2) || std::isnan(g3)) continue;
            const double tie = std::fabs(std::fabs(a1) - std::fabs(a2));          // (exactly 0: equal or opposite normals, the same bits in f32 -- no decision to flip)
            if (tie != 0.0 && tie < 2e-6) { frag += 3; continue; }
            frag += edge_distance((g1 + 3.14159265358979323846) / (2.0 * 3.14159265358979323846)) < 1e-5 ? 1 : 0;
            frag += edge_distance((g2 + 1.0) * 0.5) < 1e-5 ? 1 : 0;
            frag += edge_distance((g3 + 1.0) * 0.5) < 1e-5 ? 1 : 0;
        }
        k[i] = int32_t(nb.size());
        if (fragile) fragile[i] = frag;
    }
}

void fr_fpfh(const float *pts4, int n, const int32_t *counts, const int32_t *k, float radius, float *feat)
{
    std::vector<float> val(size_t(n) * FGR_DIM);
    for (int i = 0; i < n; ++i) for (int b = 0; b < FGR_DIM; ++b) val[size_t(i) * FGR_DIM + b] = fgr_spfh_value(counts[size_t(i) * FGR_DIM + b], k[i]);
    for (int i = 0; i < n; ++i) {
        const std::vector<Nbr> nb = neighbours(pts4, n, i, radius);
        float *h = feat + size_t(i) * FGR_DIM, sum[3] = {0.f, 0.f, 0.f};
        std::fill(h, h + FGR_DIM, 0.f);
        for (const Nbr &q : nb) {
            if (q.d2 == 0.f) continue;
            const float w = 1.0f / q.d2;
            for (int blk = 0; blk < 3; ++blk)
                for (int b = 0; b < FGR_BINS; ++b) {
                    const float v = val[size_t(q.idx) * FGR_DIM + blk * FGR_BINS + b] * w;
                    sum[blk] += v;
                    h[blk * FGR_BINS + b] += v;
                }
        }
        for (int blk = 0; blk < 3; ++blk) { const float s = fgr_block_scale(sum[blk]); for (int b = 0; b < FGR_BINS; ++b) h[blk * FGR_BINS + b] *= s; }
    }
}

static int nearest_row(const float *q, const float *D, int nd)
{
    if (!fgr_row_finite(q)) return -1;
    int best = -1;
    float best_d = 0.f;
    for (int r = 0; r < nd; ++r) {
        if (!fgr_row_finite(D + size_t(r) * FGR_DIM)) continue;
        const float d = fgr_l2_33(q, D + size_t(r) * FGR_DIM);
        if (best < 0 || d < best_d) { best = r; best_d = d; }
    }
    return best;
}

// AdvancedMatching up to the cross check, as app.cpp:113-235 walks it (the i_to_j cache, corres_ij / corres_ji, Mi / Mj), then the un-swap of app.cpp:309-316.
// pairs [2 x min(n0, n1)]: (cloud 0 index, cloud 1 index); returns their number; *swapped_out <- cloud 1 was i.
int fr_match(const float *f0, int n0, const float *f1, int n1, int32_t *pairs, int32_t *swapped_out)
{
    const bool swapped = n1 > n0;
    const float *Fi = swapped ? f1 : f0, *Fj = swapped ? f0 : f1;
    const int nPti = swapped ? n1 : n0, nPtj = swapped ? n0 : n1;
    if (swapped_out) *swapped_out = swapped ? 1 : 0;
    const size_t sz_i = size_t(nPti), sz_j = size_t(nPtj);
    std::vector<int> i_to_j(sz_i, -1);
    std::vector<std::pair<int, int>> corres_ij, corres_ji;
    for (int j = 0; j < nPtj; ++j) {
        const int i = nearest_row(Fj + size_t(j) * FGR_DIM, Fi, nPti);
        if (i < 0) continue;                                   // CHOSEN: a non-finite row matches nothing
        if (i_to_j[size_t(i)] == -1) i_to_j[size_t(i)] = nearest_row(Fi + size_t(i) * FGR_DIM, Fj, nPtj);
        corres_ji.push_back(std::make_pair(i, j));
    }
    for (int i = 0; i < nPti; ++i) if (i_to_j[size_t(i)] != -1) corres_ij.push_back(std::make_pair(i, i_to_j[size_t(i)]));
    std::vector<std::vector<int>> Mi(sz_i), Mj(sz_j);
    for (const auto &c : corres_ij) Mi[size_t(c.first)].push_back(c.second);
    for (const auto &c : corres_ji) Mj[size_t(c.second)].push_back(c.first);
    int cnt = 0;
    for (int i = 0; i < nPti; ++i)
        for (int j : Mi[size_t(i)])
            for (int ii : Mj[size_t(j)])
                if (ii == i) { pairs[2 * cnt] = swapped ? j : i; pairs[2 * cnt + 1] = swapped ? i : j; ++cnt; }
    return cnt;
}

// NormalizePoints, app.cpp:324-390: np0 [n0 x 3], np1 [n1 x 3], means [6], scales [2] = {GlobalScale, StartScale}
void fr_normalize(const float *p0, int n0, const float *p1, int n1, int use_absolute_scale, float *np0, float *np1, float *means, float *scales)
{
    float scale = 0.f;
    for (int c = 0; c < 2; ++c) {
        const float *p = c ? p1 : p0;
        float *o = c ? np1 : np0;
        const int n = c ? n1 : n0;
        float m[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) m[d] = m[d] + p[4 * i + d];
        for (int d = 0; d < 3; ++d) m[d] = n > 0 ? m[d] / float(n) : 0.f;
        float max_scale = 0.f;
        for (int i = 0; i < n; ++i) {
            for (int d = 0; d < 3; ++d) o[3 * i + d] = p[4 * i + d] - m[d];
            const float t = std::sqrt((o[3 * i] * o[3 * i] + o[3 * i + 1] * o[3 * i + 1]) + o[3 * i + 2] * o[3 * i + 2]);
            if (t > max_scale) max_scale = t;
        }
        if (max_scale > scale) scale = max_scale;
        for (int d = 0; d < 3; ++d) means[3 * c + d] = m[d];
    }
    scales[0] = use_absolute_scale ? 1.0f : scale;
    scales[1] = use_absolute_scale ? scale : 1.0f;
    for (int i = 0; i < 3 * n0; ++i) np0[i] /= scales[0];
    for (int i = 0; i < 3 * n1; ++i) np1[i] /= scales[0];
}

// the tail on given pairs (cloud 0 index, cloud 1 index) of the two RAW clouds: NormalizePoints here, then fgr_host.hpp's tuple test, OptimizePairwise, GetOutputTrans
void fr_tail(const float *p0, int n0, const float *p1, int n1, const int32_t *pairs, int n_pairs, int swapped, const mlh_fgr_opts *o, mlh_fgr_result *res)
{
    std::vector<float> np0(size_t(3 * n0) + 1), np1(size_t(3 * n1) + 1);
    float means[6], scales[2];
    fr_normalize(p0, n0, p1, n1, o->use_absolute_scale, np0.data(), np1.data(), means, scales);
    std::vector<FgrPair> recs(static_cast<size_t>(n_pairs));
    for (int e = 0; e < n_pairs; ++e) {
        FgrPair &r = recs[size_t(e)];
        r.i = pairs[2 * e]; r.j = pairs[2 * e + 1];
        for (int d = 0; d < 3; ++d) { r.p[d] = np0[size_t(3 * r.i + d)]; r.q[d] = np1[size_t(3 * r.j + d)]; }
    }
    std::memset(res, 0, sizeof(*res));
    fgr_host_tail(recs, swapped != 0, means, means + 3, scales[0], scales[1], *o, *res);
}

// performGlobalRegistration end to end. Optional overrides per cloud c (null: computed): normals_in[c] [n x 4]; counts_in[c] [n x 33] with k_in[c] [n];
// feat_in[c] [n x 33]. pairs_out [2 x min(n0, n1)] (may be null), *n_pairs_out.
void fr_register(const float *p0, int n0, const float *p1, int n1, const mlh_fgr_opts *o, const float *const *normals_in, const int32_t *const *counts_in,
                 const int32_t *const *k_in, const float *const *feat_in, mlh_fgr_result *res, int32_t *pairs_out, int32_t *n_pairs_out)
{
    std::vector<float> f[2];
    for (int c = 0; c < 2; ++c)
        features_of(c ? p1 : p0, c ? n1 : n0, o->normal_radius, o->fpfh_radius, normals_in ? normals_in[c] : nullptr, counts_in ? counts_in[c] : nullptr,
                    k_in ? k_in[c] : nullptr, feat_in ? feat_in[c] : nullptr, f[c]);
    std::vector<int32_t> pairs(size_t(2 * std::min(n0, n1)) + 2);
    int32_t swapped = 0;
    const int cnt = fr_match(f[0].data(), n0, f[1].data(), n1, pairs.data(), &swapped);
    fr_tail(p0, n0, p1, n1, pairs.data(), cnt, swapped, o, res);
    if (pairs_out) std::memcpy(pairs_out, pairs.data(), sizeof(int32_t) * 2 * size_t(cnt));
    if (n_pairs_out) *n_pairs_out = cnt;
}

// ---- the shared header's pieces, one at a time (tests/test_fgr_cases.py)
int fr_pair_features(const float *p1, const float *n1, const float *p2, const float *n2, float *f3_out)
{
    float f1, f2, f3;
    const bool ok = fgr_pair_features<float>(p1, n1, p2, n2, f1, f2, f3);
    f3_out[0] = f1; f3_out[1] = f2; f3_out[2] = f3;
    return ok ? 1 : 0;
}
void fr_bins(const float *f, int32_t *bins) { bins[0] = fgr_bin(fgr_unit_f1(f[0])); bins[1] = fgr_bin(fgr_unit_f23(f[1])); bins[2] = fgr_bin(fgr_unit_f23(f[2])); }
float fr_spfh_value(int count, int k) { return fgr_spfh_value(count, k); }
float fr_l2(const float *a, const float *b) { return fgr_l2_33(a, b); }
int fr_opts_fault(const mlh_fgr_opts *o) { return fgr_opts_fault(*o) ? 1 : 0; }
void fr_opts_default(mlh_fgr_opts *o) { fgr_opts_defaults(*o); }
// the tuple test on pairs given as records of normalised points [n x 6] (p, q): corres [3 x tuple_max_cnt] <- indices into the pairs; returns the tuples; *trials
int fr_tuple_test(const float *pq, int n, int swapped, float tuple_scale, int tuple_max_cnt, uint64_t seed, int32_t *corres, int32_t *trials)
{
    std::vector<FgrPair> recs(static_cast<size_t>(n));
    for (int e = 0; e < n; ++e) { recs[size_t(e)].i = recs[size_t(e)].j = e; for (int d = 0; d < 3; ++d) { recs[size_t(e)].p[d] = pq[6 * e + d]; recs[size_t(e)].q[d] = pq[6 * e + 3 + d]; } }
    std::vector<int32_t> c;
    int t = 0;
    const int cnt = fgr_tuple_test(recs, swapped != 0, tuple_scale, tuple_max_cnt, seed, c, &t);
    std::copy(c.begin(), c.end(), corres);
    *trials = t;
    return cnt;
}
uint32_t fr_rng_draw(uint64_t seed, int skip) { FgrRng r(seed); uint32_t v = 0; for (int i = 0; i <= skip; ++i) v = r.next(); return v; }
// OptimizePairwise on n correspondences (p, q) [n x 6]: trans [16] f32 row-major, cost [2] = {final_cost, final_cost_normalize}; returns 1 when it ran
int fr_optimize(const float *pq, int n, double start_scale, double div_factor, double max_corr_dist, int iteration_number, float *trans, double *cost)
{
    std::vector<FgrPair> recs(static_cast<size_t>(n));
    std::vector<int32_t> c(static_cast<size_t>(n));
    for (int e = 0; e < n; ++e) { c[size_t(e)] = e; recs[size_t(e)].i = recs[size_t(e)].j = e; for (int d = 0; d < 3; ++d) { recs[size_t(e)].p[d] = pq[6 * e + d]; recs[size_t(e)].q[d] = pq[6 * e + 3 + d]; } }
    const FgrTail t = fgr_optimize_pairwise(recs, c, start_scale, div_factor, max_corr_dist, iteration_number);
    std::memcpy(trans, t.trans, sizeof(t.trans));
    cost[0] = t.final_cost; cost[1] = t.final_cost_normalize;
    return t.optimised ? 1 : 0;
}

}  // extern "C"

namespace {

void features_of(const float *pts4, int n, float normal_radius, float fpfh_radius, const float *normals_in, const int32_t *counts_in, const int32_t *k_in, const float *feat_in,
                 std::vector<float> &feat)
{
    feat.assign(size_t(n) * FGR_DIM + 1, 0.f);
    if (feat_in) { std::copy(feat_in, feat_in + size_t(n) * FGR_DIM, feat.begin()); return; }
    std::vector<int32_t> counts(size_t(n) * FGR_DIM + 1), k(size_t(n) + 1);
    if (counts_in) { std::copy(counts_in, counts_in + size_t(n) * FGR_DIM, counts.begin()); std::copy(k_in, k_in + n, k.begin()); }
    else {
        std::vector<float> normals(size_t(n) * 4 + 1);
        if (normals_in) std::copy(normals_in, normals_in + size_t(n) * 4, normals.begin());
        else fr_normals(pts4, n, normal_radius, normals.data(), nullptr, nullptr, nullptr, nullptr);
        fr_spfh(pts4, n, normals.data(), fpfh_radius, counts.data(), k.data(), nullptr);
    }
    fr_fpfh(pts4, n, counts.data(), k.data(), fpfh_radius, feat.data());
}

}  // namespace
