// The online-calibration branch of Estimator::optimizeMap through the facade (addCalibFeatures, useCalibFactors, solveWindow with extra_const_mask,
// marginalizeWindow, clearCalibFactors, calibFactorInfo) against the plain C-ABI calls (mlh_calib_add, mlh_calib_use, mlh_pure_odom_gn_solve,
// mlh_window_marginalize, mlh_calib_clear, mlh_calib_info) on a second context: four consecutive windows, once with one frame and three LiDARs and once with
// three frames and two LiDARs. The reference LiDAR's features are window factors; the other LiDARs' pivot-frame features accumulate in the calibration store every window and enter the solve and the
// marginalisation on every 2nd one, after which the store is cleared (estimator.cpp:687-785, 852-861, 871-1063). The poses of every window and the prior's bits
// must be equal. The device route into the store -- WindowFactorTable::accumulateStagedMatches against mlh_calib_accumulate, a match pass on a small ground
// plane -- must leave equal stores and equal normal equations.
// Usage: calib_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

constexpr int N_WINDOWS = 4, N_WINDOW_FACTORS = 60, N_CALIB[3] = {0, 150, 97};
using P7 = std::array<double, 7>;

Pose to_pose(const P7 &p)
{
    Pose o;
    o.t_(0) = p[0]; o.t_(1) = p[1]; o.t_(2) = p[2];
    o.q_.x = p[3]; o.q_.y = p[4]; o.q_.z = p[5]; o.q_.w = p[6];
    return o;
}

P7 yaw_pose(double x, double y, double z, double yaw, double roll)
{
    const double cz = std::cos(yaw / 2), sz = std::sin(yaw / 2), cx = std::cos(roll / 2), sx = std::sin(roll / 2);
    return P7{x, y, z, cz * sx, sz * sx, sz * cx, cz * cx};
}

// n features of one LiDAR: a point in the LiDAR frame, moved with the TRUE transform T, and a plane through / a line near the moved point
std::vector<PointPlaneFeature> make_features(std::mt19937 &rng, const Pose &T, int n)
{
    std::uniform_real_distribution<double> u(-15.0, 15.0);
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<PointPlaneFeature> out;
    for (int k = 0; k < n; ++k) {
        const double p[3] = {u(rng), u(rng), u(rng)};
        double x[3];
        detail::quat_rotate(T.q_, p, x);
        for (int c = 0; c < 3; ++c) x[c] += T.t_(c) + 0.01 * g(rng);
        double v[3] = {g(rng), g(rng), g(rng)};
        const double vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int c = 0; c < 3; ++c) v[c] /= vn;
        PointPlaneFeature f;
        f.point_ = {p[0], p[1], p[2]};
        if (k % 2 == 0) { f.type_ = 's'; f.coeffs_ = {v[0], v[1], v[2], -(v[0] * x[0] + v[1] * x[1] + v[2] * x[2])}; }
        else { f.type_ = 'c'; f.coeffs_ = {x[0] + 0.1 * v[0], x[1] + 0.1 * v[1], x[2] + 0.1 * v[2], x[0] - 0.1 * v[0], x[1] - 0.1 * v[1], x[2] - 0.1 * v[2]}; }
        out.push_back(f);
    }
    return out;
}

struct Flat { std::vector<int32_t> type, fi, ei; std::vector<double> points, coeffs; };
void flatten(const std::vector<PointPlaneFeature> &fs, int frame, int laser, Flat &t)
{
    for (const PointPlaneFeature &f : fs) {
        t.type.push_back(f.type_ == 's' ? 0 : 1); t.fi.push_back(frame); t.ei.push_back(laser);
        for (int c = 0; c < 3; ++c) t.points.push_back(f.point_[size_t(c)]);
        for (int c = 0; c < 6; ++c) t.coeffs.push_back(c < (int)f.coeffs_.size() ? f.coeffs_[size_t(c)] : 0.0);
    }
}

struct PriorBits { mlh_window_prior_info info; std::vector<int32_t> ids; std::vector<double> x0, J0, r0; };
PriorBits read_prior(Device &dev)
{
    PriorBits b;
    dev.check(mlh_window_prior_get(dev.ctx(), &b.info, nullptr, nullptr, nullptr, nullptr));
    if (!b.info.valid) return b;
    const size_t n = size_t(b.info.n);
    b.ids.resize(size_t(b.info.n_keep)); b.x0.resize(7 * size_t(b.info.n_keep)); b.J0.resize(n * n); b.r0.resize(n);
    dev.check(mlh_window_prior_get(dev.ctx(), nullptr, b.ids.data(), b.x0.data(), b.J0.data(), b.r0.data()));
    return b;
}

template <class T> bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0); }

// the chain of four windows with n_frames frames and n_ext LiDARs; false (after printing why) when the two routes differ
bool run_chain(int n_frames, int n_ext)
{
    Device facade_dev(0), abi_dev(0);
    std::mt19937 rng(2025u + unsigned(10 * n_frames + n_ext));
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<P7> traj;
    for (int k = 0; k <= N_WINDOWS + n_frames; ++k) traj.push_back(yaw_pose(0.4 * k, 0.05 * std::sin(0.7 * k), 0.01 * k, 0.02 * k, 0.003 * k));
    std::vector<P7> exts_true = {P7{0, 0, 0, 0, 0, 0, 1}, yaw_pose(0.1, -0.45, 0.02, 0.2, 0.01), yaw_pose(-0.2, 0.4, 0.05, -0.3, 0.02)};
    exts_true.resize(size_t(n_ext));
    auto perturbed = [&](const P7 &p) {
        P7 o = p;
        for (int c = 0; c < 3; ++c) o[size_t(c)] += 0.02 * g(rng);
        const Pose d = poseMul(to_pose(p), to_pose(yaw_pose(0, 0, 0, 0.004 * g(rng), 0.003 * g(rng))));
        o[3] = d.q_.x; o[4] = d.q_.y; o[5] = d.q_.z; o[6] = d.q_.w;
        return o;
    };
    // the PriorFactor of every extrinsic, in the marginalisation only
    std::vector<std::array<double, 3>> tbl;
    std::vector<std::array<double, 4>> qbl;
    std::vector<double> rows;
    for (const P7 &e : exts_true) {
        tbl.push_back({e[0], e[1], e[2]}); qbl.push_back({e[3], e[4], e[5], e[6]});
        for (int c = 0; c < 7; ++c) rows.push_back(e[size_t(c)]);
        rows.push_back(5.0); rows.push_back(10.0);
    }
    setExtrinsicPrior(facade_dev, tbl, qbl, 5.0, 10.0, false);
    abi_dev.check(mlh_window_ext_prior_set(abi_dev.ctx(), n_ext, rows.data(), 1u));

    P7 pivot_f = traj[0], pivot_a = traj[0];
    std::vector<P7> exts_f = {exts_true[0]};
    for (int n = 1; n < n_ext; ++n) exts_f.push_back(perturbed(exts_true[size_t(n)]));
    std::vector<P7> exts_a = exts_f, frames_f, frames_a;
    for (int i = 1; i <= n_frames; ++i) frames_f.push_back(perturbed(traj[size_t(i)]));
    frames_a = frames_f;
    uint32_t other_exts = 0;                                    // blocks [pivot | frames | extrinsics]
    int n_calib = 0;
    for (int n = 1; n < n_ext; ++n) { other_exts |= 1u << (1 + n_frames + n); n_calib += N_CALIB[n]; }
    const uint32_t ref_mask = 1u | (1u << (1 + n_frames));
    int calibrated = 0;
    for (int k = 0; k < N_WINDOWS; ++k) {
        const bool use = k % 2 == 1;                            // the frame_cnt % N_CUMU_FEATURE == 0 gate
        if (k > 0) {
            const P7 fresh = perturbed(traj[size_t(k + n_frames)]);
            frames_f.erase(frames_f.begin()); frames_f.push_back(fresh);
            frames_a.erase(frames_a.begin()); frames_a.push_back(fresh);
        }
        Flat win;
        for (int i = 0; i < n_frames; ++i) {
            const Pose T0 = poseMul(poseMul(poseInverse(to_pose(traj[size_t(k)])), to_pose(traj[size_t(k + 1 + i)])), to_pose(exts_true[0]));
            flatten(make_features(rng, T0, N_WINDOW_FACTORS), i, 0, win);
        }
        std::vector<std::vector<PointPlaneFeature>> cal{size_t(n_ext)};
        for (int n = 1; n < n_ext; ++n) cal[size_t(n)] = make_features(rng, to_pose(exts_true[size_t(n)]), N_CALIB[n]);
        const std::vector<P7> exts_before = exts_f;
        // the facade
        facade_dev.check(mlh_pure_odom_set(facade_dev.ctx(), (int)win.type.size(), win.type.data(), win.points.data(), win.coeffs.data(), nullptr, win.fi.data(), win.ei.data()));
        for (int n = 1; n < n_ext; ++n) addCalibFeatures(facade_dev, cal[size_t(n)], n);
        useCalibFactors(facade_dev, use);
        if (solveWindow(facade_dev, pivot_f.data(), frames_f, exts_f, 1.0, 5, nullptr, 0, nullptr, use ? 0u : other_exts) != 0) { std::printf("FAIL: window %d not solved (facade)\n", k); return false; }
        const mlh_window_prior_info info_f = marginalizeWindow(facade_dev, pivot_f.data(), frames_f, exts_f, 1.0);
        const mlh_calib_store_info ci_f = calibFactorInfo(facade_dev);
        if (use) clearCalibFactors(facade_dev);
        // the plain calls
        abi_dev.check(mlh_pure_odom_set(abi_dev.ctx(), (int)win.type.size(), win.type.data(), win.points.data(), win.coeffs.data(), nullptr, win.fi.data(), win.ei.data()));
        for (int n = 1; n < n_ext; ++n) {
            Flat c;
            flatten(cal[size_t(n)], 0, n, c);
            abi_dev.check(mlh_calib_add(abi_dev.ctx(), (int)c.type.size(), c.type.data(), c.points.data(), c.coeffs.data(), nullptr, c.ei.data()));
        }
        abi_dev.check(mlh_calib_use(abi_dev.ctx(), use ? 1 : 0));
        int32_t n_res = 0, status = 0;
        double cost = 0.0;
        abi_dev.check(mlh_pure_odom_gn_solve(abi_dev.ctx(), pivot_a.data(), frames_a[0].data(), n_frames, exts_a[0].data(), n_ext, 1.0, 5, ref_mask | (use ? 0u : other_exts), nullptr,
                                             &cost, &n_res, &status));
        mlh_window_prior_info info_a;
        abi_dev.check(mlh_window_marginalize(abi_dev.ctx(), pivot_a.data(), frames_a[0].data(), n_frames, exts_a[0].data(), n_ext, 1.0, &info_a));
        mlh_calib_store_info ci_a;
        abi_dev.check(mlh_calib_info(abi_dev.ctx(), &ci_a));
        if (use) abi_dev.check(mlh_calib_clear(abi_dev.ctx()));
        const int expect_res = n_frames * N_WINDOW_FACTORS + (use ? 2 * n_calib : 0);       // a calibration window holds two windows' accumulation
        if (status != 0 || n_res != expect_res) { std::printf("FAIL: window %d: status %d, %d residuals (expected %d)\n", k, status, n_res, expect_res); return false; }
        if (std::memcmp(&ci_f, &ci_a, sizeof(ci_f)) != 0 || ci_f.in_use != (use ? 1 : 0) || ci_f.n_valid <= 0) { std::printf("FAIL: window %d: the two stores differ\n", k); return false; }
        if (!same(frames_f, frames_a) || !same(exts_f, exts_a)) { std::printf("FAIL: window %d: the two paths' poses differ\n", k); return false; }
        const PriorBits pf = read_prior(facade_dev), pa = read_prior(abi_dev);
        if (!pf.info.valid || !pa.info.valid || pf.info.n_keep != n_frames + n_ext || info_f.kept_rr != info_a.kept_rr || info_f.kept_mm != info_a.kept_mm ||
            !same(pf.ids, pa.ids) || !same(pf.x0, pa.x0) || !same(pf.J0, pa.J0) || !same(pf.r0, pa.r0)) {
            std::printf("FAIL: window %d: the two paths' priors differ\n", k);
            return false;
        }
        // the other extrinsics move on calibration windows and only there
        bool moved = false;
        for (int n = 1; n < n_ext; ++n) moved = moved || std::memcmp(exts_f[size_t(n)].data(), exts_before[size_t(n)].data(), sizeof(P7)) != 0;
        if (moved != use) { std::printf("FAIL: window %d: extrinsics %s\n", k, moved ? "moved without calibration factors" : "did not move"); return false; }
        calibrated += use;
        pivot_f = frames_f[0]; pivot_a = frames_a[0];
    }
    if (calibFactorInfo(facade_dev).n_valid != 0 || calibFactorInfo(facade_dev).in_use != 0) { std::printf("FAIL: clearCalibFactors left a store\n"); return false; }
    if (calibrated != N_WINDOWS / 2) { std::printf("FAIL: calibration windows\n"); return false; }
    return true;
}

// the device route into the store: a ground plane 1.5 m below the LiDAR as the calibration map, surf features on it staged on the device, one match pass each
bool run_accumulate()
{
    Device facade_dev(0), abi_dev(0);
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> u(-6.0, 6.0);
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<float> map, feats;
    for (int i = -32; i <= 32; ++i)
        for (int j = -32; j <= 32; ++j) { map.push_back(0.25f * i); map.push_back(0.25f * j); map.push_back(float(-1.5 + 0.001 * g(rng))); map.push_back(0.f); }
    while (feats.size() < 4 * 300) {
        const double x = u(rng), y = u(rng);
        if (x * x + y * y < 4.0) continue;                      // (inside the 30 degree cone around the LiDAR's axis the FOV check drops a feature)
        feats.push_back(float(x)); feats.push_back(float(y)); feats.push_back(float(-1.5 + 0.01 * g(rng))); feats.push_back(1.f);
    }
    const P7 ext1 = yaw_pose(0.01, -0.02, 0.005, 0.004, 0.002);
    const std::vector<P7> exts = {P7{0, 0, 0, 0, 0, 0, 1}, ext1};
    const P7 ident{0, 0, 0, 0, 0, 0, 1};
    mlh_calib_store_info info[2];
    WindowNormalEquations ne[2];
    Device *devs[2] = {&facade_dev, &abi_dev};
    for (int d = 0; d < 2; ++d) {
        Device &dev = *devs[d];
        dev.check(mlh_map_set(dev.ctx(), MLH_SURF, map.data(), 16, (int)map.size() / 4, 1.0f, MLH_MEM_HOST));
        dev.check(mlh_features_set(dev.ctx(), MLH_SURF, feats.data(), 16, (int)feats.size() / 4, 12, -1, MLH_MEM_HOST));
        if (d == 0) {
            WindowFactorTable table(dev);
            table.accumulateStagedMatches('s', to_pose(ext1), 1);                       // N_NEIGH 10, FOV check: the defaults
        } else {
            const Params &P = params();
            dev.check(mlh_pure_odom_begin(dev.ctx()));
            dev.check(mlh_calib_accumulate(dev.ctx(), MLH_SURF, ext1.data(), 10, MLH_FLAG_CHECK_FOV, P.MIN_MATCH_SQ_DIS, P.MIN_PLANE_DIS, 1));
        }
        useCalibFactors(dev, true);
        info[d] = calibFactorInfo(dev);
        evalWindowNormalEquations(dev, ident.data(), std::vector<P7>{ident}, exts, 1.0, ne[d]);      // an empty factor table: the store's system alone
    }
    if (std::memcmp(&info[0], &info[1], sizeof(info[0])) != 0 || info[0].n_valid < 100 || info[0].n_valid > 300 || info[0].max_ext != 1) {
        std::printf("FAIL: accumulateStagedMatches: stores differ or are empty (%d / %d factors)\n", info[0].n_valid, info[1].n_valid);
        return false;
    }
    if (ne[0].n_residuals != info[0].n_valid || !same(ne[0].JtJ, ne[1].JtJ) || !same(ne[0].Jtr, ne[1].Jtr) || ne[0].cost != ne[1].cost) {
        std::printf("FAIL: accumulateStagedMatches: the two routes' normal equations differ\n");
        return false;
    }
    std::printf("calibration store: accumulateStagedMatches equals mlh_calib_accumulate (%d of 300 features matched)\n", info[0].n_valid);
    return true;
}

}  // namespace

int main()
{
    try {
        if (!run_chain(1, 3) || !run_chain(3, 2) || !run_accumulate()) return 1;
        std::printf("calibration store: facade equals the C-ABI over %d windows of (1 frame, 3 LiDARs) and (3 frames, 2 LiDARs) (poses and prior bits)\n", N_WINDOWS);
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
}
