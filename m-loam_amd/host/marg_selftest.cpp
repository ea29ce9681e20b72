// The window's marginalisation prior through the facade (solveWindow, marginalizeWindow, setExtrinsicPrior, windowPriorInfo) against the plain C-ABI calls
// (mlh_pure_odom_gn_solve, mlh_window_marginalize, mlh_window_ext_prior_set, mlh_window_prior_get) on a second context: four consecutive windows of one frame
// and two LiDARs, each solve -> marginalise -> slide -> new frame (estimator.cpp:658-665, 852-861, 871-1063). The poses of every window and the prior's bits
// (block map, x0, linearized_jacobians, linearized_residuals) must be equal.
// Usage: marg_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

constexpr int N_EXT = 2, N_WINDOWS = 4, PER_GROUP = 60;
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
    // q = qz(yaw) * qx(roll)
    const double cz = std::cos(yaw / 2), sz = std::sin(yaw / 2), cx = std::cos(roll / 2), sx = std::sin(roll / 2);
    return P7{x, y, z, cz * sx, sz * sx, sz * cx, cz * cx};
}

struct Table { std::vector<int32_t> type, fi, ei; std::vector<double> points, coeffs; };

// factors of (frame 0, every LiDAR): a point in the LiDAR frame, moved with the TRUE T_pivot^-1 T_frame T_ext, and a plane through / a line near the moved point
Table make_table(std::mt19937 &rng, const P7 &pivot, const P7 &frame, const std::vector<P7> &exts)
{
    std::uniform_real_distribution<double> u(-15.0, 15.0);
    std::normal_distribution<double> g(0.0, 1.0);
    Table t;
    for (int e = 0; e < N_EXT; ++e) {
        const Pose T = poseMul(poseMul(poseInverse(to_pose(pivot)), to_pose(frame)), to_pose(exts[size_t(e)]));
        for (int k = 0; k < PER_GROUP; ++k) {
            const double p[3] = {u(rng), u(rng), u(rng)};
            double x[3];
            detail::quat_rotate(T.q_, p, x);
            for (int c = 0; c < 3; ++c) x[c] += T.t_(c) + 0.01 * g(rng);
            double v[3] = {g(rng), g(rng), g(rng)};
            const double vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int c = 0; c < 3; ++c) v[c] /= vn;
            t.type.push_back(k % 2); t.fi.push_back(0); t.ei.push_back(e);
            for (int c = 0; c < 3; ++c) t.points.push_back(p[c]);
            if (k % 2 == 0) {
                for (int c = 0; c < 3; ++c) t.coeffs.push_back(v[c]);
                t.coeffs.push_back(-(v[0] * x[0] + v[1] * x[1] + v[2] * x[2]));
                t.coeffs.push_back(0.0); t.coeffs.push_back(0.0);
            } else {
                for (int c = 0; c < 3; ++c) t.coeffs.push_back(x[c] + 0.1 * v[c]);
                for (int c = 0; c < 3; ++c) t.coeffs.push_back(x[c] - 0.1 * v[c]);
            }
        }
    }
    return t;
}

void stage(Device &dev, const Table &t)
{
    dev.check(mlh_pure_odom_set(dev.ctx(), (int)t.type.size(), t.type.data(), t.points.data(), t.coeffs.data(), nullptr, t.fi.data(), t.ei.data()));
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

}  // namespace

int main()
{
    try {
        Device facade_dev(0), abi_dev(0);
        std::mt19937 rng(2024);
        std::normal_distribution<double> g(0.0, 1.0);
        std::vector<P7> traj;
        for (int k = 0; k <= N_WINDOWS; ++k) traj.push_back(yaw_pose(0.4 * k, 0.05 * std::sin(0.7 * k), 0.01 * k, 0.02 * k, 0.003 * k));
        const std::vector<P7> exts_true = {P7{0, 0, 0, 0, 0, 0, 1}, yaw_pose(0.1, -0.45, 0.02, 0.2, 0.01)};
        auto perturbed = [&](const P7 &p) {
            P7 o = p;
            for (int c = 0; c < 3; ++c) o[size_t(c)] += 0.02 * g(rng);
            const Pose d = poseMul(to_pose(p), to_pose(yaw_pose(0, 0, 0, 0.004 * g(rng), 0.003 * g(rng))));
            o[3] = d.q_.x; o[4] = d.q_.y; o[5] = d.q_.z; o[6] = d.q_.w;
            return o;
        };
        // the PriorFactor of both extrinsics, in the marginalisation only (ESTIMATE_EXTRINSIC == 0)
        std::vector<std::array<double, 3>> tbl;
        std::vector<std::array<double, 4>> qbl;
        std::vector<double> rows;
        for (const P7 &e : exts_true) {
            tbl.push_back({e[0], e[1], e[2]}); qbl.push_back({e[3], e[4], e[5], e[6]});
            for (int c = 0; c < 7; ++c) rows.push_back(e[size_t(c)]);
            rows.push_back(5.0); rows.push_back(10.0);
        }
        setExtrinsicPrior(facade_dev, tbl, qbl, 5.0, 10.0, false);
        abi_dev.check(mlh_window_ext_prior_set(abi_dev.ctx(), N_EXT, rows.data(), 1u));

        P7 pivot_f = traj[0], pivot_a = traj[0];
        std::vector<P7> exts_f = {exts_true[0], perturbed(exts_true[1])}, exts_a = exts_f;
        int moved = 0;
        for (int k = 0; k < N_WINDOWS; ++k) {
            const Table t = make_table(rng, traj[size_t(k)], traj[size_t(k) + 1], exts_true);
            const P7 start = perturbed(traj[size_t(k) + 1]);
            // the facade
            stage(facade_dev, t);
            std::vector<P7> frames_f = {start};
            if (solveWindow(facade_dev, pivot_f.data(), frames_f, exts_f, 1.0, 5) == 2) { std::printf("FAIL: window %d not solved (facade)\n", k); return 1; }
            const mlh_window_prior_info info_f = marginalizeWindow(facade_dev, pivot_f.data(), frames_f, exts_f, 1.0);
            // the plain calls
            stage(abi_dev, t);
            std::vector<P7> frames_a = {start};
            int32_t n_res = 0, status = 0;
            double cost = 0.0;
            abi_dev.check(mlh_pure_odom_gn_solve(abi_dev.ctx(), pivot_a.data(), frames_a[0].data(), 1, exts_a[0].data(), N_EXT, 1.0, 5, 1u | (1u << 2), nullptr, &cost, &n_res,
                                                 &status));
            mlh_window_prior_info info_a;
            abi_dev.check(mlh_window_marginalize(abi_dev.ctx(), pivot_a.data(), frames_a[0].data(), 1, exts_a[0].data(), N_EXT, 1.0, &info_a));
            if (std::memcmp(frames_f[0].data(), frames_a[0].data(), sizeof(P7)) != 0 || std::memcmp(exts_f[1].data(), exts_a[1].data(), sizeof(P7)) != 0) {
                std::printf("FAIL: window %d: the two paths' poses differ\n", k);
                return 1;
            }
            const PriorBits pf = read_prior(facade_dev), pa = read_prior(abi_dev);
            const mlh_window_prior_info wi = windowPriorInfo(facade_dev);
            if (!pf.info.valid || !pa.info.valid || !wi.valid || wi.n_keep != 1 + N_EXT || info_f.kept_rr != info_a.kept_rr || info_f.kept_mm != info_a.kept_mm ||
                !same(pf.ids, pa.ids) || !same(pf.x0, pa.x0) || !same(pf.J0, pa.J0) || !same(pf.r0, pa.r0)) {
                std::printf("FAIL: window %d: the two paths' priors differ\n", k);
                return 1;
            }
            if (pf.ids[0] != 0 || pf.ids[1] != 2 || pf.ids[2] != 3 || std::memcmp(pf.x0.data(), frames_f[0].data(), sizeof(P7)) != 0) {
                std::printf("FAIL: window %d: block map / x0 are not the slid window's\n", k);
                return 1;
            }
            moved += info_f.kept_rr > 0;
            // slide: frame 0 becomes the pivot
            pivot_f = frames_f[0]; pivot_a = frames_a[0];
        }
        clearWindowPrior(facade_dev);
        if (windowPriorInfo(facade_dev).valid) { std::printf("FAIL: clearWindowPrior left a prior\n"); return 1; }
        if (moved != N_WINDOWS) { std::printf("FAIL: a window's prior kept no eigenvalue\n"); return 1; }
        std::printf("window prior: facade equals the C-ABI over %d windows (poses and prior bits)\n", N_WINDOWS);
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
}
