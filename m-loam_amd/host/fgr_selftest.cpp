// LoopRegistration::performGlobalRegistration through the facade (FPFH + Fast Global Registration on the device, include/mloam_hip.h (f13)) on a room of a floor,
// two walls, a box and a tilted board, 600 points no two of which are closer than 0.15 m, and its copy seen from a frame moved by yaw 0.3 rad and 1.5 m:
//   - the host-cloud form (the reference's signature shape) finds the transform that made the scene within 1e-4 and accepts it;
//   - the overload on the clouds left on the device returns the same bits, with one host wait (the features are reused);
//   - chained as checkGeometricConsistency chains it, performLocalRegistration starts from that transform with the four clouds handed over again and runs;
//   - with the tail on the device (setGlobalRegistrationTail(true)) the same call returns the same counts and tuples' number, T within 1e-6 of the host tail's,
//     one host wait; back on the host tail the first call's bits return;
//   - with a tuple scale of 1 no tuple passes: T = GetOutputTrans of the identity, not accepted.
// Usage: fgr_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

void room(std::mt19937 &rng, size_t n, PointICloud &out)
{
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::normal_distribution<double> g(0.0, 0.02);
    std::vector<std::array<double, 3>> kept;
    while (kept.size() < n) {
        const double r = u(rng), a = u(rng), b = u(rng);
        std::array<double, 3> p;
        if (r < 0.30) p = {-1.4 + 2.8 * a, -1.4 + 2.8 * b, -1.2};
        else if (r < 0.52) p = {-1.4, -1.4 + 2.8 * a, -1.2 + 2.5 * b};
        else if (r < 0.74) p = {-1.4 + 2.8 * a, 1.4, -1.2 + 2.5 * b};
        else if (r < 0.80) p = {0.5 + 0.6 * a, -1.3 + 0.6 * b, -0.6};
        else if (r < 0.84) p = {0.5, -1.3 + 0.6 * a, -1.2 + 0.6 * b};
        else if (r < 0.88) p = {0.5 + 0.6 * a, -0.7, -1.2 + 0.6 * b};
        else p = {-1.3 + a * std::cos(0.61), -0.9 + 0.8 * b, -1.1 + a * std::sin(0.61)};
        for (double &c : p) c += g(rng);
        bool far = true;
        for (const auto &q : kept) far = far && ((p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]) >= 0.15 * 0.15);
        if (far) kept.push_back(p);
    }
    for (const auto &q : kept) { PointI p; p.x = float(q[0]); p.y = float(q[1]); p.z = float(q[2]); p.intensity = 0.f; out.push_back(p); }
}

}  // namespace

int main()
{
    Device dev(0);
    std::mt19937 rng(11);
    PointICloud model, data, no_corner;
    room(rng, 600, model);
    const double c = std::cos(0.3), s = std::sin(0.3), t[3] = {0.9, -0.8, 0.9};
    const Mat4 truth{c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2], 0, 0, 0, 1};
    for (const PointI &p : model.points) {                    // data = R^T (model - t)
        const double x = p.x - t[0], y = p.y - t[1], z = p.z - t[2];
        PointI q; q.x = float(c * x + s * y); q.y = float(-s * x + c * y); q.z = float(z); q.intensity = 0.f;
        data.push_back(q);
    }
    LoopRegistration reg(dev);
    const std::pair<bool, Mat4> got = reg.performGlobalRegistration(model, data);
    double err = 0.0;
    for (int i = 0; i < 16; ++i) err = std::max(err, std::fabs(got.second[size_t(i)] - truth[size_t(i)]));
    const mlh_fgr_result r0 = reg.lastGlobalResult();
    std::printf("performGlobalRegistration: accepted %d, max |T - truth| %.2e, cost %.3e, %d mutual pairs, %d tuples, %d host waits\n", int(got.first), err,
                r0.final_cost_normalize, r0.n_mutual, r0.n_tuples, r0.host_waits);
    EXPECT(got.first && err < 1e-4 && r0.n_mutual > 500 && r0.n_corres == 3 * r0.n_tuples && r0.swapped == 0);
    const std::pair<bool, Mat4> again = reg.performGlobalRegistration();
    EXPECT(again.first == got.first && std::memcmp(again.second.data(), got.second.data(), sizeof(double) * 16) == 0);
    EXPECT(reg.lastGlobalResult().host_waits == 1);
    // the local registration that follows it in checkGeometricConsistency (no corner clouds in this scene: the surf factors alone)
    const std::pair<bool, Mat4> local = reg.performLocalRegistration(model, no_corner, data, no_corner, got.second);
    double lerr = 0.0;
    for (int i = 0; i < 16; ++i) lerr = std::max(lerr, std::fabs(local.second[size_t(i)] - truth[size_t(i)]));
    std::printf("performLocalRegistration from it: accepted %d, max |T - truth| %.2e, cost %.3e\n", int(local.first), lerr, reg.lastResult().opti_cost);
    EXPECT(local.first && lerr < 5e-2);
    // the tail on the device: the same tuples, T within the f32 bar, one wait; then the host tail again, bit for bit
    EXPECT(!reg.globalRegistrationTailOnDevice());
    (void)reg.performGlobalRegistration(model, data);
    reg.setGlobalRegistrationTail(true);
    const std::pair<bool, Mat4> on_dev = reg.performGlobalRegistration();
    const mlh_fgr_result rd = reg.lastGlobalResult();
    double derr = 0.0;
    for (int i = 0; i < 16; ++i) derr = std::max(derr, std::fabs(on_dev.second[size_t(i)] - got.second[size_t(i)]));
    std::printf("performGlobalRegistration, device tail: accepted %d, max |T - host tail's T| %.2e, cost %.3e, %d tuples of %d trials, %d host waits\n", int(on_dev.first), derr,
                rd.final_cost_normalize, rd.n_tuples, rd.n_trials, rd.host_waits);
    EXPECT(on_dev.first == got.first && derr <= 1e-6 && rd.host_waits == 1);
    EXPECT(rd.n_mutual == r0.n_mutual && rd.n_tuples == r0.n_tuples && rd.n_corres == r0.n_corres && rd.n_trials == r0.n_trials && rd.swapped == r0.swapped);
    reg.setGlobalRegistrationTail(false);
    const std::pair<bool, Mat4> back = reg.performGlobalRegistration();
    EXPECT(std::memcmp(back.second.data(), got.second.data(), sizeof(double) * 16) == 0);
    reg.globalOptions().tuple_scale = 1.0f;
    const std::pair<bool, Mat4> none = reg.performGlobalRegistration(model, data);
    const mlh_fgr_result r1 = reg.lastGlobalResult();
    EXPECT(!none.first && r1.n_corres == 0 && std::isnan(r1.final_cost_normalize) && none.second[0] == 1.0 && none.second[1] == 0.0 && none.second[5] == 1.0);
    EXPECT(std::fabs(none.second[3] - (r1.means[0] - r1.means[3])) < 1e-6);
    if (fails) { std::printf("fgr_selftest: %d check(s) FAILED\n", fails); return 1; }
    std::printf("fgr_selftest: ok\n");
    return 0;
}
