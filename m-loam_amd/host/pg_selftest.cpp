// PoseGraph through the facade (pose-graph optimisation on the device, include/mloam_hip.h (f14)) on 30 keyframes 1 m apart on a gentle curve whose estimate has
// drifted, with one loop 28 -> 2 measured at the true relative pose:
//   - addKeyFrame hands out 0, 1, 2, ...; optimizePoseGraph is refused (false, pgoFlag stays clear) while there is no loop;
//   - after updateLoopInfo one pass runs: M = 27 keyframes, L = 1, the cost falls, the relative pose of the looped pair moves towards the measurement, keyframes 0 and
//     1 keep their bits, the last pose of every problem keyframe is its pose before the pass, keyframe 29 is pose_drift * its old pose;
//   - the same calls through the plain C-ABI on a second context end in the same bits;
//   - a second pass from the optimised poses runs and leaves the first pass's poses as the last poses;
//   - the capacity of loop edges is 128 until reserveLoops raises it, a value outside 128 .. MLH_PG_LOOPS_LIMIT is refused, and a new PoseGraph on the same device
//     (its constructor resets the store) keeps what was reserved.
// Usage: pg_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// planar poses are enough here: yaw about z and a translation
Pose planar(double x, double y, double z, double yaw)
{
    Pose p;
    p.t_(0) = x; p.t_(1) = y; p.t_(2) = z;
    p.q_.w = std::cos(yaw / 2); p.q_.x = 0; p.q_.y = 0; p.q_.z = std::sin(yaw / 2);
    return p;
}

// T_a^-1 T_b of two planar poses
Pose relative(const Pose &a, double yaw_a, const Pose &b, double yaw_b)
{
    const double dx = b.t_(0) - a.t_(0), dy = b.t_(1) - a.t_(1), c = std::cos(yaw_a), s = std::sin(yaw_a);
    return planar(c * dx + s * dy, -s * dx + c * dy, b.t_(2) - a.t_(2), yaw_b - yaw_a);
}

double pair_error(const Pose &a, const Pose &b, const Pose &meas)
{
    // |R_a^T (t_b - t_a) - t_meas| with the planar rotation read off the quaternion
    const double yaw = 2.0 * std::atan2(a.q_.z, a.q_.w), c = std::cos(yaw), s = std::sin(yaw);
    const double dx = b.t_(0) - a.t_(0), dy = b.t_(1) - a.t_(1);
    const double ex = c * dx + s * dy - meas.t_(0), ey = -s * dx + c * dy - meas.t_(1), ez = b.t_(2) - a.t_(2) - meas.t_(2);
    return std::sqrt(ex * ex + ey * ey + ez * ez);
}

bool same_bits(const Pose &a, const Pose &b)
{
    double pa[7], pb[7];
    a.toParam(pa); b.toParam(pb);
    return std::memcmp(pa, pb, sizeof(pa)) == 0;
}

}  // namespace

int main()
{
    const int N = 30;
    std::vector<Pose> truth, est;
    std::vector<double> yaw_t, yaw_e;
    double x = 0, y = 0, xe = 0, ye = 0;
    for (int k = 0; k < N; ++k) {
        const double yt = 0.03 * k, yev = 0.03 * k + 0.002 * k;          // the estimate's heading drifts by 2 mrad per step
        if (k) { x += std::cos(yt); y += std::sin(yt); xe += 1.004 * std::cos(yev); ye += 1.004 * std::sin(yev); }
        truth.push_back(planar(x, y, 0.0, yt)); yaw_t.push_back(yt);
        est.push_back(planar(xe, ye, 0.002 * k, yev)); yaw_e.push_back(yev);
    }
    const Pose loop_info = relative(truth[2], yaw_t[2], truth[28], yaw_t[28]);

    Device dev(0), plain(0);
    PoseGraph<Pose> pg(dev);
    for (int k = 0; k < N; ++k) EXPECT(pg.addKeyFrame(est[size_t(k)]) == k);
    EXPECT(pg.getKeyFrameSize() == N && pg.earliestLoopIndex() == -1);
    EXPECT(!pg.optimizePoseGraph(10) && !pg.pgoFlag());
    pg.updateLoopInfo(28, 2, loop_info);
    EXPECT(pg.earliestLoopIndex() == 2);
    EXPECT(!pg.optimizePoseGraph(1));                                      // before the earliest looped keyframe
    const double before = pair_error(est[2], est[28], loop_info);
    EXPECT(pg.optimizePoseGraph(28) && pg.pgoFlag());
    const mlh_pg_result r = pg.lastResult();
    EXPECT(r.n_keyframes == 27 && r.n_loops == 1 && r.first_index == 2 && r.host_waits == 1);
    EXPECT(r.num_iterations >= 1 && r.num_successful_steps >= 1 && r.final_cost < r.initial_cost);
    std::vector<Pose> got;
    pg.getPoses(got);
    EXPECT(int(got.size()) == N);
    const double after = pair_error(got[2], got[28], loop_info);
    std::printf("loop pair translation error: %.4f m before, %.4f m after; cost %.3f -> %.3f in %d iterations\n", before, after, r.initial_cost, r.final_cost,
                r.num_iterations);
    EXPECT(after < 0.8 * before);
    EXPECT(same_bits(got[0], est[0]) && same_bits(got[1], est[1]));
    for (int k = 2; k < N; ++k) { Pose last; pg.getLastPose(k, last); EXPECT(same_bits(last, est[size_t(k)])); }
    Pose one;
    pg.getPose(17, one);
    EXPECT(same_bits(one, got[17]));

    // the plain C-ABI on a second context
    double p[7];
    for (int k = 0; k < N; ++k) { est[size_t(k)].toParam(p); plain.check(mlh_pg_add_keyframe(plain.ctx(), p, nullptr)); }
    loop_info.toParam(p);
    plain.check(mlh_pg_set_loop(plain.ctx(), 28, 2, p));
    mlh_pg_result r2;
    plain.check(mlh_pg_optimize(plain.ctx(), 28, nullptr, &r2));
    std::vector<double> all(7 * size_t(N));
    plain.check(mlh_pg_poses(plain.ctx(), 0, N, all.data(), nullptr));
    for (int k = 0; k < N; ++k) { got[size_t(k)].toParam(p); EXPECT(std::memcmp(p, all.data() + 7 * k, sizeof(p)) == 0); }
    EXPECT(std::memcmp(&r.initial_cost, &r2.initial_cost, sizeof(double)) == 0 && std::memcmp(&r.final_cost, &r2.final_cost, sizeof(double)) == 0);
    EXPECT(std::memcmp(r.drift, r2.drift, sizeof(r.drift)) == 0);

    // keyframe 29 = pose_drift * its old pose
    {
        const double *d = r.drift, qx = d[3], qy = d[4], qz = d[5], qw = d[6];
        const Pose &o = est[29];
        const double v[3] = {o.t_(0), o.t_(1), o.t_(2)};
        const double uv[3] = {2 * (qy * v[2] - qz * v[1]), 2 * (qz * v[0] - qx * v[2]), 2 * (qx * v[1] - qy * v[0])};
        const double w[3] = {v[0] + qw * uv[0] + (qy * uv[2] - qz * uv[1]) + d[0], v[1] + qw * uv[1] + (qz * uv[0] - qx * uv[2]) + d[1],
                             v[2] + qw * uv[2] + (qx * uv[1] - qy * uv[0]) + d[2]};
        for (int c = 0; c < 3; ++c) EXPECT(std::fabs(got[29].t_(c) - w[c]) < 1e-12);
    }

    // a second pass
    pg.clearPgoFlag();
    EXPECT(pg.optimizePoseGraph(29) && pg.pgoFlag());
    for (int k = 2; k < N; ++k) { Pose last; pg.getLastPose(k, last); EXPECT(same_bits(last, got[size_t(k)])); }

    // the capacity of loop edges
    EXPECT(pg.maxLoops() == 128);
    pg.reserveLoops(300);
    EXPECT(pg.maxLoops() == 300);
    bool refused = false;
    try { pg.reserveLoops(MLH_PG_LOOPS_LIMIT + 1); } catch (const std::exception &) { refused = true; }
    EXPECT(refused && pg.maxLoops() == 300);
    { PoseGraph<Pose> again(dev); EXPECT(again.getKeyFrameSize() == 0 && again.maxLoops() == 300); }

    if (fails) { std::printf("pg_selftest: %d check(s) failed\n", fails); return 1; }
    std::printf("pg_selftest: ok\n");
    return 0;
}
