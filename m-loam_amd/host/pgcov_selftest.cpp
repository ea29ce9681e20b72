// PoseGraph::computeMarginals / marginalCov and the covariance route of KeyframeMap::updateKeyframe / PipelinedMapper::applyLoopInfo through the facade (pose-graph
// marginal covariances on the device, include/mloam_hip.h (f18)) on 20 keyframes 1.2 m apart whose estimate has drifted, a pose graph on a Device of its own that
// holds the first 18 of them and one loop 16 -> 1:
//   - computeMarginals is refused (false) while there is no loop; after optimizePoseGraph(16) it runs: M = 16 keyframes, one host wait, the block of `first` is
//     zero, every other block is symmetric to the bit with a positive diagonal, and marginalCov equals what the plain C-ABI hands out in the store form;
//   - the uncertainty grows away from the anchor: the trace of keyframe 9 exceeds that of keyframe 2 (in the store's convention rho carries phi x t, so the far
//     end of the loop, 19 m from the origin, is no smaller);
//   - optimizePoseGraph makes the result stale: marginalCov throws until the next computeMarginals;
//   - WITHOUT the opt-in updateKeyframe(pg), on a second mapper, leaves every stored covariance and the KeyframePolicy's copies alone (the behaviour before this
//     row);
//   - with MLH_KF_COV_RELATIVE through PipelinedMapper::applyLoopInfo the store takes the same pose bits on 0 .. 16 (the tail to rounding), the keys 2 .. 16 take their blocks (store and policy
//     alike), keys 0, 1 (the anchor) and the tail 17 .. 19 keep theirs, and the local map is rebuilt.
// Usage: pgcov_selftest  (exit status 0 = pass)
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

Pose planar(double x, double y, double z, double yaw)
{
    Pose p;
    p.t_(0) = x; p.t_(1) = y; p.t_(2) = z;
    p.q_.w = std::cos(yaw / 2); p.q_.x = 0; p.q_.y = 0; p.q_.z = std::sin(yaw / 2);
    for (int i = 0; i < 6; ++i) p.cov_[size_t(i * 6 + i)] = i < 3 ? 4e-4 : 1e-5;
    return p;
}

Pose relative(const Pose &a, double yaw_a, const Pose &b, double yaw_b)
{
    const double dx = b.t_(0) - a.t_(0), dy = b.t_(1) - a.t_(1), c = std::cos(yaw_a), s = std::sin(yaw_a);
    return planar(c * dx + s * dy, -s * dx + c * dy, b.t_(2) - a.t_(2), yaw_b - yaw_a);
}

void frame_clouds(std::mt19937 &rng, int n_surf, int n_corner, PointICovCloud &surf, PointICovCloud &corner)
{
    std::uniform_real_distribution<float> u(-12.f, 12.f), h(0.f, 3.f);
    surf.clear(); corner.clear();
    for (int i = 0; i < n_surf; ++i) { PointIWithCov p; p.x = u(rng); p.y = u(rng); p.z = -1.f + 0.01f * h(rng); p.intensity = 0.f; surf.push_back(p); }
    for (int i = 0; i < n_corner; ++i) { PointIWithCov p; p.x = float(int(u(rng)) / 3 * 3); p.y = float(int(u(rng)) / 3 * 3); p.z = h(rng); p.intensity = 0.f; corner.push_back(p); }
}

double trace(const std::array<double, 36> &c)
{
    double t = 0.0;
    for (int i = 0; i < 6; ++i) t += c[size_t(i * 6 + i)];
    return t;
}

std::vector<double> store_covs(Device &dev, int n)
{
    std::vector<double> c(36 * size_t(n));
    dev.check(mlh_keyframe_poses(dev.ctx(), 0, n, nullptr, c.data(), nullptr));
    return c;
}

}  // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        Params &P = params();
        P.DISTANCE_KEYFRAMES = 1.0f; P.ORIENTATION_KEYFRAMES = 10.0f;
        P.SURROUNDING_KF_RADIUS = 5.0f;
        const int N = 20, N_PG = 18, CUR = 16, FIRST = 1;
        std::mt19937 rng(18);
        std::vector<Pose> truth, est, ext(1);
        std::vector<double> yaw_t;
        double x = 0, y = 0, xe = 0, ye = 0;
        for (int k = 0; k < N; ++k) {
            const double yt = 0.03 * k, yev = 0.03 * k + 0.002 * k;
            if (k) { x += 1.2 * std::cos(yt); y += 1.2 * std::sin(yt); xe += 1.205 * std::cos(yev); ye += 1.205 * std::sin(yev); }
            truth.push_back(planar(x, y, 0.0, yt)); yaw_t.push_back(yt);
            est.push_back(planar(xe, ye, 0.002 * k, yev));
        }
        Device dev_a, dev_b, dev_g;
        KeyframePolicy kf_a, kf_b;
        KeyframeMap km_a(dev_a, kf_a, true), km_b(dev_b, kf_b, true);
        km_a.setExtrinsics(ext); km_b.setExtrinsics(ext);
        for (int k = 0; k < N; ++k) {
            PointICovCloud s, c;
            frame_clouds(rng, 300 + 3 * k, 60 + k, s, c);
            EXPECT(km_a.saveKeyframe(est[size_t(k)], s, c) == k);
            EXPECT(km_b.saveKeyframe(est[size_t(k)], s, c) == k);
        }
        EXPECT(km_a.extractSurroundingKeyFrames(est[12]) && !km_a.lastIds().empty());
        const std::vector<double> cov0 = store_covs(dev_a, N);

        PoseGraph<Pose> pg(dev_g);
        for (int k = 0; k < N_PG; ++k) EXPECT(pg.addKeyFrame(est[size_t(k)]) == k);
        EXPECT(!pg.computeMarginals(10) && pg.marginalsCur() == -1);
        pg.updateLoopInfo(CUR, FIRST, relative(truth[FIRST], yaw_t[FIRST], truth[CUR], yaw_t[CUR]));
        EXPECT(pg.optimizePoseGraph(CUR));
        EXPECT(pg.computeMarginals(CUR));
        const mlh_pg_marginals_result &r = pg.lastMarginals();
        EXPECT(r.ok == 1 && r.n_keyframes == CUR - FIRST + 1 && r.n_loops == 1 && r.first_index == FIRST && r.host_waits == 1 && r.launches == 14);
        EXPECT(pg.marginalsFirst() == FIRST && pg.marginalsCur() == CUR);
        std::vector<double> plain(36 * size_t(r.n_keyframes));
        mlh_pg_marginals_result r2;
        dev_g.check(mlh_pg_marginals(dev_g.ctx(), CUR, &pg.options(), MLH_PG_COV_STORE, plain.data(), &r2));
        for (int k = FIRST; k <= CUR; ++k) {
            const std::array<double, 36> c = pg.marginalCov(k);
            EXPECT(std::memcmp(c.data(), plain.data() + 36 * size_t(k - FIRST), sizeof(double) * 36) == 0);
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) EXPECT(std::memcmp(&c[size_t(a * 6 + b)], &c[size_t(b * 6 + a)], sizeof(double)) == 0);
            if (k == FIRST) EXPECT(trace(c) == 0.0);
            else for (int a = 0; a < 6; ++a) EXPECT(c[size_t(a * 6 + a)] > 0.0);
        }
        EXPECT(trace(pg.marginalCov(9)) > trace(pg.marginalCov(2)));
        bool threw = false;
        try { (void)pg.marginalCov(CUR + 1); } catch (const Error &) { threw = true; }
        EXPECT(threw);

        // stale after an optimise
        EXPECT(pg.optimizePoseGraph(CUR));
        threw = false;
        try { (void)pg.marginalCov(5); } catch (const Error &) { threw = true; }
        EXPECT(threw);
        threw = false;
        try { (void)km_a.updateKeyframe(pg, MLH_KF_COV_RELATIVE); } catch (const Error &) { threw = true; }
        EXPECT(threw);
        EXPECT(store_covs(dev_a, N) == cov0);

        // without the opt-in (a second mapper): poses only
        (void)km_b.updateKeyframe(pg);
        EXPECT(km_b.lastChanged() >= N - 2 && km_b.lastChanged() <= N - 1);
        EXPECT(store_covs(dev_b, N) == cov0);
        for (int k = 0; k < N; ++k) EXPECT(kf_b.pose_keyframes_6d[size_t(k)].cov_ == est[size_t(k)].cov_);

        // the opt-in through the mapper's hook: the same poses, and the covariances
        EXPECT(pg.computeMarginals(CUR));
        PipelinedMapper pm(dev_a, km_a);
        (void)pm.applyLoopInfo(pg, est[12], MLH_KF_COV_RELATIVE);
        EXPECT(km_a.lastChanged() == km_b.lastChanged());
        {
            std::vector<double> pa(7 * size_t(N)), pb(7 * size_t(N));
            dev_a.check(mlh_keyframe_poses(dev_a.ctx(), 0, N, pa.data(), nullptr, nullptr));
            dev_b.check(mlh_keyframe_poses(dev_b.ctx(), 0, N, pb.data(), nullptr, nullptr));
            // 0 .. cur are the pose graph's bits on both; behind cur one side took the pose graph's own tail, the other the drift of keyframe cur on the host
            EXPECT(std::memcmp(pa.data(), pb.data(), sizeof(double) * 7 * size_t(CUR + 1)) == 0);
            for (size_t i = 7 * size_t(CUR + 1); i < pa.size(); ++i) EXPECT(std::fabs(pa[i] - pb[i]) < 1e-9);
        }
        const std::vector<double> cov1 = store_covs(dev_a, N);
        for (int k = 0; k < N; ++k) {
            const bool takes = k > FIRST && k <= CUR;
            const double *want = takes ? nullptr : cov0.data() + 36 * size_t(k);
            std::array<double, 36> blk{};
            if (takes) { blk = pg.marginalCov(k); want = blk.data(); }
            EXPECT(std::memcmp(cov1.data() + 36 * size_t(k), want, sizeof(double) * 36) == 0);
            EXPECT(std::memcmp(kf_a.pose_keyframes_6d[size_t(k)].cov_.data(), want, sizeof(double) * 36) == 0);
        }
        int32_t n_surf = 0;
        (void)km_a.surfMapDevice(&n_surf);
        EXPECT(n_surf > 0);                                  // rebuilt by the hook

        std::printf("pgcov selftest: M %d, launches %d, trace of keyframe 2 / 9 / 16: %.3e / %.3e / %.3e\n", r.n_keyframes, r.launches, trace(pg.marginalCov(2)),
                    trace(pg.marginalCov(9)), trace(pg.marginalCov(CUR)));
        if (fails) { std::printf("pgcov_selftest: %d check(s) failed\n", fails); return 1; }
        std::printf("pgcov_selftest: ok\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("pgcov_selftest: exception: %s\n", e.what());
        return 1;
    }
}
