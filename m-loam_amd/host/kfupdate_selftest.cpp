// KeyframeMap::updateKeyframe (loop-corrected poses into the mapper's keyframe store, include/mloam_hip.h (f15)) through the facade, on 20 keyframes 1.2 m apart
// whose estimate has drifted, with a pose graph on a Device of its own that holds the first 18 of them (the mapper saved two more after the loop side's snapshot)
// and one loop 16 -> 1:
//   - before the update the mapper's local map is built, so its cache is filled;
//   - PipelinedMapper::applyLoopInfo with updateKeyframe(PoseGraph &): the store's poses 0..17 are the pose graph's bit for bit, keyframe 0 keeps its bits,
//     keyframes 18 and 19 are drift * their old pose, the drift is the pose graph's own to rounding, the KeyframePolicy holds the store's poses, and the local
//     map has been rebuilt around drift * the current pose;
//   - a second mapper that saved the same clouds and takes the same poses as a /loop_info-shaped list ends with the same pose bits, and its local map -- built
//     from an empty cache -- has the same bits as the first one's, which was rebuilt over a filled cache;
//   - an update with the poses the store already holds changes nothing: no keyframe counted, the identity drift, no rebuild.
// Usage: kfupdate_selftest  (exit status 0 = pass)
#include <hip/hip_runtime.h>
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

// a frame's clouds in the body frame, intensity = LiDAR id: a ground patch (surf) and posts (corner)
void frame_clouds(std::mt19937 &rng, int n_surf, int n_corner, PointICovCloud &surf, PointICovCloud &corner)
{
    std::uniform_real_distribution<float> u(-12.f, 12.f), h(0.f, 3.f);
    surf.clear(); corner.clear();
    for (int i = 0; i < n_surf; ++i) { PointIWithCov p; p.x = u(rng); p.y = u(rng); p.z = -1.f + 0.01f * h(rng); p.intensity = float(i & 1); surf.push_back(p); }
    for (int i = 0; i < n_corner; ++i) { PointIWithCov p; p.x = float(int(u(rng)) / 3 * 3); p.y = float(int(u(rng)) / 3 * 3); p.z = h(rng); p.intensity = float(i & 1); corner.push_back(p); }
}

bool same_pose_bits(const Pose &a, const Pose &b)
{
    double pa[7], pb[7];
    a.toParam(pa); b.toParam(pb);
    return std::memcmp(pa, pb, sizeof(pa)) == 0;
}

std::vector<float> fetch(KeyframeMap &km, bool surf)
{
    int32_t n = 0;
    const void *p = surf ? km.surfMapDevice(&n) : km.cornerMapDevice(&n);
    std::vector<float> rec(size_t(n) * 12);
    km.device().check(mlh_synchronize(km.device().ctx()));
    if (n > 0 && hipMemcpy(rec.data(), p, rec.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw Error("hipMemcpy");
    for (size_t i = 0; i < size_t(n); ++i) rec[12 * i + 11] = 0.f;      // the record's padding word
    return rec;
}

void store_poses(Device &dev, int n, std::vector<double> &p)
{
    p.assign(7 * size_t(n), 0.0);
    dev.check(mlh_keyframe_poses(dev.ctx(), 0, n, p.data(), nullptr, nullptr));
}

}  // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        Params &P = params();
        P.DISTANCE_KEYFRAMES = 1.0f; P.ORIENTATION_KEYFRAMES = 10.0f;
        P.SURROUNDING_KF_RADIUS = 5.0f;          // around keyframe 12 the radius holds corrected keyframes only: the rebuilt cache has a fresh store's order
        const int N = 20, N_PG = 18;
        std::mt19937 rng(15);
        std::vector<Pose> truth, est, ext(2);
        std::vector<double> yaw_t;
        ext[1].t_(0) = 0.1; ext[1].t_(1) = -0.05;
        double x = 0, y = 0, xe = 0, ye = 0;
        for (int k = 0; k < N; ++k) {
            const double yt = 0.03 * k, yev = 0.03 * k + 0.002 * k;          // the estimate's heading drifts by 2 mrad per step
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
            frame_clouds(rng, 2500 + 31 * k, 400 + 7 * k, s, c);
            EXPECT(km_a.saveKeyframe(est[size_t(k)], s, c) == k);
            EXPECT(km_b.saveKeyframe(est[size_t(k)], s, c) == k);
        }
        EXPECT(km_a.extractSurroundingKeyFrames(est[12]) && !km_a.lastIds().empty());      // the cache is filled at the uncorrected poses

        PoseGraph<Pose> pg(dev_g);
        for (int k = 0; k < N_PG; ++k) EXPECT(pg.addKeyFrame(est[size_t(k)]) == k);
        pg.updateLoopInfo(16, 1, relative(truth[1], yaw_t[1], truth[16], yaw_t[16]));
        EXPECT(pg.optimizePoseGraph(16));
        std::vector<Pose> corrected;
        pg.getPoses(corrected);
        EXPECT(int(corrected.size()) == N_PG);

        // the records in HBM, through the mapper's hook
        PipelinedMapper pm(dev_a, km_a);
        const Pose drift = pm.applyLoopInfo([&](KeyframeMap &km) { return km.updateKeyframe(pg); }, est[12]);
        EXPECT(km_a.lastChanged() >= N - 2 && km_a.lastChanged() <= N - 1);       // keyframe 0 keeps its bits; the constant block 1 is normalised and may keep them
        std::vector<double> pa, pb;
        store_poses(dev_a, N, pa);
        for (int k = 0; k < N_PG; ++k) { double p[7]; corrected[size_t(k)].toParam(p); EXPECT(std::memcmp(p, pa.data() + 7 * k, sizeof(p)) == 0); }
        { double p[7]; est[0].toParam(p); EXPECT(std::memcmp(p, pa.data(), sizeof(p)) == 0); }
        const double *dg = pg.lastResult().drift;
        double dp[7];
        drift.toParam(dp);
        for (int c = 0; c < 7; ++c) EXPECT(std::fabs(dp[c] - dg[c]) < 1e-12);
        for (int k = N_PG; k < N; ++k) {
            const Pose want = poseMul(drift, est[size_t(k)]);
            double w[7];
            want.toParam(w);
            for (int c = 0; c < 7; ++c) EXPECT(std::fabs(w[c] - pa[size_t(7 * k + c)]) < 1e-12);
            EXPECT(std::fabs(pa[size_t(7 * k)] - est[size_t(k)].t_(0)) + std::fabs(pa[size_t(7 * k + 1)] - est[size_t(k)].t_(1)) > 1e-3);      // it moved
        }
        for (int k = 0; k < N; ++k) {
            Pose s;
            s.fromParam(pa.data() + 7 * k);
            EXPECT(same_pose_bits(kf_a.pose_keyframes_6d[size_t(k)], s));
            EXPECT(kf_a.pose_keyframes_3d.points[size_t(k)].x == float(pa[size_t(7 * k)]) && kf_a.pose_keyframes_3d.points[size_t(k)].y == float(pa[size_t(7 * k + 1)]));
            EXPECT(kf_a.pose_keyframes_6d[size_t(k)].cov_ == est[size_t(k)].cov_);
        }

        // the /loop_info-shaped list on a mapper whose cache is empty
        const Pose drift_b = km_b.updateKeyframe(corrected);
        EXPECT(same_pose_bits(drift, drift_b) && km_b.lastChanged() == km_a.lastChanged());
        store_poses(dev_b, N, pb);
        EXPECT(pa == pb);
        const Pose cur = poseMul(drift, est[12]);
        EXPECT(km_b.extractSurroundingKeyFrames(cur));
        EXPECT(km_a.lastIds() == km_b.lastIds() && km_a.lastIds().size() >= 3);
        for (int32_t id : km_a.lastIds()) EXPECT(id != 0);
        const std::vector<float> sa = fetch(km_a, true), sb = fetch(km_b, true), ca = fetch(km_a, false), cb = fetch(km_b, false);
        EXPECT(!sa.empty() && !ca.empty());
        EXPECT(sa.size() == sb.size() && std::memcmp(sa.data(), sb.data(), sa.size() * sizeof(float)) == 0);
        EXPECT(ca.size() == cb.size() && std::memcmp(ca.data(), cb.data(), ca.size() * sizeof(float)) == 0);

        // the poses the store already holds: nothing changes, nothing is rebuilt
        std::vector<Pose> held(static_cast<size_t>(N));
        for (int k = 0; k < N; ++k) held[size_t(k)].fromParam(pa.data() + 7 * k);
        const Pose none = km_a.updateKeyframe(held);
        EXPECT(km_a.lastChanged() == 0 && same_pose_bits(none, Pose()));
        EXPECT(!km_a.extractSurroundingKeyFrames(cur));

        std::printf("kfupdate selftest: %d keyframes changed, drift (%.4f, %.4f, %.4f) m, local map of %zu + %zu records\n", km_b.lastChanged(), dp[0], dp[1], dp[2],
                    sa.size() / 12, ca.size() / 12);
        if (fails) { std::printf("kfupdate_selftest: %d check(s) failed\n", fails); return 1; }
        std::printf("kfupdate_selftest: ok\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("kfupdate_selftest: %s\n", e.what());
        return 1;
    }
}
