// The pose covariance on its way into the keyframe store: 12 frames through PipelinedMapper over a KeyframeMap, every frame solved by scan2MapOptimization
// (mlh_scan2map_begin / _end) and every frame a keyframe. With with_ua_flag the covariance saveKeyframe stores with a frame's pose is zero while the mapper holds at
// most 10 keyframes (lidar_mapper_keyframe.cpp:607-608) and from then on the bits mlh_scan2map_cov reports for that frame (cpp:606, 632); without the flag it is
// zero throughout (cpp:621). Usage: posecov_selftest  (exit status 0 = pass)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

std::vector<std::array<float, 3>> world_planes, world_edges;

void make_world()
{
    for (float x = -12.f; x <= 32.f; x += 0.25f)
        for (float y = -8.f; y <= 8.f; y += 0.25f) world_planes.push_back({x, y, 0.f});                 // ground
    for (float x = -12.f; x <= 32.f; x += 0.25f)
        for (float z = 0.25f; z <= 4.f; z += 0.25f) { world_planes.push_back({x, -8.f, z}); world_planes.push_back({x, 8.f, z}); }   // corridor walls
    for (float y = -8.f; y <= 8.f; y += 0.25f)
        for (float z = 0.25f; z <= 4.f; z += 0.25f) { world_planes.push_back({-12.f, y, z}); world_planes.push_back({32.f, y, z}); }
    for (int k = 0; k < 12; ++k)                                                                           // posts: vertical edges
        for (float z = 0.1f; z <= 3.f; z += 0.1f) world_edges.push_back({-8.f + 3.3f * k, k % 2 ? 5.5f : -5.5f, z});
    for (float x = -12.f; x <= 32.f; x += 0.1f) { world_edges.push_back({x, -8.f, 4.f}); world_edges.push_back({x, 8.f, 4.f}); }   // wall tops
}

Pose pose_at(double x, double y, double yaw)
{
    Pose p;
    p.t_(0) = x; p.t_(1) = y; p.t_(2) = 1.0;
    p.q_.w = std::cos(yaw / 2); p.q_.z = std::sin(yaw / 2);
    return p;
}

// the features a frame at `body` sees (within 18 m), in the body frame, intensity = LiDAR id
void frame_clouds(const Pose &body, std::mt19937 &rng, PointICovCloud &surf, PointICovCloud &corner)
{
    std::normal_distribution<float> noise(0.f, 0.01f);
    const double c = body.q_.w * body.q_.w - body.q_.z * body.q_.z, s = 2 * body.q_.w * body.q_.z;     // yaw-only rotation
    auto to_body = [&](const std::array<float, 3> &w, int lidar, PointICovCloud &out) {
        const double dx = w[0] - body.t_(0), dy = w[1] - body.t_(1), dz = w[2] - body.t_(2);
        if (dx * dx + dy * dy > 18.0 * 18.0) return;
        PointIWithCov p;
        p.x = float(c * dx + s * dy) + noise(rng); p.y = float(-s * dx + c * dy) + noise(rng); p.z = float(dz) + noise(rng);
        p.intensity = float(lidar);
        out.push_back(p);
    };
    surf.clear(); corner.clear();
    for (size_t i = 0; i < world_planes.size(); i += 3) to_body(world_planes[i], int(i / 3) & 1, surf);
    for (size_t i = 0; i < world_edges.size(); ++i) to_body(world_edges[i], int(i) & 1, corner);
}

struct Saved { int idx; std::array<double, 36> cov, reported; bool have_reported; };

}  // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        make_world();
        Params &P = params();
        P.SURROUNDING_KF_RADIUS = 6.0f; P.DISTANCE_KEYFRAMES = 0.2f; P.ORIENTATION_KEYFRAMES = 10.0f;      // 0.45 m per frame: every frame is saved
        const int n_frames = 12;
        std::vector<Pose> truth, wodom;
        std::vector<PointICovCloud> fs(n_frames), fc(n_frames);
        std::mt19937 rng(7);
        for (int k = 0; k < n_frames; ++k) {
            truth.push_back(pose_at(0.45 * k, 0.3 * std::sin(0.2 * k), 0.02 * std::sin(0.3 * k)));
            wodom.push_back(pose_at(0.45 * k * 1.02, 0.3 * std::sin(0.2 * k) + 0.01 * k, 0.02 * std::sin(0.3 * k)));
            frame_clouds(truth[k], rng, fs[k], fc[k]);
        }
        std::vector<Pose> ext(2);
        ext[1].t_(0) = 0.1; ext[1].t_(1) = -0.05;
        // the initial map: the first frame's clouds at its true pose, thinned as a local map
        PointICovCloud ms, mc;
        {
            Device d0;
            KeyframePolicy k0;
            KeyframeMap m0(d0, k0);
            m0.setExtrinsics(ext);
            m0.saveKeyframe(truth[0], fs[0], fc[0]);
            m0.extractSurroundingKeyFrames(truth[0]);
            int32_t ns = 0, nc = 0;
            const void *s = m0.surfMapDevice(&ns), *c = m0.cornerMapDevice(&nc);
            mlh_synchronize(d0.ctx());
            ms.points.resize(size_t(ns)); mc.points.resize(size_t(nc));
            if (hipMemcpy(ms.points.data(), s, sizeof(PointIWithCov) * ns, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(mc.points.data(), c, sizeof(PointIWithCov) * nc, hipMemcpyDeviceToHost) != hipSuccess) throw Error("hipMemcpy");
        }
        bool ok = true;
        for (int with_ua = 1; with_ua >= 0; --with_ua) {
            Device dev;
            KeyframePolicy kf;
            KeyframeMap km(dev, kf, with_ua != 0);
            km.setExtrinsics(ext);
            PipelinedMapper mapper(dev, km, 3, with_ua != 0);
            mapper.useScan2Map(true);
            std::vector<Saved> saved;
            // called right behind the store of a saved frame, with the pose that was stored: the solve collected last is that frame's
            mapper.setOnKeyframe([&](int idx, const Pose &pose) {
                Saved s;
                s.idx = idx; s.cov = pose.cov_;
                double cov[36];
                s.have_reported = mlh_scan2map_cov(dev.ctx(), cov, nullptr) == MLH_OK;
                for (int i = 0; i < 36; ++i) s.reported[size_t(i)] = s.have_reported ? cov[i] : 0.0;
                saved.push_back(s);
            });
            mapper.setInitialMap(ms, mc);
            mapper.setInitialPose(truth[0], wodom[0]);
            std::vector<Pose> got;
            for (int k = 0; k < n_frames; ++k) { Pose prev; if (mapper.process(fs[k], fc[k], wodom[k], prev)) got.push_back(prev); }
            got.push_back(mapper.finish());
            double worst_truth = 0.0;
            for (int k = 0; k < n_frames; ++k) worst_truth = std::max(worst_truth, std::hypot(got[size_t(k)].t_(0) - truth[k].t_(0), got[size_t(k)].t_(1) - truth[k].t_(1)));
            if (int(saved.size()) != n_frames || worst_truth > 0.1) { std::printf("implausible run: %zu keyframes of %d frames, max |t - truth| %.3f\n", saved.size(), n_frames, worst_truth); ok = false; }
            int zero = 0, equal = 0;
            for (const Saved &s : saved) {
                bool all_zero = true;
                for (double v : s.cov) all_zero = all_zero && v == 0.0;
                const bool want_zero = !with_ua || s.idx <= 10;        // idx keyframes were held when the frame was solved
                if (want_zero) {
                    if (!all_zero) { std::printf("with_ua %d, keyframe %d: a covariance was stored where the reference stores zero\n", with_ua, s.idx); ok = false; }
                    else ++zero;
                } else {
                    double trace = 0.0;
                    for (int i = 0; i < 6; ++i) trace += s.cov[size_t(i * 7)];
                    if (!s.have_reported || std::memcmp(s.cov.data(), s.reported.data(), sizeof(double) * 36) != 0 || !(trace > 0.0) || !std::isfinite(trace)) {
                        std::printf("with_ua %d, keyframe %d: the stored covariance is not mlh_scan2map_cov's (trace %.3e)\n", with_ua, s.idx, trace);
                        ok = false;
                    } else ++equal;
                }
                if (with_ua != 0 && !s.have_reported) { std::printf("with_ua 1, keyframe %d: mlh_scan2map_cov had nothing\n", s.idx); ok = false; }
            }
            std::printf("posecov selftest: with_ua %d: %zu keyframes, %d stored with a zero covariance, %d with mlh_scan2map_cov's bits; max |t - truth| %.4f m\n",
                        with_ua, saved.size(), zero, equal, worst_truth);
            if (with_ua ? (zero != 11 || equal != 1) : (zero != n_frames || equal != 0)) { std::printf("with_ua %d: expected %s\n", with_ua, with_ua ? "11 zero + 1 reported" : "12 zero"); ok = false; }
        }
        std::printf("posecov selftest: %s\n", ok ? "pass" : "FAIL");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::printf("posecov selftest: %s\n", e.what());
        return 1;
    }
}
