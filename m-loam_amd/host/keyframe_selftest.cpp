// KeyframeMap + PipelinedMapper on the device path against the callback path with host clouds: a 30-frame run over a synthetic corridor. The callback path's
// local map is made by a second KeyframeMap on its own context and handed over as host clouds (what INTEGRATION.md section 4b's fallback does with the
// per-keyframe loop); both runs must return the same pose bits and the same counters. Usage: keyframe_selftest  (exit status 0 = pass)
#include <hip/hip_runtime.h>
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

}  // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        make_world();
        Params &P = params();
        P.SURROUNDING_KF_RADIUS = 6.0f; P.DISTANCE_KEYFRAMES = 1.0f; P.ORIENTATION_KEYFRAMES = 10.0f;
        const int n_frames = 30;
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
        // (a) the device path
        std::vector<Pose> got_a;
        Device dev_a;
        KeyframePolicy kf_a;
        KeyframeMap km_a(dev_a, kf_a);
        km_a.setExtrinsics(ext);
        PipelinedMapper map_a(dev_a, km_a, 3);
        map_a.setInitialMap(ms, mc);
        map_a.setInitialPose(truth[0], wodom[0]);
        for (int k = 0; k < n_frames; ++k) { Pose prev; if (map_a.process(fs[k], fc[k], wodom[k], prev)) got_a.push_back(prev); }
        got_a.push_back(map_a.finish());
        // (b) the callback path: host clouds, assembled by a KeyframeMap of another context and fetched
        std::vector<Pose> got_b;
        Device dev_b, dev_c;
        KeyframePolicy kf_b;
        KeyframeMap km_c(dev_c, kf_b);
        km_c.setExtrinsics(ext);
        int closing = 0;
        auto assemble = [&](const std::vector<int> &, const Pose &prior, PointICovCloud &s_out, PointICovCloud &c_out) {
            km_c.clearCloud();
            km_c.extractSurroundingKeyFrames(prior);
            int32_t ns = 0, nc = 0;
            const void *s = km_c.surfMapDevice(&ns), *c = km_c.cornerMapDevice(&nc);
            dev_c.check(mlh_synchronize(dev_c.ctx()));
            s_out.points.resize(size_t(ns)); c_out.points.resize(size_t(nc));
            if (hipMemcpy(s_out.points.data(), s, sizeof(PointIWithCov) * ns, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(c_out.points.data(), c, sizeof(PointIWithCov) * nc, hipMemcpyDeviceToHost) != hipSuccess) throw Error("hipMemcpy");
        };
        auto on_kf = [&](int, const Pose &pose) { km_c.store(pose, fs[closing], fc[closing]); };
        PipelinedMapper map_b(dev_b, kf_b, assemble, on_kf, 3);
        map_b.setInitialMap(ms, mc);
        map_b.setInitialPose(truth[0], wodom[0]);
        for (int k = 0; k < n_frames; ++k) { Pose prev; closing = k - 1; if (map_b.process(fs[k], fc[k], wodom[k], prev)) got_b.push_back(prev); }
        closing = n_frames - 1;
        got_b.push_back(map_b.finish());

        bool ok = got_a.size() == size_t(n_frames) && got_b.size() == size_t(n_frames);
        double worst_truth = 0.0;
        for (int k = 0; ok && k < n_frames; ++k) {
            double a[7], b[7];
            got_a[k].toParam(a); got_b[k].toParam(b);
            if (std::memcmp(a, b, sizeof(a)) != 0) { std::printf("frame %d: poses differ\n", k); ok = false; }
            worst_truth = std::max(worst_truth, std::hypot(a[0] - truth[k].t_(0), a[1] - truth[k].t_(1)));
        }
        const auto &A = map_a.counters, &B = map_b.counters;
        if (A.frames != B.frames || A.overlapped != B.overlapped || A.waited != B.waited || A.redone != B.redone || A.keyframes != B.keyframes) {
            std::printf("counters differ\n");
            ok = false;
        }
        if (A.keyframes < 5 || worst_truth > 0.1) { std::printf("implausible run: keyframes %d, max |t - truth| %.3f\n", A.keyframes, worst_truth); ok = false; }
        int32_t n_kf = 0, n_cached = 0;
        int64_t store_b = 0, cache_b = 0;
        dev_a.check(mlh_local_map_info(dev_a.ctx(), &n_kf, &n_cached, &store_b, &cache_b));
        std::printf("keyframe selftest: %d frames, staged beside the solve %d, waited %d, solved again %d, keyframes %d (store %d, cached %d, %lld + %lld bytes); "
                    "max |t - truth| %.4f m; device path %s the callback path\n", A.frames, A.overlapped, A.waited, A.redone, A.keyframes, n_kf, n_cached,
                    (long long)store_b, (long long)cache_b, worst_truth, ok ? "equals" : "DIFFERS FROM");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::printf("keyframe selftest: %s\n", e.what());
        return 1;
    }
}
