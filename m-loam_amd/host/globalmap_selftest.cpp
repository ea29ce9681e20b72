// KeyframeMap::pubGlobalMap / saveGlobalMap (the global map built on the device from the keyframe store) against the per-keyframe C-ABI loop it replaces
// (mlh_cloud_uct_associate_to_map per keyframe and kind, concatenation on the host, mlh_voxel_filter) on a second context: keyframes with outlier clouds are
// saved through the facade, both maps are built and compared field for field, bit for bit. Usage: globalmap_selftest  (exit status 0 = pass)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

Pose pose_at(double x, double y, double yaw, std::mt19937 &rng)
{
    Pose p;
    p.t_(0) = x; p.t_(1) = y; p.t_(2) = 1.0;
    p.q_.w = std::cos(yaw / 2); p.q_.z = std::sin(yaw / 2);
    std::normal_distribution<double> g(0.0, 1.0);
    double a[36];
    for (double &v : a) v = g(rng);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) { double s = 0; for (int k = 0; k < 6; ++k) s += a[r * 6 + k] * a[c * 6 + k]; p.cov_[size_t(r * 6 + c)] = s * 2e-5; }
    return p;
}

// a frame's clouds in the body frame, intensity = LiDAR id: a ground patch (surf), posts (corner), scattered returns (outlier)
void frame_clouds(std::mt19937 &rng, int n_surf, int n_corner, int n_outlier, PointICovCloud &surf, PointICovCloud &corner, PointICloud &outlier)
{
    std::uniform_real_distribution<float> u(-15.f, 15.f), h(0.f, 3.f);
    surf.clear(); corner.clear(); outlier.clear();
    for (int i = 0; i < n_surf; ++i) { PointIWithCov p; p.x = u(rng); p.y = u(rng); p.z = -1.f + 0.01f * h(rng); p.intensity = float(i & 1); surf.push_back(p); }
    for (int i = 0; i < n_corner; ++i) { PointIWithCov p; p.x = float(int(u(rng)) / 3 * 3); p.y = float(int(u(rng)) / 3 * 3); p.z = h(rng); p.intensity = float(i & 1); corner.push_back(p); }
    for (int i = 0; i < n_outlier; ++i) { PointI p; p.x = 2.f * u(rng); p.y = 2.f * u(rng); p.z = 2.f * h(rng); p.intensity = float(i & 1); outlier.push_back(p); }
}

bool same_bits(const PointICovCloud &a, const PointICovCloud &b, const char *what)
{
    if (a.size() != b.size()) { std::printf("%s: %zu records against %zu\n", what, a.size(), b.size()); return false; }
    for (size_t i = 0; i < a.size(); ++i) {
        const PointIWithCov &p = a[i], &q = b[i];
        if (std::memcmp(&p.x, &q.x, 12) != 0 || std::memcmp(&p.intensity, &q.intensity, 4) != 0 || std::memcmp(p.cov_vec, q.cov_vec, 24) != 0 ||
            std::memcmp(&p.cov_trace, &q.cov_trace, 4) != 0) { std::printf("%s: record %zu differs\n", what, i); return false; }
    }
    return true;
}

PointICovCloud with_cov(const PointICloud &c)
{
    PointICovCloud o;
    for (const PointI &p : c.points) { PointIWithCov q; q.x = p.x; q.y = p.y; q.z = p.z; q.intensity = p.intensity; o.push_back(q); }
    return o;
}

}  // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        Params &P = params();
        P.DISTANCE_KEYFRAMES = 1.0f; P.ORIENTATION_KEYFRAMES = 10.0f;
        P.GLOBALMAP_KF_RES = 2.0f;               // keyframes 1.2 m apart share 2 m position voxels: some do not reach the map
        P.TRACE_THRESHOLD_MAPPING = 0.3;         // the gate cuts far points
        const bool with_ua = true;
        std::mt19937 rng(11);
        std::vector<Pose> ext(2);
        ext[1].t_(0) = 0.1; ext[1].t_(1) = -0.05;
        for (int i = 0; i < 6; ++i) ext[1].cov_[size_t(i * 6 + i)] = i < 3 ? 0.0025 : 0.00030461;

        Device dev_a, dev_b;
        KeyframePolicy kf_a, kf_b;
        KeyframeMap km(dev_a, kf_a, with_ua), side(dev_b, kf_b, with_ua);      // `side`: the loop's context (its KeyframeMap only thins the outlier clouds)
        km.setExtrinsics(ext); side.setExtrinsics(ext);
        const int n_frames = 14;
        std::vector<Pose> poses;
        std::vector<PointICovCloud> fs(n_frames), fc(n_frames);
        std::vector<PointICovCloud> fo(n_frames);
        int n_saved = 0;
        for (int k = 0; k < n_frames; ++k) {
            poses.push_back(pose_at(1.2 * k, 0.4 * std::sin(0.5 * k), 0.05 * k, rng));
            PointICloud outlier;
            frame_clouds(rng, 3000 + 37 * k, 500 + 11 * k, k == 5 ? 0 : 900 + 13 * k, fs[k], fc[k], outlier);
            const int idx = km.saveKeyframe(poses[k], fs[k], fc[k], outlier);
            if (idx != k) throw Error("every frame of this run is a keyframe");
            fo[k] = with_cov(side.downsampleOutlier(outlier));
            ++n_saved;
        }
        auto copy = [](void *dst, const void *src, size_t bytes) { if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw Error("hipMemcpy"); };
        // the per-keyframe loop on the side context
        auto loop = [&](const std::vector<int32_t> &ids, const std::vector<std::vector<const PointICovCloud *>> &kinds, float leaf, std::vector<PointICovCloud> &out) {
            out.clear();
            for (const auto &order : kinds) {
                PointICovCloud pre, ds;
                for (int32_t id : ids)
                    for (const PointICovCloud *per_frame : order) {
                        PointICovCloud g;
                        cloudUCTAssociateToMap(dev_b, per_frame[id], g, poses[size_t(id)], ext, with_ua);
                        pre.points.insert(pre.points.end(), g.points.begin(), g.points.end());
                    }
                VoxelGridCovarianceMLOAM<PointIWithCov> f(dev_b);
                f.setLeafSize(leaf, leaf, leaf);
                f.setTraceThreshold(float(P.TRACE_THRESHOLD_MAPPING));
                f.setInputCloud(pre);
                f.filter(ds);
                out.push_back(ds);
            }
        };
        bool ok = true;
        // pubGlobalMap around the middle of the trajectory
        PointICovCloud got;
        std::vector<PointICovCloud> want;
        km.fetchCloud(km.pubGlobalMap(poses[7]), got, copy);
        const std::vector<int32_t> pub_ids = km.lastGlobalIds();
        loop(pub_ids, {{fs.data(), fc.data(), fo.data()}}, P.MAP_SURF_RES, want);
        ok = same_bits(got, want[0], "pubGlobalMap") && ok;
        const size_t n_pub = got.size();
        // saveGlobalMap
        PointICovCloud got_s, got_c;
        const auto maps = km.saveGlobalMap();
        km.fetchCloud(maps.first, got_s, copy);
        km.fetchCloud(maps.second, got_c, copy);
        const std::vector<int32_t> save_ids = km.lastGlobalIds();
        loop(save_ids, {{fs.data(), fo.data()}, {fc.data()}}, 2 * P.MAP_SURF_RES, want);
        ok = same_bits(got_s, want[0], "saveGlobalMap (surf + outlier)") && ok;
        ok = same_bits(got_c, want[1], "saveGlobalMap (corner)") && ok;
        if (pub_ids.empty() || pub_ids.size() >= size_t(n_saved) || save_ids.size() >= size_t(n_saved) || n_pub == 0 || got_s.size() == 0 || got_c.size() == 0) {
            std::printf("implausible run: %zu / %zu of %d keyframes selected, %zu + %zu + %zu records\n", pub_ids.size(), save_ids.size(), n_saved, n_pub, got_s.size(),
                        got_c.size());
            ok = false;
        }
        std::printf("globalmap selftest: %d keyframes, %zu (publish) / %zu (save) selected; maps of %zu, %zu + %zu records; the device maps %s the per-keyframe loop's\n",
                    n_saved, pub_ids.size(), save_ids.size(), n_pub, got_s.size(), got_c.size(), ok ? "equal" : "DIFFER FROM");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::printf("globalmap selftest: %s\n", e.what());
        return 1;
    }
}
