// SlidingWindowMap (the odometry's window kept in HBM: mlh_window_*) against the host-cloud loop it replaces (transformPointCloud + VoxelGrid per slot and
// LiDAR, MapIndex::setInputCloud, WindowFactorTable::addMatches with host clouds) on a second context: ten odometry frames of two LiDARs driven through
// Estimator::process's own sequence (estimator.cpp:485-527: INITIAL with its double slide, then NON_LINEAR); every frame whose window is full builds the local
// maps and the factor table both ways and ends in mlh_pure_odom_normal_eq: H, g, the cost and the residual count must be bit-equal.
// Usage: window_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

constexpr int NUM_OF_LASER = 2, WINDOW_SIZE = 3, OPT_WINDOW_SIZE = 2, N_SCANS = 16, N_FRAMES = 10;

// utility/CircularBuffer.h:61-67, 134-137, 186-197 -- what the host path keeps its clouds and poses in
template <class T> struct Circular {
    explicit Circular(size_t capacity) : buf(capacity) {}
    T &operator[](size_t i) { return buf[(start + i) % buf.size()]; }
    void push(const T &e)
    {
        const T copy = e;
        if (size < buf.size()) buf[size++] = copy;
        else { buf[start] = copy; start = (start + 1) % buf.size(); }
    }
    std::vector<T> buf;
    size_t size = 0, start = 0;
};

Pose body_pose(int k)
{
    Pose p;
    const double yaw = 0.02 * k;
    p.t_(0) = 0.35 * k; p.t_(1) = 0.1 * std::sin(0.4 * k); p.t_(2) = 0.0;
    p.q_.w = std::cos(yaw / 2); p.q_.z = std::sin(yaw / 2);
    return p;
}

// what LiDAR `pose_w_l` sees of a flat ground at z = -1.2 (surf) and of posts on a 3 m grid (corner), in its own frame, already thinned: intensity = ring-like
void scan_clouds(std::mt19937 &rng, const Pose &pose_w_l, int n_surf, int n_corner, PointICloud &surf, PointICloud &corner)
{
    std::uniform_real_distribution<double> u(-14.0, 14.0), h(-1.0, 2.0);
    std::normal_distribution<double> noise(0.0, 0.005);
    const Pose inv = poseInverse(pose_w_l);
    auto to_lidar = [&](double x, double y, double z, float intensity) {
        const double w[3] = {x, y, z};
        double r[3];
        detail::quat_rotate(inv.q_, w, r);
        PointI p;
        p.x = float(r[0] + inv.t_(0)); p.y = float(r[1] + inv.t_(1)); p.z = float(r[2] + inv.t_(2)); p.intensity = intensity;
        return p;
    };
    surf.clear(); corner.clear();
    for (int i = 0; i < n_surf; ++i) surf.push_back(to_lidar(pose_w_l.t_(0) + u(rng), pose_w_l.t_(1) + u(rng), -1.2 + noise(rng), float(i % N_SCANS)));
    for (int i = 0; i < n_corner; ++i) {
        const double gx = 3.0 * std::floor((pose_w_l.t_(0) + u(rng)) / 3.0) + 1.5, gy = 3.0 * std::floor((pose_w_l.t_(1) + u(rng)) / 3.0) + 1.5;
        corner.push_back(to_lidar(gx + noise(rng), gy + noise(rng), h(rng), float(i % N_SCANS)));
    }
}

bool same_bits(const WindowNormalEquations &a, const WindowNormalEquations &b)
{
    return a.D == b.D && a.n_residuals == b.n_residuals && std::memcmp(&a.cost, &b.cost, sizeof(double)) == 0 &&
           std::memcmp(a.JtJ.data(), b.JtJ.data(), a.JtJ.size() * sizeof(double)) == 0 && std::memcmp(a.Jtr.data(), b.Jtr.data(), a.Jtr.size() * sizeof(double)) == 0;
}

}  // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        std::mt19937 rng(17);
        std::vector<Pose> ext(NUM_OF_LASER);
        ext[1].t_(0) = 0.1; ext[1].t_(1) = -0.5; ext[1].t_(2) = 0.02;
        ext[1].q_.w = std::cos(0.05); ext[1].q_.z = std::sin(0.05);
        const int pivot_idx = WINDOW_SIZE - OPT_WINDOW_SIZE;
        const float ratio = 0.4 * std::min(2.0, std::max(0.75, 1.0 / 192 * float(N_SCANS * NUM_OF_LASER * WINDOW_SIZE)));      // cpp:1196

        Device dev_a, dev_b;
        SlidingWindowMap win(dev_a, NUM_OF_LASER, WINDOW_SIZE, N_SCANS);
        std::vector<Circular<PointICloud>> surf_stack(NUM_OF_LASER, Circular<PointICloud>(WINDOW_SIZE + 1)), corner_stack(NUM_OF_LASER, Circular<PointICloud>(WINDOW_SIZE + 1));
        Circular<Pose> Ps(WINDOW_SIZE + 1);
        auto slide = [&](size_t cnt) {
            win.slideWindow(cnt);
            Ps.push(Ps[cnt]);
            for (int n = 0; n < NUM_OF_LASER; ++n) { surf_stack[size_t(n)].push(surf_stack[size_t(n)][cnt]); corner_stack[size_t(n)].push(corner_stack[size_t(n)][cnt]); }
        };

        size_t cir_buf_cnt = 0;
        bool initial = true, ok = true;
        int n_problems = 0, n_res_total = 0;
        for (int k = 0; k < N_FRAMES; ++k) {
            Ps[cir_buf_cnt] = body_pose(k);
            for (int n = 0; n < NUM_OF_LASER; ++n) {
                PointICloud s, c;
                scan_clouds(rng, poseMul(Ps[cir_buf_cnt], ext[size_t(n)]), 2600 + 41 * k + 300 * n, 420 + 13 * k, s, c);
                surf_stack[size_t(n)][cir_buf_cnt] = s; corner_stack[size_t(n)][cir_buf_cnt] = c;
                win.setCloud(size_t(n), cir_buf_cnt, s, c);
            }
            if (initial) {                                                       // cpp:502-519
                slide(cir_buf_cnt);
                if (cir_buf_cnt < size_t(WINDOW_SIZE)) { ++cir_buf_cnt; if (cir_buf_cnt == size_t(WINDOW_SIZE)) slide(cir_buf_cnt); }
                if (cir_buf_cnt == size_t(WINDOW_SIZE)) initial = false;
                continue;
            }
            // NON_LINEAR: optimizeMap's inputs (cpp:1159-1266), then slideWindow
            const Pose pose_pivot = Ps[size_t(pivot_idx)];
            std::vector<std::vector<Pose>> pose_local(NUM_OF_LASER, std::vector<Pose>(WINDOW_SIZE + 1));
            for (int n = 0; n < NUM_OF_LASER; ++n)
                for (int i = 0; i <= WINDOW_SIZE; ++i) pose_local[size_t(n)][size_t(i)] = poseMul(poseMul(poseInverse(pose_pivot), Ps[size_t(i)]), ext[size_t(n)]);
            double pivot[7];
            pose_pivot.toParam(pivot);
            std::vector<std::array<double, 7>> frames(OPT_WINDOW_SIZE), exts(NUM_OF_LASER);
            for (int i = 0; i < OPT_WINDOW_SIZE; ++i) Ps[size_t(pivot_idx + 1 + i)].toParam(frames[size_t(i)].data());
            for (int n = 0; n < NUM_OF_LASER; ++n) ext[size_t(n)].toParam(exts[size_t(n)].data());

            // the device window
            WindowNormalEquations ne_dev, ne_host;
            {
                win.buildLocalMap(pose_local);
                WindowFactorTable table(dev_a);
                for (int n = 0; n < NUM_OF_LASER; ++n) {
                    win.useLocalMap(size_t(n));
                    for (int i = pivot_idx + 1; i <= WINDOW_SIZE; ++i)
                        for (int kind = 0; kind < 2; ++kind)
                            if (win.useFeatures(size_t(n), size_t(i), kind)) table.addStagedMatches(kind == MLH_SURF ? 's' : 'c', pose_local[size_t(n)][size_t(i)], i - pivot_idx, n);
                }
                evalWindowNormalEquations(dev_a, pivot, frames, exts, 0.1, ne_dev);
            }
            // the host-cloud path
            {
                WindowFactorTable table(dev_b);
                MapIndex<PointI> kd_surf(dev_b, MLH_SURF), kd_corner(dev_b, MLH_CORNER);
                for (int n = 0; n < NUM_OF_LASER; ++n) {
                    PointICloud map[2], map_ds[2];
                    for (int i = 0; i < WINDOW_SIZE; ++i) {
                        PointICloud t;
                        transformPointCloud(dev_b, surf_stack[size_t(n)][size_t(i)], t, pose_local[size_t(n)][size_t(i)]);
                        map[0].points.insert(map[0].points.end(), t.points.begin(), t.points.end());
                        transformPointCloud(dev_b, corner_stack[size_t(n)][size_t(i)], t, pose_local[size_t(n)][size_t(i)]);
                        map[1].points.insert(map[1].points.end(), t.points.begin(), t.points.end());
                    }
                    for (int kind = 0; kind < 2; ++kind) {
                        VoxelGrid f(dev_b);
                        f.setLeafSize(ratio, ratio, ratio);
                        f.setInputCloud(map[kind]);
                        f.filter(map_ds[kind]);
                    }
                    if (map_ds[0].size() != win.mapSize(size_t(n), MLH_SURF) || map_ds[1].size() != win.mapSize(size_t(n), MLH_CORNER)) {
                        std::printf("frame %d LiDAR %d: local maps of %zu + %zu points against %zu + %zu\n", k, n, win.mapSize(size_t(n), MLH_SURF),
                                    win.mapSize(size_t(n), MLH_CORNER), map_ds[0].size(), map_ds[1].size());
                        ok = false;
                    }
                    kd_surf.setInputCloud(map_ds[0]);
                    kd_corner.setInputCloud(map_ds[1]);
                    for (int i = pivot_idx + 1; i <= WINDOW_SIZE; ++i) {
                        table.addMatches(surf_stack[size_t(n)][size_t(i)], 's', pose_local[size_t(n)][size_t(i)], i - pivot_idx, n);
                        table.addMatches(corner_stack[size_t(n)][size_t(i)], 'c', pose_local[size_t(n)][size_t(i)], i - pivot_idx, n);
                    }
                }
                evalWindowNormalEquations(dev_b, pivot, frames, exts, 0.1, ne_host);
            }
            ++n_problems;
            n_res_total += ne_dev.n_residuals;
            if (!same_bits(ne_dev, ne_host)) {
                std::printf("frame %d: %d residuals, cost %.17g (device window) against %d, %.17g (host clouds)\n", k, ne_dev.n_residuals, ne_dev.cost, ne_host.n_residuals,
                            ne_host.cost);
                ok = false;
            }
            slide(cir_buf_cnt);
        }
        if (n_problems != N_FRAMES - WINDOW_SIZE || n_res_total < 1000 * n_problems) {
            std::printf("implausible run: %d window problems, %d residuals\n", n_problems, n_res_total);
            ok = false;
        }
        std::printf("window selftest: %d frames, %d window problems, %d residuals; %s\n", N_FRAMES, n_problems, n_res_total,
                    ok ? "device window equals the host-cloud path" : "the device window DIFFERS FROM the host-cloud path");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::printf("window selftest: %s\n", e.what());
        return 1;
    }
}
