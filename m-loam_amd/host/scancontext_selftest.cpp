// The front of PoseGraph::detectLoop through the facade (SCManager::setParameter, makeAndSaveScancontextAndKeys, detectLoopClosureID, getDataBaseSize,
// distanceBtnScanContext, fetchScanContext and the detectLoop helper) against the plain C-ABI calls (mlh_sc_reset, mlh_sc_add, mlh_sc_detect, mlh_sc_distance,
// mlh_sc_fetch) on a second context: 40 keyframes of a scene of pillars along a straight road, the last 12 driving it again with the heading turned by five
// sectors and one of them reported far away. Every result must be equal, the revisits must be found with the shift the turn implies, the far one must be
// rejected by distance, and a descriptor must be the maximum of z + lidar_height per cell as a plain loop over the cloud makes it.
// Usage: scancontext_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

struct Pillar { double x, y, h; };

// the scene from (px, py) with heading `yaw`, in the sensor frame; points on the axes and near sector edges are as good as any here: both sides call the library
PointICloud scan_of(const std::vector<Pillar> &w, double px, double py, double yaw, double lidar_height, std::mt19937 &rng)
{
    std::normal_distribution<double> g(0.0, 0.02);
    const double c = std::cos(yaw), s = std::sin(yaw);
    PointICloud cloud;
    for (const Pillar &p : w)
        for (int k = 1; k <= 6; ++k) {
            const double dx = p.x - px, dy = p.y - py;
            PointI q;
            q.x = float(c * dx + s * dy + g(rng)); q.y = float(-s * dx + c * dy + g(rng)); q.z = float(p.h * k / 6.0 - lidar_height);
            cloud.push_back(q);
        }
    return cloud;
}

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

}  // namespace

int main()
{
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> ux(-150.0, 150.0), uy(-45.0, 45.0), uh(0.5, 9.0);
    std::vector<Pillar> world;
    for (int i = 0; i < 170; ++i) world.push_back(Pillar{ux(rng), uy(rng), uh(rng)});

    Device dev_a(0), dev_b(0);
    SCManager sc(dev_a);
    const int R = 20, S = 60, EXCLUDE = 5;
    sc.setParameter(2.0, R, S, 80.0, 360.0 / S, 80.0 / R, EXCLUDE, 4, 0.1, 0.5, 3, 30.0);
    mlh_sc_opts o = sc.options();
    dev_b.check(mlh_sc_reset(dev_b.ctx(), &o));

    int found = 0, rejected = 0;
    for (int i = 0; i < 40; ++i) {
        const bool again = i >= 28;
        const double px = again ? -40.0 + 3.0 * (i - 28) + 0.2 : -40.0 + 3.0 * i, py = again ? 0.1 : 0.0, yaw = again ? 5 * 2.0 * M_PI / S : 0.0;
        const PointICloud full = scan_of(world, px, py, yaw, 2.0, rng);
        PointICloud outlier;
        for (int k = 0; k < 40; ++k) { PointI q; q.x = float(ux(rng) / 4); q.y = float(uy(rng)); q.z = -1.9f; outlier.push_back(q); }
        const double t[3] = {px, i == 33 ? py + 31.0 : py, 0.0};          // keyframe 33 claims to be 31 m to the side
        const std::pair<int, double> lp = detectLoop(sc, full, outlier, t, i);
        const mlh_sc_result fa = sc.lastResult();
        const void *clouds[2] = {full.points.data(), outlier.points.data()};
        const int32_t n[2] = {int32_t(full.size()), int32_t(outlier.size())};
        int32_t idx = -1;
        dev_b.check(mlh_sc_add(dev_b.ctx(), clouds, n, 2, int(sizeof(PointI)), MLH_MEM_HOST, t, &idx));
        mlh_sc_result rb;
        dev_b.check(mlh_sc_detect(dev_b.ctx(), i, &rb));
        EXPECT(idx == i && int(sc.getDataBaseSize()) == i + 1);
        EXPECT(fa.match_index == rb.match_index && fa.nearest_index == rb.nearest_index && fa.shift == rb.shift && fa.score == rb.score &&
               fa.yaw_diff_rad == rb.yaw_diff_rad && fa.n_candidates_scored == rb.n_candidates_scored && fa.rejected_by_distance == rb.rejected_by_distance);
        EXPECT(lp.first == rb.match_index && lp.second == double(rb.yaw_diff_rad));
        if (i <= EXCLUDE) EXPECT(rb.match_index == -1 && rb.score == -1.0 && rb.n_candidates_scored == 0);
        if (again && i != 33) { EXPECT(rb.match_index == i - 28 && rb.shift == S - 5); found += rb.match_index == i - 28; }
        if (i == 33) { EXPECT(rb.match_index == -1 && rb.nearest_index == 5 && rb.rejected_by_distance == 1); rejected += rb.rejected_by_distance; }
        if (i == 39) {
            // the descriptor against a plain loop (points in the library's band fall on either side of an edge by ulps: compare only cells no such point touches)
            std::vector<double> want(size_t(R) * S, -1000.0), got = sc.fetchScanContext(i);
            std::vector<char> unsure(size_t(R) * S, 0);
            const PointICloud *both[2] = {&full, &outlier};
            for (const PointICloud *c : both)
                for (const PointI &p : c->points) {
                    const double range = std::sqrt(double(p.x) * p.x + double(p.y) * p.y);
                    if (range > 80.0) continue;
                    double ang = std::atan2(double(p.y), double(p.x)) * 180.0 / M_PI;
                    if (ang < 0) ang += 360.0;
                    const double sv = ang / 360.0 * S, rv = range / 80.0 * R;
                    const int ring = std::max(std::min(R, int(std::ceil(rv))), 1), sector = std::max(std::min(S, int(std::ceil(sv))), 1);
                    const size_t cell = size_t(sector - 1) * R + size_t(ring - 1);
                    if (std::fabs(sv - std::rint(sv)) < 1e-3 || std::fabs(rv - std::rint(rv)) < 1e-4) {
                        unsure[cell] = 1;
                        for (int ds = -1; ds <= 1; ++ds) for (int dr = -1; dr <= 1; ++dr) {
                            const int s2 = (sector - 1 + ds + S) % S, r2 = ring - 1 + dr;
                            if (r2 >= 0 && r2 < R) unsure[size_t(s2) * R + size_t(r2)] = 1;
                        }
                        continue;
                    }
                    want[cell] = std::max(want[cell], double(float(double(p.z) + 2.0)));
                }
            int compared = 0;
            for (size_t b = 0; b < want.size(); ++b) {
                if (unsure[b]) continue;
                EXPECT(got[b] == (want[b] == -1000.0 ? 0.0 : want[b]));
                ++compared;
            }
            EXPECT(compared > 1000);
            const std::pair<double, int> d = sc.distanceBtnScanContext(i, i - 28);
            double d2 = 0.0; int32_t s2 = 0;
            dev_b.check(mlh_sc_distance(dev_b.ctx(), i, i - 28, &d2, &s2));
            EXPECT(d.first == d2 && d.second == s2 && d.first == rb.score && d.second == rb.shift);
        }
    }
    EXPECT(found == 11 && rejected == 1);
    mlh_sc_store_info info;
    dev_a.check(mlh_sc_info(dev_a.ctx(), &info));
    std::printf("scancontext_selftest: %d entries, %d revisits found, %d rejected by distance, %lld points decided on the host, %lld bytes in HBM: %s\n", info.n_entries, found,
                rejected, (long long)info.points_host_decided, (long long)info.bytes_hbm, fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
