// The arithmetic of one Scan Context keyframe as a plain single-threaded C++ loop on the host CPU, for comparison with the device (scripts/scbench.py compiles and
// runs it): makeScancontext of one cloud + the keys ("add"), and the exact key search over N entries + alignment and column cosines of the candidates + the
// ordered argmin ("detect"), with the shared per-point arithmetic of m-loam_amd/csrc/sc_host.hpp. No heap allocation per shift (the reference's MatrixXd copies are
// not imitated: this is the arithmetic alone).
//   scbench_cpu N_ENTRIES N_POINTS REPS   -> one JSON line
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "sc_host.hpp"

using namespace mlh;
constexpr int R = 20, S = 60, K = 50;

struct Entry { std::vector<float> desc; float ring[R]; double sector[S], norm[S]; };

static void finish(Entry &e)
{
    for (int r = 0; r < R; ++r) { double a = 0; for (int c = 0; c < S; ++c) a += e.desc[size_t(c) * R + r]; e.ring[r] = float(a / S); }
    for (int c = 0; c < S; ++c) { double a = 0, q = 0; for (int r = 0; r < R; ++r) { const double v = e.desc[size_t(c) * R + r]; a += v; q += v * v; } e.sector[c] = a / R; e.norm[c] = std::sqrt(q); }
}

static Entry make(const std::vector<float> &pts)
{
    Entry e;
    std::vector<int> grid(size_t(R) * S, sc_encode(SC_NO_POINT));
    for (size_t i = 0; i + 2 < pts.size(); i += 3) {
        const float x = pts[i], y = pts[i + 1], z = pts[i + 2];
        const float range = sc_range(x, y);
        if (double(range) > 80.0) continue;
        const int b = sc_bin(sc_ring(range, 80.0, R), sc_sector(sc_sector_value(sc_xy2theta(x, y), S), S), R);
        grid[size_t(b)] = std::max(grid[size_t(b)], sc_encode(sc_height(z, 2.0)));
    }
    e.desc.resize(grid.size());
    for (size_t b = 0; b < grid.size(); ++b) { const float v = sc_decode(grid[b]); e.desc[b] = v == SC_NO_POINT ? 0.f : v; }
    finish(e);
    return e;
}

static double detect(const std::vector<Entry> &db, const Entry &q, int *idx_out)
{
    std::vector<std::pair<float, int>> d(db.size());
    for (size_t i = 0; i < db.size(); ++i) {
        float res = 0.f;
        int k = 0;
        for (; k + 3 < R; k += 4) {
            const float d0 = q.ring[k] - db[i].ring[k], d1 = q.ring[k + 1] - db[i].ring[k + 1], d2 = q.ring[k + 2] - db[i].ring[k + 2], d3 = q.ring[k + 3] - db[i].ring[k + 3];
            res += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
        for (; k < R; ++k) { const float d0 = q.ring[k] - db[i].ring[k]; res += d0 * d0; }
        d[i] = std::make_pair(res, int(i));
    }
    const size_t k = std::min<size_t>(K, d.size());
    std::partial_sort(d.begin(), d.begin() + long(k), d.end());
    const int radius = sc_search_radius(0.1, S);
    double min_dist = 1e7;
    int nn = -1;
    for (size_t ci = 0; ci < k; ++ci) {
        const Entry &c = db[size_t(d[ci].second)];
        double best = 1e7;
        int align = 0;
        for (int s = 0; s < S; ++s) {
            double sq = 0;
            for (int col = 0; col < S; ++col) { const double t = q.sector[col] - c.sector[(col - s + S) % S]; sq += t * t; }
            const double nrm = std::sqrt(sq);
            if (nrm < best) { best = nrm; align = s; }
        }
        double cbest = 1e7;
        std::vector<int> space;
        for (int j = -radius; j <= radius; ++j) space.push_back(((align + j) % S + S) % S);
        std::sort(space.begin(), space.end());
        for (int s : space) {
            double sum = 0;
            int n = 0;
            for (int col = 0; col < S; ++col) {
                const int cc = (col - s + S) % S;
                if (q.norm[col] == 0 || c.norm[cc] == 0) continue;
                double dot = 0;
                for (int r = 0; r < R; ++r) dot += double(q.desc[size_t(col) * R + r]) * double(c.desc[size_t(cc) * R + r]);
                sum += dot / (q.norm[col] * c.norm[cc]);
                ++n;
            }
            const double dist = 1.0 - sum / n;
            if (dist < cbest) cbest = dist;
        }
        if (cbest < min_dist) { min_dist = cbest; nn = d[ci].second; }
    }
    *idx_out = nn;
    return min_dist;
}

int main(int argc, char **argv)
{
    const int n_entries = argc > 1 ? std::atoi(argv[1]) : 1000, n_points = argc > 2 ? std::atoi(argv[2]) : 120000, reps = argc > 3 ? std::atoi(argv[3]) : 10;
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> u(-85.f, 85.f), uz(-2.f, 10.f);
    auto cloud = [&](int n) { std::vector<float> p(size_t(n) * 3); for (int i = 0; i < n; ++i) { p[3 * size_t(i)] = u(rng); p[3 * size_t(i) + 1] = u(rng); p[3 * size_t(i) + 2] = uz(rng); } return p; };
    std::vector<Entry> db;
    for (int i = 0; i < n_entries; ++i) db.push_back(make(cloud(600)));
    const std::vector<float> big = cloud(n_points);
    std::vector<double> t_add, t_det;
    double sink = 0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        const Entry q = make(big);
        const auto t1 = std::chrono::steady_clock::now();
        int idx;
        sink += detect(db, q, &idx) + idx;
        const auto t2 = std::chrono::steady_clock::now();
        t_add.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        t_det.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::sort(t_add.begin(), t_add.end());
    std::sort(t_det.begin(), t_det.end());
    std::printf("{\"entries\": %d, \"points\": %d, \"reps\": %d, \"add_median_ms\": %.4f, \"detect_median_ms\": %.4f, \"sink\": %.3f}\n", n_entries, n_points, reps,
                t_add[t_add.size() / 2], t_det[t_det.size() / 2], sink);
    return 0;
}
