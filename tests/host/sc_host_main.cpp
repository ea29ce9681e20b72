// m-loam_amd/csrc/sc_host.hpp in a program of its own (tests/test_sc_cases.py builds it with -fsanitize=address,undefined and runs it): option validation, the
// searched-prefix / period bookkeeping, the integer encoding of f32, the yaw conversion and the distance rejection are checked here; with a file of float32
// xyz records as argument it also prints, per point, what the header's arithmetic makes of it -- the test holds those lines against the NumPy restatement.
//   sc_host_main [points.f32 n max_radius lidar_height R S]
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "sc_host.hpp"

using namespace mlh;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main(int argc, char **argv)
{
    mlh_sc_opts o{};
    o.lidar_height = 2.0; o.num_ring = 20; o.num_sector = 60; o.max_radius = 80.0; o.num_exclude_recent = 3; o.num_candidates = 3; o.search_ratio = 0.1;
    o.dist_thres = 0.5; o.tree_making_period = 4; o.loop_distance_threshold = 50.0;
    CHECK(sc_opts_fault(o) == nullptr);
    { mlh_sc_opts b = o; b.num_ring = 0; CHECK(sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.num_sector = 0; CHECK(sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.num_ring = 128; b.num_sector = 65; CHECK(sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.num_ring = 64; b.num_sector = 128; CHECK(!sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.num_ring = 2147483647; b.num_sector = 2147483647; CHECK(sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.num_candidates = 0; CHECK(sc_opts_fault(b)); b.num_candidates = 257; CHECK(sc_opts_fault(b)); b.num_candidates = 256; CHECK(!sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.max_radius = 0.0; CHECK(sc_opts_fault(b)); b.max_radius = -1.0; CHECK(sc_opts_fault(b)); b.max_radius = std::numeric_limits<double>::infinity(); CHECK(sc_opts_fault(b));
      b.max_radius = std::numeric_limits<double>::quiet_NaN(); CHECK(sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.tree_making_period = 0; CHECK(sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.num_exclude_recent = -1; CHECK(sc_opts_fault(b)); b.num_exclude_recent = 0; CHECK(!sc_opts_fault(b)); }
    { mlh_sc_opts b = o; b.loop_distance_threshold = -1.0; CHECK(!sc_opts_fault(b)); }

    // the encoding keeps the order and inverts
    const float vals[] = {-std::numeric_limits<float>::infinity(), -1200.f, -1000.f, -1.f, -1e-30f, 0.f, 1e-30f, 1.f, 999.5f, std::numeric_limits<float>::infinity()};
    for (size_t i = 0; i + 1 < sizeof(vals) / sizeof(vals[0]); ++i) CHECK(sc_encode(vals[i]) < sc_encode(vals[i + 1]));
    for (float v : vals) CHECK(sc_decode(sc_encode(v)) == v);
    CHECK(sc_encode(sc_height(-0.f, 0.0)) == 0);

    // the period bookkeeping: early returns do not count; the prefix is the one of the last rebuild
    ScBook b;
    std::vector<int> prefixes;
    for (int que = 0; que < 14; ++que) {
        if (sc_early_return(que, o)) { CHECK(que < 4); continue; }
        prefixes.push_back(sc_book_query(b, que, o));
    }
    const int want[10] = {1, 1, 1, 1, 5, 5, 5, 5, 9, 9};
    CHECK(prefixes.size() == 10);
    for (size_t i = 0; i < prefixes.size() && i < 10; ++i) CHECK(prefixes[i] == want[i]);
    CHECK(b.counter == 10);

    CHECK(sc_search_radius(0.1, 60) == 3 && sc_search_radius(0.1, 7) == 0 && sc_search_radius(0.1, 128) == 6 && sc_search_radius(0.5, 5) == 1 && sc_search_radius(100.0, 60) == 60);
    CHECK(sc_yaw(0, 60) == 0.f && sc_yaw(55, 60) == 5.759586334228516f && sc_yaw(3, 60) == 0.3141592741012573f);
    const double p0[3] = {0, 0, 0}, p1[3] = {30, 40, 0};
    CHECK(sc_too_far(p0, p1, 49.9) && !sc_too_far(p0, p1, 50.0) && !sc_too_far(p0, p1, -1.0));
    CHECK(sc_ring(80.f, 80.0, 20) == 20 && sc_ring(0.f, 80.0, 20) == 1 && sc_ring(4.f, 80.0, 20) == 1 && sc_ring(4.0000005f, 80.0, 20) == 2);
    CHECK(sc_sector(std::numeric_limits<double>::quiet_NaN(), 60) == 1 && sc_sector(-15.0, 60) == 1 && sc_sector(75.0, 60) == 60 && sc_sector(0.0, 60) == 1 && sc_sector(59.2, 60) == 60);
    CHECK(sc_bin(1, 1, 20) == 0 && sc_bin(20, 60, 20) == 1199);

    if (argc == 7) {
        const int n = std::atoi(argv[2]), R = std::atoi(argv[5]), S = std::atoi(argv[6]);
        const double max_radius = std::atof(argv[3]), h = std::atof(argv[4]);
        std::vector<float> pts(size_t(n) * 3);
        FILE *f = std::fopen(argv[1], "rb");
        if (!f || std::fread(pts.data(), sizeof(float), pts.size(), f) != pts.size()) { std::printf("cannot read %s\n", argv[1]); return 2; }
        std::fclose(f);
        for (int i = 0; i < n; ++i) {
            const float x = pts[3 * size_t(i)], y = pts[3 * size_t(i) + 1], z = pts[3 * size_t(i) + 2];
            const float range = sc_range(x, y);
            if (double(range) > max_radius) { std::printf("P %d out\n", i); continue; }
            const double sv = sc_sector_value(sc_xy2theta(x, y), S);
            std::printf("P %d %d %d %d %d\n", i, sc_ring(range, max_radius, R), sc_sector(sv, S), sc_in_band(sv) ? 1 : 0, sc_encode(sc_height(z, h)));
        }
    }
    std::printf(failures ? "sc_host: %d FAILED\n" : "sc_host: ok\n", failures);
    return failures ? 1 : 0;
}
