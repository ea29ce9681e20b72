// m-loam_amd/csrc/fgr_host.hpp in a stand-alone program, built with -fsanitize=address,undefined and run directly (tests/test_fgr_cases.py): the hand-computed
// cases of that test file once more through the header alone, and with arguments the values the test compares with the restatement:
//   (none)                 the self-checks below
//   tuple <file> <n> <swapped> <scale> <max> <seed>    <file>: n x 6 f32 (p, q); prints "C <corres ...>" and "T <tuples> <trials>"
//   optimize <file> <n> <start_scale> <div> <max_corr> <iterations>     prints "M <16 floats>" and "K <cost> <cost_normalize> <ran>"
// Prints "fgr_host: ok" and returns 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "fgr_host.hpp"

using namespace mlh;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static std::vector<FgrPair> read_pairs(const char *path, int n)
{
    std::vector<float> v(size_t(n) * 6);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) { std::printf("cannot read %s\n", path); std::exit(2); }
    std::fclose(f);
    std::vector<FgrPair> p(static_cast<size_t>(n));
    for (int e = 0; e < n; ++e) { p[size_t(e)].i = p[size_t(e)].j = e; for (int d = 0; d < 3; ++d) { p[size_t(e)].p[d] = v[size_t(6 * e + d)]; p[size_t(e)].q[d] = v[size_t(6 * e + 3 + d)]; } }
    return p;
}

static void self_checks()
{
    // options
    mlh_fgr_opts o;
    fgr_opts_defaults(o);
    CHECK(fgr_opts_fault(o) == nullptr);
    CHECK(o.normal_radius == 1.0f && o.fpfh_radius == 1.5f && o.div_factor == 1.4 && o.use_absolute_scale == 1 && o.max_corr_dist == 0.025 && o.iteration_number == 64);
    CHECK(o.tuple_scale == 0.95f && o.tuple_max_cnt == 1000 && o.global_registration_threshold == 2.0 && o.seed == 1);
    { mlh_fgr_opts b = o; b.normal_radius = std::nanf(""); CHECK(std::string(fgr_opts_fault(b)) == "normal_radius"); }
    { mlh_fgr_opts b = o; b.fpfh_radius = 0.f; CHECK(std::string(fgr_opts_fault(b)) == "fpfh_radius"); }
    { mlh_fgr_opts b = o; b.div_factor = 1.0; CHECK(std::string(fgr_opts_fault(b)) == "div_factor"); }
    { mlh_fgr_opts b = o; b.use_absolute_scale = 2; CHECK(std::string(fgr_opts_fault(b)) == "use_absolute_scale"); }
    { mlh_fgr_opts b = o; b.max_corr_dist = 0.0; CHECK(std::string(fgr_opts_fault(b)) == "max_corr_dist"); }
    { mlh_fgr_opts b = o; b.iteration_number = -1; CHECK(std::string(fgr_opts_fault(b)) == "iteration_number"); }
    { mlh_fgr_opts b = o; b.tuple_scale = 1.01f; CHECK(std::string(fgr_opts_fault(b)) == "tuple_scale"); }
    { mlh_fgr_opts b = o; b.tuple_max_cnt = 0; CHECK(std::string(fgr_opts_fault(b)) == "tuple_max_cnt"); }
    { mlh_fgr_opts b = o; b.global_registration_threshold = std::nan(""); CHECK(std::string(fgr_opts_fault(b)) == "global_registration_threshold"); }
    // the radius is strict: a neighbour exactly at distance r is excluded
    CHECK(!(fgr_sqdist3(0, 0, 0, 1, 0, 0) < 1.0f * 1.0f) && fgr_sqdist3(0, 0, 0, 0.99999994f, 0, 0) < 1.0f);
    // a 5 x 5 planar patch at z = 2: normal -z (flipped towards the origin), curvature 0
    {
        float a[9] = {0};
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) {
            const float x = 0.25f * float(i) - 0.5f, y = 0.25f * float(j) - 0.5f, z = 2.f;
            a[0] += x * x; a[1] += x * y; a[2] += x * z; a[3] += y * y; a[4] += y * z; a[5] += z * z; a[6] += x; a[7] += y; a[8] += z;
        }
        const float p[3] = {0.f, 0.f, 2.f};
        float out[4], ev[3], cf;
        fgr_normal_from_sums<float>(a, 25, p, out, ev, &cf);
        CHECK(std::fabs(out[0]) < 1e-6f && std::fabs(out[1]) < 1e-6f && out[2] < -0.999999f && out[3] < 1e-6f);
        CHECK(cf < 0.f);                                   // eigen33 returned +z: (0 - p) . n = -2, so the flip turned it
        fgr_normal_from_sums<float>(a, 2, p, out, ev, &cf);
        CHECK(std::isnan(out[0]) && std::isnan(out[1]) && std::isnan(out[2]) && std::isnan(out[3]));
    }
    // a pair with known features: p1 = 0, n1 = z; p2 = (1, 0, 0), n2 = (s, 0, c) with s = sin 0.5, c = cos 0.5: angle1 = 0, angle2 = s; acos(0) > acos(s): SWAP --
    // n1 = (s, 0, c), n2 = z, dp = -x, f3 = -s; v = dp x n1 = +y; w = n1 x v = (-c, 0, s); f2 = v . n2 = 0; f1 = atan2(w . n2, n1 . n2) = atan2(s, c) = 0.5.
    // The other way round (source (s, 0, c), target z) nothing swaps: f3 = +s, v = -y, w = (c, 0, -s), f1 = -0.5
    {
        const float p1[3] = {0, 0, 0}, n1[3] = {0, 0, 1}, p2[3] = {1, 0, 0}, n2[3] = {std::sin(0.5f), 0.f, std::cos(0.5f)};
        float f1, f2, f3;
        CHECK(fgr_pair_features<float>(p1, n1, p2, n2, f1, f2, f3));
        CHECK(std::fabs(f1 - 0.5f) < 1e-6f && f2 == 0.f && f3 == -n2[0]);
        CHECK(fgr_bin(fgr_unit_f1(f1)) == 6 && fgr_bin(fgr_unit_f23(f2)) == 5 && fgr_bin(fgr_unit_f23(f3)) == 2);      // 11 (0.5 + pi) / (2 pi) = 6.38; 11 (1 - s) / 2 = 2.86
        CHECK(fgr_pair_features<float>(p1, n2, p2, n1, f1, f2, f3));
        CHECK(std::fabs(f1 + 0.5f) < 1e-6f && f2 == 0.f && f3 == n2[0]);
        CHECK(fgr_bin(fgr_unit_f1(f1)) == 4 && fgr_bin(fgr_unit_f23(f2)) == 5 && fgr_bin(fgr_unit_f23(f3)) == 8);      // 11 (pi - 0.5) / (2 pi) = 4.62; 11 (1 + s) / 2 = 8.14
        CHECK(!fgr_pair_features<float>(p1, n1, p1, n2, f1, f2, f3));                          // zero distance
        const float up[3] = {0, 0, 2};
        CHECK(!fgr_pair_features<float>(p1, n1, up, n1, f1, f2, f3));                          // dp parallel to n1: |v| = 0
        const float nn[3] = {std::nanf(""), 0, 0};
        CHECK(fgr_pair_features<float>(p1, nn, p2, n2, f1, f2, f3) && std::isnan(f1) && std::isnan(f2) && std::isnan(f3));
        CHECK(fgr_bin(fgr_unit_f1(f1)) == 0 && fgr_bin(fgr_unit_f23(f2)) == 0);                // NaN: bin 0
    }
    CHECK(fgr_bin(-0.2) == 0 && fgr_bin(0.0) == 0 && fgr_bin(1.0) == 10 && fgr_bin(1.3) == 10 && fgr_bin(0.5) == 5 && fgr_bin(10.0 / 11.0 + 1e-9) == 10);
    // count -> value: sequential f32 additions; k = 4: 100 / 3 three times is not 100
    {
        const float inc = 100.0f / 3.0f;
        CHECK(fgr_spfh_value(3, 4) == (inc + inc) + inc && fgr_spfh_value(0, 4) == 0.f && fgr_spfh_value(1, 2) == 100.f && fgr_spfh_value(0, 1) == 0.f);
    }
    CHECK(fgr_block_scale(0.f) == 0.f && fgr_block_scale(50.f) == 2.f && fgr_block_scale(3.f) == float(100.0 / 3.0));
    // FLANN's L2 order: groups of four, the 33rd alone
    {
        float a[33], b[33];
        for (int i = 0; i < 33; ++i) { a[i] = 0.1f * float(i) + 1e-3f * float(i * i); b[i] = 0.07f * float(33 - i); }
        float want = 0.f;
        for (int g = 0; g < 32; g += 4) {
            const float d0 = a[g] - b[g], d1 = a[g + 1] - b[g + 1], d2 = a[g + 2] - b[g + 2], d3 = a[g + 3] - b[g + 3];
            want += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
        want += (a[32] - b[32]) * (a[32] - b[32]);
        CHECK(fgr_l2_33(a, b) == want);
        CHECK(fgr_row_finite(a));
        a[32] = std::nanf(""); CHECK(!fgr_row_finite(a));
        a[32] = 0.f; a[0] = HUGE_VALF; CHECK(!fgr_row_finite(a));
    }
    // the generator: deterministic, 31 bits, seeds differ
    {
        FgrRng r1(1), r2(1), r3(2);
        bool same = true, differ = false, in_range = true;
        for (int i = 0; i < 1000; ++i) { const uint32_t a = r1.next(), b = r2.next(), c = r3.next(); same = same && a == b; differ = differ || a != c; in_range = in_range && a < (1u << 31); }
        CHECK(same && differ && in_range);
    }
    // 20 exact correspondences of a rigid motion: OptimizePairwise recovers it
    {
        double R[9];
        fgr_zyx_rotation(0.1, -0.2, 0.3, R);
        std::vector<FgrPair> pr(20);
        std::vector<int32_t> c(20);
        FgrRng rng(5);
        for (int e = 0; e < 20; ++e) {
            c[size_t(e)] = e;
            FgrPair &r = pr[size_t(e)];
            r.i = r.j = e;
            for (int d = 0; d < 3; ++d) r.q[d] = float(rng.next() % 2000u) * 1e-3f - 1.f;
            for (int d = 0; d < 3; ++d) r.p[d] = float(R[3 * d] * r.q[0] + R[3 * d + 1] * r.q[1] + R[3 * d + 2] * r.q[2] + (d == 0 ? 0.3 : d == 1 ? -0.2 : 0.1));
        }
        const FgrTail t = fgr_optimize_pairwise(pr, c, 2.0, 1.4, 0.025, 64);
        CHECK(t.optimised && t.final_cost_normalize < 1e-9);
        for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) CHECK(std::fabs(double(t.trans[r * 4 + k]) - R[3 * r + k]) < 1e-5);
        CHECK(std::fabs(t.trans[3] - 0.3f) < 1e-5f && std::fabs(t.trans[7] + 0.2f) < 1e-5f && std::fabs(t.trans[11] - 0.1f) < 1e-5f);
        // GetOutputTrans: t = -R m1 + t G + m0
        const float m0[3] = {1.f, 2.f, 3.f}, m1[3] = {0.f, 0.f, 0.f};
        double T[16];
        fgr_output_trans(t.trans, m0, m1, 1.f, T);
        CHECK(T[3] == double(t.trans[3] + 1.f) && T[7] == double(t.trans[7] + 2.f) && T[15] == 1.0 && T[12] == 0.0);
        // nine correspondences: nothing runs
        c.resize(9);
        const FgrTail few = fgr_optimize_pairwise(pr, c, 2.0, 1.4, 0.025, 64);
        CHECK(!few.optimised && std::isnan(few.final_cost_normalize) && few.trans[0] == 1.f && few.trans[1] == 0.f && few.trans[3] == 0.f);
        // the whole tail with no pair at all
        mlh_fgr_opts o2;
        fgr_opts_defaults(o2);
        mlh_fgr_result res;
        std::memset(&res, 0, sizeof(res));
        fgr_host_tail(std::vector<FgrPair>(), false, m0, m1, 1.f, 2.f, o2, res);
        CHECK(res.accepted == 0 && res.n_mutual == 0 && res.n_corres == 0 && res.n_trials == 0 && std::isnan(res.final_cost_normalize) && res.T_relative[3] == 1.0);
    }
}

int main(int argc, char **argv)
{
    if (argc >= 8 && std::string(argv[1]) == "tuple") {
        const std::vector<FgrPair> p = read_pairs(argv[2], std::atoi(argv[3]));
        std::vector<int32_t> c;
        int trials = 0;
        const int cnt = fgr_tuple_test(p, std::atoi(argv[4]) != 0, float(std::atof(argv[5])), std::atoi(argv[6]), std::strtoull(argv[7], nullptr, 10), c, &trials);
        std::printf("C");
        for (int32_t v : c) std::printf(" %d", v);
        std::printf("\nT %d %d\n", cnt, trials);
    } else if (argc >= 8 && std::string(argv[1]) == "optimize") {
        const int n = std::atoi(argv[3]);
        const std::vector<FgrPair> p = read_pairs(argv[2], n);
        std::vector<int32_t> c(static_cast<size_t>(n));
        for (int e = 0; e < n; ++e) c[size_t(e)] = e;
        const FgrTail t = fgr_optimize_pairwise(p, c, std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6]), std::atoi(argv[7]));
        std::printf("M");
        for (int i = 0; i < 16; ++i) std::printf(" %.9g", double(t.trans[i]));
        std::printf("\nK %.17g %.17g %d\n", t.final_cost, t.final_cost_normalize, t.optimised ? 1 : 0);
    } else
        self_checks();
    if (failures) return 1;
    std::printf("fgr_host: ok\n");
    return 0;
}
