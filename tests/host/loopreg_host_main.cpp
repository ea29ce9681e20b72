// m-loam_amd/csrc/loopreg_host.hpp in a program of its own (tests/test_loopreg_cases.py builds it with -fsanitize=address,undefined and runs it): option
// validation, the 0.2 rule with its NaN and its feature-per-point ratio, the acceptance test, the rigid inverse and the pose conversions on every branch of
// Eigen's matrix-to-quaternion conversion are checked here; with arguments it prints what the header makes of the caller's input, and the test holds those lines
// against its Python transcription of pose_graph.cpp:374-410 and against the restatement.
//   loopreg_host_main
//   loopreg_host_main select <que_index> <match_index> <history> <n_keyframes> [missing index ...]
//   loopreg_host_main chain <file of 48 doubles: T_ini, T_cur (= T_old), T_kf>
//   loopreg_host_main quat <file of 16 doubles: T>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>
#include "loopreg_host.hpp"

using namespace mlh;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool read_doubles(const char *path, double *out, size_t n)
{
    FILE *f = std::fopen(path, "rb");
    const bool ok = f && std::fread(out, sizeof(double), n, f) == n;
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    mlh_loop_opts o;
    loop_opts_defaults(o);
    CHECK(loop_opts_fault(o) == nullptr);
    CHECK(o.leaf_surf == 0.4f && o.leaf_corner == 0.4f && o.history_search_num == 20 && o.max_outer == 2 && o.max_lm_iterations == 5);
    CHECK(o.local_registration_threshold == 2000.0 && o.huber_delta == 1.0 && o.match_sq_dis_surf == 2.0f && o.match_sq_dis_corner == 5.0f);
    CHECK(o.plane_dis == 0.2 && o.line_eig_ratio == 3.f && o.min_match_ratio == 0.2);
    { mlh_loop_opts b = o; b.leaf_surf = 0.f; CHECK(loop_opts_fault(b)); b.leaf_surf = float(nan); CHECK(loop_opts_fault(b)); b.leaf_surf = float(inf); CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.leaf_corner = -0.4f; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.history_search_num = -1; CHECK(loop_opts_fault(b)); b.history_search_num = 0; CHECK(!loop_opts_fault(b)); b.history_search_num = 4097; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.max_outer = 0; CHECK(loop_opts_fault(b)); b.max_outer = LOOP_MAX_OUTER; CHECK(!loop_opts_fault(b)); b.max_outer = LOOP_MAX_OUTER + 1; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.max_lm_iterations = -1; CHECK(loop_opts_fault(b)); b.max_lm_iterations = 0; CHECK(!loop_opts_fault(b)); b.max_lm_iterations = 201; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.local_registration_threshold = nan; CHECK(loop_opts_fault(b)); b.local_registration_threshold = -1.0; CHECK(!loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.huber_delta = 0.0; CHECK(loop_opts_fault(b)); b.huber_delta = nan; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.match_sq_dis_surf = 0.f; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.match_sq_dis_corner = float(nan); CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.plane_dis = -0.1; CHECK(loop_opts_fault(b)); b.plane_dis = 0.0; CHECK(!loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.line_eig_ratio = -1.f; CHECK(loop_opts_fault(b)); }
    { mlh_loop_opts b = o; b.min_match_ratio = nan; CHECK(loop_opts_fault(b)); }

    // loop_registration.cpp:158-159 as written
    CHECK(loop_too_few_matches(0, 100, 0, 10, 0.2));
    CHECK(loop_too_few_matches(20, 100, 2, 10, 0.2));                // both exactly at 0.2: <=
    CHECK(!loop_too_few_matches(21, 100, 0, 10, 0.2));
    CHECK(!loop_too_few_matches(0, 100, 3, 10, 0.2));                // the corner ratio alone keeps the loop going
    CHECK(!loop_too_few_matches(0, 100, 20, 10, 0.2));               // ... it counts two features per point: 2.0
    CHECK(!loop_too_few_matches(0, 100, 0, 0, 0.2));                 // no corner data: 0 / 0 is NaN, NaN <= 0.2 is false
    CHECK(!loop_too_few_matches(0, 0, 0, 10, 0.2));
    CHECK(!loop_too_few_matches(0, 0, 0, 0, 0.2));
    CHECK(loop_accepted(2000.0, 2000.0) && !loop_accepted(2000.0000001, 2000.0) && !loop_accepted(1e7, 2000.0) && !loop_accepted(nan, 2000.0));

    // the conversions, one rotation per branch of the matrix-to-quaternion conversion (trace > 0; the largest diagonal entry at 0, 1, 2)
    const double qs[4][4] = {{0.1, -0.2, 0.3, 0.9273618495495704}, {0.9, 0.1, -0.2, 0.3741657386773941}, {0.1, 0.9, 0.2, 0.3741657386773941}, {-0.2, 0.1, 0.9, 0.3741657386773941}};
    for (int k = 0; k < 4; ++k) {
        double T[16] = {0}, q[4], pose[7], T2[16] = {0};
        T[15] = T2[15] = 1.0;
        loop_quat_to_mat(qs[k], T);
        T[3] = 1.5; T[7] = -2.5; T[11] = 0.25;
        loop_mat_to_quat(T, q);
        const double tr = T[0] + T[5] + T[10];
        CHECK(k == 0 ? tr > 0.0 : tr <= 0.0);
        for (int i = 0; i < 4; ++i) CHECK(std::fabs(q[i] - qs[k][i]) < 1e-12);
        loop_pose_of(T, pose);
        CHECK(pose[0] == 1.5 && pose[1] == -2.5 && pose[2] == 0.25 && pose[3] == q[0] && pose[6] == q[3]);
        loop_mat_of(pose, T2);
        for (int i = 0; i < 16; ++i) CHECK(std::fabs(T2[i] - T[i]) < 1e-12);
        double Ti[16], I[16];
        loop_rigid_inverse(T, Ti);
        loop_mat_mul(T, Ti, I);
        for (int i = 0; i < 16; ++i) CHECK(std::fabs(I[i] - (i % 5 == 0 ? 1.0 : 0.0)) < 1e-12);
    }
    {   // the windows (pose_graph.cpp:374-380, 398-404)
        const auto all = [](int) { return true; };
        CHECK((loop_data_window(2, 20, all) == std::vector<int>{0, 1, 2}));
        CHECK((loop_model_window(9, 7, 3, all) == std::vector<int>{4, 5, 6, 7, 8}));      // match_index + j == que_index - 1 kept, == que_index dropped
        CHECK(loop_data_window(5, 0, all) == std::vector<int>{5});
        CHECK(loop_model_window(0, 0, 20, all).empty());
    }

    if (argc >= 6 && std::string(argv[1]) == "select") {
        const int que = std::atoi(argv[2]), match = std::atoi(argv[3]), history = std::atoi(argv[4]), n = std::atoi(argv[5]);
        std::set<int> missing;
        for (int a = 6; a < argc; ++a) missing.insert(std::atoi(argv[a]));
        const auto has = [&](int i) { return i >= 0 && i < n && !missing.count(i); };
        std::printf("D");
        for (int i : loop_data_window(que, history, has)) std::printf(" %d", i);
        std::printf("\nM");
        for (int i : loop_model_window(que, match, history, has)) std::printf(" %d", i);
        std::printf("\n");
    } else if (argc == 3 && std::string(argv[1]) == "chain") {
        double m[48];
        if (!read_doubles(argv[2], m, 48)) { std::printf("cannot read %s\n", argv[2]); return 2; }
        float d[16], mo[16];
        loop_data_transform(m, m + 16, m + 32, d);
        loop_model_transform(m + 16, m + 32, mo);
        std::printf("CD");
        for (int i = 0; i < 16; ++i) std::printf(" %.9g", double(d[i]));
        std::printf("\nCM");
        for (int i = 0; i < 16; ++i) std::printf(" %.9g", double(mo[i]));
        std::printf("\n");
    } else if (argc == 3 && std::string(argv[1]) == "quat") {
        double T[16], pose[7], T2[16];
        if (!read_doubles(argv[2], T, 16)) { std::printf("cannot read %s\n", argv[2]); return 2; }
        loop_pose_of(T, pose);
        std::memcpy(T2, T, sizeof(T2));
        loop_mat_of(pose, T2);
        std::printf("Q");
        for (int i = 0; i < 7; ++i) std::printf(" %.17g", pose[i]);
        std::printf("\nR");
        for (int i = 0; i < 16; ++i) std::printf(" %.17g", T2[i]);
        std::printf("\n");
    }
    std::printf(failures ? "loopreg_host: %d FAILED\n" : "loopreg_host: ok\n", failures);
    return failures ? 1 : 0;
}
