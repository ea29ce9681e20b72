// TEST INFRASTRUCTURE ONLY. m-loam_amd/csrc/pg_host.hpp (the arithmetic of one pose-graph edge, shared by the kernels and the host) in a stand-alone program, so
// that tests/test_pg_cases.py can build it with -fsanitize=address,undefined and run it directly.
//   (no argument)        the header's own checks: option defaults and validation, an exact measurement gives a zero residual, pose * pose^-1, Plus with a zero step,
//                        the sequential measurement makes its own edge's residual vanish, Huber on both sides of delta
//   edge <file>          21 doubles (pose_i, pose_j, measurement) -> "R" 6 residuals, "I" 36 of Ji, "J" 36 of Jj (t_var 0.1, q_var 0.01)
//   plus <file>          13 doubles (pose, delta) -> "P" 7
//   compose <file>       14 doubles (a, b) -> "M" 7 of a * b, "V" 7 of a^-1, "S" 7 of the sequential measurement (prev = a, cur = b)
#include "pg_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mlh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("pg_host: CHECK FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static std::vector<double> read_doubles(const char *path, size_t n)
{
    std::vector<double> v(n, 0.0);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(double), n, f) != n) { std::printf("pg_host: cannot read %s\n", path); std::exit(2); }
    std::fclose(f);
    return v;
}

static void print_row(const char *tag, const double *v, int n)
{
    std::printf("%s", tag);
    for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
    std::printf("\n");
}

static void self_checks()
{
    mlh_pg_opts o;
    pg_opts_defaults(o);
    CHECK(o.max_num_iterations == 5 && o.n_sequential == 4 && o.t_var == 0.1 && o.q_var == 0.01 && o.huber_delta == 1.0);
    CHECK(pg_opts_fault(o) == nullptr);
    mlh_pg_opts b = o;
    b.t_var = 0.0; CHECK(pg_opts_fault(b) != nullptr);
    b = o; b.q_var = NAN; CHECK(pg_opts_fault(b) != nullptr);
    b = o; b.n_sequential = 3; CHECK(pg_opts_fault(b) != nullptr);
    b = o; b.max_num_iterations = -1; CHECK(pg_opts_fault(b) != nullptr);
    b = o; b.huber_delta = -1.0; CHECK(pg_opts_fault(b) != nullptr);

    const double id[7] = {0, 0, 0, 0, 0, 0, 1};
    double r[6], Ji[36], Jj[36];
    pg_edge_eval(id, id, id, 0.1, 0.01, r, Ji, Jj);
    for (int c = 0; c < 6; ++c) CHECK(r[c] == 0.0);
    for (int a = 0; a < 3; ++a) {
        CHECK(std::fabs(Jj[6 * a + 3 + a] - 10.0) < 1e-13 && std::fabs(Ji[6 * a + 3 + a] + 10.0) < 1e-13);
        CHECK(std::fabs(Jj[6 * (3 + a) + a] - 200.0) < 1e-12 && std::fabs(Ji[6 * (3 + a) + a] + 200.0) < 1e-12);
    }
    pg_edge_eval(id, id, id, 0.1, 0.01, r, nullptr, nullptr);

    const double a[7] = {1.0, -2.0, 0.5, 0.1825741858350554, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214};
    const double c[7] = {2.0, -1.5, 0.7, -0.5, 0.5, 0.5, 0.5};
    double inv[7], prod[7], m[7];
    pg_pose_inverse(a, inv);
    pg_pose_mul(a, inv, prod);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(prod[k]) < 1e-15);
    CHECK(std::fabs(std::fabs(prod[6]) - 1.0) < 1e-15);
    pg_sequential_measurement(a, c, m);
    pg_edge_eval(a, c, m, 0.1, 0.01, r, Ji, Jj);
    for (int k = 0; k < 6; ++k) CHECK(std::fabs(r[k]) < 1e-12);
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    double out[7];
    pg_plus(a, zero, out);
    CHECK(std::memcmp(out, a, sizeof(out)) == 0);
    double rho = 0.0;
    CHECK(pg_huber(0.25, 1.0, &rho) == 1.0 && rho == 0.25);
    const double sc = pg_huber(4.0, 1.0, &rho);
    CHECK(rho == 3.0 && std::fabs(sc - std::sqrt(0.5)) < 1e-16);
}

int main(int argc, char **argv)
{
    if (argc == 1) {
        self_checks();
    } else if (argc == 3 && std::strcmp(argv[1], "edge") == 0) {
        const std::vector<double> v = read_doubles(argv[2], 21);
        double r[6], Ji[36], Jj[36];
        pg_edge_eval(&v[0], &v[7], &v[14], 0.1, 0.01, r, Ji, Jj);
        print_row("R", r, 6); print_row("I", Ji, 36); print_row("J", Jj, 36);
    } else if (argc == 3 && std::strcmp(argv[1], "plus") == 0) {
        const std::vector<double> v = read_doubles(argv[2], 13);
        double out[7];
        pg_plus(&v[0], &v[7], out);
        print_row("P", out, 7);
    } else if (argc == 3 && std::strcmp(argv[1], "compose") == 0) {
        const std::vector<double> v = read_doubles(argv[2], 14);
        double m[7], inv[7], s[7];
        pg_pose_mul(&v[0], &v[7], m);
        pg_pose_inverse(&v[0], inv);
        pg_sequential_measurement(&v[0], &v[7], s);
        print_row("M", m, 7); print_row("V", inv, 7); print_row("S", s, 7);
    } else {
        std::printf("usage: pg_host_main [edge|plus|compose <file>]\n");
        return 2;
    }
    if (failures) return 1;
    std::printf("pg_host: ok\n");
    return 0;
}
