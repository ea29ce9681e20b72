// TEST INFRASTRUCTURE ONLY. The host side of the pose graph's marginal covariances (m-loam_amd/csrc/pg_marg_host.hpp: the launch plan, the buffer sizes, the window
// indexing of the band's selected inversion, the conversion to the keyframe store's convention) in a stand-alone program, so that tests/test_pg_marg_cases.py can
// build it with -fsanitize=address,undefined and run it directly. Checked:
//   launches   pgm_launches(M, L) for every L = 0 .. the limit: 4 for M == 1; else 14 up to L = 128 and 13 + 3 ceil(6 L / 64) beyond, the same for every M >= 2
//   buffers    both forms 72 M doubles; the band's inverse 180 (M - 1); the packed factor (ceil(6 L / 64) 64)^2 up to 128 loops and nothing beyond; the factor
//              lies behind the band's inverse, aligned, inside pgm_work_doubles
//   window     for NB = 1 .. 12 blocks: Takahashi's recursion replayed on a random block-banded SPD matrix through a 25-slot window addressed by pgm_win_slot
//              exactly as pgm_selinv_kernel addresses it -- every slot read holds the block the recursion means (tagged), a slot is overwritten only when its
//              block has been read for the last time, and the blocks equal those of the dense inverse to 1e-10 of the largest entry
//   conversion pgm_to_store == A S A^T written out; symmetric to the bit; A is the first-order map from pg_plus's tangent to the left perturbation
//   (no argument)      everything; prints "pg_marg: ok"
//   count <M> <L>      "N <launches> <out> <band> <factor> <work>"
#include "pg_marg_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mlh;

static long failures = 0;
#define CHECK(cond) do { if (!(cond)) { if (failures < 20) std::printf("pg_marg: CHECK FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static double rnd(unsigned &s)
{
    s = s * 1664525u + 1013904223u;
    return double(s >> 8) / double(1u << 24) - 0.5;
}

static void check_plan()
{
    CHECK(PG_MAX_LOOPS == 128 && PG_PANEL == 64 && PG_SLOTS == 5);
    for (int L = 0; L <= int(MLH_PG_LOOPS_LIMIT); ++L) {
        CHECK(pgm_launches(1, L) == 4);
        const int want = L <= 128 ? 14 : 13 + 3 * ((6 * L + 63) / 64);
        for (int M : {2, 3, 7, 130, 6577}) CHECK(pgm_launches(M, L) == want);
        const size_t mp = pgm_panel_cols(L);
        CHECK(mp % 64 == 0 && mp >= size_t(6 * L) && mp < size_t(6 * L) + 64);
        CHECK(pgm_factor_doubles(L) == (L <= 128 ? mp * mp : 0));
        for (int M : {1, 2, 5, 131, 6577}) {
            CHECK(pgm_out_doubles(M) == size_t(72) * M);
            CHECK(pgm_band_doubles(M) == size_t(180) * (M - 1));
            CHECK(pgm_factor_offset(M) >= pgm_band_doubles(M) && pgm_factor_offset(M) % 16 == 0 && pgm_factor_offset(M) < pgm_band_doubles(M) + 16);
            CHECK(pgm_factor_offset(M) + pgm_factor_doubles(L) <= pgm_work_doubles(M, L));
        }
    }
}

// dense helpers over n x n row-major
static void chol(std::vector<double> &A, int n)
{
    for (int j = 0; j < n; ++j) {
        double p = A[size_t(j) * n + j];
        for (int q = 0; q < j; ++q) p -= A[size_t(j) * n + q] * A[size_t(j) * n + q];
        const double d = std::sqrt(p);
        A[size_t(j) * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double v = A[size_t(i) * n + j];
            for (int q = 0; q < j; ++q) v -= A[size_t(i) * n + q] * A[size_t(j) * n + q];
            A[size_t(i) * n + j] = v / d;
        }
        for (int i = 0; i < j; ++i) A[size_t(i) * n + j] = 0.0;
    }
}
static std::vector<double> spd_inverse(const std::vector<double> &L, int n)
{
    std::vector<double> X(size_t(n) * n, 0.0);
    for (int c = 0; c < n; ++c) {
        std::vector<double> y(size_t(n), 0.0);
        for (int i = 0; i < n; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int q = 0; q < i; ++q) v -= L[size_t(i) * n + q] * y[size_t(q)];
            y[size_t(i)] = v / L[size_t(i) * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double v = y[size_t(i)];
            for (int q = i + 1; q < n; ++q) v -= L[size_t(q) * n + i] * X[size_t(q) * n + c];
            X[size_t(i) * n + c] = v / L[size_t(i) * n + i];
        }
    }
    return X;
}

struct Blk { double v[36]; };
static Blk blk_of(const std::vector<double> &A, int n, int i, int j)
{
    Blk b;
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) b.v[a * 6 + c] = A[size_t(6 * i + a) * n + 6 * j + c];
    return b;
}

static void check_window(int NB, unsigned seed)
{
    const int n = 6 * NB;
    unsigned s = seed;
    // B = R^T R + n I restricted to the block band of half-width 4, made SPD by the diagonal
    std::vector<double> B(size_t(n) * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            if (i / 6 - j / 6 > 4) continue;
            const double v = i == j ? 40.0 + rnd(s) : rnd(s);
            B[size_t(i) * n + j] = v; B[size_t(j) * n + i] = v;
        }
    std::vector<double> L = B;
    chol(L, n);
    for (int i = 0; i < n; ++i) CHECK(L[size_t(i) * n + i] > 0.0);
    // the factor of a block band stays inside the band
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (i / 6 - j / 6 > 4) CHECK(L[size_t(i) * n + j] == 0.0);
    const std::vector<double> X = spd_inverse(L, n);
    double scale = 0.0;
    for (double v : X) scale = std::fmax(scale, std::fabs(v));
    // the window, as pgm_selinv_kernel keeps it
    Blk W[25];
    int tag_i[25], tag_k[25];
    for (int q = 0; q < 25; ++q) tag_i[q] = tag_k[q] = -1;
    const auto rd = [&](int i, int k) -> const Blk & {
        const int q = pgm_win_slot(i, k);
        CHECK(q >= 0 && q < 25 && tag_i[q] == i && tag_k[q] == k);
        return W[q];
    };
    const auto wr = [&](int i, int k, const Blk &b, int step) {
        const int q = pgm_win_slot(i, k);
        CHECK(q >= 0 && q < 25);
        // what it held is not needed any more: a block (i', k') is read at the steps max(i', k') - 4 .. min(i', k') only, and the steps still to come are <= step
        if (tag_i[q] >= 0) CHECK(std::max(tag_i[q], tag_k[q]) - 4 > step);
        W[q] = b; tag_i[q] = i; tag_k[q] = k;
    };
    for (int j = NB - 1; j >= 0; --j) {
        // L_jj^-1 and G_kj = L_kj L_jj^-1
        const Blk Ljj = blk_of(L, n, j, j);
        double Mi[36] = {0};
        for (int c = 0; c < 6; ++c) {
            Mi[c * 6 + c] = 1.0 / Ljj.v[c * 6 + c];
            for (int r = c + 1; r < 6; ++r) {
                double v = 0.0;
                for (int q = c; q < r; ++q) v -= Ljj.v[r * 6 + q] * Mi[q * 6 + c];
                Mi[r * 6 + c] = v / Ljj.v[r * 6 + r];
            }
        }
        Blk G[5];
        for (int d = 1; d <= 4; ++d) {
            if (j + d >= NB) continue;
            const Blk Lkj = blk_of(L, n, j + d, j);
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 6; ++c) {
                    double v = 0.0;
                    for (int q = 0; q < 6; ++q) v += Lkj.v[a * 6 + q] * Mi[q * 6 + c];
                    G[d].v[a * 6 + c] = v;
                }
        }
        Blk off[5];
        for (int d = 1; d <= 4; ++d) {
            const int i = j + d;
            if (i >= NB) continue;
            for (int e = 0; e < 36; ++e) off[d].v[e] = 0.0;
            for (int dk = 1; dk <= 4; ++dk) {
                const int k = j + dk;
                if (k >= NB) continue;
                const Blk &Sik = rd(i, k);
                for (int a = 0; a < 6; ++a)
                    for (int c = 0; c < 6; ++c)
                        for (int q = 0; q < 6; ++q) off[d].v[a * 6 + c] -= Sik.v[a * 6 + q] * G[dk].v[q * 6 + c];
            }
        }
        for (int d = 1; d <= 4; ++d) {
            const int i = j + d;
            if (i >= NB) continue;
            Blk tr;
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 6; ++c) tr.v[c * 6 + a] = off[d].v[a * 6 + c];
            wr(i, j, off[d], j); wr(j, i, tr, j);
        }
        Blk D;
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
                for (int q = 0; q < 6; ++q) v += Mi[q * 6 + a] * Mi[q * 6 + c];
                D.v[a * 6 + c] = v;
            }
        for (int dk = 1; dk <= 4; ++dk) {
            const int k = j + dk;
            if (k >= NB) continue;
            const Blk &Sjk = rd(j, k);
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 6; ++c)
                    for (int q = 0; q < 6; ++q) D.v[a * 6 + c] -= Sjk.v[a * 6 + q] * G[dk].v[q * 6 + c];
        }
        wr(j, j, D, j);
        // against the dense inverse: the column just finished
        for (int d = 0; d <= 4 && j + d < NB; ++d) {
            const Blk want = blk_of(X, n, j + d, j);
            const Blk &got = W[pgm_win_slot(j + d, j)];
            for (int e = 0; e < 36; ++e) CHECK(std::fabs(got.v[e] - want.v[e]) <= 1e-10 * scale);
        }
    }
}

static void check_conversion()
{
    unsigned s = 77u;
    for (int trial = 0; trial < 50; ++trial) {
        double R[36], S[36], t[3], A[36], out[36];
        for (int e = 0; e < 36; ++e) R[e] = rnd(s);
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c <= a; ++c) {
                double v = a == c ? 0.5 : 0.0;
                for (int q = 0; q < 6; ++q) v += R[a * 6 + q] * R[c * 6 + q];
                S[a * 6 + c] = v; S[c * 6 + a] = v;
            }
        for (int c = 0; c < 3; ++c) t[c] = 200.0 * rnd(s);
        pgm_store_A(t, A);
        pgm_to_store(S, t, out);
        double scale = 0.0;
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
                for (int p = 0; p < 6; ++p)
                    for (int q = 0; q < 6; ++q) v += A[a * 6 + p] * S[p * 6 + q] * A[c * 6 + q];
                scale = std::fmax(scale, std::fabs(v));
                CHECK(std::fabs(v - out[a * 6 + c]) <= 1e-12 * std::fmax(1.0, scale) * 100.0);
                CHECK(std::memcmp(&out[a * 6 + c], &out[c * 6 + a], sizeof(double)) == 0);
            }
        // first order: pg_plus(x, delta) against exp((A delta)^) T, on the translation and the rotation of a point
        double x[7], delta[6], xp[7];
        for (int c = 0; c < 3; ++c) x[c] = t[c];
        double qn = 0.0;
        for (int c = 3; c < 7; ++c) { x[c] = rnd(s); qn += x[c] * x[c]; }
        for (int c = 3; c < 7; ++c) x[c] /= std::sqrt(qn);
        for (int c = 0; c < 6; ++c) delta[c] = 1e-5 * rnd(s);
        pg_plus(x, delta, xp);
        double xi[6];
        for (int a = 0; a < 6; ++a) { xi[a] = 0.0; for (int q = 0; q < 6; ++q) xi[a] += A[a * 6 + q] * delta[q]; }
        // translation of exp(xi^) T to first order: t + phi x t + rho
        const double *rho = xi, *phi = xi + 3;
        const double tl[3] = {t[0] + phi[1] * t[2] - phi[2] * t[1] + rho[0], t[1] + phi[2] * t[0] - phi[0] * t[2] + rho[1], t[2] + phi[0] * t[1] - phi[1] * t[0] + rho[2]};
        for (int c = 0; c < 3; ++c) CHECK(std::fabs(tl[c] - xp[c]) <= 1e-12 * 200.0);
        // rotation: q' = (cos |d|, sin |d| d / |d|) (x) q against the axis-angle phi on the left: (cos |phi| / 2, sin(|phi| / 2) phi / |phi|) (x) q
        const double pn = std::sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
        const double ql[4] = {std::cos(pn / 2), std::sin(pn / 2) * phi[0] / pn, std::sin(pn / 2) * phi[1] / pn, std::sin(pn / 2) * phi[2] / pn};
        double q0[4], want[4], got[4];
        pg_q_of_pose(x, q0);
        pg_qmul(ql, q0, want);
        pg_q_of_pose(xp, got);
        for (int c = 0; c < 4; ++c) CHECK(std::fabs(want[c] - got[c]) <= 1e-14);
    }
}

int main(int argc, char **argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "count")) {
        const int M = std::atoi(argv[2]), L = std::atoi(argv[3]);
        std::printf("N %d %zu %zu %zu %zu\npg_marg: ok\n", pgm_launches(M, L), pgm_out_doubles(M), pgm_band_doubles(M), pgm_factor_doubles(L), pgm_work_doubles(M, L));
        return 0;
    }
    check_plan();
    for (int NB = 1; NB <= 12; ++NB) check_window(NB, 1000u + unsigned(NB));
    check_conversion();
    if (failures) { std::printf("pg_marg: %ld checks failed\n", failures); return 1; }
    std::printf("pg_marg: ok\n");
    return 0;
}
