// Host arithmetic check (no GPU): mlh::inv6_lu (m-loam_amd/csrc/inv6.hpp), the 6 x 6 inverse behind mlh_scan2map_cov -- LU with partial pivoting, solved against
// the identity -- against the checker's Gauss-Jordan inverse (oracle/linalg.hpp: inverse_d) on 10 000 random SPD matrices J^T J whose column scalings spread the
// condition number from 1 to 1e10: the two agree within 100 eps cond2, relative to the largest entry of the inverse. Also one matrix with an exactly zero pivot
// column (nothing is special-cased: inf / NaN come out, nothing traps), and the count of matrices on which the two methods pivot in a different order.
// Compiled with -fsanitize=address,undefined and run by tests/test_pose_cov_host.py.
#include "inv6.hpp"
#include "linalg.hpp"
#include <cstdio>
#include <random>

// inverse_d's pivot rows, in the order it picks them (its elimination, without the right-hand side)
static void gauss_jordan_pivots(const double *A, int perm[6])
{
    double a[36];
    int rows[6];
    for (int i = 0; i < 36; ++i) a[i] = A[i];
    for (int i = 0; i < 6; ++i) rows[i] = i;
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r) if (std::fabs(a[r * 6 + c]) > std::fabs(a[piv * 6 + c])) piv = r;
        if (piv != c) { for (int j = 0; j < 6; ++j) std::swap(a[c * 6 + j], a[piv * 6 + j]); std::swap(rows[c], rows[piv]); }
        const double d = a[c * 6 + c];
        for (int j = 0; j < 6; ++j) a[c * 6 + j] /= d;
        for (int r = 0; r < 6; ++r) if (r != c) {
            const double f = a[r * 6 + c];
            if (f != 0.0) for (int j = 0; j < 6; ++j) a[r * 6 + j] -= f * a[c * 6 + j];
        }
    }
    for (int i = 0; i < 6; ++i) perm[i] = rows[i];
}

int main()
{
    const double eps = 2.220446049250313e-16;      // 2^-52
    const int N = 10000;
    std::mt19937_64 rng(20240611);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> unif(-0.5, 0.5);
    int bad = 0, pivot_diff = 0;
    double worst = 0.0, cond_lo = 1e300, cond_hi = 0.0;
    for (int n = 0; n < N; ++n) {
        double A[36];
        if (n == 0) {
            for (int i = 0; i < 36; ++i) A[i] = (i % 7 == 0) ? 1.0 : 0.0;       // condition number 1
        } else {
            // J: 12 x 6 normal; columns scaled by 10^(t r_j), r in [-1/2, 1/2] with both ends taken, t from 0 to 4: J^T J's condition number up to ~1e10
            const double t = 4.0 * double(n) / double(N - 1);
            double sc[6], J[72];
            for (int j = 0; j < 6; ++j) sc[j] = std::pow(10.0, t * unif(rng));
            sc[n % 6] = std::pow(10.0, -0.5 * t); sc[(n + 1 + (n / 6) % 5) % 6] = std::pow(10.0, 0.5 * t);
            for (int i = 0; i < 72; ++i) J[i] = normal(rng) * sc[i % 6];
            for (int r = 0; r < 6; ++r)
                for (int c = r; c < 6; ++c) {
                    double s = 0.0;
                    for (int k = 0; k < 12; ++k) s += J[k * 6 + r] * J[k * 6 + c];
                    A[r * 6 + c] = s; A[c * 6 + r] = s;
                }
        }
        double ev[6], V[36];
        orc::jacobi_eig_sym_d(A, 6, ev, V);
        double lo = ev[0], hi = ev[0];
        for (int i = 1; i < 6; ++i) { lo = std::min(lo, ev[i]); hi = std::max(hi, ev[i]); }
        const double cond = hi / lo;
        if (!(cond <= 1e10)) { --n; continue; }           // (outside the range under test: draw again)
        cond_lo = std::min(cond_lo, cond); cond_hi = std::max(cond_hi, cond);
        double X[36], R[36];
        int perm[6], perm_ref[6];
        mlh::inv6_lu(A, X, perm);
        if (!orc::inverse_d(A, 6, R)) { ++bad; std::printf("MISMATCH matrix %d: the checker's inverse refused a regular matrix\n", n); continue; }
        gauss_jordan_pivots(A, perm_ref);
        bool same = true;
        for (int i = 0; i < 6; ++i) same = same && perm[i] == perm_ref[i];
        if (!same) ++pivot_diff;
        double xmax = 0.0, dmax = 0.0;
        for (int i = 0; i < 36; ++i) { xmax = std::max(xmax, std::fabs(R[i])); dmax = std::max(dmax, std::fabs(X[i] - R[i])); }
        const double ratio = dmax / (eps * cond * xmax);
        worst = std::max(worst, ratio);
        if (!(ratio <= 100.0)) { ++bad; std::printf("MISMATCH matrix %d: cond2 %.3e, difference %.3e of %.3e = %.1f eps cond2\n", n, cond, dmax, xmax, ratio); }
    }
    // an exactly zero pivot column: the checker refuses, the product's form divides as IEEE does
    {
        double A[36], X[36], R[36];
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) A[r * 6 + c] = (c == 2) ? 0.0 : (r == c ? 2.0 : 0.25);
        mlh::inv6_lu(A, X);
        int nonfinite = 0;
        for (int i = 0; i < 36; ++i) if (!std::isfinite(X[i])) ++nonfinite;
        if (orc::inverse_d(A, 6, R) || nonfinite == 0) { ++bad; std::printf("MISMATCH zero pivot column: %d non-finite entries\n", nonfinite); }
        std::printf("zero pivot column: %d non-finite entries\n", nonfinite);
    }
    std::printf("%d matrices, cond2 %.3e .. %.3e, worst difference %.2f eps cond2, %d pivot orders differ, %d mismatches\n", N, cond_lo, cond_hi, worst, pivot_diff, bad);
    return bad ? 1 : 0;
}
