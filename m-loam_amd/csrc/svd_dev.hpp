// One-sided (Hestenes) Jacobi SVD of a tall matrix with NC <= 4 columns (initext.hip: Q_ 1200 x 4, A 3N x 3, G 2N x 4), written once for the kernel and for the
// host (tests/host/initext_host_main.cpp, host/initext_selftest.cpp, scripts/iebench.py's CPU leg): the rows are reached through a `Rows` policy -- on the device
// each thread's own rows in registers (SvdRegRows), on the host all rows behind a pointer (SvdPtrRows: one "lane" looping) -- and the column sums through a `Red`
// policy that returns the sum over ALL rows to every participant with the same bits (device: a __shfl_xor butterfly per wavefront, the wavefronts' results combined
// in wavefront order; host: the identity). Every participant therefore takes the same decisions and holds the same V, and nothing is shared but the sums.
//   cyclic sweeps over the pairs (p, q), p < q: alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q; the pair is rotated when |gamma| > tol sqrt(alpha beta)
//   (and the product is not zero: a zero column is never touched, so the zero matrix keeps V = I): zeta = (beta - alpha) / (2 gamma),
//   t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t; a_p <- c a_p - s a_q, a_q <- s a_p + c a_q, the same on V's columns.
//   Sweeps run until one rotates nothing (at most SVD_MAX_SWEEPS). Then sigma_j = |a_j|, sorted descending, equal values in column order.
// The Gram matrix A^T A is never formed: its eigenvalues are sigma^2, which squares the condition number and loses the small singular values the rotation's
// convergence test and the translation's rank rule read.
// Translation units that include this header are compiled with -ffp-contract=off.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MLH_SVD_HD __host__ __device__ inline
#define MLH_SVD_UNROLL _Pragma("unroll")
#else
#define MLH_SVD_HD inline
#define MLH_SVD_UNROLL
#endif

namespace mlh {

constexpr int SVD_MAX_SWEEPS = 60;

// the host's rows: n x NC row-major behind a pointer
template <int NC> struct SvdPtrRows {
    double *a;
    int n;
    MLH_SVD_HD int count() const { return n; }
    MLH_SVD_HD double &at(int r, int c) { return a[r * NC + c]; }
};
// a device thread's rows: RPT x NC in registers (every loop over them is unrolled); rows beyond the matrix are zeros
template <int NC, int RPT> struct SvdRegRows {
    double v[RPT * NC];
    MLH_SVD_HD constexpr int count() const { return RPT; }
    MLH_SVD_HD double &at(int r, int c) { return v[r * NC + c]; }
};
// the host's reduction: the one participant already holds the sum
struct SvdNoRed {
    template <int N> MLH_SVD_HD void sum(double (&)[N]) {}
};

// sigma[NC] descending, V (NC x NC row-major, column j belongs to sigma[j]), the rows left as U Sigma in the ORIGINAL column order with perm[j] = the original column
// of sorted position j; returns the number of sweeps
template <int NC, class Rows, class Red>
MLH_SVD_HD int svd_onesided_jacobi(Rows &A, Red &red, double tol, double *sigma, double *V, int *perm)
{
    double W[NC * NC];
MLH_SVD_UNROLL
    for (int i = 0; i < NC * NC; ++i) W[i] = (i / NC == i % NC) ? 1.0 : 0.0;
    int sweeps = 0;
    for (bool rotated = true; rotated && sweeps < SVD_MAX_SWEEPS; ++sweeps) {
        rotated = false;
MLH_SVD_UNROLL
        for (int p = 0; p < NC - 1; ++p)
MLH_SVD_UNROLL
            for (int q = p + 1; q < NC; ++q) {
                double s3[3] = {0.0, 0.0, 0.0};
MLH_SVD_UNROLL
                for (int r = 0; r < A.count(); ++r) {
                    const double x = A.at(r, p), y = A.at(r, q);
                    s3[0] += x * x; s3[1] += y * y; s3[2] += x * y;
                }
                red.template sum<3>(s3);
                const double alpha = s3[0], beta = s3[1], gamma = s3[2], lim = sqrt(alpha * beta);
                if (lim > 0.0 && fabs(gamma) > tol * lim) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
MLH_SVD_UNROLL
                    for (int r = 0; r < A.count(); ++r) {
                        const double x = A.at(r, p), y = A.at(r, q);
                        A.at(r, p) = c * x - s * y;
                        A.at(r, q) = s * x + c * y;
                    }
MLH_SVD_UNROLL
                    for (int r = 0; r < NC; ++r) {
                        const double x = W[r * NC + p], y = W[r * NC + q];
                        W[r * NC + p] = c * x - s * y;
                        W[r * NC + q] = s * x + c * y;
                    }
                }
            }
    }
    double n2[NC];
MLH_SVD_UNROLL
    for (int c = 0; c < NC; ++c) n2[c] = 0.0;
MLH_SVD_UNROLL
    for (int r = 0; r < A.count(); ++r)
MLH_SVD_UNROLL
        for (int c = 0; c < NC; ++c) n2[c] += A.at(r, c) * A.at(r, c);
    red.template sum<NC>(n2);
    double sg[NC];
    int pm[NC];
MLH_SVD_UNROLL
    for (int c = 0; c < NC; ++c) { sg[c] = sqrt(n2[c]); pm[c] = c; }
    // insertion sort, descending, stable
MLH_SVD_UNROLL
    for (int i = 1; i < NC; ++i)
MLH_SVD_UNROLL
        for (int j = i; j > 0; --j)
            if (sg[j] > sg[j - 1]) {
                const double ts = sg[j]; sg[j] = sg[j - 1]; sg[j - 1] = ts;
                const int tp = pm[j]; pm[j] = pm[j - 1]; pm[j - 1] = tp;
            }
MLH_SVD_UNROLL
    for (int j = 0; j < NC; ++j) {
        sigma[j] = sg[j]; perm[j] = pm[j];
MLH_SVD_UNROLL
        for (int r = 0; r < NC; ++r) {
            // (pm[j] is a run-time index into registers: selected by comparison so that W stays in registers)
            double w = 0.0;
MLH_SVD_UNROLL
            for (int c = 0; c < NC; ++c) w = (pm[j] == c) ? W[r * NC + c] : w;
            V[r * NC + j] = w;
        }
    }
    return sweeps;
}

// x = V Sigma^+ U^T b of the decomposition above: utb[j] = a_perm[j] . b over all rows (already reduced); singular values not above
// diag_size * epsilon * sigma_max are dropped (the rank rule of Eigen's JacobiSVD::solve); returns the rank
template <int NC>
MLH_SVD_HD int svd_solve(const double *sigma, const double *V, const double *utb, double *x)
{
    const double thr = double(NC) * 2.220446049250313e-16 * sigma[0];
    int rank = 0;
MLH_SVD_UNROLL
    for (int r = 0; r < NC; ++r) x[r] = 0.0;
MLH_SVD_UNROLL
    for (int j = 0; j < NC; ++j)
        if (sigma[j] > thr && sigma[j] > 0.0) {
            ++rank;
            const double w = (utb[j] / sigma[j]) / sigma[j];
MLH_SVD_UNROLL
            for (int r = 0; r < NC; ++r) x[r] += V[r * NC + j] * w;
        }
    return rank;
}

}  // namespace mlh
