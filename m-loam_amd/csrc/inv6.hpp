// The inverse of a 6 x 6 matrix in f64, as the mapper takes its pose covariance from the Hessian (lidar_mapper_keyframe.cpp:606: cov_mapping = mat_H.inverse()).
// Eigen's fixed-size Matrix<double, 6, 6>::inverse() is PartialPivLU -- unblocked at this size -- followed by the solve against the identity; these are its
// operations: per column the largest magnitude on or below the diagonal becomes the pivot (the first one on a tie), whole rows are exchanged, the multipliers are
// the quotients by the pivot, the trailing block takes a rank-1 update; then the unit-lower solve and the upper solve. A zero pivot is not special-cased: the
// quotients are the inf / NaN IEEE division yields, as Eigen's are.
// This header compiles for the host and the device. inv6_lu is the arithmetic, written once; solver_dev.hpp: inv6_wave spreads it over the lanes of one
// wavefront -- the same operations in the same order, element for element.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MLH_INV6_HD __host__ __device__
#else
#define MLH_INV6_HD
#endif

namespace mlh {

// A, X: row-major 6 x 6 (X may not alias A). perm_out (nullable): row i of the factorised matrix is row perm_out[i] of A.
// The right-hand side (the identity) is eliminated along with the matrix: row exchanges and multipliers are applied to it in the step that makes them, which is the
// unit-lower solve of P I column by column -- y(i) = e(i) - sum_{k < i} L(i, k) y(k), the terms in ascending k.
MLH_INV6_HD inline void inv6_lu(const double *A, double *X, int *perm_out = nullptr)
{
    double a[36], b[36];
    int perm[6];
    for (int i = 0; i < 36; ++i) { a[i] = A[i]; b[i] = ((i % 7) == 0) ? 1.0 : 0.0; }
    for (int i = 0; i < 6; ++i) perm[i] = i;
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double best = fabs(a[k * 6 + k]);
        for (int i = k + 1; i < 6; ++i) { const double v = fabs(a[i * 6 + k]); if (v > best) { best = v; p = i; } }
        if (p != k) {
            for (int j = 0; j < 6; ++j) {
                double t = a[k * 6 + j]; a[k * 6 + j] = a[p * 6 + j]; a[p * 6 + j] = t;
                t = b[k * 6 + j]; b[k * 6 + j] = b[p * 6 + j]; b[p * 6 + j] = t;
            }
            const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
        }
        const double piv = a[k * 6 + k];
        for (int i = k + 1; i < 6; ++i) {
            const double m = a[i * 6 + k] / piv;
            a[i * 6 + k] = m;
            for (int j = k + 1; j < 6; ++j) a[i * 6 + j] -= m * a[k * 6 + j];
            for (int c = 0; c < 6; ++c) b[i * 6 + c] -= m * b[k * 6 + c];
        }
    }
    // U x = y, column by column: x(i) = (y(i) - sum_{j > i} U(i, j) x(j)) / U(i, i), the terms in ascending j
    for (int c = 0; c < 6; ++c)
        for (int i = 5; i >= 0; --i) {
            double s = b[i * 6 + c];
            for (int j = i + 1; j < 6; ++j) s -= a[i * 6 + j] * X[j * 6 + c];
            X[i * 6 + c] = s / a[i * 6 + i];
        }
    if (perm_out) for (int i = 0; i < 6; ++i) perm_out[i] = perm[i];
}

}  // namespace mlh
