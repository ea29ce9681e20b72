// Pose-graph optimisation (posegraph.hip; include/mloam_hip.h section (f14)): the arithmetic of ONE edge that exists once -- for the kernels (__host__ __device__),
// for the host side of the stage entries and for a stand-alone host program that runs it under a sanitizer (tests/host/pg_host_main.cpp) -- and the option
// validation. The tests' restatement (tests/host/pg_ref.cpp) does NOT include this header: it evaluates the factor over a dual-number type.
// Restated from the reference, with its lines: RelativeRTError::operator() (mloam_loop/include/mloam_loop/pose_graph.h:299-337) and QuaternionInverse (121-127);
// the sequential edges' measurement (mloam_loop/src/pose_graph.cpp:559-563); KeyFrame::updatePose (keyframe.cpp:89-93); Pose(q, t), Pose::inverse, Pose::operator*
// (utility/pose.cpp:34-40, 96-99, 108-111).
// Restated FROM MEMORY of Ceres 1.12 and Eigen 3.3 -- neither library's source is available to this project, so none of this could be checked against it:
//   ceres::QuaternionProduct (rotation.h): zw[0] = z0 w0 - z1 w1 - z2 w2 - z3 w3; zw[1] = z0 w1 + z1 w0 + z2 w3 - z3 w2; zw[2] = z0 w2 - z1 w3 + z2 w0 + z3 w1;
//     zw[3] = z0 w3 + z1 w2 - z2 w1 + z3 w0, quaternions as (w, x, y, z);
//   ceres::QuaternionRotatePoint: the quaternion is normalised first (scale = 1 / sqrt(q . q)), then UnitQuaternionRotatePoint's nine products t2 .. t9, t1;
//   ceres::QuaternionParameterization::Plus: norm = |delta|; q_delta = (cos norm, sin(norm) / norm * delta); x_plus = q_delta (x) x; delta == 0 leaves x;
//     ::ComputeJacobian: the 4 x 3 matrix whose column k is (0, e_k) (x) x;
//   ceres::HuberLoss(a): s > a^2: rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s); else rho = s, rho' = 1;  Corrector with rho'' <= 0: residual and Jacobian scaled by
//     sqrt(rho');
//   Eigen::Quaterniond product, inverse (conjugate / squaredNorm), normalize (coefficients divided by the norm) and q * v (uv = 2 (q.vec x v);
//     v + w uv + q.vec x uv).
// The Jacobian is the closed form of "ambient 6 x 4 times the 4 x 3 parameterisation Jacobian": with q' = (1, d) (x) q,
//   translation rows: d/dd_i = (2 / t_var) R_i^T [t_j - t_i]x, d/dt_i = -R_i^T / t_var, d/dt_j = R_i^T / t_var, d/dd_j = 0 (R_i of the NORMALISED q_i: the
//     rotation does not change along q_i itself, so the product with the tangent columns is this for any non-zero q_i);
//   rotation rows: the quaternion mismatch is linear in q_i and in q_j: column k of d/dd_j = (2 / q_var) vec(a (x) (0, e_k) (x) q_j) with a = m^-1 (x) q_i^-1, and d/dd_i is its
//     negative.
// Local block order per keyframe, as Ceres orders the two parameter blocks (q added before t, pose_graph.cpp:546-547): [rotation 3, translation 3].
// Translation units that include this header are compiled with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../include/mloam_hip.h"

#if defined(__HIPCC__)
#define MLH_PG_HD __host__ __device__ inline
#else
#define MLH_PG_HD inline
#endif

namespace mlh {

constexpr int PG_MAX_LOOPS = 128;            // a context's capacity of loop edges until mlh_pg_reserve raises it (up to MLH_PG_LOOPS_LIMIT), and the largest L whose
                                             // dense stage is the one-workgroup pg_dense_kernel (its right-hand side in LDS: 6 x 128 doubles); beyond it the blocked stage
constexpr int PG_PANEL = 64;                 // the blocked dense stage's panel width: a 64 x 64 f64 diagonal block is 32 KiB of LDS
constexpr int PG_SEQ = 4;                    // sequential edges per keyframe (pose_graph.cpp:555)
constexpr int PG_SLOTS = PG_SEQ + 1;         // edge slots per keyframe: to i - 1 .. i - 4, then the loop edge

inline void pg_opts_defaults(mlh_pg_opts &o)
{
    o.max_num_iterations = 5; o.n_sequential = PG_SEQ; o.t_var = 0.1; o.q_var = 0.01; o.huber_delta = 1.0;
}
// the argument at fault, or nullptr
inline const char *pg_opts_fault(const mlh_pg_opts &o)
{
    if (o.max_num_iterations < 0 || o.max_num_iterations > 200) return "max_num_iterations";
    if (o.n_sequential != PG_SEQ) return "n_sequential (the band's shape is fixed at 4)";
    if (!std::isfinite(o.t_var) || !(o.t_var > 0.0)) return "t_var";
    if (!std::isfinite(o.q_var) || !(o.q_var > 0.0)) return "q_var";
    if (!std::isfinite(o.huber_delta) || !(o.huber_delta > 0.0)) return "huber_delta";
    return nullptr;
}

// ---- the blocked dense stage's launch plan (posegraph.hip: L > PG_MAX_LOOPS). The bordered matrix [C; r^T] (m = 6 L columns, m + 1 rows: the last row is the
// right-hand side, which the panel solves turn into L^-1 r) is cut into PG_PANEL-wide tiles: T = ceil(m / 64) column panels, Tb = ceil((m + 1) / 64) row tiles. The
// factorisation is LEFT-looking; one entry below is one kernel launch whose workgroup w covers tile (or row tile) lo + w:
//   PG_STEP_SUM            every tile (k, i), k < T, k <= i < Tb: the Gram partials summed in split order (workgroups = the number of those tiles)
//   PG_STEP_UPDATE  k      tiles (k, i), i = lo .. hi - 1 (lo = k): minus the products of the panels 0 .. k - 1 (k >= 1)
//   PG_STEP_PANEL   k      tile (k, k) factored (every workgroup READS it and factors it for itself; workgroup lo = k stores the factor in the diagonal buffer,
//                          never over the tile), tiles (k, i), i = k + 1 .. hi - 1 solved in place
//   PG_STEP_BACK    k      the backward substitution's panel k, from T - 1 down: row tile k solved, row tiles lo = 0 .. k - 1 updated with it
// 3 T launches in all, a function of m alone.
enum { PG_STEP_SUM = 0, PG_STEP_UPDATE, PG_STEP_PANEL, PG_STEP_BACK };
struct PgDenseStep { int kind, k, lo, hi; };
inline int pg_dense_panels(int m) { return (m + PG_PANEL - 1) / PG_PANEL; }
inline int pg_dense_row_tiles(int m) { return (m + 1 + PG_PANEL - 1) / PG_PANEL; }
inline int pg_dense_launches(int m) { return m > 0 ? 3 * pg_dense_panels(m) : 0; }
// launch `index` (0 .. pg_dense_launches(m) - 1) of the stage: what the host enqueues, in this order
inline PgDenseStep pg_dense_step(int m, int index)
{
    const int T = pg_dense_panels(m), Tb = pg_dense_row_tiles(m);
    if (index == 0) return {PG_STEP_SUM, 0, 0, T * Tb - T * (T - 1) / 2};
    if (index < 2 * T) {
        const int k = index / 2;
        return {index % 2 ? PG_STEP_PANEL : PG_STEP_UPDATE, k, k, Tb};
    }
    const int k = T - 1 - (index - 2 * T);
    return {PG_STEP_BACK, k, 0, k + 1};
}
// workgroup w of PG_STEP_SUM -> its tile (k, i): the tiles row by row of the upper-stored factor, row k holding i = k .. Tb - 1
MLH_PG_HD void pg_dense_sum_tile(int w, int Tb, int *k_out, int *i_out)
{
    int k = 0;
    while (w >= Tb - k) { w -= Tb - k; ++k; }
    *k_out = k; *i_out = k + w;
}

// quaternions below are (w, x, y, z); poses in memory are [t, q(xyzw)]
MLH_PG_HD void pg_q_of_pose(const double p[7], double q[4]) { q[0] = p[6]; q[1] = p[3]; q[2] = p[4]; q[3] = p[5]; }
MLH_PG_HD void pg_q_to_pose(const double q[4], double p[7]) { p[6] = q[0]; p[3] = q[1]; p[4] = q[2]; p[5] = q[3]; }

MLH_PG_HD void pg_qmul(const double z[4], const double w[4], double zw[4])
{
    zw[0] = z[0] * w[0] - z[1] * w[1] - z[2] * w[2] - z[3] * w[3];
    zw[1] = z[0] * w[1] + z[1] * w[0] + z[2] * w[3] - z[3] * w[2];
    zw[2] = z[0] * w[2] - z[1] * w[3] + z[2] * w[0] + z[3] * w[1];
    zw[3] = z[0] * w[3] + z[1] * w[2] - z[2] * w[1] + z[3] * w[0];
}
MLH_PG_HD void pg_qconj(const double q[4], double c[4]) { c[0] = q[0]; c[1] = -q[1]; c[2] = -q[2]; c[3] = -q[3]; }

// ceres::QuaternionRotatePoint
MLH_PG_HD void pg_rotate_point(const double q[4], const double pt[3], double out[3])
{
    const double scale = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double u0 = scale * q[0], u1 = scale * q[1], u2 = scale * q[2], u3 = scale * q[3];
    const double t2 = u0 * u1, t3 = u0 * u2, t4 = u0 * u3, t5 = -u1 * u1, t6 = u1 * u2, t7 = u1 * u3, t8 = -u2 * u2, t9 = u2 * u3, t1 = -u3 * u3;
    out[0] = 2.0 * ((t8 + t1) * pt[0] + (t6 - t4) * pt[1] + (t3 + t7) * pt[2]) + pt[0];
    out[1] = 2.0 * ((t4 + t6) * pt[0] + (t5 + t1) * pt[1] + (t9 - t2) * pt[2]) + pt[1];
    out[2] = 2.0 * ((t7 - t3) * pt[0] + (t2 + t9) * pt[1] + (t5 + t8) * pt[2]) + pt[2];
}

// the rows of R(normalised q)^T: Rt[3 r + c]
MLH_PG_HD void pg_rot_transposed(const double q[4], double Rt[9])
{
    double c[4];
    pg_qconj(q, c);
    for (int k = 0; k < 3; ++k) {
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double col[3];
        pg_rotate_point(c, e, col);
        Rt[k] = col[0]; Rt[3 + k] = col[1]; Rt[6 + k] = col[2];
    }
}

// QuaternionParameterization::Plus on q and the sum on t; delta = [rotation 3, translation 3]
MLH_PG_HD void pg_plus(const double x[7], const double delta[6], double out[7])
{
    out[0] = x[0] + delta[3]; out[1] = x[1] + delta[4]; out[2] = x[2] + delta[5];
    const double norm = sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
    if (norm > 0.0) {
        const double s = sin(norm) / norm;
        const double qd[4] = {cos(norm), s * delta[0], s * delta[1], s * delta[2]};
        double q[4], r[4];
        pg_q_of_pose(x, q);
        pg_qmul(qd, q, r);
        pg_q_to_pose(r, out);
    } else {
        out[3] = x[3]; out[4] = x[4]; out[5] = x[5]; out[6] = x[6];
    }
}

// RelativeRTError over (q_i, t_i, q_j, t_j) with the measurement m = [t, q(xyzw)]: r[6]; Ji, Jj (may be null): 6 x 6 row-major over [rotation, translation]
MLH_PG_HD void pg_edge_eval(const double pi[7], const double pj[7], const double m[7], double t_var, double q_var, double r[6], double *Ji, double *Jj)
{
    double qi[4], qj[4], qm[4], iqw[4], mi[4], qij[4], eq[4];
    pg_q_of_pose(pi, qi); pg_q_of_pose(pj, qj); pg_q_of_pose(m, qm);
    const double v[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
    pg_qconj(qi, iqw);
    double tij[3];
    pg_rotate_point(iqw, v, tij);
    r[0] = (tij[0] - m[0]) / t_var; r[1] = (tij[1] - m[1]) / t_var; r[2] = (tij[2] - m[2]) / t_var;
    pg_qmul(iqw, qj, qij);
    pg_qconj(qm, mi);
    pg_qmul(mi, qij, eq);
    r[3] = 2.0 * eq[1] / q_var; r[4] = 2.0 * eq[2] / q_var; r[5] = 2.0 * eq[3] / q_var;
    if (!Ji || !Jj) return;
    double Rt[9];
    pg_rot_transposed(qi, Rt);
    // [v]x
    const double vx[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
            const double rv = Rt[3 * a] * vx[c] + Rt[3 * a + 1] * vx[3 + c] + Rt[3 * a + 2] * vx[6 + c];
            Ji[6 * a + c] = 2.0 * rv / t_var;
            Ji[6 * a + 3 + c] = -Rt[3 * a + c] / t_var;
            Jj[6 * a + c] = 0.0;
            Jj[6 * a + 3 + c] = Rt[3 * a + c] / t_var;
            Ji[6 * (3 + a) + 3 + c] = 0.0;
            Jj[6 * (3 + a) + 3 + c] = 0.0;
        }
    double am[4];
    pg_qmul(mi, iqw, am);
    for (int k = 0; k < 3; ++k) {
        const double ek[4] = {0.0, k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double t1[4], t2[4];
        pg_qmul(ek, qj, t1);
        pg_qmul(am, t1, t2);
        for (int a = 0; a < 3; ++a) {
            const double d = 2.0 * t2[1 + a] / q_var;
            Jj[6 * (3 + a) + k] = d;
            Ji[6 * (3 + a) + k] = -d;
        }
    }
}

// ceres::HuberLoss(delta) at s = |r|^2: *rho <- rho(s); returns sqrt(rho') (what Corrector scales the block by: rho'' <= 0)
MLH_PG_HD double pg_huber(double s, double delta, double *rho)
{
    const double b = delta * delta;
    if (s > b) {
        const double rs = sqrt(s);
        *rho = 2.0 * delta * rs - b;
        return sqrt(delta / rs);
    }
    *rho = s;
    return 1.0;
}

// Eigen: q.inverse()
MLH_PG_HD void pg_eigen_qinv(const double q[4], double out[4])
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n2 > 0.0) { out[0] = q[0] / n2; out[1] = -q[1] / n2; out[2] = -q[2] / n2; out[3] = -q[3] / n2; }
    else { out[0] = out[1] = out[2] = out[3] = 0.0; }
}
// Eigen: q * v
MLH_PG_HD void pg_eigen_qrot(const double q[4], const double v[3], double out[3])
{
    double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    out[0] = v[0] + q[0] * uv[0] + (q[2] * uv[2] - q[3] * uv[1]);
    out[1] = v[1] + q[0] * uv[1] + (q[3] * uv[0] - q[1] * uv[2]);
    out[2] = v[2] + q[0] * uv[2] + (q[1] * uv[1] - q[2] * uv[0]);
}
// Pose(q, t): q_.normalize()
MLH_PG_HD void pg_pose_make(const double q[4], const double t[3], double out[7])
{
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    double u[4] = {q[0], q[1], q[2], q[3]};
    if (n != 0.0) { u[0] = q[0] / n; u[1] = q[1] / n; u[2] = q[2] / n; u[3] = q[3] / n; }
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
    pg_q_to_pose(u, out);
}
// Pose::inverse
MLH_PG_HD void pg_pose_inverse(const double p[7], double out[7])
{
    double q[4], qi[4], t[3];
    pg_q_of_pose(p, q);
    pg_eigen_qinv(q, qi);
    pg_eigen_qrot(qi, p, t);
    t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2];
    pg_pose_make(qi, t, out);
}
// Pose::operator*
MLH_PG_HD void pg_pose_mul(const double a[7], const double b[7], double out[7])
{
    double qa[4], qb[4], q[4], t[3];
    pg_q_of_pose(a, qa); pg_q_of_pose(b, qb);
    pg_qmul(qa, qb, q);
    pg_eigen_qrot(qa, b, t);
    t[0] += a[0]; t[1] += a[1]; t[2] += a[2];
    pg_pose_make(q, t, out);
}
// the measurement of a sequential edge from the two current poses (pose_graph.cpp:559-563): m = [q_prev^-1 (t_i - t_prev), q_prev^-1 q_i], not normalised
MLH_PG_HD void pg_sequential_measurement(const double prev[7], const double cur[7], double m[7])
{
    double qp[4], qc[4], qi[4], q[4];
    pg_q_of_pose(prev, qp); pg_q_of_pose(cur, qc);
    pg_eigen_qinv(qp, qi);
    const double v[3] = {cur[0] - prev[0], cur[1] - prev[1], cur[2] - prev[2]};
    pg_eigen_qrot(qi, v, m);
    pg_qmul(qi, qc, q);
    pg_q_to_pose(q, m);
}

}  // namespace mlh
