// The initial extrinsic calibration (initext.hip; include/mloam_hip.h section (f16)): the arithmetic that exists once -- for the kernel (__host__ __device__), for the
// host side of the entries and for a stand-alone host program that runs it under a sanitizer (tests/host/initext_host_main.cpp) -- with the option validation, the
// bookkeeping of addPose and a host-only run of both solves over svd_dev.hpp (one "lane" looping).
// Restated from the reference, with its lines (estimator/src/initial/initial_extrinsics.{h,cpp}): rotCmp (h:34-40), setParameter / clearState (cpp:26-63),
// setCovRotation / setCovTranslation (cpp:65-77), addPose (cpp:79-102), checkScrewMotion (cpp:104-116), the block huber (L - R) (cpp:128-153), the decision (cpp:194-201),
// the rows of A, b (cpp:264-274) and of G, w (cpp:286-302), the tails (cpp:277, 304-307); Utility::skewSymmetric (utility/utility.h:188-195); Pose(q, t) and
// Pose::inverse (estimator/pose.cpp:34-41, 99-102) through pg_host.hpp.
// Restated FROM MEMORY of Eigen 3.3 -- its source is not available to this project, so none of this could be checked against it:
//   AngleAxisd(Quaterniond): n = |q.vec|; below epsilon the norm is taken again with scaling (stableNorm); n != 0: angle = 2 atan2(n, |w|), axis = q.vec / (w < 0 ? -n : n);
//     otherwise angle 0, axis (1, 0, 0);
//   Quaterniond::angularDistance(o): d = q * o.conjugate(); 2 atan2(|d.vec|, |d.w|);
//   Quaterniond::toRotationMatrix: the twelve products tx = 2x .. tzz = tz z, R(0,0) = 1 - (tyy + tzz), R(0,1) = txy - twz, R(0,2) = txz + twy, ...;
//   Quaterniond(Vector4d): the argument is the coefficient vector (x, y, z, w);   Quaterniond(AngleAxisd(a, axis)): w = cos(a / 2), vec = sin(a / 2) axis;
//   Quaterniond product, inverse, normalize, q * v: as pg_host.hpp lists them;
//   JacobiSVD::solve: x = V Sigma^+ U^T b over the singular values above diagSize * epsilon * sigma_max (the default threshold); three-element dot products summed
//     left to right.
// Reproduced quirks:
//   - rotCmp reads second[0].q_.w(): LiDAR 0's w, not idx_ref's (IeHeapEntry keeps exactly that number; the heap is std::priority_queue under the reference's
//     comparator, so equal keys fall as libstdc++ leaves them);
//   - Q_'s block is written only inside calibExRotation, for the set last accepted (pose_laser_add_): sets accepted while the heap was smaller than WINDOW_SIZE, or
//     between two calibrations, never enter Q_; a call without a new accepted set rewrites the same block with a new weight;
//   - the Huber weight of the block uses calib_ext_ of that moment, which every calibExRotation overwrites (q_ only, converged or not);
//   - b and w are not weighted while A and G are;
//   - rot_cov(1) of singularValues().tail<3>() is the second-smallest of the four;
//   - `if (x[0] < 0) x = -x` acts on the quaternion's x: L and R are laid out (x, y, z, w) and Quaterniond(Vector4d) reads coefficients in that order, whatever the
//     reference's comment says;
//   - pq_pose_.size() < WINDOW_SIZE returns before anything is written.
// Chosen:
//   - abs(double) is the double overload (the reference's unqualified abs under `using namespace Eigen` could bind to the int one on some toolchains);
//   - reset also empties the heap (clearState forgets to, so a second run of the reference would start with the first run's heap);
//   - non-finite poses are refused by the entry (MLH_ERR_INVALID, nothing changed);
//   - the block is computed on the host: its Huber weight goes through atan2, whose last bit may differ between the host's and the device's libraries, and the
//     tests hold Q_ bit for bit.
// Quaternions in this header: poses in memory are [t, q(xyzw)]; four-element quaternion arguments are (w, x, y, z) as in pg_host.hpp unless named xyzw.
// Translation units that include this header are compiled with -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>
#include <queue>
#include <vector>
#include "pg_host.hpp"
#include "svd_dev.hpp"

#define MLH_IE_HD MLH_PG_HD

namespace mlh {

constexpr int IE_MAX_LIDAR = MLH_INITEXT_MAX_LIDAR;
constexpr int IE_N_POSE = MLH_INITEXT_N_POSE;        // N_POSE (cpp:22)
constexpr int IE_Q_ROWS = 4 * IE_N_POSE;
constexpr double IE_SVD_TOL = 8e-15;                 // ~ sqrt(1200) epsilon: the rounding of a 1200-term dot product

inline void ie_opts_defaults(mlh_initext_opts &o)
{
    std::memset(&o, 0, sizeof(o));
    o.n_lidar = 2; o.idx_ref = 0; o.planar_movement = 0; o.window_size = 4; o.n_pose = IE_N_POSE;
    o.eps_r = 0.05; o.eps_t = 0.1; o.rot_cov_thre = 0.0;
    for (int l = 0; l < IE_MAX_LIDAR; ++l) o.qbl[l][3] = 1.0;
}
// the argument at fault, or nullptr
inline const char *ie_opts_fault(const mlh_initext_opts &o)
{
    if (o.n_lidar < 1 || o.n_lidar > IE_MAX_LIDAR) return "n_lidar";
    if (o.idx_ref < 0 || o.idx_ref >= o.n_lidar) return "idx_ref";
    if (o.window_size < 1) return "window_size";
    if (o.n_pose < 1 || o.n_pose > IE_N_POSE) return "n_pose";
    if (!std::isfinite(o.eps_r) || !(o.eps_r > 0.0)) return "eps_r";
    if (!std::isfinite(o.eps_t) || !(o.eps_t > 0.0)) return "eps_t";
    if (!std::isfinite(o.rot_cov_thre) || o.rot_cov_thre < 0.0) return "rot_cov_thre";
    for (int l = 0; l < o.n_lidar; ++l) {
        double n2 = 0.0;
        for (int c = 0; c < 4; ++c) { if (!std::isfinite(o.qbl[l][c])) return "qbl"; n2 += o.qbl[l][c] * o.qbl[l][c]; }
        if (!(n2 > 0.0)) return "qbl";
        for (int c = 0; c < 3; ++c) if (!std::isfinite(o.tbl[l][c])) return "tbl";
    }
    return nullptr;
}
// rot_cov_thre_ (cpp:58)
inline double ie_rot_cov_thre(const mlh_initext_opts &o) { return o.rot_cov_thre > 0.0 ? o.rot_cov_thre : (o.planar_movement ? 0.05 : 0.25); }

// Eigen: AngleAxisd(Quaterniond)
MLH_IE_HD void ie_angle_axis(const double q[4], double *angle, double axis[3])
{
    double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (n < DBL_EPSILON) {
        const double m = fmax(fabs(q[1]), fmax(fabs(q[2]), fabs(q[3])));
        n = 0.0;
        if (m > 0.0) { const double a = q[1] / m, b = q[2] / m, c = q[3] / m; n = m * sqrt(a * a + b * b + c * c); }
    }
    if (n != 0.0) {
        *angle = 2.0 * atan2(n, fabs(q[0]));
        if (q[0] < 0.0) n = -n;
        axis[0] = q[1] / n; axis[1] = q[2] / n; axis[2] = q[3] / n;
    } else {
        *angle = 0.0; axis[0] = 1.0; axis[1] = 0.0; axis[2] = 0.0;
    }
}
// Eigen: a.angularDistance(b)
MLH_IE_HD double ie_angular_distance(const double a[4], const double b[4])
{
    double bc[4], d[4];
    pg_qconj(b, bc);
    pg_qmul(a, bc, d);
    return 2.0 * atan2(sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]), fabs(d[0]));
}
// Eigen: q.toRotationMatrix(), row-major
MLH_IE_HD void ie_rotation_matrix(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
                 tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// the two distances of checkScrewMotion (cpp:106-109); poses [t, q(xyzw)]
MLH_IE_HD void ie_screw_distances(const double pose_ref[7], const double pose_data[7], double *r_dis, double *t_dis)
{
    double qr[4], qd[4], ar, ad, xr[3], xd[3];
    pg_q_of_pose(pose_ref, qr); pg_q_of_pose(pose_data, qd);
    ie_angle_axis(qr, &ar, xr); ie_angle_axis(qd, &ad, xd);
    *r_dis = fabs(ar - ad);
    *t_dis = fabs((pose_ref[0] * xr[0] + pose_ref[1] * xr[1] + pose_ref[2] * xr[2]) - (pose_data[0] * xd[0] + pose_data[1] * xd[1] + pose_data[2] * xd[2]));
}
MLH_IE_HD bool ie_check_screw_motion(const double pose_ref[7], const double pose_data[7], double eps_r, double eps_t)
{
    double r_dis, t_dis;
    ie_screw_distances(pose_ref, pose_data, &r_dis, &t_dis);
    return (r_dis < eps_r) && (t_dis < eps_t);
}

// huber (L - R) of cpp:128-153 with calib_ext_ = ext: blk 4 x 4 row-major, columns (x, y, z, w). Host only (see "Chosen").
inline void ie_rot_block(const double pose_ref[7], const double pose_data[7], const double ext[7], double blk[16])
{
    double r1[4], qd[4], qe[4], qi[4], t[4], r2[4];
    pg_q_of_pose(pose_ref, r1); pg_q_of_pose(pose_data, qd); pg_q_of_pose(ext, qe);
    pg_eigen_qinv(qe, qi);
    { const double n = std::sqrt(qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3]); if (n != 0.0) for (int c = 0; c < 4; ++c) qi[c] /= n; }      // Pose(q^-1, ..)
    pg_qmul(qe, qd, t);
    pg_qmul(t, qi, r2);
    const double angular_distance = 180 / M_PI * ie_angular_distance(r1, r2);
    const double huber = angular_distance > 5.0 ? 5.0 / angular_distance : 1.0;
    double L[16], R[16];
    const auto fill = [](double *M, double w, const double *q, double sgn) {
        const double S[9] = {0.0, -q[2], q[1], q[2], 0.0, -q[0], -q[1], q[0], 0.0};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) M[4 * r + c] = w * (r == c ? 1.0 : 0.0) + sgn * S[3 * r + c];
            M[4 * r + 3] = q[r];
            M[12 + r] = -q[r];
        }
        M[15] = w;
    };
    fill(L, r1[0], r1 + 1, 1.0);
    fill(R, qd[0], qd + 1, -1.0);
    for (int i = 0; i < 16; ++i) blk[i] = huber * (L[i] - R[i]);
}

// the Huber weight of the translation rows (cpp:270-271, 292-293)
MLH_IE_HD double ie_trans_huber(const double pose_ref[7], const double pose_data[7])
{
    double r_dis, t_dis;
    ie_screw_distances(pose_ref, pose_data, &r_dis, &t_dis);
    return t_dis > 0.04 ? 0.04 / t_dis : 1.0;
}
// row `comp` (0..2) of one set's block of A | b (cpp:272-273); q_zyx (w, x, y, z)
MLH_IE_HD void ie_row_nonplanar(const double pose_ref[7], const double pose_data[7], const double q_zyx[4], int comp, double A[3], double *b)
{
    const double huber = ie_trans_huber(pose_ref, pose_data);
    double qr[4], R[9], rt[3];
    pg_q_of_pose(pose_ref, qr);
    ie_rotation_matrix(qr, R);
    for (int c = 0; c < 3; ++c) A[c] = huber * (R[3 * comp + c] - (c == comp ? 1.0 : 0.0));
    pg_eigen_qrot(q_zyx, pose_data, rt);
    *b = rt[comp] - pose_ref[comp];
}
// row `comp` (0..1) of one set's block of G | w (cpp:294-301); q_yx (w, x, y, z)
MLH_IE_HD void ie_row_planar(const double pose_ref[7], const double pose_data[7], const double q_yx[4], int comp, double G[4], double *w)
{
    const double huber = ie_trans_huber(pose_ref, pose_data);
    double qr[4], R[9], Ryx[9], p[3];
    pg_q_of_pose(pose_ref, qr);
    ie_rotation_matrix(qr, R);
    ie_rotation_matrix(q_yx, Ryx);
    const double n[3] = {Ryx[6], Ryx[7], Ryx[8]};
    const double tn = pose_data[0] * n[0] + pose_data[1] * n[1] + pose_data[2] * n[2];
    const double v[3] = {pose_data[0] - tn * n[0], pose_data[1] - tn * n[1], pose_data[2] - tn * n[2]};
    pg_eigen_qrot(q_yx, v, p);
    const double J[2] = {R[3 * comp] - (comp == 0 ? 1.0 : 0.0), R[3 * comp + 1] - (comp == 1 ? 1.0 : 0.0)};
    const double K[2] = {comp == 0 ? p[0] : p[1], comp == 0 ? -p[1] : p[0]};
    G[0] = huber * J[0]; G[1] = huber * J[1]; G[2] = huber * K[0]; G[3] = huber * K[1];
    *w = pose_ref[comp];
}
// calib_ext_ = Pose(q_zyx, x) (cpp:277)
MLH_IE_HD void ie_tail_nonplanar(const double q_zyx[4], const double x[3], double pose[7]) { pg_pose_make(q_zyx, x, pose); }
// cpp:304-307: x = (-m0, -m1, 0), yaw = atan2(m3, m2), calib_ext_ = Pose(q_z q_yx, x)
MLH_IE_HD void ie_tail_planar(const double q_yx[4], const double m[4], double pose[7])
{
    const double x[3] = {-m[0], -m[1], 0.0};
    const double yaw = atan2(m[3], m[2]);
    const double qz[4] = {cos(yaw / 2.0), 0.0, 0.0, sin(yaw / 2.0)};
    double q[4];
    pg_qmul(qz, q_yx, q);
    pg_pose_make(q, x, pose);
}
// cpp:194-196: the null vector (x, y, z, w) under the sign rule
MLH_IE_HD void ie_null_vector(const double V[16], double q_xyzw[4])
{
    double x[4] = {V[3], V[7], V[11], V[15]};
    if (x[0] < 0.0) { x[0] = -x[0]; x[1] = -x[1]; x[2] = -x[2]; x[3] = -x[3]; }
    q_xyzw[0] = x[0]; q_xyzw[1] = x[1]; q_xyzw[2] = x[2]; q_xyzw[3] = x[3];
}

// ---------------------------------------------------------------- the bookkeeping of addPose and the cov states (host)
struct IeHeapEntry { size_t first; double w0; };      // pose_laser_add_.first and what rotCmp reads of .second: second[0].q_.w()
struct IeRotCmp {
    bool operator()(const IeHeapEntry &pose_r, const IeHeapEntry &pose_l) const { return (pose_l.w0 > pose_r.w0); }     // h:36-39
};
struct IeBook {
    mlh_initext_opts opts;
    double rot_cov_thre = 0.25;
    std::priority_queue<IeHeapEntry, std::vector<IeHeapEntry>, IeRotCmp> pq;
    size_t n_sets = 0;                                   // v_pose_.size()
    long add_first = -1;                                 // pose_laser_add_.first (-1: default-constructed)
    double add_poses[IE_MAX_LIDAR * 7];                  // pose_laser_add_.second
    double calib_ext[IE_MAX_LIDAR * 7];                  // calib_ext_ as [t, q(xyzw)]
    bool cov_rot[IE_MAX_LIDAR], cov_pos[IE_MAX_LIDAR];
    bool full_cov_rot = false, full_cov_pos = false;

    // clearState + setParameter (cpp:26-63), and the heap emptied
    void reset(const mlh_initext_opts &o)
    {
        opts = o;
        rot_cov_thre = ie_rot_cov_thre(o);
        pq = decltype(pq)();
        n_sets = 0; add_first = -1;
        std::memset(add_poses, 0, sizeof(add_poses));
        for (int l = 0; l < IE_MAX_LIDAR; ++l) {
            const double q[4] = {o.qbl[l][3], o.qbl[l][0], o.qbl[l][1], o.qbl[l][2]};
            if (l < o.n_lidar) pg_pose_make(q, o.tbl[l], calib_ext + 7 * l);
            else { std::memset(calib_ext + 7 * l, 0, sizeof(double) * 7); calib_ext[7 * l + 6] = 1.0; }
            cov_rot[l] = cov_pos[l] = (l == o.idx_ref);
        }
        full_cov_rot = full_cov_pos = false;
    }
    // the check of cpp:83 over every LiDAR
    bool screw_ok(const double *poses) const
    {
        bool b_check = true;
        for (int i = 0; i < opts.n_lidar; ++i) b_check = (b_check && ie_check_screw_motion(poses + 7 * opts.idx_ref, poses + 7 * i, opts.eps_r, opts.eps_t));
        return b_check;
    }
    // cpp:86-98 for an accepted set: the slot of v_pose_ it takes
    size_t accept(const double *poses)
    {
        const double w0 = poses[6];
        size_t slot;
        if (pq.size() < size_t(opts.n_pose)) {
            slot = pq.size();
            ++n_sets;
            pq.push(IeHeapEntry{slot, w0});
        } else {
            slot = pq.top().first;
            pq.pop();
            pq.push(IeHeapEntry{slot, w0});
        }
        add_first = long(slot);
        std::memcpy(add_poses, poses, sizeof(double) * 7 * size_t(opts.n_lidar));
        return slot;
    }
    bool window_full() const { return pq.size() >= size_t(opts.window_size); }       // cpp:125, negated
    void set_cov_rotation(int idx)
    {
        cov_rot[idx] = true;
        full_cov_rot = true;
        for (int l = 0; l < opts.n_lidar; ++l) full_cov_rot = full_cov_rot && cov_rot[l];
    }
    void set_cov_translation(int idx)
    {
        cov_pos[idx] = true;
        full_cov_pos = true;
        for (int l = 0; l < opts.n_lidar; ++l) full_cov_pos = full_cov_pos && cov_pos[l];
    }
};

// ---------------------------------------------------------------- both solves on the host (one "lane" looping over svd_dev.hpp)
struct IeHostSolve {
    double q[4], t[3];                       // q (x, y, z, w)
    double rot_sv[4], trans_sv[4];
    int rot_converged, trans_solved, trans_rank, rot_sweeps, trans_sweeps;
};
// the SVD, the null vector and the decision of cpp:154-201 on Q (IE_Q_ROWS x 4, left untouched)
inline void ie_host_rotation(const double *Q, double rot_cov_thre, IeHostSolve &S)
{
    std::vector<double> a(Q, Q + size_t(IE_Q_ROWS) * 4);
    SvdPtrRows<4> rows{a.data(), IE_Q_ROWS};
    SvdNoRed red;
    double V[16];
    int perm[4];
    S.rot_sweeps = svd_onesided_jacobi<4>(rows, red, IE_SVD_TOL, S.rot_sv, V, perm);
    ie_null_vector(V, S.q);
    S.rot_converged = S.rot_sv[2] > rot_cov_thre ? 1 : 0;
}
// calibExTranslation (cpp:243-309) over the n_sets stored sets (300 x n_lidar x 7) with the rotation q_xyzw; S.q / S.t <- the new calib_ext_
inline void ie_host_translation(const double *sets, int n_sets, int n_lidar, int idx_ref, int lidar, int planar, const double q_xyzw[4], IeHostSolve &S)
{
    const double q[4] = {q_xyzw[3], q_xyzw[0], q_xyzw[1], q_xyzw[2]};
    double pose[7];
    SvdNoRed red;
    for (int c = 0; c < 4; ++c) S.trans_sv[c] = 0.0;
    if (!planar) {
        const int rows_n = 3 * n_sets;
        std::vector<double> a(size_t(rows_n) * 3 + 1), b(size_t(rows_n) + 1);
        for (int r = 0; r < rows_n; ++r) ie_row_nonplanar(sets + size_t(r / 3 * n_lidar + idx_ref) * 7, sets + size_t(r / 3 * n_lidar + lidar) * 7, q, r % 3, &a[size_t(r) * 3], &b[size_t(r)]);
        SvdPtrRows<3> rows{a.data(), rows_n};
        double V[9], utb[3] = {0.0, 0.0, 0.0}, dots[3] = {0.0, 0.0, 0.0}, x[3];
        int perm[3];
        S.trans_sweeps = svd_onesided_jacobi<3>(rows, red, IE_SVD_TOL, S.trans_sv, V, perm);
        for (int r = 0; r < rows_n; ++r) for (int c = 0; c < 3; ++c) dots[c] += a[size_t(r) * 3 + c] * b[size_t(r)];
        for (int j = 0; j < 3; ++j) utb[j] = dots[perm[j]];
        S.trans_rank = svd_solve<3>(S.trans_sv, V, utb, x);
        ie_tail_nonplanar(q, x, pose);
    } else {
        const int rows_n = 2 * n_sets;
        std::vector<double> a(size_t(rows_n) * 4 + 1), b(size_t(rows_n) + 1);
        for (int r = 0; r < rows_n; ++r) ie_row_planar(sets + size_t(r / 2 * n_lidar + idx_ref) * 7, sets + size_t(r / 2 * n_lidar + lidar) * 7, q, r % 2, &a[size_t(r) * 4], &b[size_t(r)]);
        SvdPtrRows<4> rows{a.data(), rows_n};
        double V[16], utb[4] = {0.0, 0.0, 0.0, 0.0}, dots[4] = {0.0, 0.0, 0.0, 0.0}, m[4];
        int perm[4];
        S.trans_sweeps = svd_onesided_jacobi<4>(rows, red, IE_SVD_TOL, S.trans_sv, V, perm);
        for (int r = 0; r < rows_n; ++r) for (int c = 0; c < 4; ++c) dots[c] += a[size_t(r) * 4 + c] * b[size_t(r)];
        for (int j = 0; j < 4; ++j) utb[j] = dots[perm[j]];
        S.trans_rank = svd_solve<4>(S.trans_sv, V, utb, m);
        ie_tail_planar(q, m, pose);
    }
    S.q[0] = pose[3]; S.q[1] = pose[4]; S.q[2] = pose[5]; S.q[3] = pose[6];
    S.t[0] = pose[0]; S.t[1] = pose[1]; S.t[2] = pose[2];
    S.trans_solved = 1;
}

}  // namespace mlh
