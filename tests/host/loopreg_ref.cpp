// TEST INFRASTRUCTURE: the restatement of the loop closure's local registration, written from the reference's text and never from the kernels. Every GPU result of
// tests/test_gpu_loopreg.py is compared against this file; tests/test_loopreg_cases.py holds it against hand-computed values. Built with plain g++
// (-O2 -ffp-contract=off) into a shared object over the checker's headers as they are: kdtree.hpp (the exact k-NN standing in for pcl::KdTreeFLANN, ties to the
// lower index), linalg.hpp (Eigen's SelfAdjointEigenSolver<Matrix3f> and ColPivHouseholderQR<MatrixXf> restated), lm.hpp (ceres::Solve restated), geometry.hpp.
//   pointAssociateToMap(Matrix4f)     mloam_loop/include/mloam_loop/utility/feature_extract.hpp:28-43
//   matchCornerFromMap                hpp:77-171
//   matchSurfFromMap                  hpp:174-247
//   LidarMapPlaneNormFactor::Evaluate mloam_loop/include/mloam_loop/factor/lidar_map_plane_norm_factor.hpp:56-87 (sqrt_info_ = I: the identity covariance is passed)
//   performLocalRegistration          mloam_loop/src/loop_registration.cpp:104-211 (max_solver_time_in_seconds is a wall-clock limit and is not restated)
//   pcl::transformPointCloud          PCL 1.8 common/impl/transforms.hpp: x' = m00 x + m01 y + m02 z + m03, f32
// Library arithmetic the reference leaves to Eigen is restated as the project's other restatements do: three-term f32 sums left to right; `double * Vector3f` with
// the double converted to float first (Eigen's scalar promotion); `Vector3f /= double` likewise; Quaterniond(Matrix3d) and toRotationMatrix from Eigen's Geometry
// module; HuberLoss and the loss correction of a residual block from Ceres (rho'' <= 0 outside the inlier band: the block is scaled by sqrt(rho')).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "kdtree.hpp"
#include "linalg.hpp"
#include "lm.hpp"
#include "geometry.hpp"

namespace {

struct V3f { float x, y, z; };
inline V3f sub(const V3f &a, const V3f &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3f cross(const V3f &a, const V3f &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float sqnorm(const V3f &a) { return (a.x * a.x + a.y * a.y) + a.z * a.z; }
inline float norm(const V3f &a) { return std::sqrt(sqnorm(a)); }
inline V3f normalized(const V3f &a)
{
    const float z = sqnorm(a);
    if (z > 0.f) { const float s = std::sqrt(z); return {a.x / s, a.y / s, a.z / s}; }
    return a;
}

// T: row-major 4 x 4 f32
inline V3f associate(const float *T, const float *p)
{
    return {((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3], ((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7], ((T[8] * p[0] + T[9] * p[1]) + T[10] * p[2]) + T[11]};
}

struct Feature { double point[3]; double coeffs[4]; };

struct Cloud {
    const float *p; int n;      // n x 4 floats {x, y, z, intensity}
    orc::KdTree tree;
    void build() { tree.build(p, 4, n); }
};

// returns features.size(); valid / coeffs per data point may be null
// dbg (may be null): per data point sq_dis[4] and the largest |n . q + d| over the five neighbours, as f32 (2 floats; +inf / 0 where the search or the test ended it)
int match_surf(const Cloud &map, const float *data, int m, const float *T, float sq_thr, double plane_dis, std::vector<Feature> &features, uint8_t *valid, double *coeffs,
               float *dbg = nullptr)
{
    const int num_neighbors = 5;
    features.clear();
    for (int i = 0; i < m; ++i) {
        const float *point_ori = data + 4 * size_t(i);
        const V3f point_sel = associate(T, point_ori);
        if (valid) valid[i] = 0;
        if (coeffs) for (int q = 0; q < 4; ++q) coeffs[4 * size_t(i) + q] = 0.0;
        if (dbg) { dbg[2 * size_t(i)] = INFINITY; dbg[2 * size_t(i) + 1] = 0.f; }
        int idx[5]; float sq_dis[5];
        const float q[3] = {point_sel.x, point_sel.y, point_sel.z};
        if (map.tree.knn(q, num_neighbors, idx, sq_dis) < num_neighbors) continue;
        if (dbg) dbg[2 * size_t(i)] = sq_dis[4];
        if (!(sq_dis[num_neighbors - 1] < sq_thr)) continue;
        float mat_A[15], mat_B[5];
        for (int j = 0; j < num_neighbors; ++j) {
            mat_A[3 * j + 0] = map.p[4 * size_t(idx[j]) + 0]; mat_A[3 * j + 1] = map.p[4 * size_t(idx[j]) + 1]; mat_A[3 * j + 2] = map.p[4 * size_t(idx[j]) + 2];
            mat_B[j] = -1.f;
        }
        float nrm[3];
        orc::colpiv_qr_solve_f(mat_A, mat_B, num_neighbors, nrm);
        V3f n{nrm[0], nrm[1], nrm[2]};
        const float negative_OA_dot_norm = 1 / norm(n);
        n = normalized(n);
        if (dbg)
            for (int j = 0; j < num_neighbors; ++j)
                dbg[2 * size_t(i) + 1] = std::max(dbg[2 * size_t(i) + 1], std::fabs(n.x * mat_A[3 * j + 0] + n.y * mat_A[3 * j + 1] + n.z * mat_A[3 * j + 2] + negative_OA_dot_norm));
        bool plane_valid = true;
        for (int j = 0; j < num_neighbors; ++j) {
            const float v = n.x * mat_A[3 * j + 0] + n.y * mat_A[3 * j + 1] + n.z * mat_A[3 * j + 2] + negative_OA_dot_norm;
            if (double(std::fabs(v)) > plane_dis) { plane_valid = false; break; }
        }
        if (!plane_valid) continue;
        Feature f;
        for (int q2 = 0; q2 < 3; ++q2) f.point[q2] = double(point_ori[q2]);
        f.coeffs[0] = double(n.x); f.coeffs[1] = double(n.y); f.coeffs[2] = double(n.z); f.coeffs[3] = double(negative_OA_dot_norm);
        features.push_back(f);
        if (valid) valid[i] = 1;
        if (coeffs) for (int q2 = 0; q2 < 4; ++q2) coeffs[4 * size_t(i) + q2] = f.coeffs[q2];
    }
    return int(features.size());
}

// dbg (may be null): per data point w1[3], w2[3], ld_p1, ld_p2, eig[3], sq_dis[4] as f32 (12 floats)
int match_corner(const Cloud &map, const float *data, int m, const float *T, float sq_thr, float eig_ratio, std::vector<Feature> &features, uint8_t *valid, double *coeffs,
                 float *dbg)
{
    const int num_neighbors = 5;
    features.clear();
    for (int i = 0; i < m; ++i) {
        const float *point_ori = data + 4 * size_t(i);
        const V3f point_sel = associate(T, point_ori);
        if (valid) valid[i] = 0;
        if (coeffs) for (int q = 0; q < 8; ++q) coeffs[8 * size_t(i) + q] = 0.0;
        if (dbg) for (int q = 0; q < 12; ++q) dbg[12 * size_t(i) + q] = 0.f;
        int idx[5]; float sq_dis[5];
        const float q[3] = {point_sel.x, point_sel.y, point_sel.z};
        if (map.tree.knn(q, num_neighbors, idx, sq_dis) < num_neighbors) continue;
        if (dbg) dbg[12 * size_t(i) + 11] = sq_dis[4];
        if (!(sq_dis[num_neighbors - 1] < sq_thr)) continue;
        V3f near[5], center{0.f, 0.f, 0.f};
        for (int j = 0; j < num_neighbors; ++j) {
            near[j] = {map.p[4 * size_t(idx[j]) + 0], map.p[4 * size_t(idx[j]) + 1], map.p[4 * size_t(idx[j]) + 2]};
            center.x += near[j].x; center.y += near[j].y; center.z += near[j].z;
        }
        const float k = float(1.0 * num_neighbors);      // Vector3f::operator/=(const float &): the double is converted
        center.x /= k; center.y /= k; center.z /= k;
        float cov[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        for (int j = 0; j < num_neighbors; ++j) {
            const V3f z = sub(near[j], center);
            const float zz[3] = {z.x, z.y, z.z};
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) cov[r][c] += zz[r] * zz[c];
        }
        const orc::Eig3f es = orc::eig3_sym_f(cov);
        const V3f unit_direction{es.vec[0][2], es.vec[1][2], es.vec[2][2]};
        if (dbg) { dbg[12 * size_t(i) + 8] = es.val[0]; dbg[12 * size_t(i) + 9] = es.val[1]; dbg[12 * size_t(i) + 10] = es.val[2]; }
        if (!(es.val[2] > eig_ratio * es.val[1])) continue;
        const V3f X0 = point_sel, point_on_line = center;
        const float s = float(0.1), ms = float(-0.1);     // Eigen promotes the double literal to the expression's scalar
        const V3f X1{s * unit_direction.x + point_on_line.x, s * unit_direction.y + point_on_line.y, s * unit_direction.z + point_on_line.z};
        const V3f X2{ms * unit_direction.x + point_on_line.x, ms * unit_direction.y + point_on_line.y, ms * unit_direction.z + point_on_line.z};
        const V3f n = cross(sub(X1, X0), sub(X2, X0));
        const V3f w2 = normalized(n);
        const V3f w1 = normalized(cross(w2, sub(X2, X1)));
        const float ld_1 = norm(n) / norm(sub(X1, X2));
        const float ld_2 = 0.0;
        const float ld_p1 = -(w1.x * point_sel.x + w1.y * point_sel.y + w1.z * point_sel.z - ld_1);
        const float ld_p2 = -(w2.x * point_sel.x + w2.y * point_sel.y + w2.z * point_sel.z - ld_2);
        Feature f1, f2;
        for (int q2 = 0; q2 < 3; ++q2) f1.point[q2] = f2.point[q2] = double(point_ori[q2]);
        f1.coeffs[0] = double(w1.x) * 0.5; f1.coeffs[1] = double(w1.y) * 0.5; f1.coeffs[2] = double(w1.z) * 0.5; f1.coeffs[3] = double(ld_p1) * 0.5;
        f2.coeffs[0] = double(w2.x) * 0.5; f2.coeffs[1] = double(w2.y) * 0.5; f2.coeffs[2] = double(w2.z) * 0.5; f2.coeffs[3] = double(ld_p2) * 0.5;
        features.push_back(f1);
        features.push_back(f2);
        if (valid) valid[i] = 1;
        if (coeffs) for (int q2 = 0; q2 < 4; ++q2) { coeffs[8 * size_t(i) + q2] = f1.coeffs[q2]; coeffs[8 * size_t(i) + 4 + q2] = f2.coeffs[q2]; }
        if (dbg) {
            float *d = dbg + 12 * size_t(i);
            d[0] = w1.x; d[1] = w1.y; d[2] = w1.z; d[3] = w2.x; d[4] = w2.y; d[5] = w2.z; d[6] = ld_p1; d[7] = ld_p2;
        }
    }
    return int(features.size());
}

// LidarMapPlaneNormFactor::Evaluate with sqrt_info_ = I: residuals[3], jacobian 3 x 7 row-major (last column zero)
void factor_evaluate(const double point[3], const double coeff[4], const double *param, double *residuals, double *jac)
{
    const orc::Quatd q{param[3], param[4], param[5], param[6]};
    const orc::Vec3d t{param[0], param[1], param[2]};
    const double w[3] = {coeff[0], coeff[1], coeff[2]};
    const double d = coeff[3];
    const orc::Vec3d lp0 = orc::quat_rotate(q, orc::Vec3d{point[0], point[1], point[2]});
    const double lp[3] = {lp0.x + t.x, lp0.y + t.y, lp0.z + t.z};
    const double a = ((w[0] * lp[0] + w[1] * lp[1]) + w[2] * lp[2]) + d;
    for (int r = 0; r < 3; ++r) residuals[r] = a * w[r];
    if (!jac) return;
    double R[9], W[9], S[9], WR[9], WRS[9];
    orc::quat_to_rot(q, R);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) W[r * 3 + c] = w[r] * w[c];      // w.asDiagonal() * [w^T; w^T; w^T]
    orc::skew(orc::Vec3d{point[0], point[1], point[2]}, S);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { double s = 0.0; for (int k = 0; k < 3; ++k) s += (-W[r * 3 + k]) * R[k * 3 + c]; WR[r * 3 + c] = s; }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { double s = 0.0; for (int k = 0; k < 3; ++k) s += WR[r * 3 + k] * S[k * 3 + c]; WRS[r * 3 + c] = s; }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { jac[r * 7 + c] = W[r * 3 + c]; jac[r * 7 + 3 + c] = WRS[r * 3 + c]; }
        jac[r * 7 + 6] = 0.0;
    }
}

// the problem's normal equations as Ceres hands them to the linear solver: every block loss-corrected (HuberLoss(delta) on s = |r|^2), J restricted to the six
// local parameters (PoseLocalParameterization::ComputeJacobian is [I6; 0]); *outside (may be null) <- blocks outside the inlier band
void problem_evaluate(const std::vector<Feature> &fs, const double *x, double delta, orc::NormalEq &ne, int *outside)
{
    std::memset(&ne, 0, sizeof(ne));
    int out = 0;
    for (const Feature &f : fs) {
        double r[3], J[21];
        factor_evaluate(f.point, f.coeffs, x, r, J);
        const double s = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        double rho0 = s, rho1 = 1.0;
        const double b = delta * delta;
        if (s > b) { const double rr = std::sqrt(s); rho0 = 2.0 * delta * rr - b; rho1 = std::max(std::numeric_limits<double>::min(), delta / rr); ++out; }
        const double sc = std::sqrt(rho1);
        for (int k = 0; k < 3; ++k) {
            const double rk = r[k] * sc;
            double Jk[6];
            for (int c = 0; c < 6; ++c) Jk[c] = J[k * 7 + c] * sc;
            for (int a = 0; a < 6; ++a) { ne.g[a] += Jk[a] * rk; for (int c = 0; c < 6; ++c) ne.H[a * 6 + c] += Jk[a] * Jk[c]; }
        }
        ne.cost += 0.5 * rho0;
        ne.n += 1;
    }
    if (outside) *outside = out;
}

// Eigen::Quaterniond(Matrix3d) (Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>); T row-major 4 x 4; q = (x, y, z, w)
void mat_to_quat(const double *T, double *q)
{
    auto m = [&](int r, int c) { return T[r * 4 + c]; };
    double t = m(0, 0) + m(1, 1) + m(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m(2, 1) - m(1, 2)) * t; q[1] = (m(0, 2) - m(2, 0)) * t; q[2] = (m(1, 0) - m(0, 1)) * t;
    } else {
        int i = 0;
        if (m(1, 1) > m(0, 0)) i = 1;
        if (m(2, 2) > m(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m(k, j) - m(j, k)) * t; q[j] = (m(j, i) + m(i, j)) * t; q[k] = (m(k, i) + m(i, k)) * t;
    }
}

// PoseLocalParameterization::Plus with V_update = I: t += dx_t, q = (q * deltaQ(dx_theta)).normalized()
void pose_plus(const double *x, const double *delta, double *out)
{
    const orc::Quatd q{x[3], x[4], x[5], x[6]};
    const orc::Quatd dq = orc::delta_q(orc::Vec3d{delta[3], delta[4], delta[5]});
    const orc::Quatd p = orc::quat_normalized(orc::quat_mul(q, dq));
    out[0] = x[0] + delta[0]; out[1] = x[1] + delta[1]; out[2] = x[2] + delta[2];
    out[3] = p.x; out[4] = p.y; out[5] = p.z; out[6] = p.w;
}

}  // namespace

extern "C" {

struct lr_opts { int max_outer, max_lm_iterations; double huber_delta, min_match_ratio, threshold; float sq_surf, sq_corner; double plane_dis; float eig_ratio; int pad; };
struct lr_outer { int entered, ran, surf_num, corner_num, lm_iterations, successful_steps, termination, outside; double initial_cost, final_cost; };
struct lr_result { double T[16], para_pose[7], opti_cost; int accepted, n_outer; lr_outer outer[8]; };

void lr_transform(const float *pts, int n, const float *T, float *out)
{
    for (int i = 0; i < n; ++i) {
        const V3f v = associate(T, pts + 4 * size_t(i));
        out[4 * size_t(i) + 0] = v.x; out[4 * size_t(i) + 1] = v.y; out[4 * size_t(i) + 2] = v.z; out[4 * size_t(i) + 3] = pts[4 * size_t(i) + 3];
    }
}

int lr_match_surf(const float *map, int n, const float *data, int m, const float *T, float sq_thr, double plane_dis, uint8_t *valid, double *coeffs, float *dbg)
{
    Cloud c{map, n, {}};
    c.build();
    std::vector<Feature> f;
    return match_surf(c, data, m, T, sq_thr, plane_dis, f, valid, coeffs, dbg);
}

int lr_match_corner(const float *map, int n, const float *data, int m, const float *T, float sq_thr, float eig_ratio, uint8_t *valid, double *coeffs, float *dbg)
{
    Cloud c{map, n, {}};
    c.build();
    std::vector<Feature> f;
    return match_corner(c, data, m, T, sq_thr, eig_ratio, f, valid, coeffs, dbg);
}

void lr_factor(const double *point, const double *coeff, const double *pose, double *residuals, double *jac) { factor_evaluate(point, coeff, pose, residuals, jac); }

void lr_mat_to_quat(const double *T, double *q) { mat_to_quat(T, q); }
void lr_quat_to_mat(const double *q, double *R9) { orc::quat_to_rot(orc::Quatd{q[0], q[1], q[2], q[3]}, R9); }

// both matches at T_match (f32), then the problem's normal equations at `pose`
void lr_evaluate(const float *map_s, int ns, const float *map_c, int nc, const float *data_s, int ms, const float *data_c, int mc, const float *T_match, const double *pose,
                 const lr_opts *o, double *H, double *g, double *cost, int *counts, int *outside)
{
    Cloud cs{map_s, ns, {}}, cc{map_c, nc, {}};
    cs.build(); cc.build();
    std::vector<Feature> fs, fc;
    counts[0] = match_surf(cs, data_s, ms, T_match, o->sq_surf, o->plane_dis, fs, nullptr, nullptr);
    counts[1] = match_corner(cc, data_c, mc, T_match, o->sq_corner, o->eig_ratio, fc, nullptr, nullptr, nullptr);
    fs.insert(fs.end(), fc.begin(), fc.end());
    orc::NormalEq ne;
    problem_evaluate(fs, pose, o->huber_delta, ne, outside);
    std::memcpy(H, ne.H, sizeof(ne.H)); std::memcpy(g, ne.g, sizeof(ne.g));
    *cost = ne.cost;
}

void lr_register(const float *map_s, int ns, const float *map_c, int nc, const float *data_s, int ms, const float *data_c, int mc, const double *T_ini, const lr_opts *o,
                 lr_result *res)
{
    Cloud cs{map_s, ns, {}}, cc{map_c, nc, {}};
    cs.build(); cc.build();
    std::memset(res, 0, sizeof(*res));
    double opti_cost = 1e7;
    double T_relative[16];
    for (int i = 0; i < 16; ++i) T_relative[i] = T_ini[i];
    mat_to_quat(T_relative, res->para_pose + 3);
    res->para_pose[0] = T_relative[3]; res->para_pose[1] = T_relative[7]; res->para_pose[2] = T_relative[11];
    for (int iter_cnt = 0; iter_cnt < o->max_outer; ++iter_cnt) {
        double para_pose[7];
        mat_to_quat(T_relative, para_pose + 3);
        para_pose[0] = T_relative[3]; para_pose[1] = T_relative[7]; para_pose[2] = T_relative[11];
        float Tf[16];
        for (int i = 0; i < 16; ++i) Tf[i] = float(T_relative[i]);
        std::vector<Feature> all_surf_features, all_corner_features;
        const size_t surf_num = size_t(match_surf(cs, data_s, ms, Tf, o->sq_surf, o->plane_dis, all_surf_features, nullptr, nullptr));
        const size_t corner_num = size_t(match_corner(cc, data_c, mc, Tf, o->sq_corner, o->eig_ratio, all_corner_features, nullptr, nullptr, nullptr));
        lr_outer &os = res->outer[iter_cnt];
        os.entered = 1; os.surf_num = int(surf_num); os.corner_num = int(corner_num);
        res->n_outer = iter_cnt + 1;
        if (1.0 * surf_num / size_t(ms) <= o->min_match_ratio && 1.0 * corner_num / size_t(mc) <= o->min_match_ratio) break;
        os.ran = 1;
        std::vector<Feature> all = all_surf_features;
        all.insert(all.end(), all_corner_features.begin(), all_corner_features.end());
        orc::SolveSummary summary;
        int outside0 = -1;
        orc::ceres_like_solve_generic([&](const double *x, orc::NormalEq &ne) { int out; problem_evaluate(all, x, o->huber_delta, ne, &out); if (outside0 < 0) outside0 = out; },
                                      [&](const double *x, const double *d, double *out) { pose_plus(x, d, out); }, para_pose, o->max_lm_iterations, summary);
        os.lm_iterations = summary.num_iterations; os.successful_steps = summary.num_successful_steps; os.termination = summary.termination;
        os.initial_cost = summary.initial_cost; os.final_cost = summary.final_cost; os.outside = outside0;
        opti_cost = std::min(summary.final_cost, opti_cost);
        for (int i = 0; i < 7; ++i) res->para_pose[i] = para_pose[i];
        double R[9];
        orc::quat_to_rot(orc::Quatd{para_pose[3], para_pose[4], para_pose[5], para_pose[6]}, R);
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T_relative[r * 4 + c] = R[r * 3 + c]; T_relative[r * 4 + 3] = para_pose[r]; }
    }
    for (int i = 0; i < 16; ++i) res->T[i] = T_relative[i];
    res->opti_cost = opti_cost;
    res->accepted = opti_cost <= o->threshold ? 1 : 0;
}

}  // extern "C"
