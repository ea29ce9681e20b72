// The host side of the loop closure's local registration (loopreg.hip; the facade's LoopLocalMap / LoopRegistration), host arithmetic only, f64 unless said
// otherwise: option validation, the keyframe windows and matrix chains of PoseGraph::constructLocalMap (mloam_loop/src/pose_graph.cpp:374-410), and the rules of
// LoopRegistration::performLocalRegistration (mloam_loop/src/loop_registration.cpp:114-210) that run between its device launches -- the pose conversions, the
// 0.2 rule, the cost and the acceptance. A header of its own so that a stand-alone host program can run it under a sanitizer (tests/host/loopreg_host_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/mloam_hip.h"

namespace mlh {

constexpr int LOOP_MAX_OUTER = 8;            // mlh_loop_result::outer has this many records

// the argument at fault, or nullptr
inline const char *loop_opts_fault(const mlh_loop_opts &o)
{
    const auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!pos(o.leaf_surf)) return "leaf_surf";
    if (!pos(o.leaf_corner)) return "leaf_corner";
    if (o.history_search_num < 0 || o.history_search_num > 4096) return "history_search_num";
    if (o.max_outer < 1 || o.max_outer > LOOP_MAX_OUTER) return "max_outer";
    if (o.max_lm_iterations < 0 || o.max_lm_iterations > 200) return "max_lm_iterations";
    if (std::isnan(o.local_registration_threshold)) return "local_registration_threshold";
    if (!pos(o.huber_delta)) return "huber_delta";
    if (!pos(o.match_sq_dis_surf)) return "match_sq_dis_surf";
    if (!pos(o.match_sq_dis_corner)) return "match_sq_dis_corner";
    if (!std::isfinite(o.plane_dis) || o.plane_dis < 0.0) return "plane_dis";
    if (!std::isfinite(o.line_eig_ratio) || o.line_eig_ratio < 0.f) return "line_eig_ratio";
    if (std::isnan(o.min_match_ratio)) return "min_match_ratio";
    return nullptr;
}

inline void loop_opts_defaults(mlh_loop_opts &o)
{
    o = mlh_loop_opts();
    o.leaf_surf = 0.4f; o.leaf_corner = 0.4f;                 // pose_graph.cpp:33-34
    o.history_search_num = 20;                                // LOOP_HISTORY_SEARCH_NUM (config_loop_realvehicle.yaml)
    o.max_outer = 2; o.max_lm_iterations = 5;                 // loop_registration.cpp:117, 187
    o.local_registration_threshold = 2000.0;                  // LOOP_LOCAL_REGISTRATION_THRESHOLD
    o.huber_delta = 1.0;                                      // cpp:121
    o.match_sq_dis_surf = 2.0f; o.match_sq_dis_corner = 5.0f; // feature_extract.hpp:203, 105
    o.plane_dis = 0.2;                                        // hpp:221
    o.line_eig_ratio = 3.f;                                   // hpp:130
    o.min_match_ratio = 0.2;                                  // cpp:158-159
}

// ---- 4 x 4 row-major rigid transforms
inline void loop_mat_mul(const double A[16], const double B[16], double C[16])
{
    double t[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = A[r * 4] * B[c];
            for (int k = 1; k < 4; ++k) s += A[r * 4 + k] * B[k * 4 + c];
            t[r * 4 + c] = s;
        }
    for (int i = 0; i < 16; ++i) C[i] = t[i];
}
// CHOSEN: the inverse of a rigid transform as [R^T, -R^T t] (the reference calls Matrix4d::inverse(), a general 4 x 4 inverse whose rounding is the library's)
inline void loop_rigid_inverse(const double T[16], double Ti[16])
{
    double t[16] = {0};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) t[r * 4 + c] = T[c * 4 + r];
        t[r * 4 + 3] = -((T[0 * 4 + r] * T[3] + T[1 * 4 + r] * T[7]) + T[2 * 4 + r] * T[11]);
    }
    t[15] = 1.0;
    for (int i = 0; i < 16; ++i) Ti[i] = t[i];
}
inline void loop_mat_cast(const double T[16], float Tf[16]) { for (int i = 0; i < 16; ++i) Tf[i] = float(T[i]); }

// Eigen::Quaterniond::toRotationMatrix into the 3 x 3 block of a row-major 4 x 4; q = (x, y, z, w)
inline void loop_quat_to_mat(const double q[4], double T[16])
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    T[0] = 1.0 - (tyy + tzz); T[1] = txy - twz;         T[2] = txz + twy;
    T[4] = txy + twz;         T[5] = 1.0 - (txx + tzz); T[6] = tyz - twx;
    T[8] = txz - twy;         T[9] = tyz + twx;         T[10] = 1.0 - (txx + tyy);
}
// Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h: quaternionbase_assign_impl<Other, 3, 3>), not normalised; the trace summed left to right
inline void loop_mat_to_quat(const double T[16], double q[4])
{
    const auto m = [&](int r, int c) { return T[r * 4 + c]; };
    double t = (m(0, 0) + m(1, 1)) + m(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m(2, 1) - m(1, 2)) * t;
        q[1] = (m(0, 2) - m(2, 0)) * t;
        q[2] = (m(1, 0) - m(0, 1)) * t;
    } else {
        int i = 0;
        if (m(1, 1) > m(0, 0)) i = 1;
        if (m(2, 2) > m(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m(k, j) - m(j, k)) * t;
        q[j] = (m(j, i) + m(i, j)) * t;
        q[k] = (m(k, i) + m(i, k)) * t;
    }
}
// loop_registration.cpp:124-132: para_pose [t, q(xyzw)] of T_relative
inline void loop_pose_of(const double T[16], double pose[7])
{
    loop_mat_to_quat(T, pose + 3);
    pose[0] = T[3]; pose[1] = T[7]; pose[2] = T[11];
}
// cpp:194-197: the rotation and translation blocks of T_relative are overwritten, its last row stays
inline void loop_mat_of(const double pose[7], double T[16])
{
    loop_quat_to_mat(pose + 3, T);
    T[3] = pose[0]; T[7] = pose[1]; T[11] = pose[2];
}

// cpp:158-159, as written: features.size() against the data cloud's points. corner_num counts two features per matched point, so its ratio reaches 2; an empty
// cloud gives 0 / 0 = NaN, and NaN <= ratio is false: that kind alone keeps the loop going.
inline bool loop_too_few_matches(size_t surf_num, size_t surf_size, size_t corner_num, size_t corner_size, double ratio)
{
    return 1.0 * double(surf_num) / double(surf_size) <= ratio && 1.0 * double(corner_num) / double(corner_size) <= ratio;
}
inline bool loop_accepted(double opti_cost, double threshold) { return opti_cost <= threshold; }        // cpp:202

// ---- PoseGraph::constructLocalMap's keyframe windows (pose_graph.cpp:374-380, 398-404). has(index): getKeyFrame(index) != NULL.
template <typename Has> inline std::vector<int> loop_data_window(int que_index, int history, Has has)
{
    std::vector<int> out;
    for (int j = -history; j <= 0; ++j) {
        if (que_index + j < 0) continue;
        if (!has(que_index + j)) continue;
        out.push_back(que_index + j);
    }
    return out;
}
template <typename Has> inline std::vector<int> loop_model_window(int que_index, int match_index, int history, Has has)
{
    std::vector<int> out;
    for (int j = -history; j <= history; ++j) {
        if (match_index + j < 0 || match_index + j >= que_index) continue;
        if (!has(match_index + j)) continue;
        out.push_back(match_index + j);
    }
    return out;
}
// cpp:381-382: T_ini_map_kf = pose_ini.T_ * (cur_kf.T_^-1 * tmp_kf.T_); cpp:405: T_relative = old_kf.T_^-1 * tmp_kf.T_; then .cast<float>()
inline void loop_data_transform(const double T_ini[16], const double T_cur[16], const double T_kf[16], float out[16])
{
    double inv[16], rel[16], m[16];
    loop_rigid_inverse(T_cur, inv);
    loop_mat_mul(inv, T_kf, rel);
    loop_mat_mul(T_ini, rel, m);
    loop_mat_cast(m, out);
}
inline void loop_model_transform(const double T_old[16], const double T_kf[16], float out[16])
{
    double inv[16], rel[16];
    loop_rigid_inverse(T_old, inv);
    loop_mat_mul(inv, T_kf, rel);
    loop_mat_cast(rel, out);
}

}  // namespace mlh
