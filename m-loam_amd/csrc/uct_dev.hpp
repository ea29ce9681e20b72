// Per-point uncertainty of the mapper (associate_uct.hpp:196-215) as device functions: one body for every kernel that evaluates it (voxel.hip:
// point_uncertainty_kernel and the thinning pipeline's fused aggregate; keyframes.hip: the keyframe cache's batched association), so that all of
// them perform the same operations in the same order and agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_math.hpp"

namespace mlh {

// evalPointUncertainty of one record (associate_uct.hpp:196-215) as downsampleCurrentScan / cloudUCTAssociateToMap call it: the point is taken back into its
// LiDAR's frame through that LiDAR's extrinsic (pointAssociateToMap: f64 math, f32 store), then cov = G diag(pose covariance, measurement covariance) G^T with
// G = [ I | -[T p]x | R ]. One body for point_uncertainty_kernel and the thinning pipeline's fused aggregate (vsp_aggregate_kernel): the same operations in the same order.
__device__ __forceinline__ void eval_point_cov(const double *ext, const double *upose, const double *upose_cov, int n_lidar, const double *meas, int with_ua,
                                               float x, float y, float z, float inten, double (&cov)[3][3])
{
    int idx = int(inten);
    idx = idx < 0 ? 0 : (idx >= n_lidar ? n_lidar - 1 : idx);
    for (int r_ = 0; r_ < 3; ++r_) for (int c_ = 0; c_ < 3; ++c_) cov[r_][c_] = 0.0;
    if (with_ua) {
        const double *e = ext + idx * 7;
        const q4 qe{e[3], e[4], e[5], e[6]};
        const d3 te{e[0], e[1], e[2]};
        // point_sel = pose_ext^-1 * point_ori, through pointAssociateToMap (f64 math, f32 store) -- cpp:382 / cpp:1148
        const q4 qi{-qe.x, -qe.y, -qe.z, qe.w};
        const d3 mt = qrot(qi, te);
        const d3 ps = qrot(qi, d3{double(x), double(y), double(z)});
        const float sel[3] = {float(ps.x - mt.x), float(ps.y - mt.y), float(ps.z - mt.z)};
        const double *u = upose + idx * 7;
        const q4 q{u[3], u[4], u[5], u[6]};
        const d3 t{u[0], u[1], u[2]};
        // T * [p; 1]
        double R[9];
        qtorot(q, R);
        const double p[3] = {double(sel[0]), double(sel[1]), double(sel[2])};
        double tp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) tp[r] = R[r * 3 + 0] * p[0] + R[r * 3 + 1] * p[1] + R[r * 3 + 2] * p[2] + (r == 0 ? t.x : (r == 1 ? t.y : t.z));
        // G = [ I | -[tp]x | R ]  (3 x 9)
        double G[3][9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) { G[r][c] = (r == c) ? 1.0 : 0.0; G[r][6 + c] = R[r * 3 + c]; }
        G[0][3] = 0.0;    G[0][4] = tp[2];  G[0][5] = -tp[1];
        G[1][3] = -tp[2]; G[1][4] = 0.0;    G[1][5] = tp[0];
        G[2][3] = tp[1];  G[2][4] = -tp[0]; G[2][5] = 0.0;
        const double *Cp = upose_cov + idx * 36;
        double GC[3][9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) s += G[r][k] * Cp[k * 6 + c];
                GC[r][c] = s;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) s += G[r][6 + k] * meas[k * 3 + c];
                GC[r][6 + c] = s;
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) s += GC[r][k] * G[c][k];
                cov[r][c] = s;
            }
    }
}

// evalPointUncertainty + the trace gate of one record (cpp:1146-1150 / cpp:380-386): the f32 cov_vec, the trace (f64) and the verdict
struct UctPoint { double tr; float c6[6]; int keep; };
__device__ __forceinline__ UctPoint uct_point(const double *ext, const double *upose, const double *upose_cov, int n_lidar, const double *meas, int with_ua,
                                              double trace_thr, float x, float y, float z, float inten)
{
    double cov[3][3];
    eval_point_cov(ext, upose, upose_cov, n_lidar, meas, with_ua, x, y, z, inten, cov);
    UctPoint u;
    u.tr = cov[0][0] + cov[1][1] + cov[2][2];
    u.keep = (with_ua && trace_thr > 0.0 && u.tr > trace_thr) ? 0 : 1;
    u.c6[0] = float(cov[0][0]); u.c6[1] = float(cov[0][1]); u.c6[2] = float(cov[0][2]);
    u.c6[3] = float(cov[1][1]); u.c6[4] = float(cov[1][2]); u.c6[5] = float(cov[2][2]);
    return u;
}

// pointAssociateToMap(point_ori, point_cov, pose_global) (cpp:1152): f64 math, f32 store
__device__ __forceinline__ void uct_to_map(const double *gpose, float x, float y, float z, float *out)
{
    const d3 g = qrot(q4{gpose[3], gpose[4], gpose[5], gpose[6]}, d3{double(x), double(y), double(z)});
    out[0] = float(g.x + gpose[0]); out[1] = float(g.y + gpose[1]); out[2] = float(g.z + gpose[2]);
}

}  // namespace mlh
