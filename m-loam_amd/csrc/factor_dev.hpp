// What the window's factor tables share on the device (odom.hip: LidarPureOdom factors, calib.hip: LidarOnlineCalib factors, track.hip: scan-to-scan
// factors), on dev_math.hpp's d3: the f64 row / matrix helpers, the Huber correction of a squared residual, the point-to-line front of the two edge
// factors, and the scan that packs a match pass's valid correspondences into table slots. Every translation unit is compiled with -ffp-contract=off, so
// an expression keeps its bits wherever it is inlined -- as long as its tree is kept: these bodies are the callers' former text, term for term.
// Deliberately NOT here: the row that multiplies d(lp) in the two edge factors (the window factor forms eta [ba - bb]x from the two point differences,
// the calibration factor eta [la - lb]x: different roundings), the tracker's three-row vector edge factor, and pg_host.hpp's pg_huber (another form,
// shared with the pose graph's host restatement).
#pragma once
#include "ctx.hpp"
#include "dev_math.hpp"
#include <cfloat>

namespace mlh {

// M: 9 doubles, row-major
__device__ __forceinline__ d3 rowmul(const d3 &a, const double *M)       // a^T M
{
    return {a.x * M[0] + a.y * M[3] + a.z * M[6], a.x * M[1] + a.y * M[4] + a.z * M[7], a.x * M[2] + a.y * M[5] + a.z * M[8]};
}
__device__ __forceinline__ d3 matmul(const double *M, const d3 &v)       // M v
{
    return {M[0] * v.x + M[1] * v.y + M[2] * v.z, M[3] * v.x + M[4] * v.y + M[5] * v.z, M[6] * v.x + M[7] * v.y + M[8] * v.z};
}
__device__ __forceinline__ d3 tmatmul(const double *M, const d3 &v)      // M^T v
{
    return {M[0] * v.x + M[3] * v.y + M[6] * v.z, M[1] * v.x + M[4] * v.y + M[7] * v.z, M[2] * v.x + M[5] * v.y + M[8] * v.z};
}
__device__ __forceinline__ d3 row_skew(const d3 &a, const d3 &v)         // a^T [v]x
{
    return {a.y * v.z - a.z * v.y, a.z * v.x - a.x * v.z, a.x * v.y - a.y * v.x};
}

// ceres::HuberLoss(delta) at the squared residual sq (delta <= 0: no loss): rho0 = rho(sq), rho1 = rho'(sq); a row is corrected by sqrt(rho1), its cost is rho0 / 2
__device__ __forceinline__ void huber_correct(double sq, double delta, double &rho0, double &rho1)
{
    rho0 = sq; rho1 = 1.0;
    if (delta > 0.0) {
        const double bb = delta * delta;
        if (sq > bb) { const double rr = sqrt(sq); rho0 = 2.0 * delta * rr - bb; rho1 = fmax(DBL_MIN, delta / rr); }
    }
}

// The front LidarPureOdomEdgeFactor (lidar_pure_odom_factor.hpp:209-282) and LidarOnlineCalibEdgeFactor (lidar_online_calib_factor.hpp:135-165) have in
// common, for the moved point lp and the line's two points la, lb: nu = (lp - la) x (lp - lb), de = la - lb, the residual |nu| / |de| and
// eta = nu.normalized() / |de| (Eigen's normalized(): zero stays zero, so nu = 0 gives a zero row). Each factor goes on from ba, bb, de in its own way.
struct LineFront {
    d3 ba, bb, de, eta;
    double res;
};
__device__ __forceinline__ LineFront point_to_line(const d3 &lp, const d3 &la, const d3 &lb)
{
    LineFront F;
    F.ba = d3{lp.x - la.x, lp.y - la.y, lp.z - la.z}; F.bb = d3{lp.x - lb.x, lp.y - lb.y, lp.z - lb.z};
    const d3 nu = cross3(F.ba, F.bb);
    F.de = d3{la.x - lb.x, la.y - lb.y, la.z - lb.z};
    const double n2 = nu.x * nu.x + nu.y * nu.y + nu.z * nu.z, de_n = sqrt(F.de.x * F.de.x + F.de.y * F.de.y + F.de.z * F.de.z);
    F.res = sqrt(n2) / de_n;
    d3 nh = nu;
    if (n2 > 0.0) { const double nn = sqrt(n2); nh = d3{nu.x / nn, nu.y / nn, nu.z / nn}; }
    const double k = 1.0 / de_n;
    F.eta = d3{k * nh.x, k * nh.y, k * nh.z};
    return F;
}

// The valid correspondences of a match pass -> factor rows (point[3], coeff[6], sqrt_info = 1.0: the reference constructs these factors with s = 1.0,
// estimator.cpp:728, 735, 751, 774) in the slots behind base_slot, packed IN FEATURE ORDER; the rest of the cap_slots reserved slots is padding (perm = -1).
// The region is reserved from the STAGED feature count (no host round trip for the number of valid ones), so cap_slots >= m. One workgroup of 1024: per
// chunk of 1024 features a ballot per wavefront, the 16 wavefront counts through LDS, a running count across chunks -- deterministic. sink(slot) stores the
// table's side words of a filled slot. Returns the number of rows written (to every thread).
template <class Sink>
__device__ __forceinline__ int append_valid_matches(const float4 *feat, const Corr *corr, int m, int base_slot, int cap_slots, double *tab, int *perm, Sink sink)
{
    __shared__ int wsum[16];
    __shared__ int s_running;
    if (threadIdx.x == 0) s_running = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < m; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const bool v = i < m && corr[i].valid != 0 && feat[i].w >= 0.f;
        const unsigned long long b = __ballot(v);
        const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int x = wsum[w]; if (w < wave) before += x; total += x; }
        const int running = s_running;
        if (v) {
            const int slot = base_slot + running + before + in_wave;        // running + before + in_wave < m <= cap_slots
            const float4 f = feat[i];
            const Corr c = corr[i];
            double *t = tab + size_t(slot) * 10;
            t[0] = double(f.x); t[1] = double(f.y); t[2] = double(f.z);
#pragma unroll
            for (int k = 0; k < 6; ++k) t[3 + k] = double(c.c[k]);
            t[9] = 1.0;
            sink(slot);
            perm[slot] = slot;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_running = running + total;
        __syncthreads();
    }
    for (int q = s_running + threadIdx.x; q < cap_slots; q += 1024) perm[base_slot + q] = -1;
    return s_running;
}

// host side: a table's row buffer, side-word buffer (side_bytes per slot) and perm brought to n slots, the first `have` slots kept
inline hipError_t grow_factor_slots(DevBuf &tab, DevBuf &side, size_t side_bytes, DevBuf &perm, size_t n, size_t have, hipStream_t st)
{
    hipError_t e;
    if ((e = tab.grow(sizeof(double) * 10 * n, sizeof(double) * 10 * have, st)) != hipSuccess) return e;
    if ((e = side.grow(side_bytes * n, side_bytes * have, st)) != hipSuccess) return e;
    return perm.grow(sizeof(int) * n, sizeof(int) * have, st);
}

}  // namespace mlh
