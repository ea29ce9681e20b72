// Correspondence + linearisation kernels for gfx950 (the roofline kernels of the scan-to-map path).
//
// knn_features_kernel<G, MB> -- per feature: pointAssociateToMap (utility.h:103-117) -> exact K-NN (K = 5, or 10 for buildCalibMap's
//   non-reference LiDARs) in the local-map cell grid (the pcl::KdTreeFLANN::nearestKSearch role, feature_extract.hpp:666/813).
//   G lanes per feature -- 16 on a frame-sized launch (latency regime), 8 on a chip-filling one (throughput regime); the group
//   search itself lives in knn_dev.hpp: the 9 x-runs of the 27-cell neighbourhood are concatenated and the lanes stride over
//   the flat candidate list (balanced, coalesced 16 B/lane); queries with fewer than K candidates leave after the 18 cell_start
//   words; each lane keeps a sorted top-K of 64-bit (distance bits, map index) keys, the group merges with a K-round
//   all-reduce-min tournament; the K winners' coordinates + squared distances go to HBM (16 K B/feature).
//   HBM/L2-bound: ~(16 + 72 + 16*C + 16*K + 16*K) bytes per feature, C = candidates in the 27 cells.
// fit_linearize_kernel<KMAX> -- one lane per feature: line fit (3x3 scatter + f32 eigen-solver, hpp:669-783) or plane fit
//   (Kx3 column-pivoted QR, hpp:816-878) with the reference's gates -> residual and 1x6 Jacobian of LidarMapEdgeFactor /
//   LidarMapPlaneNormFactor (lidar_map_factor.hpp:44-71, 143-174) -> Huber correction (Ceres corrector, rho''<=0 branch)
//   -> transposed-butterfly + LDS reduction (reduce_dev.hpp) of the 21+6+2 packed normal-equation sums -> one partial record per
//   workgroup (no atomics, deterministic) -> fused_gn_finish: the last workgroup to arrive completes the Gauss-Newton iteration
//   (sum of the records, degeneracy test, 6x6 solve, Plus) and, on the last iteration, publishes the pose to pinned host memory.
// linearize_kernel           -- the same evaluation on the correspondences stored by the fit kernel (what ceres::Solve
//   does per LM iteration).
// blockIdx -> tile mapping is XCD-aware: consecutive tiles go to the same XCD (blockIdx % 8), so each XCD's L2 holds one
// contiguous eighth of the (spatially coherent) feature list's map neighbourhood.
#include "ctx.hpp"
#include "solve_host.hpp"
#include "match_plan_host.hpp"
#include "dev_math.hpp"
#include "solver_dev.hpp"
#include "p2p_dev.hpp"
#include "kparams.hpp"
#include <hip/hip_ext.h>
#include <cfloat>
#include <cstdlib>

namespace mlh {

// Debug build only (-DMLH_STAGE_CLOCK): per-workgroup stage timestamps (100 MHz wall clock) of the fit kernel, read back
// by mlh_debug_stage_clock. Never compiled into the product library.
#ifdef MLH_STAGE_CLOCK
__device__ unsigned long long g_stage_clk[4096 * 8];
#define MLH_STAGE(tile, i)                                                                   \
    do {                                                                                     \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                        \
        if (threadIdx.x == 0 && (tile) < 4096) g_stage_clk[(tile) * 8 + (i)] = wall_clock64(); \
    } while (0)
__device__ unsigned long long g_stage_clk_knn[4096 * 8];
#define MLH_KSTAGE(i)                                                                        \
    do {                                                                                     \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                        \
        if (threadIdx.x == 0 && blockIdx.x < 4096) g_stage_clk_knn[blockIdx.x * 8 + (i)] = wall_clock64(); \
    } while (0)
#else
#define MLH_STAGE(tile, i) do { } while (0)
#define MLH_KSTAGE(i) do { } while (0)
#endif
}  // namespace mlh
#include "knn_dev.hpp"
#include "reduce_dev.hpp"
namespace mlh {
__device__ __forceinline__ double sqrt_info_of(double trace)
{
    double s = sqrt(1 / trace);
    return s >= 3.0 ? 1.0 : s / 3.0;
}

// LidarMapPlaneNormFactor::Evaluate (lidar_map_factor.hpp:44-71)
__device__ __forceinline__ void eval_plane(const d3 &p, const float (&c)[6], double w, const q4 &q, const d3 &t, const double *R, Lin &o)
{
    d3 n{double(c[0]), double(c[1]), double(c[2])};
    double d = double(c[3]);
    d3 lp = qrot(q, p);
    lp.x += t.x; lp.y += t.y; lp.z += t.z;
    double a = (n.x * lp.x + n.y * lp.y + n.z * lp.z) + d;
    o.r = w * a;
    // -n^T R [p]x
    double wr0 = (-n.x) * R[0] + (-n.y) * R[3] + (-n.z) * R[6];
    double wr1 = (-n.x) * R[1] + (-n.y) * R[4] + (-n.z) * R[7];
    double wr2 = (-n.x) * R[2] + (-n.y) * R[5] + (-n.z) * R[8];
    // [p]x = [0 -pz py; pz 0 -px; -py px 0]
    double j0 = wr0 * 0.0 + wr1 * p.z + wr2 * (-p.y);
    double j1 = wr0 * (-p.z) + wr1 * 0.0 + wr2 * p.x;
    double j2 = wr0 * p.y + wr1 * (-p.x) + wr2 * 0.0;
    o.J[0] = w * n.x; o.J[1] = w * n.y; o.J[2] = w * n.z;
    o.J[3] = w * j0; o.J[4] = w * j1; o.J[5] = w * j2;
}

// LidarMapEdgeFactor::Evaluate (lidar_map_factor.hpp:143-174)
__device__ __forceinline__ void eval_edge(const d3 &p, const float (&c)[6], double w, const q4 &q, const d3 &t, const double *R, Lin &o)
{
    d3 lpa{double(c[0]), double(c[1]), double(c[2])};
    d3 lpb{double(c[3]), double(c[4]), double(c[5])};
    d3 lp = qrot(q, p);
    lp.x += t.x; lp.y += t.y; lp.z += t.z;
    d3 a{lp.x - lpa.x, lp.y - lpa.y, lp.z - lpa.z};
    d3 b{lp.x - lpb.x, lp.y - lpb.y, lp.z - lpb.z};
    d3 nu = cross3(a, b);
    d3 de{lpa.x - lpb.x, lpa.y - lpb.y, lpa.z - lpb.z};
    double nu_n = sqrt(nu.x * nu.x + nu.y * nu.y + nu.z * nu.z);
    double de_n = sqrt(de.x * de.x + de.y * de.y + de.z * de.z);
    o.r = w * nu_n / de_n;
    double k = 1.0 / de_n;
    double n2 = nu.x * nu.x + nu.y * nu.y + nu.z * nu.z;
    double ex = nu.x, ey = nu.y, ez = nu.z;
    if (n2 > 0.0) { double nn = sqrt(n2); ex /= nn; ey /= nn; ez /= nn; }
    ex = k * ex; ey = k * ey; ez = k * ez;
    // eta * [de]x
    double eD0 = ex * 0.0 + ey * de.z + ez * (-de.y);
    double eD1 = ex * (-de.z) + ey * 0.0 + ez * de.x;
    double eD2 = ex * de.y + ey * (-de.x) + ez * 0.0;
    double eDR0 = eD0 * R[0] + eD1 * R[3] + eD2 * R[6];
    double eDR1 = eD0 * R[1] + eD1 * R[4] + eD2 * R[7];
    double eDR2 = eD0 * R[2] + eD1 * R[5] + eD2 * R[8];
    double j0 = eDR0 * 0.0 + eDR1 * p.z + eDR2 * (-p.y);
    double j1 = eDR0 * (-p.z) + eDR1 * 0.0 + eDR2 * p.x;
    double j2 = eDR0 * p.y + eDR1 * (-p.x) + eDR2 * 0.0;
    o.J[0] = w * (-eD0); o.J[1] = w * (-eD1); o.J[2] = w * (-eD2);
    o.J[3] = w * j0; o.J[4] = w * j1; o.J[5] = w * j2;
}

// residual and 1 x 6 Jacobian of one factor at the pose (q, t); a slot without a valid correspondence contributes a zero row
__device__ __forceinline__ Lin eval_factor(bool valid, int kind, const d3 &p, const float (&coef)[6], double w, const q4 &q, const d3 &t)
{
    Lin L;
    L.r = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) L.J[i] = 0.0;
    if (valid) {
        double R[9];
        qtorot(q, R);
        if (kind == MLH_SURF) eval_plane(p, coef, w, q, t, R, L);
        else eval_edge(p, coef, w, q, t, R, L);
    }
    return L;
}

// feature_extract.hpp:696-715
__device__ __forceinline__ bool in_laser_fov(const q4 &q, const d3 &t, float sx, float sy, float sz)
{
    d3 zt = qrot(q, d3{0.0, 0.0, 10.0});
    float zx = float(zt.x + t.x), zy = float(zt.y + t.y), zz = float(zt.z + t.z);
    double a0 = t.x - double(sx), a1 = t.y - double(sy), a2 = t.z - double(sz);
    float squared_side1 = float(a0 * a0 + a1 * a1 + a2 * a2);
    float b0 = zx - sx, b1 = zy - sy, b2 = zz - sz;
    float squared_side2 = b0 * b0 + b1 * b1 + b2 * b2;
    float check1 = 100.0f + squared_side1 - squared_side2 - 10.0f * sqrtf(3.0f) * sqrtf(squared_side1);
    float check2 = 100.0f + squared_side1 - squared_side2 + 10.0f * sqrtf(3.0f) * sqrtf(squared_side1);
    return check1 < 0 && check2 > 0;
}

__device__ __forceinline__ int block_of_slot(const KindP &K, int n_blocks, int f)
{
    int b = 0;
    for (int i = 1; i < n_blocks; ++i) if (f >= K.blk_start[i]) b = i;
    return b;
}

__device__ __forceinline__ const double *block_pose(const KParams &P, int b)
{
    return b == 0 ? (P.pose_sel ? P.state->cand : P.state->x) : P.state->xb[b];
}

__device__ __forceinline__ void load_pose(const KParams &P, int b, q4 &q, d3 &t)
{
    if (P.use_init && b == 0) {            // uniform: straight from the kernel-argument segment
        t = d3{P.init_pose[0], P.init_pose[1], P.init_pose[2]};
        q = q4{P.init_pose[3], P.init_pose[4], P.init_pose[5], P.init_pose[6]};
    } else {                               // where the host found this launch's poses (KParams::pose_b0 / pose_bn): one trip behind the arguments
        const double *pose = b == 0 ? P.pose_b0 : P.pose_bn + 7 * b;
        t = d3{pose[0], pose[1], pose[2]};
        q = q4{pose[3], pose[4], pose[5], pose[6]};
    }
}

// ---- kernel arguments: one batch of scalar loads at kernel entry
// Left alone, the compiler fetches an argument where it is first used: inside the branch that needs it, behind whatever that branch already waited for. The fit
// kernel then pays seven scalar-memory round trips in series before its first vector load (profiles/r07_launch_floor.txt prices a trip at ~0.16 us on the
// chain). Each kernel of the Gauss-Newton path therefore names what its path reads as the inputs of ONE empty asm statement at entry: all of them have to be in
// registers there, so their loads are issued together and wait once, and a later use of the same field is the same value, whatever branch it sits in. (One
// statement, not one per value: the scheduler places a load between two statements if it likes, behind the first one's wait. Neighbouring words go in as one
// vector operand -- a statement takes 30.)
typedef int arg_i4 __attribute__((ext_vector_type(4)));
typedef float arg_f4 __attribute__((ext_vector_type(4)));
typedef float arg_f2 __attribute__((ext_vector_type(2)));
typedef double arg_d2 __attribute__((ext_vector_type(2)));
typedef double arg_d4 __attribute__((ext_vector_type(4)));
typedef unsigned long long arg_u4 __attribute__((ext_vector_type(4)));      // four neighbouring pointers
#define MLH_KIND_COUNTS(K_) arg_i4{(K_).m, (K_).tiles_a, (K_).tiles_b, (K_).nbr_stride}
#define MLH_WORDS(P_) arg_i4{int((P_).flags), (P_).own_mode, (P_).n_blocks, (P_).use_init}
#define MLH_GRID_ORIGIN(K_) arg_f4{(K_).grid.ox, (K_).grid.oy, (K_).grid.oz, (K_).grid.inv_h}
#define MLH_GRID_DIMS(K_) arg_i4{(K_).grid.nx, (K_).grid.ny, (K_).grid.nz, (K_).grid.n}

// the workgroup's kind, selected field by field from the two copies the entry batch left in registers (an index into the argument segment instead would be a
// second round trip behind the tile counts)
__device__ __forceinline__ KindL pick_kind(bool second, const KindL &a, const KindL &b)
{
    KindL k;
    k.feat = second ? b.feat : a.feat;
    k.covd = second ? b.covd : a.covd;
    k.nbr = second ? b.nbr : a.nbr;
    k.corr = second ? b.corr : a.corr;
    k.r_out = second ? b.r_out : a.r_out;
    k.J_out = second ? b.J_out : a.J_out;
    k.m = second ? b.m : a.m;
    k.tiles_a = second ? b.tiles_a : a.tiles_a;
    k.tiles_b = second ? b.tiles_b : a.tiles_b;
    k.nbr_stride = second ? b.nbr_stride : a.nbr_stride;
    k.lanes = second ? b.lanes : a.lanes;
    k.pad_ = 0;
    k.grid.sorted = second ? b.grid.sorted : a.grid.sorted;
    k.grid.raw = second ? b.grid.raw : a.grid.raw;
    k.grid.cell_start = second ? b.grid.cell_start : a.grid.cell_start;
    k.grid.ox = second ? b.grid.ox : a.grid.ox;
    k.grid.oy = second ? b.grid.oy : a.grid.oy;
    k.grid.oz = second ? b.grid.oz : a.grid.oz;
    k.grid.inv_h = second ? b.grid.inv_h : a.grid.inv_h;
    k.grid.nx = second ? b.grid.nx : a.grid.nx;
    k.grid.ny = second ? b.grid.ny : a.grid.ny;
    k.grid.nz = second ? b.grid.nz : a.grid.nz;
    k.grid.n = second ? b.grid.n : a.grid.n;
    return k;
}

// pointAssociateToMap (utility.h:103-117): f64 q*p + t, stored to f32
__device__ __forceinline__ void associate_to_map(const q4 &q, const d3 &t, const float4 &fp, float &sx, float &sy, float &sz)
{
    d3 w = qrot(q, d3{double(fp.x), double(fp.y), double(fp.z)});
    sx = float(w.x + t.x); sy = float(w.y + t.y); sz = float(w.z + t.z);
}

// (own_mode: KParams::own_mode, as the caller holds it)
__device__ __forceinline__ bool owns(const KParams &P, int own_mode, int f, float sx, float sy, float sz)
{
    if (own_mode == 0) return true;            // one rank (uniform): one word of the arguments
    // sharded: the ownership fields in one batch -- both planes evaluated whether set or not (an unset one is all zeros), so that no field waits inside a branch
    const int own_mod = P.own_mod, own_rem = P.own_rem;
    const float l0 = P.lo[0], l1 = P.lo[1], l2 = P.lo[2], l3 = P.lo[3], h0 = P.hi[0], h1 = P.hi[1], h2 = P.hi[2], h3 = P.hi[3];
    bool own = !(own_mode & 4) || (f % (own_mod > 1 ? own_mod : 1)) == own_rem;
    const bool in_lo = (((l0 * sx + l1 * sy) + l2 * sz) + l3) >= 0.f, in_hi = (((h0 * sx + h1 * sy) + h2 * sz) + h3) < 0.f;
    own = own && (!(own_mode & 1) || in_lo);
    own = own && (!(own_mode & 2) || in_hi);
    return own;
}
__device__ __forceinline__ bool owns(const KParams &P, int f, float sx, float sy, float sz) { return owns(P, P.own_mode, f, sx, sy, sz); }

// ---- correspondence kernel: 8 lanes per feature, 32 features per workgroup, both feature kinds in one launch

// the K winners' coordinates + squared distances -> the feature's neighbour records. A macro, expanded in the function that owns `keys`: as a function taking the
// array by reference, the lane's pick (a select chain over keys[t]) is folded into ONE load at a selected offset before the array is scalarised, and the
// keys then live in scratch / LDS instead of registers (seen in the ISA: 48 bytes of scratch, +10 KB of LDS per workgroup).
// lane t (< K <= G) fetches winner t: one load per lane, all in flight together
#define MLH_STORE_WINNERS(K_, G_, Kd_, f_, gl_, keys_, HAND_, lds_)                                                        \
    do {                                                                                                        \
        unsigned long long kk_ = keys_[0];                                                                      \
        _Pragma("unroll") for (int t_ = 1; t_ < (K_); ++t_) kk_ = ((gl_) == t_ % (G_)) ? keys_[t_] : kk_;      \
        if ((K_) <= (G_)) {                                                                                     \
            if ((gl_) < (K_)) {                                                                                 \
                float4 o_ = make_float4(0.f, 0.f, 0.f, __uint_as_float(0x7f800000u));                           \
                if (kk_ != KEY_INF) {                                                                           \
                    const float4 np_ = (Kd_).grid.raw[(unsigned)kk_];                                           \
                    o_ = make_float4(np_.x, np_.y, np_.z, __uint_as_float((unsigned)(kk_ >> 32)));              \
                }                                                                                               \
                (Kd_).nbr[size_t(f_) * (Kd_).nbr_stride + (gl_)] = o_;                                          \
                if constexpr (HAND_) (lds_)[(gl_)] = o_;                                                        \
            }                                                                                                   \
        } else {                                                                                                \
            _Pragma("unroll") for (int t_ = 0; t_ < (K_); ++t_) {                                               \
                if ((t_ % (G_)) == (gl_)) {                                                                     \
                    const unsigned long long k2_ = keys_[t_];                                                   \
                    float4 o_ = make_float4(0.f, 0.f, 0.f, __uint_as_float(0x7f800000u));                       \
                    if (k2_ != KEY_INF) {                                                                       \
                        const float4 np_ = (Kd_).grid.raw[(unsigned)k2_];                                       \
                        o_ = make_float4(np_.x, np_.y, np_.z, __uint_as_float((unsigned)(k2_ >> 32)));          \
                    }                                                                                           \
                    (Kd_).nbr[size_t(f_) * (Kd_).nbr_stride + t_] = o_;                                         \
                }                                                                                               \
            }                                                                                                   \
        }                                                                                                       \
    } while (0)

// HAND (the fused launches, knn_features_wide_kernel<.., FIT>): the lanes that store the K = 5 winners also leave them in LDS at lds_nbr[0 .. 4], for the lane
// that fits this feature behind the search
template <int K, int G, bool HAND = false>
__device__ __forceinline__ void knn_feature(const KParams &P, const KindL &Kd, int f, float sx, float sy, float sz, int gl, int *lds_run, float4 *lds_nbr = nullptr)
{
    static_assert(!HAND || K <= G, "the hand-over is the one-record-per-lane store's");
    unsigned long long keys[K];
    if constexpr (G == 32) knn_group_bounded<K, 32, true>(Kd.grid, sx, sy, sz, gl, lds_run, 0x7f800000u, keys);
    else if constexpr (G == 16) knn_group16_pruned<K>(Kd.grid, sx, sy, sz, gl, lds_run, keys);
    else knn_group8_pruned<K>(Kd.grid, sx, sy, sz, gl, lds_run, keys);
    MLH_KSTAGE(4);
    MLH_STORE_WINNERS(K, G, Kd, f, gl, keys, HAND, lds_nbr);
    MLH_KSTAGE(5);
}

// The same feature one Gauss-Newton iteration later: `old` is this lane's share (lane t: records t, t + G, ... below K) of the neighbour records the previous
// iteration left -- K points of the SAME map. Their largest squared distance from the query's new position bounds the K-th neighbour's from above, so the search
// is a single walk over the cells within that bound (knn_group_bounded). A feature that had fewer than K neighbours (w = +inf) searches as before.
template <int K, int G, int NREC, bool HAND = false>
__device__ __forceinline__ void knn_feature_warm(const KParams &P, const KindL &Kd, int f, float sx, float sy, float sz, int gl, int *lds_run, const float4 (&old)[NREC],
                                                 float4 *lds_nbr = nullptr)
{
    unsigned bits = 0u;
#pragma unroll
    for (int r = 0; r < NREC; ++r) {
        if (gl + r * G < K) {
            const float dx = old[r].x - sx, dy = old[r].y - sy, dz = old[r].z - sz;
            const float d = knn_sqdist(dx, dy, dz);
            const unsigned bb = (old[r].w < __uint_as_float(0x7f800000u) && d < __uint_as_float(0x7f800000u)) ? __float_as_uint(d) : 0x7f800000u;
            bits = bb > bits ? bb : bits;
        }
    }
    bits = group_max_u32<G>(bits);
    if (bits >= 0x7f800000u) { knn_feature<K, G, HAND>(P, Kd, f, sx, sy, sz, gl, lds_run, lds_nbr); return; }     // uniform over the group
    unsigned long long keys[K];
    knn_group_bounded<K, G>(Kd.grid, sx, sy, sz, gl, lds_run, bits, keys);
    MLH_KSTAGE(4);
    MLH_STORE_WINNERS(K, G, Kd, f, gl, keys, HAND, lds_nbr);
    MLH_KSTAGE(5);
}

// MB = more than one pose block in the launch (config 4); without it the block bookkeeping (a per-lane block index and the
// per-block K lookup it drags along) compiles away
// W: threads per workgroup (TPB, or 512 / 1024 in the wide prologue forms)
// HAND: the K = 5 winners also go to s_nbr[5 * query of the workgroup ..] (knn_feature)
template <int G, bool MB, bool K10, bool PRE, bool WARM, int W = TPB, bool HAND = false>
__device__ __forceinline__ void knn_features_body(const KParams &P, const KindL &K, int kind, int own_mode, int tile, int *s_run, const double *s_pose, int m_feat,
                                                  float4 *s_nbr = nullptr)
{
    constexpr int FPB = W / G;            // queries per workgroup
    constexpr int RUNW = 2 * KNN_RUN_WORDS;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int f = tile * FPB + grp;
    MLH_KSTAGE(0);
    if (f >= m_feat) return;
    const float4 fp = K.feat[f];
    if (fp.w < 0.f) return;               // padding slot
    const int b = MB ? block_of_slot(P.k[kind], P.n_blocks, f) : 0;
    constexpr int NREC = WARM ? ((K10 ? 10 : 5) + G - 1) / G : 1;
    float4 old[NREC];
    if constexpr (WARM) {                  // requested together with the feature, before the pose is known
        const int kq = K10 ? (MB ? P.kb[b] : P.kb[0]) : 5;
#pragma unroll
        for (int r = 0; r < NREC; ++r) {
            old[r] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0x7f800000u));
            if (gl + r * G < kq) old[r] = K.nbr[size_t(f) * K.nbr_stride + gl + r * G];
        }
    }
    q4 q;
    d3 t;
    if constexpr (PRE) {
        t = d3{s_pose[0], s_pose[1], s_pose[2]};
        q = q4{s_pose[3], s_pose[4], s_pose[5], s_pose[6]};
    } else {
        load_pose(P, b, q, t);
    }
    float sx, sy, sz;
    associate_to_map(q, t, fp, sx, sy, sz);
    MLH_KSTAGE(1);
    if (!owns(P, own_mode, f, sx, sy, sz)) return;     // uniform over the lane group
    // K10: some pose block of the launch asks for 10 neighbours (buildCalibMap's non-reference LiDARs); without it the K = 10 search is not
    // even compiled in, so the ordinary frame's kernel keeps the K = 5 register footprint
    if constexpr (WARM) {
        if (K10 && (MB ? P.kb[b] : P.kb[0]) == 10) knn_feature_warm<10, G, NREC>(P, K, f, sx, sy, sz, gl, s_run + grp * RUNW, old);
        else knn_feature_warm<5, G, NREC, HAND>(P, K, f, sx, sy, sz, gl, s_run + grp * RUNW, old, s_nbr + (HAND ? grp * 5 : 0));
    } else {
        if (K10 && (MB ? P.kb[b] : P.kb[0]) == 10) knn_feature<10, G>(P, K, f, sx, sy, sz, gl, s_run + grp * RUNW);
        else knn_feature<5, G, HAND>(P, K, f, sx, sy, sz, gl, s_run + grp * RUNW, s_nbr + (HAND ? grp * 5 : 0));
    }
}

// The prologue of a correspondence launch that completes a Gauss-Newton iteration first (all W threads of the workgroup, converged; the first GN_SUM_THREADS of
// them sum, the first wavefront solves, the others of a wide workgroup only stand at the barriers):
//   s_pose <- the pose that iteration linearised at; the records its fit launch left are summed (sum_partials<TPB, 12>'s arithmetic -- same slices, same four chains,
//   same association: the same bits --, inlined: the record loads leave at once instead of behind an argument block's trip through scratch, and nobody waits for the
//   per-kind counts, which only statistics read); gn_finish_wave solves and applies Plus on the first wavefront; s_pose holds the updated pose when this returns.
// MODE 1: an iteration of the running solve. MODE 2: the LAST iteration of the PREVIOUS solve (thresholds from the launch arguments).
// b: the pose block this workgroup's features belong to (0 without blocks): the records summed are that block's tiles -- its surf tiles, then its corner tiles, as the
// classic finish walks them -- and the thresholds that block's.
constexpr int GN_SUM_THREADS = 256;      // the sum's geometry: 8 slices x 32 columns, whatever the workgroup's width (the association is part of the result's bits)
// ROWS (the wide kernels and gn_final_kernel): the records may be a fused launch's wavefront rows, four per tile (P.pre_rows == 4): a tile's value is then formed where
// it is loaded, ((w0 + w1) + w2) + w3 -- what the fit kernel's workgroup stores as the tile's record -- and enters the same slices and chains.
template <int MODE, bool MB = false, int W = TPB, bool ROWS = false>
__device__ __forceinline__ void gn_prologue(const KParams &P, int b, double *s_pose, double *f_ne, double *f_cnt2, double *f_scratch)
{
    // (the pose is requested here and stored behind the records' sum: its trip and the records' run together, not one behind the other)
    double pose_v = 0.0;
    if (threadIdx.x < 7) {
        if (P.pre_from_init) pose_v = P.init_pose[threadIdx.x];
        else if (MB && P.pre_from_state) pose_v = (b == 0 ? P.state->x : P.state->xb[b])[threadIdx.x];
        else pose_v = P.x_prev[7 * b + threadIdx.x];
    }
    static_assert(W >= GN_SUM_THREADS && W % 64 == 0, "the sum takes the first 256 threads of the workgroup");
    {
        constexpr int NS = GN_SUM_THREADS / 32, U = 12;
        const int c = threadIdx.x & 31, sl = threadIdx.x >> 5;
        const bool sums = W == GN_SUM_THREADS || threadIdx.x < GN_SUM_THREADS;      // (uniform over a wavefront; the others of a wide workgroup walk no records)
        int lo0 = 0, n0 = P.pre_tiles, lo1 = 0, n1 = 0;
        if constexpr (MB) {
            lo0 = P.k[0].m > 0 ? P.k[0].blk_start[b] / TPB : 0;
            n0 = P.k[0].m > 0 ? (P.k[0].blk_start[b + 1] + TPB - 1) / TPB - lo0 : 0;
            lo1 = P.k[0].tiles_b + (P.k[1].m > 0 ? P.k[1].blk_start[b] / TPB : 0);
            n1 = P.k[1].m > 0 ? (P.k[0].tiles_b + (P.k[1].blk_start[b + 1] + TPB - 1) / TPB) - lo1 : 0;
            n0 = max(n0, 0); n1 = max(n1, 0);
        }
        const int ntot = sums ? n0 + n1 : 0;
        const double *__restrict__ rec = P.partials;
        double ch[4] = {0.0, 0.0, 0.0, 0.0};
        bool rows4 = false;
        if constexpr (ROWS) rows4 = P.pre_rows == 4;
        if (ROWS && rows4) {                 // (uniform)
            static_assert(!ROWS || !MB, "wavefront rows: single-block launches only");
            if constexpr (W > GN_SUM_THREADS) {
                // Four times the loads of a record sum: a wide workgroup shares them out by CHAIN. Part p (threads 256 p .. 256 p + 255; 2 or 4 parts) walks slice sl, column c
                // like the summing thread it mirrors, but only the tiles of chains p, p + parts, ...: chain k takes u = k, k + 4, k + 8 of every batch, in that order, so
                // each chain is the same sequence of additions as in one thread. The chains meet in LDS and the summing thread adds them (ch0 + ch1) + (ch2 + ch3).
                constexpr int PARTS = W / GN_SUM_THREADS >= 4 ? 4 : 2, CPP = 4 / PARTS;
                __shared__ double s_ch[4 * GN_SUM_THREADS];
                const int part = threadIdx.x / GN_SUM_THREADS, t8 = threadIdx.x % GN_SUM_THREADS, pc = t8 & 31, psl = t8 >> 5, nall = n0 + n1;
                if (part < PARTS) {
                    double chp[CPP];
#pragma unroll
                    for (int kk = 0; kk < CPP; ++kk) chp[kk] = 0.0;
                    for (int j = psl; j < nall; j += U * NS) {
                        double wv[CPP][U / 4][4];
#pragma unroll
                        for (int kk = 0; kk < CPP; ++kk)
#pragma unroll
                            for (int v = 0; v < U / 4; ++v) {
                                const int jj = j + NS * (part + PARTS * kk + 4 * v);
#pragma unroll
                                for (int w = 0; w < 4; ++w) wv[kk][v][w] = jj < nall ? rec[(size_t(jj) * 4 + w) * NE_STRIDE + pc] : 0.0;
                            }
#pragma unroll
                        for (int kk = 0; kk < CPP; ++kk)
#pragma unroll
                            for (int v = 0; v < U / 4; ++v) chp[kk] += ((wv[kk][v][0] + wv[kk][v][1]) + wv[kk][v][2]) + wv[kk][v][3];
                    }
#pragma unroll
                    for (int kk = 0; kk < CPP; ++kk) s_ch[(part + PARTS * kk) * GN_SUM_THREADS + t8] = chp[kk];
                }
                __syncthreads();
                if (sums) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) ch[k] = s_ch[k * GN_SUM_THREADS + t8];
                }
            } else {      // (gn_final_kernel: one workgroup of 256 threads)
                for (int j = sl; j < ntot; j += U * NS) {
                    double tv[U];
#pragma unroll
                    for (int h = 0; h < U; h += U / 2) {          // half a batch of tiles at a time: 24 row loads in flight
                        double wv[U / 2][4];
#pragma unroll
                        for (int u = 0; u < U / 2; ++u) {
                            const int jj = j + NS * (h + u);
#pragma unroll
                            for (int w = 0; w < 4; ++w) wv[u][w] = jj < ntot ? rec[(size_t(jj) * 4 + w) * NE_STRIDE + c] : 0.0;
                        }
#pragma unroll
                        for (int u = 0; u < U / 2; ++u) tv[h + u] = ((wv[u][0] + wv[u][1]) + wv[u][2]) + wv[u][3];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) ch[u & 3] += tv[u];
                }
            }
        } else {
            for (int j = sl; j < ntot; j += U * NS) {
                double tv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int jj = j + NS * u;
                    const int tile = jj < n0 ? lo0 + jj : lo1 + (jj - n0);
                    tv[u] = jj < ntot ? rec[size_t(tile) * NE_STRIDE + c] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) ch[u & 3] += tv[u];
            }
        }
        if (sums) f_scratch[sl * 32 + c] = (ch[0] + ch[1]) + (ch[2] + ch[3]);
        if (threadIdx.x < 7) s_pose[threadIdx.x] = pose_v;
        __syncthreads();
        if (threadIdx.x < 32) {
            double tsum = 0.0;
#pragma unroll
            for (int q = 0; q < NS; ++q) tsum += f_scratch[q * 32 + c];
            f_ne[c] = tsum;
        }
        __syncthreads();
    }
    if (threadIdx.x < 64) {
        double xo[7];
        gn_finish_wave(f_ne, f_cnt2, s_pose, nullptr, MODE == 2 ? P.pre_thre : P.thre_b[b], MODE == 2 ? P.pre_freeze : P.freeze_b[b], nullptr, f_scratch, xo);
    }
    __syncthreads();
}

// the previous solve's pose, final now: to its host record (seq stored last, system-scope release) and to the state. One thread of ONE workgroup.
__device__ __forceinline__ void publish_final_pose(const KParams &P, const double *s_pose)
{
    for (int i = 0; i < 7; ++i) P.state->x[i] = s_pose[i];
    if (P.pre_publish) {
        for (int i = 0; i < 7; ++i) P.pre_publish->x[i] = s_pose[i];
        publish_seq(P.pre_publish, P.pre_publish_seq);
    }
}

// (the fit kernel's pieces the fused correspondence launches run behind their search; defined with that kernel, below)
template <int K, int KV>
__device__ __forceinline__ bool fit_feature(float min_match_sq_dis, float min_plane_dis, int kind, const float4 (&v)[KV], float (&coef)[6]);
__device__ __forceinline__ double feature_weight_pref(uint32_t flags, double cov_measurement_trace, const KindL &K, const float4 &cd);

// G = lanes per query for both kinds, or 0: per kind (KindP::lanes -- a workgroup serves one kind, so the choice is uniform over it)
// PRE 1: the launch completes the previous Gauss-Newton iteration first -- EVERY workgroup sums the records the previous fit launch's tiles left (same order,
//   same code: the same bits everywhere), runs the 6 x 6 solve + Plus on one wavefront and goes on with the pose in LDS; the kernel boundary behind the fit
//   launch is the only synchronisation (no ticket, no fence, no last workgroup whose serial tail the other 255 compute units wait for). The workgroup of
//   tile 0 leaves the pose in HBM for the fit kernel of this iteration.
// PRE 2: iteration 0 of a chained solve whose predecessor left its LAST iteration as records: the same prologue completes that solve (tile 0's workgroup publishes its
//   pose to the host and stores it as the state's), then every workgroup computes this frame's chained start pose from it (chain_start_pose, one lane) -- the
//   predecessor's serial finish and the chain launch between the two frames are gone.
// WARM: the search is bounded by the previous iteration's neighbours (knn_feature_warm). All three only in the single-block, K = 5 launches of mlh_gn_solve*.
// DEVM: the feature counts come from P.m_dev (G = 0 only: lanes per kind); the grid was sized for a bound, the workgroups beyond the real tiles leave
// W: threads per workgroup. W / lanes queries per workgroup and as many run tables in LDS; the prologue's sum and solve take the first GN_SUM_THREADS threads
//   and the first wavefront whatever W is. One prologue per workgroup: with W = 1024 a frame-sized launch runs one per compute unit instead of four.
template <int G, bool MB, bool K10, int PRE = 0, bool WARM = false, bool DEVM = false>
__global__ __launch_bounds__(TPB) void knn_features_kernel(KParams P)
{
    constexpr int W = TPB;
    constexpr bool FIT = false;
#include "knn_features_kernel.inc"
}

// The wide forms of the single-block, K = 5 launches of mlh_gn_solve* (PRE 1 warm and cold, PRE 2, PRE 0 warm): the same body, prologue and argument batch in
// workgroups of 512 or 1024 threads. Kernels of their own: the 256-thread instantiations above keep their names and their code.
// FIT: the launch also FITS -- it is a whole Gauss-Newton iteration whose fit launch would have been fit_linearize_kernel<5, false, false> leaving records (the host's
//   knn_fit_in_search(): single block, K = 5, one rank, no dense rows, a prologue in front, every kind at 64 queries or more per workgroup). Behind the search the
//   workgroup's queries ARE the features 64 w .. 64 w + 63 of one or two wavefront rows of a 256-feature tile (a wide tile starts at a multiple of 64): the lanes that
//   stored a query's five winners left them in LDS as well, and the workgroup's first one or two wavefronts take one feature per lane -- feature f on lane f & 63 --
//   through that kernel's body: fit_feature<5>, the Corr store, eval_factor at the pose in s_pose, the Huber scaling and the butterfly, up to the wavefront's row
//   (reduce_rows_wave), which goes to P.rows_out[(tile256 * 4 + wave) * 32]. The next launch's prologue adds a tile's four rows as the fit kernel's workgroup does
//   (gn_prologue<.., ROWS>): the same bits, without the launch boundary, the trip that fetches the neighbour records back and the search's idle tail. The rows of a
//   kind's last 256-feature tile that no workgroup produces are written as zeros by the workgroup of the kind's last wide tile. No workgroup waits for another.
template <int W, int G, int PRE, bool WARM, bool FIT = false>
__global__ __launch_bounds__(W) void knn_features_wide_kernel(KParams P)
{
    static_assert(W == 512 || W == 1024, "wide workgroups: 512 or 1024 threads");
    static_assert(!FIT || (PRE != 0 && (G == 0 || W / G >= 64)), "the fused form: a prologue in front, whole wavefront rows per workgroup");
    constexpr bool MB = false, K10 = false, DEVM = false;
#include "knn_features_kernel.inc"
}

// a pending last iteration completed by itself (no chained successor took it): one workgroup, the same prologue, the same publication
__global__ __launch_bounds__(TPB) void gn_final_kernel(KParams P)
{
    __shared__ double s_pose[8], f_ne[NE_STRIDE], f_cnt2[2], f_scratch[(GN_SUM_THREADS / 32) * 32];
    gn_prologue<2, false, TPB, true>(P, 0, s_pose, f_ne, f_cnt2, f_scratch);      // (records or a fused launch's rows: P.pre_rows)
    if (threadIdx.x == 0) publish_final_pose(P, s_pose);
}

// the reference's plane fit + gate (feature_extract.hpp:816-840)
template <int K>
__device__ __forceinline__ bool fit_plane(const float (&ax)[K], const float (&ay)[K], const float (&az)[K], float min_plane_dis, float (&coef)[6])
{
    float nx, ny, nz;
    plane_fit_qr_f<K>(ax, ay, az, nx, ny, nz);
    float nn = sqrtf(nx * nx + ny * ny + nz * nz);
    float negative_OA_dot_norm = 1 / nn;
    float z = nx * nx + ny * ny + nz * nz;
    if (z > 0.f) { float s = sqrtf(z); nx /= s; ny /= s; nz /= s; }
    bool plane_valid = true;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fabsf(nx * ax[j] + ny * ay[j] + nz * az[j] + negative_OA_dot_norm) > min_plane_dis) plane_valid = false;
    coef[0] = nx; coef[1] = ny; coef[2] = nz; coef[3] = negative_OA_dot_norm;
    return plane_valid;
}

// the reference's line fit + test (feature_extract.hpp:669-693, 767-777)
template <int K>
__device__ __forceinline__ bool fit_line(const float (&ax)[K], const float (&ay)[K], const float (&az)[K], float (&coef)[6])
{
    float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) { cx += ax[j]; cy += ay[j]; cz += az[j]; }
    const float kf = float(K);
    cx /= kf; cy /= kf; cz /= kf;
    float c00 = 0.f, c10 = 0.f, c11 = 0.f, c20 = 0.f, c21 = 0.f, c22 = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        float t0 = ax[j] - cx, t1 = ay[j] - cy, t2 = az[j] - cz;
        c00 += t0 * t0; c10 += t1 * t0; c11 += t1 * t1; c20 += t2 * t0; c21 += t2 * t1; c22 += t2 * t2;
    }
    float l0, l1, l2, vx, vy, vz;
    eig3_largest_f(c00, c10, c11, c20, c21, c22, l0, l1, l2, vx, vy, vz);
    coef[0] = 0.1f * vx + cx; coef[1] = 0.1f * vy + cy; coef[2] = 0.1f * vz + cz;
    coef[3] = -0.1f * vx + cx; coef[4] = -0.1f * vy + cy; coef[5] = -0.1f * vz + cz;
    return l2 > 3 * l1;
}

__device__ __forceinline__ double feature_weight(const KParams &P, const KindP &K, int f)
{
    double trace = P.cov_measurement_trace;
    if ((P.flags & MLH_FLAG_WITH_UA)) {
        trace = 0.0;
        if (K.covd) { float4 cd = K.covd[f]; trace = (double(cd.x) + double(cd.y)) + double(cd.z); }
    }
    return sqrt_info_of(trace);
}

// the same from a covariance diagonal the caller already holds in registers (requested together with the feature: no dependent trip)
__device__ __forceinline__ double feature_weight_pref(uint32_t flags, double cov_measurement_trace, const KindL &K, const float4 &cd)
{
    double trace = cov_measurement_trace;
    if ((flags & MLH_FLAG_WITH_UA)) {
        trace = 0.0;
        if (K.covd) trace = (double(cd.x) + double(cd.y)) + double(cd.z);
    }
    return sqrt_info_of(trace);
}
__device__ __forceinline__ double feature_weight_pref(const KParams &P, const KindL &K, const float4 &cd) { return feature_weight_pref(P.flags, P.cov_measurement_trace, K, cd); }

// correspondence, feature and (with uncertainty weighting) covariance diagonal of slot f < K.m, requested together: ONE round trip, whatever `valid` turns out to be
__device__ __forceinline__ void load_tile_inputs(const KParams &P, const KindP &K, int f, Corr &c, float4 &fp, float4 &cdv)
{
    c = K.corr[f];
    fp = K.feat[f];
    if ((P.flags & MLH_FLAG_WITH_UA) && K.covd) cdv = K.covd[f];
}

// the publication of the launch-per-iteration LM forms: bit 1 from the split submission's look-ahead bookkeeping, the largest iteration count of the frame's loops
template <typename X>
__device__ __forceinline__ void lmc_publish(const KParams &P, const X &x, int done, int overflow, double used_max, int iteration)
{
    publish_pose(P.publish, P.publish_seq, x, done | (overflow ? DONE_OVERFLOWED : 0), fmax(used_max, double(iteration)));
}

// the records of pose block b: its surf tiles, then its corner tiles (one block: every record, whatever the tile size)
__device__ __forceinline__ void block_sum_args(const KParams &P, int b, int total_tiles, SumArgs &sa)
{
    sa.p = P.partials;
    sa.lo[0] = P.k[0].m > 0 ? P.k[0].blk_start[b] / TPB : 0;
    sa.hi[0] = P.k[0].m > 0 ? (P.k[0].blk_start[b + 1] + TPB - 1) / TPB : 0;
    sa.lo[1] = P.k[0].tiles_b + (P.k[1].m > 0 ? P.k[1].blk_start[b] / TPB : 0);
    sa.hi[1] = P.k[0].tiles_b + (P.k[1].m > 0 ? (P.k[1].blk_start[b + 1] + TPB - 1) / TPB : 0);
    if (P.n_blocks == 1) { sa.lo[0] = 0; sa.hi[0] = total_tiles; sa.lo[1] = 0; sa.hi[1] = 0; }
}

// Fused tail: the last workgroup to arrive (agent-scope release/acquire around an atomic ticket) sums the partial records
// in fixed order, runs the degeneracy test + the 6x6 solve + Plus for every pose block and re-arms the ticket: a GN iteration
// costs two launches.
// COV (LM only; MLH_FLAG_POSE_COV): a publication whose loop has terminated carries H at the pose and its inverse (reduce_dev.hpp: publish_pose_cov)
template <bool LM, int NT = TPB, bool COV = false>
__device__ __forceinline__ void fused_gn_finish(const KParams &P, int total_tiles)
{
    __shared__ double f_ne[NE_STRIDE], f_cnt2[2], f_scratch[(NT / 32) * 32];   // f_scratch doubles as the Jacobi work area (DEG_WORK <= 256)
    if (!last_workgroup_arrives(P.ticket, total_tiles)) return;
    MLH_STAGE(4095, 0);
    if (P.use_init && threadIdx.x < 7) P.state->x[threadIdx.x] = P.init_pose[threadIdx.x];   // the state's pose is born here
    __syncthreads();
    if constexpr (LM) {
        // scan2map on one GPU: the Levenberg-Marquardt begin / step of solver_dev.hpp runs right here, so an LM iteration is ONE launch
        SumArgs sa;
        sa.p = P.partials;
        sa.lo[0] = 0; sa.hi[0] = total_tiles; sa.lo[1] = 0; sa.hi[1] = 0;
        sum_partials<NT, (NT > 256 ? 21 : 12)>(sa, f_ne, f_cnt2, f_scratch);
        bool exchanged = true;
        if (P.p2p.n_ranks > 1) {     // sharded over several ranks: everybody's sums before anybody's LM decision (same bits, same decision on every rank)
            exchanged = p2p_exchange<NT>(P.p2p, f_ne, NE_STRIDE);
            if (threadIdx.x == 0) { f_cnt2[0] = f_ne[NE_CNT + 1]; f_cnt2[1] = f_ne[NE_CNT + 2]; }
            __syncthreads();
        }
        MLH_STAGE(4095, 1);
        if (threadIdx.x < 64) {      // one wavefront runs the LM begin / step (solver_dev.hpp: rows of the 6 x 6 objects on lanes)
            double xo[7];
            int done = 0;
            [[maybe_unused]] bool fresh = false;   // (COV) the record at the pose this call leaves is f_ne -- behind a begin or an accepted step; the state's otherwise
            if (!exchanged) {        // a peer timed out: no decision on partial sums -- the loop ends here, the pose stays, the host reports the error word
#pragma unroll
                for (int i = 0; i < 7; ++i) xo[i] = P.state->x[i];
                done = 1;
                if (threadIdx.x == 0) P.state->done = 1;
            }
            else if (P.finish == TAIL_LM_BEGIN) {
                // split submission: this outer iteration was enqueued without anybody having seen the previous LM loop end. If it has not, the frame's result is
                // not the reference's (<= max_num_iterations per outer iteration): flagged, published with the pose, and the host re-solves or reports
                if (threadIdx.x == 0 && P.lm_expect_done) {
                    P.state->lm_overflow = (P.lm_expect_done > LM_VERDICT_READ && (P.state->lm_overflow || !P.state->done)) ? 1 : 0;
                    P.state->lm_used_max = P.lm_expect_done > LM_VERDICT_READ ? fmax(P.state->lm_used_max, double(P.state->iteration)) : 0.0;      // the loop that just ended
                }
                lm_begin_body_wave(f_ne, f_cnt2, f_scratch, P.state, P.thre_b[0], P.lm_max_it, P.stat, P.lm_min_blocks, xo, done);
                if constexpr (COV) fresh = true;
            }
            else if constexpr (COV) lm_step_body_wave(f_ne, P.state, P.lm_max_it, xo, done, &fresh);
            else lm_step_body_wave(f_ne, P.state, P.lm_max_it, xo, done);
            if constexpr (COV) { if (P.publish && done && exchanged) publish_pose_cov(P.publish, fresh ? f_ne : P.state->ne); }
            if (threadIdx.x == 0) {
                *P.ticket = 0u;
                // last launch of a chunk of LM steps: the pose and the `done` flag go to the host from here
                if (P.publish) lmc_publish(P, xo, done, P.state->lm_overflow, P.state->lm_used_max, P.state->iteration);
            }
        }
        MLH_STAGE(4095, 2);
        return;
    }
    if (P.finish == TAIL_REDUCE) {
        // multi-GPU: only the local reduction happens here; the all-reduce and the (redundant, identical) solve follow
        if (P.n_blocks == 1) {
            SumArgs sa;
            sa.p = P.partials;
            sa.lo[0] = 0; sa.hi[0] = total_tiles; sa.lo[1] = 0; sa.hi[1] = 0;
            sum_partials<NT, (NT > 256 ? 21 : 12)>(sa, f_ne, f_cnt2, f_scratch);
            if (threadIdx.x < NE_STRIDE) P.state->ne[threadIdx.x] = f_ne[threadIdx.x];
        } else {
            for (int b = 0; b < P.n_blocks; ++b) {         // one record per pose block, all-reduced in one message
                SumArgs sa;
                block_sum_args(P, b, total_tiles, sa);
                sum_partials<NT, (NT > 256 ? 21 : 12)>(sa, f_ne, f_cnt2, f_scratch);
                if (threadIdx.x < NE_STRIDE) P.state->neb[b][threadIdx.x] = f_ne[threadIdx.x];
                __syncthreads();
            }
        }
        if (threadIdx.x == 0) *P.ticket = 0u;
        return;
    }
    for (int b = 0; b < P.n_blocks; ++b) {
        SumArgs sa;
        block_sum_args(P, b, total_tiles, sa);
        sum_partials<NT, (NT > 256 ? 21 : 12)>(sa, f_ne, f_cnt2, f_scratch);
        bool exchanged = true;
        if (P.p2p.n_ranks > 1) {                     // this rank's sums -> everybody's sums (rank order: the same bits on every rank)
            exchanged = p2p_exchange<NT>(P.p2p, f_ne, NE_STRIDE);
            if (threadIdx.x == 0) { f_cnt2[0] = f_ne[NE_CNT + 1]; f_cnt2[1] = f_ne[NE_CNT + 2]; }
            __syncthreads();
        }
        MLH_STAGE(4095, 1);
        if (threadIdx.x < 64 && !exchanged) {        // a peer timed out: nothing is solved on partial sums; the pose stays and is published as it is (the host reports the error word)
            if (P.publish && threadIdx.x == 0) for (int i = 0; i < 7; ++i) (b == 0 ? P.publish->x : P.publish->xb[b])[i] = (b == 0 ? P.state->x : P.state->xb[b])[i];
        } else if (threadIdx.x < 64) {
            double xo[7];
            const double *x_in = P.pose0 ? P.pose0 + 7 * b : nullptr;      // last iteration of a deferred-finish solve: the pose comes from its iteration slot
            gn_finish_wave(f_ne, f_cnt2, b == 0 ? P.state->x : P.state->xb[b], nullptr /* nothing downstream reads a mirror of ne / V_update in GN mode */, P.thre_b[b], P.freeze_b[b],
                           P.stat ? P.stat + b : nullptr, f_scratch, xo, x_in);
            if (x_in && threadIdx.x < 7) {           // ... and goes to the state whatever the solve decided (an unchanged pose included)
                const int l = threadIdx.x;
                (b == 0 ? P.state->x : P.state->xb[b])[l] = l == 0 ? xo[0] : (l == 1 ? xo[1] : (l == 2 ? xo[2] : (l == 3 ? xo[3] : (l == 4 ? xo[4] : (l == 5 ? xo[5] : xo[6])))));
            }
            // the solve's last launch hands the pose(s) to the host: straight from the finish's registers (reading the state back would be one more round trip)
            if (P.publish && threadIdx.x == 0) for (int i = 0; i < 7; ++i) (b == 0 ? P.publish->x : P.publish->xb[b])[i] = xo[i];
        }
        __syncthreads();
        MLH_STAGE(4095, 2);
    }
    if (threadIdx.x == 0) {
        *P.ticket = 0u;
        if (P.publish) publish_seq(P.publish, P.publish_seq);     // (the pose blocks went into x / xb[b] above)
    }
}

// v: the feature's neighbour records {x, y, z, sq-dist}, already in registers (the kernel requests them together with the feature itself)
template <int K, int KV>
__device__ __forceinline__ bool fit_feature(float min_match_sq_dis, float min_plane_dis, int kind, const float4 (&v)[KV], float (&coef)[6])
{
    static_assert(K <= KV, "neighbour buffer too small");
    if (!(v[K - 1].w < min_match_sq_dis)) return false;     // sq_dis[k-1] < MIN_MATCH_SQ_DIS (hpp:667/814)
    float ax[K], ay[K], az[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { ax[j] = v[j].x; ay[j] = v[j].y; az[j] = v[j].z; }
    return kind == MLH_SURF ? fit_plane<K>(ax, ay, az, min_plane_dis, coef) : fit_line<K>(ax, ay, az, coef);
}
template <int K, int KV>
__device__ __forceinline__ bool fit_feature(const KParams &P, int kind, const float4 (&v)[KV], float (&coef)[6])
{
    return fit_feature<K, KV>(P.min_match_sq_dis, P.min_plane_dis, kind, v, coef);
}

// ---- fit + gates + residual/Jacobian + normal-equation reduction: one lane per feature, both kinds in one launch
// KMAX = the largest N_NEIGH of the launch: with 5 (every mapper launch) the 10-neighbour fits are not compiled in, which halves
// the kernel's register footprint (occupancy matters once a launch has more workgroups than the chip holds at once)
// FIN = false: the launch only leaves its tiles' partial records (a deferred-finish Gauss-Newton iteration, or a caller that reduces elsewhere): no ticket, no
// finishing workgroup, and none of that code in the kernel
template <int KMAX, bool LM, bool FIN = true, bool DEVM = false>
__global__ __launch_bounds__(TPB) void fit_linearize_kernel(KParams P)
{
    __shared__ double s_red[4 * 32];
    // every argument the taken path reads, both kinds': one batch, one wait (the pose, behind its pointer, leaves as a vector load together with the feature's)
    const KindL k0 = P.k[0], k1 = P.k[1];
    {
        const arg_i4 c0 = MLH_KIND_COUNTS(k0), c1 = MLH_KIND_COUNTS(k1), w = MLH_WORDS(P);
        const arg_f2 gate{P.min_match_sq_dis, P.min_plane_dis};
        const arg_d2 loss{P.huber_delta, P.cov_measurement_trace};
        const arg_d4 ip0{P.init_pose[0], P.init_pose[1], P.init_pose[2], P.init_pose[3]};
        const arg_d2 ip1{P.init_pose[4], P.init_pose[5]};
        const double ip2 = P.init_pose[6];
        double *const partials = P.partials;
        const double *const pose_b0 = P.pose_b0, *const pose_bn = P.pose_bn;
        const int finish = P.finish;
        asm volatile("; kernel arguments in registers" ::"s"(k0.feat), "s"(k0.covd), "s"(k0.nbr), "s"(k0.corr), "s"(k0.r_out), "s"(k0.J_out), "s"(c0), "s"(k1.feat), "s"(k1.covd),
                     "s"(k1.nbr), "s"(k1.corr), "s"(k1.r_out), "s"(k1.J_out), "s"(c1), "s"(w), "s"(gate), "s"(loss), "s"(ip0), "s"(ip1), "s"(ip2), "s"(partials), "s"(pose_b0),
                     "s"(pose_bn), "s"(finish));
    }
    // what the kernel's tail reads (gates, weight, loss, the record's address), as values the compiler cannot fetch again: it would rather re-read an argument behind
    // the fit than keep it in a register, one more scalar round trip each time
    uint32_t flags = P.flags;
    int own_mode = P.own_mode;
    float min_match_sq_dis = P.min_match_sq_dis, min_plane_dis = P.min_plane_dis;
    double huber_delta = P.huber_delta, cov_measurement_trace = P.cov_measurement_trace;
    double *partials = P.partials;
    asm volatile("" : "+s"(flags), "+s"(own_mode), "+s"(min_match_sq_dis), "+s"(min_plane_dis), "+s"(huber_delta), "+s"(cov_measurement_trace), "+s"(partials));
    int m0 = k0.m, m1 = k1.m, tb0 = k0.tiles_b;
    int total = k0.tiles_b + k1.tiles_b;
    if constexpr (DEVM) {            // (the counts from the device, knn_features_kernel<.., DEVM>)
        m0 = P.m_dev[0]; m1 = P.m_dev[1];
        tb0 = (m0 + TPB - 1) / TPB;
        total = tb0 + (m1 + TPB - 1) / TPB;
        if ((int(blockIdx.x) >> 3) >= ((total + 7) >> 3)) return;
    }
    const int gtile = xcd_tile(total);
    if (gtile >= total) return;
    const int kind = gtile >= tb0 ? 1 : 0;
    const int tile = kind ? gtile - tb0 : gtile;
    const KindL K = pick_kind(kind != 0, k0, k1);
    const int m_feat = kind ? m1 : m0;
    MLH_STAGE(gtile, 0);
    const int f = tile * TPB + threadIdx.x;
    const int b = P.n_blocks > 1 ? block_of_slot(P.k[kind], P.n_blocks, tile * TPB) : 0;       // uniform over the workgroup (blocks start on tile boundaries)
    q4 q;
    d3 t;
    load_pose(P, b, q, t);
    bool valid = false;
    float coef[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 fp = make_float4(0.f, 0.f, 0.f, -1.f), cdv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f < m_feat) {
        // ONE memory round trip before the fit: the feature and all of its neighbour records are requested together (the records sit at
        // f * stride whatever the feature turns out to be; what is fetched for a padding slot or a feature another rank owns is discarded).
        // The map-frame position is only needed by the ownership planes of a sharded map and by the field-of-view gate: an ordinary
        // single-GPU launch skips the f64 transform here altogether (uniform branch).
        fp = K.feat[f];
        float4 nbv[KMAX];
        const float4 *nb = K.nbr + size_t(f) * K.nbr_stride;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) nbv[j] = nb[j];
        if ((flags & MLH_FLAG_WITH_UA) && K.covd) cdv = K.covd[f];       // the weight's covariance diagonal rides in the same trip
        MLH_STAGE(gtile, 5);
        const bool need_pos = (own_mode & 3) || (flags & MLH_FLAG_CHECK_FOV);
        float sx = 0.f, sy = 0.f, sz = 0.f;
        if (need_pos) associate_to_map(q, t, fp, sx, sy, sz);
        if (fp.w >= 0.f && owns(P, own_mode, f, sx, sy, sz)) {
            valid = (KMAX == 10 && P.kb[b] == 10) ? fit_feature<KMAX, KMAX>(min_match_sq_dis, min_plane_dis, kind, nbv, coef) : fit_feature<5, KMAX>(min_match_sq_dis, min_plane_dis, kind, nbv, coef);
            if (valid && (flags & MLH_FLAG_CHECK_FOV)) valid = in_laser_fov(q, t, sx, sy, sz);
        }
        MLH_STAGE(gtile, 6);
        Corr c;
#pragma unroll
        for (int i = 0; i < 6; ++i) c.c[i] = valid ? coef[i] : 0.f;
        c.valid = valid ? 1 : 0;
        c.pad = 0;
        K.corr[f] = c;
    }
    MLH_STAGE(gtile, 1);
    const Lin L = eval_factor(valid, kind, d3{double(fp.x), double(fp.y), double(fp.z)}, coef, valid ? feature_weight_pref(flags, cov_measurement_trace, K, cdv) : 0.0, q, t);
    if (K.r_out && f < m_feat) {
        K.r_out[f] = L.r;
#pragma unroll
        for (int i = 0; i < 6; ++i) K.J_out[size_t(f) * 6 + i] = L.J[i];
    }
    MLH_STAGE(gtile, 2);
    reduce_rows(valid, L, huber_delta, (flags & MLH_FLAG_NO_LOSS) != 0, kind, s_red, partials + size_t(gtile) * NE_STRIDE);
    MLH_STAGE(gtile, 3);
    if constexpr (FIN) { if (P.finish) fused_gn_finish<LM>(P, total); }
    MLH_STAGE(gtile, 4);
}

#ifdef MLH_STAGE_CLOCK
}  // namespace mlh
extern "C" int mlh_debug_stage_clock(unsigned long long *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mlh::g_stage_clk), sizeof(unsigned long long) * size_t(n_words));
}
extern "C" int mlh_debug_stage_clock_step(unsigned long long *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mlh::g_step_clk), sizeof(unsigned long long) * size_t(n_words));
}
extern "C" int mlh_debug_stage_clock_knn(unsigned long long *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mlh::g_stage_clk_knn), sizeof(unsigned long long) * size_t(n_words));
}
namespace mlh {
#endif

template <bool LM, bool COV = false>
__global__ __launch_bounds__(TPB) void linearize_kernel(KParams P)
{
    static_assert(LM || !COV, "the covariance rides in a Levenberg-Marquardt publication");
    __shared__ double s_red[4 * 32];
    const int total = P.k[0].tiles_b + P.k[1].tiles_b;
    const int gtile = xcd_tile(total);
    if (gtile >= total) return;
    if (P.pose_sel && P.state->done) {   // candidate evaluation after the device-side LM loop has terminated: keep the partials defined, do no work
        if (threadIdx.x < 32) P.partials[size_t(gtile) * NE_STRIDE + threadIdx.x] = 0.0;
        if constexpr (COV) { if (P.publish && gtile == 0 && threadIdx.x < 64) publish_pose_cov(P.publish, P.state->ne); }     // (the record an earlier launch left at the pose)
        if (LM && P.publish && gtile == 0 && threadIdx.x == 0)        // ... but the host may be waiting for this launch's publication
            lmc_publish(P, P.state->x, P.state->done, P.state->lm_overflow, P.state->lm_used_max, P.state->iteration);
        return;
    }
    const int kind = gtile >= P.k[0].tiles_b ? 1 : 0;
    const int tile = kind ? gtile - P.k[0].tiles_b : gtile;
    const KindP &K = P.k[kind];
    MLH_STAGE(gtile, 0);
    const int f = tile * TPB + threadIdx.x;
    const double *pose = block_pose(P, block_of_slot(K, P.n_blocks, tile * TPB));
    const q4 q{pose[3], pose[4], pose[5], pose[6]};
    const d3 t{pose[0], pose[1], pose[2]};
    Corr c;
    c.valid = 0;
    float4 fp = make_float4(0.f, 0.f, 0.f, 0.f), cdv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f < K.m) load_tile_inputs(P, K, f, c, fp, cdv);
    const bool valid = f < K.m && c.valid != 0;
    const int mult = valid ? c.valid : 1;
    const Lin L = eval_factor(valid, kind, d3{double(fp.x), double(fp.y), double(fp.z)}, c.c, valid ? feature_weight_pref(P, K, cdv) : 0.0, q, t);
    if (K.r_out && f < K.m) {
        K.r_out[f] = L.r;
#pragma unroll
        for (int i = 0; i < 6; ++i) K.J_out[size_t(f) * 6 + i] = L.J[i];
    }
    MLH_STAGE(gtile, 2);
    reduce_rows(valid, L, P.huber_delta, (P.flags & MLH_FLAG_NO_LOSS) != 0, kind, s_red, P.partials + size_t(gtile) * NE_STRIDE, mult);
    MLH_STAGE(gtile, 3);
    if constexpr (LM) { if (P.finish == TAIL_LM_BEGIN || P.finish == TAIL_LM_STEP) fused_gn_finish<true, TPB, COV>(P, total); }   // (the begin: on rows a selection kept -- scan2map with good-feature selection)
    MLH_STAGE(gtile, 4);
}

// ---- Levenberg-Marquardt, the step done by the CONSUMER of the records (the Gauss-Newton path's round-4 move, for the loop scan2MapOptimization really runs).
// linearize_kernel<true> evaluates at the candidate, leaves its tile's record, takes a ticket, and the last workgroup to arrive sums the records and runs the LM
// step while 87 others have left: fence + ticket + acquire, then sum + step, all behind the slowest tile. Here a launch ends at its records; the NEXT launch's every
// workgroup sums them (sum_partials<TPB, 12>'s slices, chains and association: the same bits in every workgroup), runs the LM begin / step on its first wavefront
// (lm_begin_wave_pp / lm_step_wave_pp: the accept / reject decision and the next candidate are a function of the records and the state, so all workgroups hold the
// same candidate), and evaluates its own tile there -- with the tile's correspondences, features and covariances requested before the sum, so that their trip
// runs under the step. The state lives in two LmState records: launch g reads [(g - 1) & 1], its tile-0 workgroup writes [g & 1] (and mirrors the accepted pose
// into SolverState::x, which only launches behind this one read); the records alternate between two buffers the same way. A launch that finds the loop terminated
// copies the state forward and leaves (the host enqueues a look-ahead of launches without reading the verdict in between, as before).
// FIRST: the launch behind a match launch whose fit kernel left records (TAIL_RECORDS) -- the records are at the state's pose (or init_pose), the LM loop begins here.
template <bool FIRST, bool COV = false>
__global__ __launch_bounds__(TPB) void lm_consume_kernel(KParams P)
{
    __shared__ double s_red[4 * 32];
    __shared__ double f_ne[NE_STRIDE], f_scratch[(TPB / 32) * 32];
    __shared__ double s_cand[8];
    __shared__ int s_done;
    const int total = P.k[0].tiles_b + P.k[1].tiles_b;
    const int gtile = xcd_tile(total);
    if (gtile >= total) return;
    const LmState *Si = P.lm_in;
    LmState *So = P.lm_out;
    const bool writer = gtile == 0;
    if constexpr (!FIRST) {
        if (Si->done) {                    // the loop ended in an earlier launch (uniform over the grid): the state goes forward as it is
            if (writer && threadIdx.x < 64) {
                const int lane = threadIdx.x;
                constexpr int NW = int(sizeof(LmState) / sizeof(double));
                static_assert(sizeof(LmState) % sizeof(double) == 0, "LmState is copied in doubles");
                const double *src = reinterpret_cast<const double *>(Si);
                double *dst = reinterpret_cast<double *>(So);
                for (int i = lane; i < NW; i += 64) dst[i] = src[i];
                if constexpr (COV) { if (P.publish) publish_pose_cov(P.publish, Si->ne); }
                if (P.publish && lane == 0) lmc_publish(P, Si->x, Si->done, Si->lm_overflow, Si->lm_used_max, Si->iteration);
            }
            return;
        }
    }
    // this tile's inputs: requested now, used after the step
    const int kind = gtile >= P.k[0].tiles_b ? 1 : 0;
    const int tile = kind ? gtile - P.k[0].tiles_b : gtile;
    const KindP &K = P.k[kind];
    const int f = tile * TPB + threadIdx.x;
    Corr c;
    c.valid = 0;
    float4 fp = make_float4(0.f, 0.f, 0.f, 0.f), cdv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f < K.m) load_tile_inputs(P, K, f, c, fp, cdv);
    lmc_sum_records(P.partials_in, total, f_ne, f_scratch);
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        LmRegs R;
        double cand[7];
        int overflow;
        double used_max;
        if constexpr (FIRST) {
            double x[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) x[i] = P.use_init ? P.init_pose[i] : P.state->x[i];
            // (split submission: this outer iteration was enqueued without anybody having seen the previous LM loop end -- fused_gn_finish's bookkeeping)
            if (P.lm_expect_done) {
                overflow = (P.lm_expect_done > LM_VERDICT_READ && (Si->lm_overflow || !Si->done)) ? 1 : 0;
                used_max = P.lm_expect_done > LM_VERDICT_READ ? fmax(Si->lm_used_max, double(Si->iteration)) : 0.0;
            } else { overflow = Si->lm_overflow; used_max = Si->lm_used_max; }
            lm_begin_wave_pp(f_ne, f_scratch, x, So, writer, P.thre_b[0], P.lm_max_it, P.lm_min_blocks, R, cand);
            if (writer && P.use_init && lane < 7) P.state->x[lane] = pick7(x, lane);       // the state's pose is born here
        } else {
            overflow = Si->lm_overflow; used_max = Si->lm_used_max;
            lm_step_wave_pp(f_ne, Si, So, writer, P.lm_max_it, R, cand);
            if (writer && lane < 7) P.state->x[lane] = pick7(R.x, lane);                   // read by the launches BEHIND this one only
        }
        if (lane < 7) s_cand[lane] = pick7(cand, lane);
        if (lane == 0) s_done = R.done;
        if constexpr (COV) {
            // the record at R.x: this launch's sums behind a begin or an accepted step (the state's count of those went up), the state's record otherwise
            bool fresh = FIRST;
            if constexpr (!FIRST) fresh = R.num_successful != Si->num_successful;
            if (writer && P.publish && R.done) publish_pose_cov(P.publish, fresh ? f_ne : Si->ne);
        }
        if (writer && lane == 0) {
            So->lm_overflow = overflow; So->lm_used_max = used_max;
            if (P.publish) lmc_publish(P, R.x, R.done, overflow, used_max, R.iteration);
        }
    }
    __syncthreads();
    if (s_done) return;                    // terminated by this launch: nothing to evaluate (the next launch finds `done` and reads no records)
    const q4 q{s_cand[3], s_cand[4], s_cand[5], s_cand[6]};
    const d3 t{s_cand[0], s_cand[1], s_cand[2]};
    const bool valid = f < K.m && c.valid != 0;
    const int mult = valid ? c.valid : 1;
    const Lin L = eval_factor(valid, kind, d3{double(fp.x), double(fp.y), double(fp.z)}, c.c, valid ? feature_weight_pref(P, K, cdv) : 0.0, q, t);
    reduce_rows(valid, L, P.huber_delta, (P.flags & MLH_FLAG_NO_LOSS) != 0, kind, s_red, P.partials + size_t(gtile) * NE_STRIDE, mult);
}

// ---- The whole Levenberg-Marquardt loop of one outer iteration in ONE launch. The consumer-side launches above still pay a launch boundary per LM iteration
// (~4.4 us of an ~8.9 us launch on the 88-tile mapper frame) and a look-ahead of launches behind the loop's end; the tiles of a frame that qualifies for the
// consumer-side schedule whose workgroups are all resident at once (the host asks the device: mlh_ctx::caps, capi.hip: set_loop_gates) can synchronise among themselves instead:
//   every workgroup: tile inputs -> registers (once); sum the fit launch's records; LM begin; then, until the loop terminates:
//     evaluate the tile at the candidate -> record (buffer (it + 1) & 1) -> grid barrier (reduce_dev.hpp: loop_barrier_arrive -- one atomic arrival, a poll of the counter)
//     -> sum all records -> LM step (the state stays in LDS: every workgroup runs the identical arithmetic on identical inputs, so they agree on accept / reject,
//     on the next candidate and on the iteration the loop ends at, without exchanging anything but the records).
// The loop ends on the device when Ceres' loop would: no look-ahead budget, no launches that find `done`, nothing for the host to poll between LM iterations,
// and the split submission cannot overflow. Same operations in the same order as the launches it replaces: the same bits.
// Barrier: P.ticket[1] counts arrivals (monotonic over the launch: iteration `it` waits for total * (it + 1)), P.ticket[2] counts workgroups that have left; the
// last one to leave zeroes both for the next launch. Residency is the HOST's business (capi.hip: loop_tiles_ok -- the occupancy query x the compute units the
// solver's stream may use, asked at mlh_create); should a barrier nevertheless not complete within P.loop_timeout_ticks of the 100 MHz wall clock (a workgroup that
// never became resident beside another context's kernels, a fault), the loop is given up: P.ticket[3] tells every workgroup still to come or still polling, DONE_GIVEN_UP
// in the published `done` word tells the host, which solves the frame again through the launch-per-iteration form (lm_consume_kernel: no residency requirement) --
// a slow frame, not a lost one. The later loop launches of such a frame (lm_overflow == LM_OVERFLOW_BARRIER_GIVEN_UP in the state) leave at once.
// The records cross the barrier as agent-scope monotonic stores / loads (write-through, read past the L2 of the reader's XCD): no L2 write-back and invalidate
// around the barrier. A waiting thread sleeps one s_sleep unit between polls (polling without it was slower, profiles/r05_knockout_experiments.txt).
// The first wavefront keeps the LM state's registers from step to step (lm_step_wave_keep) and stores them to the LDS state once, behind the loop: scan2map
// 0.184 -> 0.176 ms against a state that goes through LDS around every step, the same bits (profiles/r06_knockout_experiments.txt). Splitting the step over two
// wavefronts was not faster (profiles/r05_knockout_experiments.txt).
// FIT (round 6): the launch begins with the outer iteration's FIT -- fit_linearize_kernel's body for this tile: neighbour records -> line / plane fit + gates -> the
// correspondence record (stored: later launches and callers read it) -> residual + Jacobian at the start pose -> the tile's record, tagged with iteration 0 and
// summed by polling like every other record of the loop -- instead of reading what a fit launch in front of it left. One launch boundary fewer per outer iteration;
// the same operations on the same values: the same bits. Tagged records only (P.loop_tagged: the host's loop_fit_fusable()).
// COV (MLH_FLAG_POSE_COV, the frame's last loop launch): the publication carries H at the pose -- s_lm.ne -- and its inverse.
template <bool DEVM = false, bool FIT = false, bool COV = false>
__global__ __launch_bounds__(TPB, 2) void lm_loop_kernel(KParams P)      // (2: two workgroups per compute unit -- 256 registers in all; the residency gates count on them)
{
    __shared__ double s_red[4 * 32];
    __shared__ double f_ne[NE_STRIDE], f_scratch[(TPB / 32) * 32];
    __shared__ double s_cand[8];
    __shared__ int s_done, s_timeout;
    __shared__ LmState s_lm;
    int m0 = P.k[0].m, m1 = P.k[1].m, tb0 = P.k[0].tiles_b;
    int total = P.k[0].tiles_b + P.k[1].tiles_b;
    if constexpr (DEVM) {            // (the counts from the device: the tiles that exist are the barrier's participants)
        m0 = P.m_dev[0]; m1 = P.m_dev[1];
        tb0 = (m0 + TPB - 1) / TPB;
        total = tb0 + (m1 + TPB - 1) / TPB;
        if (total == 0) {
            // the thinning kept nothing of either kind: no tile exists, nobody would publish -- the first workgroup of the launch the host waits for does (bit 3:
            // "no features"; the host reports what mlh_scan2map reports for an empty feature set, include/mloam_hip.h)
            if (blockIdx.x == 0 && threadIdx.x == 0 && P.publish) {
                double x[7];
                for (int i = 0; i < 7; ++i) x[i] = P.use_init ? P.init_pose[i] : P.state->x[i];
                publish_pose(P.publish, P.publish_seq, x, DONE_TERMINATED | DONE_NO_FEATURES, 0.0);
            }
            return;
        }
        if ((int(blockIdx.x) >> 3) >= ((total + 7) >> 3)) return;
    }
    const int gtile = xcd_tile(total);
    if (gtile >= total) return;            // (the grid is rounded up to a multiple of 8: the padding workgroups take no part in the barrier)
    const bool writer = gtile == 0;
    const int kind = gtile >= tb0 ? 1 : 0;
    const int tile = kind ? gtile - tb0 : gtile;
    const KindP &K = P.k[kind];
    const int m_feat = kind ? m1 : m0;
    const int f = tile * TPB + threadIdx.x;
    Corr c;
    c.valid = 0;
    float4 fp = make_float4(0.f, 0.f, 0.f, 0.f), cdv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (FIT) {
        // fit_linearize_kernel<5, .., FIN = false>'s body (single block, N_NEIGH 5, no ownership planes, no field-of-view gate: what scan2MapOptimization launches)
#pragma unroll
        for (int i = 0; i < 6; ++i) c.c[i] = 0.f;
        c.pad = 0;
        if (f < m_feat) {
            fp = K.feat[f];
            float4 nbv[5];
            const float4 *nb = K.nbr + size_t(f) * K.nbr_stride;
#pragma unroll
            for (int j = 0; j < 5; ++j) nbv[j] = nb[j];
            if ((P.flags & MLH_FLAG_WITH_UA) && K.covd) cdv = K.covd[f];
            float coef[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            bool ok = false;
            if (fp.w >= 0.f) ok = fit_feature<5, 5>(P, kind, nbv, coef);
#pragma unroll
            for (int i = 0; i < 6; ++i) c.c[i] = ok ? coef[i] : 0.f;
            c.valid = ok ? 1 : 0;
            K.corr[f] = c;
        }
    } else if (f < m_feat) {
        load_tile_inputs(P, K, f, c, fp, cdv);
    }
    const bool valid = f < m_feat && c.valid != 0;
    const int mult = valid ? c.valid : 1;
    const double w = feature_weight_pref(P, K, cdv);
    const d3 p{double(fp.x), double(fp.y), double(fp.z)};
    const size_t set = size_t(NE_STRIDE) * size_t(total);
    // given up already -- by a workgroup of this launch that waited in vain, or by an earlier loop of this frame: nothing to do but leave
    if (threadIdx.x == 0)
        s_timeout = (loop_barrier_given_up(P.ticket) || (P.lm_expect_done >= LM_VERDICT_READ && P.state->lm_overflow == LM_OVERFLOW_BARRIER_GIVEN_UP)) ? 2 : 0;
    if constexpr (FIT) {
        __syncthreads();                               // s_timeout
        if (s_timeout == 0) {                          // (uniform)
            // the linearisation at the start pose, as the fit launch evaluates it (load_pose: the launch's pose argument or the state's)
            double xs[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) xs[i] = P.use_init ? P.init_pose[i] : P.state->x[i];
            const q4 q0{xs[3], xs[4], xs[5], xs[6]};
            const d3 t0{xs[0], xs[1], xs[2]};
            const Lin L0 = eval_factor(valid, kind, p, c.c, w, q0, t0);
            const unsigned tag0 = P.loop_tag_base;     // iteration byte 0: the fit's record (the loop's iterations carry 1, 2, ...)
            unsigned long long *trec0 = P.loop_tagged;  // set 0 (iteration `it` writes set (it + 1) & 1: 1, 0, 1, ...; set 0 is written again by iteration 1, which
                                                        // no workgroup reaches before every workgroup has stored its iteration-0 record -- behind its read of this one)
            reduce_rows<2>(valid, L0, P.huber_delta, (P.flags & MLH_FLAG_NO_LOSS) != 0, kind, s_red, reinterpret_cast<double *>(trec0 + size_t(gtile) * 64), 1, tag0);
            lmc_sum_records_tagged(trec0, total, tag0, f_ne, f_scratch, P.ticket, P.loop_timeout_ticks, &s_timeout);
        }
    } else {
        lmc_sum_records(P.partials_in, total, f_ne, f_scratch);
    }
    const bool skipped = s_timeout != 0;           // (uniform: written before the sum's barriers)
    if (threadIdx.x == 0 && skipped) s_done = 1;
    LmRegs Rk;                     // (first wavefront only: the LM state's registers, kept from step to step; stored to s_lm once, behind the loop)
    double candk[7], x_cost_k = 0.0;
    if (threadIdx.x < 64 && !skipped) {
        const int lane = threadIdx.x;
        LmRegs R;
        double cand[7], x[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) x[i] = P.use_init ? P.init_pose[i] : P.state->x[i];
        lm_begin_wave_pp(f_ne, f_scratch, x, &s_lm, true, P.thre_b[0], P.lm_max_it, P.lm_min_blocks, R, cand);
        if (lane < 7) s_cand[lane] = pick7(cand, lane);
        if (lane == 0) s_done = R.done;
        Rk = R; x_cost_k = f_ne[NE_COST];
#pragma unroll
        for (int i = 0; i < 7; ++i) candk[i] = cand[i];
    }
    __syncthreads();
    int it = 0;
    while (!s_done) {
        if (it == 2) MLH_STAGE(gtile, 0);                 // (debug build only: the third iteration's stages, scripts/stageclock_loop.py)
        const q4 q{s_cand[3], s_cand[4], s_cand[5], s_cand[6]};
        const d3 t{s_cand[0], s_cand[1], s_cand[2]};
        const Lin L = eval_factor(valid, kind, p, c.c, w, q, t);
        if (it == 2) MLH_STAGE(gtile, 1);
        const bool stall = P.debug_stall && it == 1 && gtile == (total > 1 ? 1 : 0);      // (tests: this workgroup's record / arrival never comes)
        if (P.loop_tagged) {
            // (round 6) the record leaves as tagged words and is summed by polling for the tag: no arrival atomic, no counter poll between the store and the loads
            const unsigned tag = P.loop_tag_base | unsigned(it + 1);
            unsigned long long *trec = P.loop_tagged + size_t(total) * 64 * size_t((it + 1) & 1);
            if (stall) {
                if (threadIdx.x == 0) { s_timeout = 1; __hip_atomic_store(P.ticket + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                __syncthreads();
            } else {
                reduce_rows<2>(valid, L, P.huber_delta, (P.flags & MLH_FLAG_NO_LOSS) != 0, kind, s_red, reinterpret_cast<double *>(trec + size_t(gtile) * 64), mult, tag);
                if (it == 2) MLH_STAGE(gtile, 2);
                if (it == 2) MLH_STAGE(gtile, 3);
                lmc_sum_records_tagged(trec, total, tag, f_ne, f_scratch, P.ticket, P.loop_timeout_ticks, &s_timeout);
            }
            if (s_timeout) break;
        } else {
            double *rec = P.partials + set * size_t((it + 1) & 1);
            reduce_rows<1>(valid, L, P.huber_delta, (P.flags & MLH_FLAG_NO_LOSS) != 0, kind, s_red, rec + size_t(gtile) * NE_STRIDE, mult);
            // (the record's 32 words are stored by the first 32 lanes of the wavefront thread 0 belongs to: its s_waitcnt covers them)
            if (it == 2) MLH_STAGE(gtile, 2);
            if (threadIdx.x == 0) {
                if (stall) __hip_atomic_store(P.ticket + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (stall || !loop_barrier_arrive(P.ticket, total, it + 1, P.loop_timeout_ticks)) s_timeout = 1;
            }
            __syncthreads();
            if (it == 2) MLH_STAGE(gtile, 3);
            if (s_timeout) break;
            lmc_sum_records<true>(rec, total, f_ne, f_scratch);
        }
        if (it == 2) MLH_STAGE(gtile, 4);
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            lm_step_wave_keep(f_ne, &s_lm, P.lm_max_it, Rk, candk, x_cost_k);
            if (lane < 7) s_cand[lane] = pick7(candk, lane);
            if (lane == 0) s_done = Rk.done;
        }
        __syncthreads();
        if (it == 2) MLH_STAGE(gtile, 5);
        ++it;
    }
    if (threadIdx.x < 64 && !skipped) {            // the state the publication below (and nothing else) reads
        lm_state_store_pp(Rk, candk, s_lm.ne, s_lm.V, &s_lm, threadIdx.x);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (writer && threadIdx.x < 64 && skipped) {
        // the loop never began here: the pose in the state is what the last loop that ran left; the failure travels on to the launch that publishes
        if (threadIdx.x == 0) {
            P.state->lm_overflow = LM_OVERFLOW_BARRIER_GIVEN_UP;
            if (P.publish) publish_pose(P.publish, P.publish_seq, P.state->x, DONE_GIVEN_UP, P.state->lm_used_max);
        }
    }
    else if (writer && threadIdx.x < 64) {
        const int lane = threadIdx.x;
        if (lane < 7) P.state->x[lane] = s_lm.x[lane];          // read by the launches BEHIND this one only (the other workgroups took their start pose long ago)
        if constexpr (COV) { if (P.publish && s_lm.done) publish_pose_cov(P.publish, s_lm.ne); }
        if (lane == 0) {
            const double used = P.lm_expect_done < LM_VERDICT_READ ? double(s_lm.iteration) : fmax(P.state->lm_used_max, double(s_lm.iteration));
            // (a barrier given up on in an EARLIER outer iteration of the frame must not be lost: lm_overflow -- unused otherwise by this schedule -- carries it to the
            // launch that publishes)
            const int failed = (s_timeout ? 1 : 0) | ((P.lm_expect_done >= LM_VERDICT_READ && P.state->lm_overflow == LM_OVERFLOW_BARRIER_GIVEN_UP) ? 1 : 0);
            P.state->lm_used_max = used;
            P.state->lm_overflow = failed ? LM_OVERFLOW_BARRIER_GIVEN_UP : 0;
            P.state->done = s_lm.done;
            P.state->iteration = s_lm.iteration;
            if (P.publish) publish_pose(P.publish, P.publish_seq, s_lm.x, (s_lm.done ? DONE_TERMINATED : 0) | (failed ? DONE_GIVEN_UP : 0), used);
        }
    }
    if (threadIdx.x == 0) loop_barrier_leave(P.ticket, total);      // the last workgroup to leave re-arms the barrier for the next launch
}

// stand-alone exact 5-NN for mlh_knn (queries already in the map frame)
__global__ __launch_bounds__(TPB) void knn_queries_kernel(GridDev grid, const float *__restrict__ q, int nq, int *__restrict__ idx,
                                                          float *__restrict__ d2)
{
    constexpr int G = 8, FPB = TPB / G;
    __shared__ int s_run[FPB * 20];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int qi = blockIdx.x * FPB + grp;
    if (qi >= nq) return;
    unsigned long long keys[5];
    knn_group<5, G, true>(grid, q[qi * 3 + 0], q[qi * 3 + 1], q[qi * 3 + 2], gl, s_run + grp * 20, keys);
    if (gl == 0) {
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const bool found = keys[t] != KEY_INF;
            idx[qi * 5 + t] = found ? int((unsigned)keys[t]) : -1;
            d2[qi * 5 + t] = __uint_as_float((unsigned)(keys[t] >> 32));
        }
    }
}

// ---------------------------------------------------------------- host launchers
// How a launch comes about -- match_launch, linearize_launch and lm_consume_launch in ONE order:
//   1. describe and plan: describe() reads MatchArgs and the context into the planners' records; pose_plan (where the launch's poses are), knn_plan (the correspondence
//      kernel, whether it carries its fit, which fit launch follows) and lm_plan (the linearise / consumer / loop kernel) answer or refuse -- pure functions of
//      match_plan_host.hpp and solve_plan_host.hpp. Every rule about which kernel a launch gets and which slot a pose lives in is written there, not in this file.
//   2. - 5. prepare(): validate the staged kinds (may refuse; nothing has allocated, released, launched or counted so far), complete a pending solve (ahead of the
//      buffers: an `ensure` may free what the pending records lie in), ensure the buffers, advance the chain state (mlh_ctx::GnChain, ::LmChain).
//   6. fill_params only reads; 7. the form's kernel out of KNN_KERNELS / LM_KERNELS, the two expansions of the lists that instantiate the kernels, is launched.
// Where an iteration's records lie is one descriptor (mlh_ctx::GnRecords: GnChain::last, GnPending::recs, LaunchPlan::front); prologue_reads points a launch at it.
//
// lanes per query, per kind. A small launch (a 16-ring frame) leaves most SIMDs idle and is bound by the latency of its trips: 16 lanes.
// A full frame keeps ~5 wavefronts per SIMD busy and is bound by VALU issue, where the per-query instruction count is what matters:
// 8 lanes (twice the queries per wavefront) for a kind whose map is sparse enough that a query's candidates fit one or two 8-lane trips,
// 16 lanes (pruned, near-cells-first) for a dense map, whose heavy queries would otherwise set the launch's duration. Measured up to 229 k
// queries per launch (un-thinned features) and on config 4's 52 k: the density rule beats "8 lanes for every kind" there too (44.5 vs 48.6 us,
// 0.325 vs 0.356 ms), so there is no upper query count at which it is switched off.
void knn_lanes_for(const mlh_ctx *ctx, int kind_mask, int lanes[2])
{
    long long queries = 0;
    for (int k = 0; k < 2; ++k) if (kind_mask & (1 << k)) queries += ctx->feat[k].m;
    for (int k = 0; k < 2; ++k) {
        const MapGrid &mg = ctx->map[k];
        // ~9 of the 27 cells around a query on a surface are occupied, each about as full as the cell an average map point lives in
        // (pop_sq / n, size-biased: the clusters of a dense edge map count by their points, not by their cells)
        const double est27 = (mg.occupied > 0 && mg.n > 0) ? 9.0 * double(mg.pop_sq) / double(mg.n) : 1e9;
        lanes[k] = queries <= KNN_LATENCY_LIMIT ? 16 : (est27 < double(KNN_TWO_PHASE_MIN) ? 8 : 16);
        if (ctx->knn_lanes_override == 8 || ctx->knn_lanes_override == 16 || ctx->knn_lanes_override == 32) lanes[k] = ctx->knn_lanes_override;
        if (ctx->knn_lanes_override > 99) {          // "SSCC": surf lanes, corner lanes (816, 832, 1632, ...)
            const int v = k == 0 ? ctx->knn_lanes_override / 100 : ctx->knn_lanes_override % 100;
            if (v == 8 || v == 16 || v == 32) lanes[k] = v;
        }
    }
}

// What the planner (match_plan_host.hpp) needs of the context, for a launch over these kinds; the caller adds what its launch is.
static KnnPlanIn plan_in_of(const mlh_ctx *ctx, int kind_mask)
{
    KnnPlanIn in;
    in.kind_mask = kind_mask;
    knn_lanes_for(ctx, kind_mask, in.lanes);
    for (int k = 0; k < 2; ++k) in.m[k] = ctx->feat[k].m;
    in.cu_solver = ctx->caps.cu_solver;
    in.wg_pin = ctx->knn_wg_override;
    in.fit_pin = ctx->gn_fit_in_search;
    in.sharded = ctx->shard_lo || ctx->shard_hi || ctx->own_mod > 1;
    return in;
}

// gn_solve_submit's question about the solve it is about to plan: a predecessor left its last iteration as wavefront rows -- can this solve's first launch (iteration
// 0 of a deferred solve that completes its predecessor: PRE 2, records only) read them? Asked of the planner itself, with what describe() will give it.
bool gn_first_launch_takes_rows(const mlh_ctx *ctx, int kind_mask)
{
    KnnPlanIn in = plan_in_of(ctx, kind_mask);
    in.pre_finish = PRE_SOLVE;
    in.rows_in = 4;
    return knn_plan(in).err == MLH_OK;
}

// A launch with a prologue sums THESE records: the three fields that say where an iteration's records are, set together.
static void prologue_reads(KParams &P, const mlh_ctx::GnRecords &recs, double *partials)
{
    P.partials = recs.p ? recs.p : partials;
    P.pre_rows = recs.rows;
    P.pre_tiles = recs.tiles;
}

// The one place that turns a slot of the pose plan (solve_plan_host.hpp) into an address in the solver state.
static double *pose_slot_ptr(SolverState *S, PoseSlot s)
{
    switch (s.kind) {
    case SLOT_STATE_X: return S->x;
    case SLOT_STATE_CAND: return S->cand;
    case SLOT_STATE_XB: return &S->xb[0][0];
    case SLOT_XI: return S->xi[s.n];
    case SLOT_XIB: return &S->xib[s.n][0][0];
    default: return nullptr;
    }
}

// the pinned record a launch described by `a` publishes to (TAIL_GN, TAIL_LM_STEP and every consumer-side launch), and the statistics record it fills
static HostPublish *publication_of(const MatchArgs &a) { return (a.finish == TAIL_GN || a.finish == TAIL_LM_STEP || a.lmc) ? a.publish : nullptr; }
static IterStatDev *stat_of(const mlh_ctx *ctx, const MatchArgs &a) { return a.stat_slot >= 0 ? ctx->stats.as<IterStatDev>() + a.stat_slot : nullptr; }

struct LaunchPlan {
    PosePlan pose;
    KnnPlanIn in;                      // (its lanes and the width that follows from it size the correspondence tiles of every launcher's block)
    KnnPlan knn;                       // match_launch
    LmPlan lm;                         // linearize_launch, lm_consume_launch
    mlh_ctx::GnRecords front;          // the records the search launch's prologue sums: the previous iteration's (GnChain::last) or the previous solve's (MatchArgs::pre_final)
    int n_blocks = 1, kmax = 5, tiles = 0;     // pose blocks, the largest N_NEIGH over them, fit / linearise tiles over the launch's kinds
    bool cov = false;                  // the covariance of MLH_FLAG_POSE_COV rides in this launch's publication
    bool search = false;               // match_launch: a correspondence launch, its iteration leaves records
    bool loop = false, tagged = false; // lm_consume_launch: the one-launch loop; it exchanges tagged records
};

// Step 1, the description: what the three planners decide on. Reads; changes nothing.
static LaunchPlan describe(const mlh_ctx *ctx, const MatchArgs &a)
{
    LaunchPlan pl;
    pl.n_blocks = a.n_blocks > 0 ? a.n_blocks : 1;
    for (int b = 0; b < pl.n_blocks; ++b) if (a.k_neigh[b] == 10) pl.kmax = 10;
    PosePlanIn pi;
    pi.gn_iter = a.gn_iter; pi.gn_blocks = a.gn_blocks; pi.pre_final = a.pre_final != nullptr; pi.init_pose = a.init_pose != nullptr;
    pi.pose_sel = a.pose_sel; pi.slot_base = a.gn_slot_base; pi.pre_slot = a.pre_final ? a.pre_final->slot : 0;
    pl.pose = pose_plan(pi);
    KnnPlanIn &in = pl.in;
    in = plan_in_of(ctx, a.kind_mask);
    in.mb = pl.n_blocks > 1; in.k10 = pl.kmax == 10; in.gn_blocks = a.gn_blocks; in.m_dev = a.m_dev != nullptr;
    in.pre_finish = pl.pose.pre_finish; in.warm = a.warm; in.tail = a.finish;
    in.no_fit = a.no_fit; in.dense = a.dense; in.lmc = a.lmc != LMC_NONE; in.stat = stat_of(ctx, a) != nullptr;
    if (in.pre_finish == PRE_ITERATION) pl.front = ctx->gn.last;
    if (in.pre_finish == PRE_SOLVE) pl.front = a.pre_final->recs;
    in.rows_in = in.pre_finish ? pl.front.rows : 1;
    for (int k = 0; k < 2; ++k) if (a.kind_mask & (1 << k)) pl.tiles += tiles_of(ctx->feat[k].m);
    pl.cov = (a.flags & MLH_FLAG_POSE_COV) != 0 && publication_of(a) != nullptr;
    return pl;
}

// ... and of a linearise / LM launch, for lm_plan. schedule_on() is read here, at launch time: tests change the switches in the middle of a context's life.
static LmPlanIn lm_in_of(const mlh_ctx *ctx, const MatchArgs &a, const LaunchPlan &pl, LmFamily family)
{
    LmPlanIn in;
    in.family = family; in.tail = a.finish; in.lmc = a.lmc; in.lmc_j = a.lmc_j;
    in.cov = pl.cov; in.m_dev = a.m_dev != nullptr; in.fit_in_loop = a.fit_in_loop;
    in.n_blocks = a.n_blocks; in.dense = a.dense;
    in.kind_mask = a.kind_mask; in.matched_mask = (ctx->feat[0].matched ? 1 : 0) | (ctx->feat[1].matched ? 2 : 0);
    // (the mailbox communicator rides in the finishing workgroup of a Gauss-Newton launch and of an LM begin / step launch; other launches exchange nothing)
    in.n_ranks = ((a.finish == TAIL_GN || a.finish == TAIL_LM_BEGIN || a.finish == TAIL_LM_STEP) && ctx->p2p.active) ? ctx->n_ranks : 1;
    in.tiles = pl.tiles; in.gate_tiles = (pl.cov ? ctx->caps.loop_max_tiles_cov : ctx->caps.loop_max_tiles)[a.m_dev ? 1 : 0];
    in.tagged = schedule_on(Schedule::LOOP_TAGGED) && a.lm_max_it <= 200;
    return in;
}

// Steps 2 to 5 of a planned launch. Up to the end of step 2 nothing allocates, releases, launches or counts; behind step 5 nothing refuses.
static int prepare(mlh_ctx *ctx, const MatchArgs &a, const LaunchPlan &pl)
{
    // 2. the staged kinds
    for (int k = 0; k < 2; ++k) {
        if (!(a.kind_mask & (1 << k))) continue;
        const FeatSet &fs = ctx->feat[k];
        const MapGrid &mg = ctx->map[k];
        if (!mg.built) return fail(ctx, MLH_ERR_STATE, "map_set has not been called for this kind");
        if (fs.m <= 0) return fail(ctx, MLH_ERR_STATE, "features_set has not been called for this kind");
        if (fs.n_blocks != pl.n_blocks) return fail(ctx, MLH_ERR_STATE, "the staged features hold a different number of pose blocks than requested");
        // the cell edge was derived from the acceptance radius given at map_set; a larger radius here would break exactness
        if (a.min_match_sq_dis > 0.f && std::sqrt(a.min_match_sq_dis) > mg.h)
            return fail(ctx, MLH_ERR_INVALID, "min_match_sq_dis exceeds the value the map grid was built for");
    }
    if (pl.tiles == 0) return fail(ctx, MLH_ERR_STATE, "no map/features staged for the requested kinds");
    // 3. a solve whose last iteration is still a set of tile records (GnChain::pending): any launch that writes records -- other than the chained successor's first,
    // which consumes them -- completes that solve first
    if (!a.pre_final) { const int frc = gn_flush_pending(ctx); if (frc) return frc; }
    // 4. the buffers
    hipError_t e;
    for (int k = 0; k < 2; ++k) {
        if (!(a.kind_mask & (1 << k))) continue;
        FeatSet &fs = ctx->feat[k];
        if ((e = fs.corr.ensure(sizeof(Corr) * size_t(fs.m))) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc corr", e);
        if (fs.nbr_stride < pl.kmax) { fs.nbr.release(); fs.nbr_stride = pl.kmax; }
        if ((e = fs.nbr.ensure(sizeof(float4) * size_t(fs.nbr_stride) * size_t(fs.m))) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc nbr", e);
        if (a.dense) {
            if ((e = fs.r.ensure(sizeof(double) * size_t(fs.m))) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc r", e);
            if ((e = fs.J.ensure(sizeof(double) * 6 * size_t(fs.m))) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc J", e);
        }
    }
    // (two sets of records: the consumer-side Levenberg-Marquardt launches alternate between them)
    if ((e = ctx->partials.ensure(sizeof(double) * NE_STRIDE * size_t(pl.tiles) * 2)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc partials", e);
    if ((e = ensure_ticket(ctx)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc ticket", e);
    if (ctx->p2p.active) (void)device_error_word(ctx);      // (the word a mailbox exchange that gives up sets: p2p_fill reads it)
    if (a.lmc && (e = ctx->lm.ensure_states(ctx->stream)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc lm state", e);
    if (pl.tagged && (e = ctx->lm.ensure_tagged(size_t(pl.tiles), ctx->stream)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "tagged records", e);
    // (a set of rows the prologue reads lies in this buffer; a reallocation would have been refused before the launch was planned: gn_solve_submit's `consume`)
    if (pl.knn.fused && (e = ctx->gn.rows.ensure(mlh_ctx::GnChain::rows_bytes(pl.tiles))) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc wavefront rows", e);
    // 5. the chain state
    ctx->n_partial_tiles = pl.tiles;
    if (a.lmc) ctx->lm.consumer_launch();
    if (pl.tagged) ctx->lm.tagged_launch();
    // (what a correspondence launch's iteration leaves for the next launch's prologue: its fit launch's tile records, or -- fused -- the set of wavefront rows it writes)
    if (pl.search && !a.m_dev) ctx->gn.launch_left(pl.knn.fused, pl.tiles);
    return MLH_OK;
}

// Step 6: the parameter block of the planned launch -- as its fit / linearise kernel reads it (`partials`: the records it writes). Only reads.
static void fill_params(const mlh_ctx *ctx, const MatchArgs &a, const LaunchPlan &pl, KParams &P)
{
    std::memset(&P, 0, sizeof(P));
    SolverState *S = ctx->state.as<SolverState>();
    P.n_blocks = pl.n_blocks;
    for (int b = 0; b < P.n_blocks; ++b) {
        P.kb[b] = a.k_neigh[b] == 10 ? 10 : 5;
        P.thre_b[b] = a.eig_thre[b];
        P.freeze_b[b] = a.freeze[b];
    }
    P.pre_finish = pl.pose.pre_finish;
    P.stat = stat_of(ctx, a);
    const int wg = knn_plan_width(pl.in);     // (tiles_a counts workgroups of this width)
    P.knn_lanes = knn_plan_lanes(pl.in);
    for (int k = 0; k < 2; ++k) {
        KindP &K = P.k[k];
        if (!(a.kind_mask & (1 << k))) continue;
        const FeatSet &fs = ctx->feat[k];
        K.grid = ctx->map[k].dev();
        K.feat = fs.pts.as<float4>();
        K.covd = fs.has_cov ? fs.covd.as<float4>() : nullptr;
        K.nbr = fs.nbr.as<float4>(); K.corr = fs.corr.as<Corr>();
        K.r_out = a.dense ? fs.r.as<double>() : nullptr; K.J_out = a.dense ? fs.J.as<double>() : nullptr;
        K.m = fs.m; K.lanes = pl.in.lanes[k];
        K.tiles_a = (fs.m + wg / K.lanes - 1) / (wg / K.lanes);
        K.tiles_b = tiles_of(fs.m);
        K.nbr_stride = fs.nbr_stride;
        for (int b = 0; b <= MAX_BLOCKS; ++b) K.blk_start[b] = fs.blk_start[std::min(b, fs.n_blocks)];
    }
    P.partials = ctx->partials.as<double>();
    P.state = S;
    P.pose_sel = a.pose_sel; P.flags = a.flags;
    P.min_match_sq_dis = a.min_match_sq_dis; P.min_plane_dis = a.min_plane_dis;
    P.huber_delta = a.huber_delta; P.cov_measurement_trace = a.cov_measurement_trace;
    P.own_mod = ctx->own_mod; P.own_rem = ctx->own_rem;
    P.own_mode = (ctx->shard_lo ? 1 : 0) | (ctx->shard_hi ? 2 : 0) | (ctx->own_mod > 1 ? 4 : 0);
    for (int i = 0; i < 4; ++i) { P.lo[i] = ctx->lo_plane[i]; P.hi[i] = ctx->hi_plane[i]; }
    P.finish = a.finish;
    P.lm_max_it = a.lm_max_it; P.lm_min_blocks = a.lm_min_blocks; P.lm_expect_done = a.lm_expect_done;
    // the mailbox communicator rides in the finishing workgroup of a Gauss-Newton launch and of an LM begin / step launch; other launches exchange nothing
    if ((a.finish == TAIL_GN || a.finish == TAIL_LM_BEGIN || a.finish == TAIL_LM_STEP) && ctx->p2p.active) p2p_fill(ctx, P.p2p);
    else { P2pDev none{}; none.n_ranks = 1; P.p2p = none; }
    for (int i = 0; i < 7; ++i) P.init_pose[i] = a.init_pose ? a.init_pose[i] : 0.0;
    P.warm = a.warm ? 1 : 0;
    // where the launch's poses are (solve_plan_host.hpp: pose_plan)
    P.use_init = pl.pose.use_init; P.pre_from_init = pl.pose.pre_from_init; P.pre_from_state = pl.pose.pre_from_state;
    P.x_prev = pose_slot_ptr(S, pl.pose.x_prev); P.x_next = pose_slot_ptr(S, pl.pose.x_next); P.pose0 = pose_slot_ptr(S, pl.pose.pose0);
    P.pose_b0 = pose_slot_ptr(S, pl.pose.pose_b0); P.pose_bn = pose_slot_ptr(S, pl.pose.pose_bn);
    if (P.pre_finish == PRE_SOLVE) {
        // iteration 0 of a chained solve that completes its predecessor first (knn_features_kernel<.., PRE = 2>): the predecessor's thresholds and host record, and
        // the two odometry poses this frame's start pose is chained with
        P.pre_publish = static_cast<HostPublish *>(a.pre_final->rec); P.pre_publish_seq = a.pre_final->seq;
        P.pre_thre = a.pre_final->thre; P.pre_freeze = a.pre_final->freeze;
        for (int i = 0; i < 7; ++i) { P.chain_prev[i] = a.chain_prev[i]; P.chain_cur[i] = a.chain_cur[i]; }
    }
    P.m_dev = a.m_dev;
    P.publish = publication_of(a);
    if (a.lmc) {
        P.lm_in = ctx->lm.state_in(); P.lm_out = ctx->lm.state_out();
        const size_t set = size_t(NE_STRIDE) * size_t(pl.tiles);
        P.partials_in = ctx->partials.as<double>() + set * size_t((a.lmc_j - 1) & 1);
        P.partials = ctx->partials.as<double>() + set * size_t(a.lmc_j & 1);
        if (a.lmc == LMC_LOOP) { P.partials_in = ctx->partials.as<double>(); P.partials = ctx->partials.as<double>(); }     // (the loop kernel alternates by itself)
    }
    if (pl.loop) {
        { const char *e = std::getenv("MLH_DEBUG_LOOP_STALL"); P.debug_stall = (e && std::atoi(e) != 0) ? 1 : 0; }
        P.loop_timeout_ticks = ctx->caps.loop_timeout_ticks;
        // the iterations' records as tagged words summed by polling (MLH_LOOP_TAGGED=0: plain records behind a grid barrier, as through round 5)
        if (pl.tagged) { P.loop_tagged = ctx->lm.tagged.as<unsigned long long>(); P.loop_tag_base = ctx->lm.tag_base(); }
    }
    P.publish_seq = a.publish_seq;
    P.ticket = ctx->ticket.as<unsigned>();
    P.pre_rows = 1;
    if (pl.knn.fused) P.rows_out = ctx->gn.last.p;      // (the set GnChain::launch_left just turned to)
}

template <typename Kern>
static void launch_timed(mlh_ctx *ctx, int kid, Kern kern, int grid, const KParams &P, int block = TPB)
{
    hipEvent_t a = nullptr, b = nullptr;
    if (prof_kernel_events(ctx, kid, &a, &b)) {
        hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, ctx->stream, a, b, 0, P);   // start/stop = the dispatch's own timestamps
        if (launch_check_enabled()) launch_check("correspondence / fit / linearise kernel (event-bracketed launch)");
    } else
        MLH_LAUNCH(kern, dim3(grid), dim3(block), 0, ctx->stream, P);
}

int gn_flush_pending(mlh_ctx *ctx)
{
    if (!ctx || !ctx->gn.pending.active) return MLH_OK;
    const mlh_ctx::GnPending pend = ctx->gn.take_pending();
    KParams P;
    std::memset(&P, 0, sizeof(P));
    SolverState *S = ctx->state.as<SolverState>();
    prologue_reads(P, pend.recs, ctx->partials.as<double>());
    P.state = S;
    P.pre_finish = PRE_SOLVE;
    P.x_prev = pose_slot_ptr(S, PoseSlot{SLOT_XI, pend.slot});
    P.pre_publish = static_cast<HostPublish *>(pend.rec); P.pre_publish_seq = pend.seq;
    P.pre_thre = pend.thre; P.pre_freeze = pend.freeze;
    launch_timed(ctx, MLH_K_SOLVE, gn_final_kernel, 1, P);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// The kernel of every form in the lists (match_plan_host.hpp: MLH_KNN_FORMS; solve_plan_host.hpp: MLH_LM_FORMS), in the lists' order: KNN_KERNELS[knn_form_index(form)],
// LM_KERNELS[lm_form_index(form)]. These expansions are what instantiates the correspondence, linearise, consumer and loop kernels; nothing else names one.
using KernelFn = void (*)(KParams);
template <int W, int G, bool MB, bool K10, int PRE, bool WARM, bool DEVM, bool FIT>
constexpr KernelFn knn_kernel_of()
{
    if constexpr (W == TPB) return knn_features_kernel<G, MB, K10, PRE, WARM, DEVM>;
    else return knn_features_wide_kernel<W, G, PRE, WARM, FIT>;
}
#define MLH_KNN_KERNEL_ENTRY(W, G, MB, K10, PRE, WARM, DEVM, FIT) knn_kernel_of<W, G, bool(MB), bool(K10), PRE, bool(WARM), bool(DEVM), bool(FIT)>(),
static const KernelFn KNN_KERNELS[KNN_FORM_COUNT] = {MLH_KNN_FORMS(MLH_KNN_KERNEL_ENTRY)};
#undef MLH_KNN_KERNEL_ENTRY
static_assert(KNN_WG_NARROW == TPB && KNN_FUSE_MIN_QUERIES == KNN_LATENCY_LIMIT, "the planner's two constants are the kernels'");
template <int F, bool A, bool B, bool C>
constexpr KernelFn lm_kernel_of()
{
    if constexpr (F == LM_LINEARIZE) return linearize_kernel<A, B>;
    else if constexpr (F == LM_CONSUME) return lm_consume_kernel<A, B>;
    else return lm_loop_kernel<A, B, C>;
}
#define MLH_LM_KERNEL_ENTRY(F, A, B, C) lm_kernel_of<F, bool(A), bool(B), bool(C)>(),
static const KernelFn LM_KERNELS[LM_FORM_COUNT] = {MLH_LM_FORMS(MLH_LM_KERNEL_ENTRY)};
#undef MLH_LM_KERNEL_ENTRY

static KernelFn fit_kernel_of(KnnFit fit)
{
    switch (fit) {
    case KNN_FIT_DEVM: return fit_linearize_kernel<5, false, false, true>;
    case KNN_FIT_LM_BEGIN: return fit_linearize_kernel<5, true>;
    case KNN_FIT_K10_RECORDS: return fit_linearize_kernel<10, false, false>;
    case KNN_FIT_K10: return fit_linearize_kernel<10, false>;
    case KNN_FIT_RECORDS: return fit_linearize_kernel<5, false, false>;
    case KNN_FIT_FINISH: return fit_linearize_kernel<5, false>;
    default: return nullptr;
    }
}

int match_launch(mlh_ctx *ctx, const MatchArgs &a)
{
    LaunchPlan pl = describe(ctx, a);
    pl.search = true;
    if (a.pre_final && (a.pre_final->slot >> 1) == (a.gn_slot_base >> 1)) return fail(ctx, MLH_ERR_STATE, "the predecessor's last pose slot lies in this solve's own pair");      // (x_prev != x_next: solve_plan_host.hpp)
    const KnnPlan &kp = pl.knn = knn_plan(pl.in);
    if (kp.err) return fail(ctx, kp.err, kp.why);
    const int form = knn_form_index(kp.form);
    if (form < 0) return fail(ctx, MLH_ERR_STATE, "the planned correspondence kernel is not in the list of forms");      // (unreachable: tests/host/match_plan_main.cpp)
    const int rc = prepare(ctx, a, pl);
    if (rc) return rc;
    KParams P;
    fill_params(ctx, a, pl, P);
    // kernel A: correspondences (8, 16 or 32 lanes per feature, form.W threads per workgroup); kernel B: fit + linearise + reduce (one lane per feature)
    const int grid_a = ((P.k[0].tiles_a + P.k[1].tiles_a + 7) / 8) * 8;
    const int grid_b = ((pl.tiles + 7) / 8) * 8;
    // (the search launch's prologue reads the previous iteration's records where and how that iteration left them; the fit launch, if there is one, writes `partials`)
    KParams S = P;
    if (P.pre_finish) prologue_reads(S, pl.front, P.partials);
    launch_timed(ctx, kp.kid, KNN_KERNELS[form], grid_a, S, kp.form.W);
    if (kp.gn_shape) ctx->knn_wg_last = kp.form.W;
    if (kp.fit != KNN_FIT_NONE) launch_timed(ctx, MLH_K_FIT, fit_kernel_of(kp.fit), grid_b, P);
    if (kp.fused && !P.m_dev) ++ctx->gn_fused_launches;
    MLH_HIP(ctx, hipGetLastError());
    // (no_fit: the loop launch behind this one writes the correspondences; both kinds, as the planner saw to)
    for (int k = 0; k < 2; ++k) if (a.kind_mask & (1 << k)) ctx->feat[k].matched = !a.no_fit;
    return MLH_OK;
}

// linearize_launch and lm_consume_launch behind their plan: the kernel is LM_KERNELS' entry for the planned form
static int lm_launch_planned(mlh_ctx *ctx, const MatchArgs &a, LmFamily family)
{
    LaunchPlan pl = describe(ctx, a);
    const LmPlanIn in = lm_in_of(ctx, a, pl, family);
    pl.lm = lm_plan(in);
    if (pl.lm.err) return fail(ctx, pl.lm.err, pl.lm.why);
    const int form = lm_form_index(pl.lm.form);
    if (form < 0) return fail(ctx, MLH_ERR_STATE, "the planned linearise kernel is not in the list of forms");      // (unreachable: tests/host/solve_plan_main.cpp)
    pl.loop = pl.lm.form.family == LM_LOOP;
    pl.tagged = pl.loop && in.tagged;
    const int rc = prepare(ctx, a, pl);
    if (rc) return rc;
    if (pl.loop && a.lm_expect_done == LM_FIRST_OF_SOLVE) ++ctx->caps.loop_launches;      // (the first loop of a frame)
    KParams P;
    fill_params(ctx, a, pl, P);
    launch_timed(ctx, MLH_K_LINEARIZE, LM_KERNELS[form], ((pl.tiles + 7) / 8) * 8, P);
    if (pl.loop && a.fit_in_loop) for (int k = 0; k < 2; ++k) ctx->feat[k].matched = true;
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

int linearize_launch(mlh_ctx *ctx, const MatchArgs &a) { return lm_launch_planned(ctx, a, LM_LINEARIZE); }
int lm_consume_launch(mlh_ctx *ctx, const MatchArgs &a) { return lm_launch_planned(ctx, a, LM_CONSUME); }

// the loop launch described by these arguments can carry its fit: tagged records (LmPlanIn::tagged), exactly one block, no dense rows
bool loop_fit_fusable(const MatchArgs &loop_args)
{
    return schedule_on(Schedule::LOOP_TAGGED) && loop_args.lm_max_it <= 200 && loop_args.n_blocks == 1 && !loop_args.dense;
}

int lm_loop_occupancy(int blocks_per_cu[2], int blocks_per_cu_cov[2])
{
    // per COV (the instantiations that publish the covariance, MLH_FLAG_POSE_COV, are gated by their own numbers) and DEVM: the forms with and without the fit in
    // front -- the smaller number gates both
    int *out[2] = {blocks_per_cu, blocks_per_cu_cov};
    bool seen[2][2] = {{false, false}, {false, false}};
    for (int i = 0; i < LM_FORM_COUNT; ++i) {
        const LmForm &f = LM_FORMS[i];      // lm_loop_kernel<DEVM = a, FIT = b, COV = c>
        if (f.family != LM_LOOP) continue;
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, LM_KERNELS[i], TPB, 0) != hipSuccess) return MLH_ERR_HIP;
        int &o = out[f.c][f.a];
        o = seen[f.c][f.a] ? std::min(o, n) : n;
        seen[f.c][f.a] = true;
    }
    return MLH_OK;
}

int knn_launch(mlh_ctx *ctx, int kind, const float *q_host, int nq, int32_t *idx, float *d2)
{
    MapGrid &mg = ctx->map[kind];
    if (!mg.built) return fail(ctx, MLH_ERR_STATE, "map_set has not been called for this kind");
    if (nq <= 0) return MLH_OK;
    MLH_HIP(ctx, ctx->knn_q.ensure(sizeof(float) * 3 * size_t(nq)));
    MLH_HIP(ctx, ctx->knn_idx.ensure(sizeof(int) * 5 * size_t(nq)));
    MLH_HIP(ctx, ctx->knn_d.ensure(sizeof(float) * 5 * size_t(nq)));
    MLH_HIP(ctx, hipMemcpyAsync(ctx->knn_q.p, q_host, sizeof(float) * 3 * size_t(nq), hipMemcpyHostToDevice, ctx->stream));
    const int grid = (nq + TPB / 8 - 1) / (TPB / 8);
    MLH_LAUNCH(knn_queries_kernel, dim3(grid), dim3(TPB), 0, ctx->stream, mg.dev(), ctx->knn_q.as<float>(), nq,
                       ctx->knn_idx.as<int>(), ctx->knn_d.as<float>());
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipMemcpyAsync(idx, ctx->knn_idx.p, sizeof(int) * 5 * size_t(nq), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipMemcpyAsync(d2, ctx->knn_d.p, sizeof(float) * 5 * size_t(nq), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MLH_OK;
}

}  // namespace mlh

// For the tests of the width rule (not part of the C-ABI header): threads per workgroup of the context's last correspondence launch that has wide forms, 0 before any
extern "C" int mlh_debug_knn_wg_threads(mlh_ctx *ctx) { return ctx ? ctx->knn_wg_last : 0; }
// ... and of the fused iterations: how many launches of the last submitted Gauss-Newton solve carried their fit (knn_fit_in_search())
extern "C" int mlh_debug_gn_fused_launches(mlh_ctx *ctx) { return ctx ? ctx->gn_fused_launches : 0; }
