// The loop closure's geometric verification on the device (gfx950): PoseGraph::constructLocalMap (mloam_loop/src/pose_graph.cpp:364-419) and
// LoopRegistration::performLocalRegistration (mloam_loop/src/loop_registration.cpp:104-211). include/mloam_hip.h, section (f12), has the contract and every
// CHOSEN / DEPARTURE; loopreg_host.hpp the host arithmetic (options, pose conversions, the 0.2 rule).
//   the clouds   model surf / corner and data surf / corner, float4 {x, y, z, intensity}, back to back in one pre-filter and one filtered buffer.
//                mlh_loop_build_clouds: the (cloud x keyframe) segments of the keyframe store in destination order and one FuseXf per list entry, handed to
//                stored_clouds_build (cloudbuild.hip: the builder shared with the window maps): ONE transform launch, then a voxel filter per cloud with known
//                bounds. Two host waits.
//   loop_match_kernel<KIND>   matchSurfFromMap / matchCornerFromMap (feature_extract.hpp:77-247): 16 lanes per data point; point_sel in f32; exact 5-NN through
//                knn_group over the context's map index; the fit by every lane of the group (plane_fit_qr_f / eig3_largest_f of dev_math.hpp, the mapper path's
//                restatements), lane 0 stores. Features go to per-point slots (surf: one, corner: two), invalid ones zeroed; no compaction. features.size() is an
//                integer count: LDS atomics per workgroup, one global atomic per workgroup.
//   loop_eval_kernel   LidarMapPlaneNormFactor::Evaluate (lidar_map_plane_norm_factor.hpp:56-87) in its scalar form + Huber + the 29 sums per 256-slot tile
//                (reduce_dev.hpp: reduce_rows), at a pose from the kernel arguments (the outer iteration's start) or at the LM state's candidate; the tiles' records
//                are summed by the LM launches of solver.hip in a fixed order.
//   the solve    lm_begin_launch / lm_step_launch / lm_finish_launch (solver.hip: lm_begin_body / lm_step_body, Ceres' trust-region semantics), launch per iteration:
//                1 + max_lm_iterations evaluate launches and as many one-workgroup LM launches per outer iteration, whatever the loop does (a terminated loop's
//                remaining launches return at once). No grid barrier, no polling: kernel boundaries only.
#include "ctx.hpp"
#include <algorithm>
#include <climits>
#include <cmath>
#include "dev_math.hpp"
#include "knn_dev.hpp"
#include "reduce_dev.hpp"
#include "loopreg_host.hpp"

namespace mlh {

namespace {

constexpr int LOOP_G = 16, LOOP_FPB = TPB / LOOP_G;      // lanes per data point, data points per workgroup
constexpr int LOOP_MAX_KEYS = 4096;
struct LoopXf { float r[9], t[3]; };
struct LoopPose { double p[7]; };

__device__ __forceinline__ float norm3_f(float x, float y, float z) { return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z))); }
// Eigen's normalized(): v / sqrt(squaredNorm) when the squared norm is positive, v otherwise
__device__ __forceinline__ void normalized3_f(float &x, float &y, float &z)
{
    const float z2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
    if (z2 > 0.f) { const float s = sqrtf(z2); x /= s; y /= s; z /= s; }
}

// One workgroup = LOOP_FPB data points. slots / valid: KIND surf: slot i; corner: slots 2 i, 2 i + 1 (feature1, feature2).
template <int KIND>
__global__ __launch_bounds__(TPB) void loop_match_kernel(GridDev grid, const float4 *__restrict__ data, int m, LoopXf T, float sq_thr, double plane_dis, float eig_ratio,
                                                         double4 *__restrict__ slots, unsigned char *__restrict__ valid, int *__restrict__ count)
{
    __shared__ int s_run[LOOP_FPB * 20];
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int grp = threadIdx.x / LOOP_G, gl = threadIdx.x % LOOP_G;
    const int i = blockIdx.x * LOOP_FPB + grp;
    if (i < m) {                                         // (uniform over the group of 16 lanes)
        const float4 p = data[i];
        // pointAssociateToMap(Matrix4f), hpp:37-41
        const float sx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T.r[0], p.x), __fmul_rn(T.r[1], p.y)), __fmul_rn(T.r[2], p.z)), T.t[0]);
        const float sy = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T.r[3], p.x), __fmul_rn(T.r[4], p.y)), __fmul_rn(T.r[5], p.z)), T.t[1]);
        const float sz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T.r[6], p.x), __fmul_rn(T.r[7], p.y)), __fmul_rn(T.r[8], p.z)), T.t[2]);
        unsigned long long keys[5];
        knn_group<5, LOOP_G>(grid, sx, sy, sz, gl, s_run + grp * 20, keys);
        const float d4 = __uint_as_float((unsigned)(keys[4] >> 32));
        bool ok = keys[4] != KEY_INF && d4 < sq_thr;     // hpp:105 / 203, strict
        float ax[5], ay[5], az[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int id = ok ? int((unsigned)keys[j]) : 0;
            const float4 q = (ok && id < grid.n) ? grid.raw[id] : make_float4(0.f, 0.f, 0.f, 0.f);
            ax[j] = q.x; ay[j] = q.y; az[j] = q.z;
        }
        if (KIND == MLH_SURF) {
            double4 out = make_double4(0.0, 0.0, 0.0, 0.0);
            if (ok) {
                float nx, ny, nz;
                plane_fit_qr_f<5>(ax, ay, az, nx, ny, nz);                       // hpp:211
                const float negative_OA_dot_norm = 1 / norm3_f(nx, ny, nz);      // hpp:212
                normalized3_f(nx, ny, nz);                                       // hpp:213
#pragma unroll
                for (int j = 0; j < 5; ++j) {                                    // hpp:217-226: fabs(float) against the double 0.2
                    const float v = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, ax[j]), __fmul_rn(ny, ay[j])), __fmul_rn(nz, az[j])), negative_OA_dot_norm);
                    if (double(fabsf(v)) > plane_dis) ok = false;
                }
                if (ok) out = make_double4(double(nx), double(ny), double(nz), double(negative_OA_dot_norm));
            }
            if (gl == 0) {
                slots[i] = out;
                valid[i] = ok ? 1 : 0;
                if (ok) atomicAdd(&s_cnt, 1);
            }
        } else {
            double4 o1 = make_double4(0.0, 0.0, 0.0, 0.0), o2 = o1;
            if (ok) {
                // hpp:109-124: centroid (divided by 5.0f) and covariance, f32, sums in loop order
                float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
                for (int j = 0; j < 5; ++j) { cx += ax[j]; cy += ay[j]; cz += az[j]; }
                cx /= 5.f; cy /= 5.f; cz /= 5.f;
                float c00 = 0.f, c10 = 0.f, c11 = 0.f, c20 = 0.f, c21 = 0.f, c22 = 0.f;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const float t0 = ax[j] - cx, t1 = ay[j] - cy, t2 = az[j] - cz;
                    c00 += t0 * t0; c10 += t1 * t0; c11 += t1 * t1; c20 += t2 * t0; c21 += t2 * t1; c22 += t2 * t2;
                }
                float l0, l1, l2, vx, vy, vz;
                eig3_largest_f(c00, c10, c11, c20, c21, c22, l0, l1, l2, vx, vy, vz);
                ok = l2 > eig_ratio * l1;                                        // hpp:130
                if (ok) {
                    // hpp:132-144
                    const float x1x = 0.1f * vx + cx, x1y = 0.1f * vy + cy, x1z = 0.1f * vz + cz;
                    const float x2x = -0.1f * vx + cx, x2y = -0.1f * vy + cy, x2z = -0.1f * vz + cz;
                    const float ax_ = x1x - sx, ay_ = x1y - sy, az_ = x1z - sz;
                    const float bx_ = x2x - sx, by_ = x2y - sy, bz_ = x2z - sz;
                    const float nx = ay_ * bz_ - az_ * by_, ny = az_ * bx_ - ax_ * bz_, nz = ax_ * by_ - ay_ * bx_;
                    float w2x = nx, w2y = ny, w2z = nz;
                    normalized3_f(w2x, w2y, w2z);
                    const float ex = x2x - x1x, ey = x2y - x1y, ez = x2z - x1z;
                    float w1x = w2y * ez - w2z * ey, w1y = w2z * ex - w2x * ez, w1z = w2x * ey - w2y * ex;
                    normalized3_f(w1x, w1y, w1z);
                    const float ld_1 = norm3_f(nx, ny, nz) / norm3_f(x1x - x2x, x1y - x2y, x1z - x2z);
                    const float ld_2 = 0.0f;
                    const float ld_p1 = -(__fadd_rn(__fadd_rn(__fmul_rn(w1x, sx), __fmul_rn(w1y, sy)), __fmul_rn(w1z, sz)) - ld_1);
                    const float ld_p2 = -(__fadd_rn(__fadd_rn(__fmul_rn(w2x, sx), __fmul_rn(w2y, sy)), __fmul_rn(w2z, sz)) - ld_2);
                    o1 = make_double4(double(w1x) * 0.5, double(w1y) * 0.5, double(w1z) * 0.5, double(ld_p1) * 0.5);      // hpp:147-154
                    o2 = make_double4(double(w2x) * 0.5, double(w2y) * 0.5, double(w2z) * 0.5, double(ld_p2) * 0.5);
                }
            }
            if (gl == 0) {
                slots[2 * size_t(i)] = o1; slots[2 * size_t(i) + 1] = o2;
                valid[2 * size_t(i)] = ok ? 1 : 0; valid[2 * size_t(i) + 1] = ok ? 1 : 0;
                if (ok) atomicAdd(&s_cnt, 2);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt > 0) atomicAdd(count, s_cnt);
}

// One workgroup = one 256-slot tile: tiles [0, tiles_s) the surf slots, the rest the corner slots (two per corner data point). pose_sel 0: `pose` (kernel
// arguments); 1: the LM state's candidate -- and nothing at all once the loop has terminated (the step launch behind it returns at once, too).
__global__ __launch_bounds__(TPB) void loop_eval_kernel(const double4 *__restrict__ slots, const unsigned char *__restrict__ valid, const float4 *__restrict__ surf, int m_s,
                                                        const float4 *__restrict__ corner, int m_c2, int tiles_s, const SolverState *__restrict__ S, int pose_sel,
                                                        LoopPose pose, double huber_delta, double *__restrict__ partials)
{
    __shared__ double s_red[4 * 32];
    if (pose_sel == 1 && S->done) return;
    const int tile = blockIdx.x;
    const int kind = tile >= tiles_s ? MLH_CORNER : MLH_SURF;
    const int f = (kind == MLH_CORNER ? tile - tiles_s : tile) * TPB + int(threadIdx.x);
    const int slot = kind == MLH_CORNER ? m_s + f : f;
    const bool ok = f < (kind == MLH_CORNER ? m_c2 : m_s) && valid[slot] != 0;
    const double *x = pose_sel == 1 ? S->cand : pose.p;
    const d3 t{x[0], x[1], x[2]};
    const q4 q{x[3], x[4], x[5], x[6]};
    Lin L;
    L.r = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) L.J[k] = 0.0;
    if (ok) {
        const double4 c = slots[slot];
        const float4 pf = kind == MLH_CORNER ? corner[f >> 1] : surf[f];
        const d3 p{double(pf.x), double(pf.y), double(pf.z)};
        double R[9];
        qtorot(q, R);
        d3 lp = qrot(q, p);
        lp.x += t.x; lp.y += t.y; lp.z += t.z;
        const double a = ((c.x * lp.x + c.y * lp.y) + c.z * lp.z) + c.w;         // hpp:63
        // r = a w, J = [W, -W R [p]x], W = w w^T: a rank-one block -- J^T J = |w|^2 j j^T, J^T r = |w|^2 a j, |r|^2 = |w|^2 a^2 with j = [w, -w^T R [p]x]
        const double wn = sqrt((c.x * c.x + c.y * c.y) + c.z * c.z);
        const double wr0 = (-c.x) * R[0] + (-c.y) * R[3] + (-c.z) * R[6];
        const double wr1 = (-c.x) * R[1] + (-c.y) * R[4] + (-c.z) * R[7];
        const double wr2 = (-c.x) * R[2] + (-c.y) * R[5] + (-c.z) * R[8];
        const double j0 = wr1 * p.z + wr2 * (-p.y);
        const double j1 = wr0 * (-p.z) + wr2 * p.x;
        const double j2 = wr0 * p.y + wr1 * (-p.x);
        L.r = wn * a;
        L.J[0] = wn * c.x; L.J[1] = wn * c.y; L.J[2] = wn * c.z;
        L.J[3] = wn * j0; L.J[4] = wn * j1; L.J[5] = wn * j2;
    }
    reduce_rows(ok, L, huber_delta, false, kind, s_red, partials + size_t(tile) * NE_STRIDE);
}

int loop_opts_take(mlh_ctx *ctx, const char *entry, const mlh_loop_opts *opts, mlh_loop_opts &o)
{
    if (opts) o = *opts; else loop_opts_defaults(o);
    if (const char *fault = loop_opts_fault(o)) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": bad " + fault).c_str());
    return MLH_OK;
}

bool finite16(const double *T) { for (int i = 0; i < 16; ++i) if (!std::isfinite(T[i])) return false; return true; }

LoopXf xf_of(const double T[16])
{
    LoopXf x;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) x.r[r * 3 + c] = float(T[r * 4 + c]); x.t[r] = float(T[r * 4 + 3]); }      // T.cast<float>()
    return x;
}

int tiles_of(int slots) { return (slots + TPB - 1) / TPB; }

// the two filtered model clouds into the context's map indexes, when they or the thresholds changed or another call restaged the maps since
int loop_stage_maps(mlh_ctx *ctx, const mlh_loop_opts &o)
{
    LoopStore &L = ctx->loop;
    const float sq[2] = {o.match_sq_dis_surf, o.match_sq_dis_corner};
    if (L.staged_gen == L.cloud_gen && L.staged_epoch == ctx->stage_epoch && L.staged_sq[0] == sq[0] && L.staged_sq[1] == sq[1]) return MLH_OK;
    L.staged_gen = ~0ull;
    for (int k = 0; k < 2; ++k) {
        if (L.flt_n[k] < 5) continue;                   // nothing can match: the launch is skipped (loop_match_enqueue)
        const int rc = mlh_map_set(ctx, k, L.flt.as<float4>() + L.off[k], int(sizeof(float4)), L.flt_n[k], sq[k], MLH_MEM_DEVICE);
        if (rc) return rc;
    }
    L.staged_gen = L.cloud_gen; L.staged_epoch = ctx->stage_epoch; L.staged_sq[0] = sq[0]; L.staged_sq[1] = sq[1];
    return MLH_OK;
}

int loop_slots_ensure(mlh_ctx *ctx)
{
    LoopStore &L = ctx->loop;
    const size_t n_slots = size_t(L.flt_n[MLH_LOOP_DATA_SURF]) + 2 * size_t(L.flt_n[MLH_LOOP_DATA_CORNER]);
    MLH_HIP(ctx, ensure_counted(L.slots, sizeof(double4) * (n_slots + 1), L.allocations));
    MLH_HIP(ctx, ensure_counted(L.valid, n_slots + 16, L.allocations));
    MLH_HIP(ctx, ensure_counted(L.counts, sizeof(int) * 4, L.allocations));
    return MLH_OK;
}

// both kinds (kind_mask) matched at T: the slots, the validity bytes and the two counts are rewritten. Nothing is waited for.
int loop_match_enqueue(mlh_ctx *ctx, const mlh_loop_opts &o, const LoopXf &T, int kind_mask)
{
    LoopStore &L = ctx->loop;
    hipStream_t st = ctx->stream;
    const int m_s = L.flt_n[MLH_LOOP_DATA_SURF], m_c = L.flt_n[MLH_LOOP_DATA_CORNER];
    double4 *slots = L.slots.as<double4>();
    unsigned char *valid = L.valid.as<unsigned char>();
    int *counts = L.counts.as<int>();
    prof_begin(ctx, MLH_K_KNN);
    for (int k = 0; k < 2; ++k) {
        if (!(kind_mask & (1 << k))) continue;
        const int m = k == MLH_SURF ? m_s : m_c;
        const size_t first = k == MLH_SURF ? 0 : size_t(m_s), n_slots = k == MLH_SURF ? size_t(m_s) : 2 * size_t(m_c);
        MLH_HIP(ctx, hipMemsetAsync(counts + k, 0, sizeof(int), st));
        if (m == 0) continue;
        if (L.flt_n[k] < 5) {                           // no index was staged for this kind: every slot invalid
            MLH_HIP(ctx, hipMemsetAsync(slots + first, 0, sizeof(double4) * n_slots, st));
            MLH_HIP(ctx, hipMemsetAsync(valid + first, 0, n_slots, st));
            continue;
        }
        const GridDev g = ctx->map[k].dev();
        const int grid = (m + LOOP_FPB - 1) / LOOP_FPB;
        const float4 *data = L.flt.as<float4>() + L.off[2 + k];
        if (k == MLH_SURF)
            MLH_LAUNCH(loop_match_kernel<MLH_SURF>, dim3(grid), dim3(TPB), 0, st, g, data, m, T, o.match_sq_dis_surf, o.plane_dis, o.line_eig_ratio, slots + first, valid + first, counts + k);
        else
            MLH_LAUNCH(loop_match_kernel<MLH_CORNER>, dim3(grid), dim3(TPB), 0, st, g, data, m, T, o.match_sq_dis_corner, o.plane_dis, o.line_eig_ratio, slots + first, valid + first, counts + k);
    }
    prof_end(ctx, MLH_K_KNN);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// one evaluation of every slot: the tiles' records go to ctx->partials (n_partial_tiles = the launch's tiles; none when there is no slot at all)
int loop_eval_enqueue(mlh_ctx *ctx, const mlh_loop_opts &o, int pose_sel, const double *pose)
{
    LoopStore &L = ctx->loop;
    const int m_s = L.flt_n[MLH_LOOP_DATA_SURF], m_c2 = 2 * L.flt_n[MLH_LOOP_DATA_CORNER];
    const int tiles_s = tiles_of(m_s), tiles = tiles_s + tiles_of(m_c2);
    ctx->n_partial_tiles = tiles;
    if (tiles == 0) return MLH_OK;
    LoopPose pa;
    for (int i = 0; i < 7; ++i) pa.p[i] = pose ? pose[i] : 0.0;
    prof_begin(ctx, MLH_K_LINEARIZE);
    MLH_LAUNCH(loop_eval_kernel, dim3(tiles), dim3(TPB), 0, ctx->stream, (const double4 *)L.slots.as<double4>(), (const unsigned char *)L.valid.as<unsigned char>(),
               (const float4 *)(L.flt.as<float4>() + L.off[MLH_LOOP_DATA_SURF]), m_s, (const float4 *)(L.flt.as<float4>() + L.off[MLH_LOOP_DATA_CORNER]), m_c2, tiles_s,
               (const SolverState *)ctx->state.as<SolverState>(), pose_sel, pa, o.huber_delta, ctx->partials.as<double>());
    prof_end(ctx, MLH_K_LINEARIZE);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// the pinned landing place: a build's 24 bound words and 4 counts, or a registration's LoopPinned
struct LoopPinned { IterStatDev stat; int counts[4]; };
constexpr size_t LOOP_PIN_BYTES = 1024;
static_assert(sizeof(LoopPinned) <= LOOP_PIN_BYTES && sizeof(int) * 32 <= LOOP_PIN_BYTES, "the pinned block holds either");
int loop_pin(mlh_ctx *ctx)
{
    MLH_HIP(ctx, ctx->loop.h_pin.ensure(LOOP_PIN_BYTES, 0, true));      // (allocated once: nothing enqueued can be copying into a block that is replaced)
    return MLH_OK;
}

int loop_state_ensure(mlh_ctx *ctx, int n_stats)
{
    LoopStore &L = ctx->loop;
    if (!ctx->state.p) {
        MLH_HIP(ctx, ctx->state.ensure(sizeof(SolverState)));
        MLH_HIP(ctx, hipMemsetAsync(ctx->state.p, 0, sizeof(SolverState), ctx->stream));
    }
    MLH_HIP(ctx, ctx->stats.ensure(sizeof(IterStatDev) * size_t(std::max(n_stats, 1))));
    const int tiles = tiles_of(L.flt_n[MLH_LOOP_DATA_SURF]) + tiles_of(2 * L.flt_n[MLH_LOOP_DATA_CORNER]);
    MLH_HIP(ctx, ctx->partials.ensure(sizeof(double) * NE_STRIDE * size_t(std::max(tiles, 1))));
    return loop_pin(ctx);
}

int build_clouds_run(mlh_ctx *ctx, const int32_t *data_keys, const float *data_T, int n_data, const int32_t *model_keys, const float *model_T, int n_model,
                     const mlh_loop_opts &o, int32_t *n_pre, int32_t *n_ds)
{
    LoopStore &L = ctx->loop;
    const KfStore &K = ctx->kf;
    if (n_data < 0 || n_model < 0 || n_data > LOOP_MAX_KEYS || n_model > LOOP_MAX_KEYS || (n_data > 0 && (!data_keys || !data_T)) || (n_model > 0 && (!model_keys || !model_T)))
        return fail(ctx, MLH_ERR_INVALID, "mlh_loop_build_clouds: bad lists (0..4096 keys each, with their matrices)");
    const int32_t *keys[2] = {model_keys, data_keys};
    const float *mats[2] = {model_T, data_T};
    const int n_list[2] = {n_model, n_data};
    for (int s = 0; s < 2; ++s)
        for (int e = 0; e < n_list[s]; ++e) {
            if (keys[s][e] < 0 || size_t(keys[s][e]) >= K.keys.size()) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_build_clouds: no such keyframe");
            for (int q = 0; q < 16; ++q) if (!std::isfinite(mats[s][16 * e + q])) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_build_clouds: non-finite matrix");
        }
    ++L.cloud_gen;
    // the transforms (model list, then data list) and the segments, in destination order: cloud 2 side + kind, list order inside a cloud
    std::vector<FuseXf> xfs(size_t(n_model + n_data));
    for (int s = 0; s < 2; ++s)
        for (int e = 0; e < n_list[s]; ++e) {
            FuseXf &x = xfs[size_t((s ? n_model : 0) + e)];
            const float *M = mats[s] + 16 * e;
            for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) x.r[r * 3 + c] = M[r * 4 + c]; x.t[r] = M[r * 4 + 3]; }
            x.id = 0.f;
        }
    std::vector<CloudSegment> segs;
    size_t N = 0;
    for (int c = 0; c < 4; ++c) {
        const int s = c >> 1, kind = c & 1;
        L.off[c] = int(N);
        for (int e = 0; e < n_list[s]; ++e) {
            const KfStore::Key &k = K.keys[size_t(keys[s][e])];
            segs.push_back(CloudSegment{k.off[kind], k.n[kind], (s ? n_model : 0) + e, c});
            N += size_t(k.n[kind]);
            if (N > size_t(INT_MAX) / 4) return fail(ctx, MLH_ERR_NOMEM, "mlh_loop_build_clouds: too many points");
        }
        L.pre_n[c] = int(N) - L.off[c];
        L.flt_n[c] = 0;
        if (n_pre) n_pre[c] = L.pre_n[c];
        if (n_ds) n_ds[c] = 0;
    }
    { const int rc = loop_pin(ctx); if (rc) return rc; }
    // every cloud reads the keyframe store's one arena; pcl::VoxelGrid<PointXYZI> per cloud, pose_graph.cpp:388-391, 411-414
    const float leaf[4] = {o.leaf_surf, o.leaf_corner, o.leaf_surf, o.leaf_corner};
    const int rc = stored_clouds_build(ctx, K.pts.as<float4>(), K.pts.as<float4>(), xfs, segs, 4, L.off, L.pre_n, leaf,
                                       CloudBuildBufs{L.pre, L.flt, L.tab, L.htab, L.allocations, L.h_pin.as<int>()}, L.flt_n);
    if (n_ds) for (int c = 0; c < 4; ++c) n_ds[c] = L.flt_n[c];
    return rc;
}

int set_clouds_run(mlh_ctx *ctx, const void *const *clouds, const int32_t *n, int stride, int ioff, int mem)
{
    LoopStore &L = ctx->loop;
    if (!clouds || !n) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_set_clouds: four clouds and their sizes are needed");
    Records r[4];
    size_t host_off[4] = {0, 0, 0, 0}, host_total = 0, N = 0;
    for (int c = 0; c < 4; ++c) {
        r[c] = records_of(clouds[c], stride, n[c], mem, ioff);
        { const int rc = records_check(ctx, "mlh_loop_set_clouds", r[c], true); if (rc) return rc; }
        host_off[c] = host_total; host_total += ((r[c].bytes() + 255) / 256) * 256;
        N += size_t(n[c]);
        if (N > size_t(INT_MAX) / 4) return fail(ctx, MLH_ERR_NOMEM, "mlh_loop_set_clouds: too many points");
    }
    hipStream_t st = ctx->stream;
    ++L.cloud_gen;
    MLH_HIP(ctx, ensure_counted(L.flt, sizeof(float4) * (N + 1), L.allocations));
    if (mem == MLH_MEM_HOST && host_total > 0) MLH_HIP(ctx, ctx->tmp.ensure(host_total));
    size_t at = 0;
    for (int c = 0; c < 4; ++c) {
        L.off[c] = int(at); L.pre_n[c] = 0; L.flt_n[c] = n[c];
        if (n[c] > 0) {
            const unsigned char *src;
            { const int rc = records_stage(ctx, r[c], ctx->tmp, st, &src, host_off[c]); if (rc) return rc; }
            pack_points_launch(st, src, stride, n[c], ioff >= 0 ? ioff : PACK_W_ZERO, 0.f, -1, L.flt.as<float4>() + at, nullptr);
        }
        at += size_t(n[c]);
    }
    MLH_HIP(ctx, hipGetLastError());
    if (mem == MLH_MEM_HOST) MLH_HIP(ctx, hipStreamSynchronize(st));      // the caller's clouds have been read when the call returns
    return MLH_OK;
}

int match_run(mlh_ctx *ctx, int kind, const double *T, const mlh_loop_opts &o, uint8_t *valid, double *coeffs, int32_t *n_features)
{
    LoopStore &L = ctx->loop;
    { const int rc = loop_process_gate(ctx, "mlh_loop_match"); if (rc) return rc; }
    int rc = loop_stage_maps(ctx, o);
    if (rc || (rc = loop_slots_ensure(ctx)) || (rc = loop_state_ensure(ctx, 1))) return rc;
    if ((rc = loop_match_enqueue(ctx, o, xf_of(T), 1 << kind))) return rc;
    const int m = L.flt_n[2 + kind], per = kind == MLH_SURF ? 1 : 2;
    const size_t first = kind == MLH_SURF ? 0 : size_t(L.flt_n[MLH_LOOP_DATA_SURF]), n_slots = size_t(m) * size_t(per);
    int cnt = 0;
    MLH_HIP(ctx, hipMemcpyAsync(&cnt, L.counts.as<int>() + kind, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<unsigned char> v(n_slots + 1);
    if (n_slots && (valid || coeffs)) {
        MLH_HIP(ctx, hipMemcpyAsync(v.data(), L.valid.as<unsigned char>() + first, n_slots, hipMemcpyDeviceToHost, ctx->stream));
        if (coeffs) MLH_HIP(ctx, hipMemcpyAsync(coeffs, L.slots.as<double4>() + first, sizeof(double4) * n_slots, hipMemcpyDeviceToHost, ctx->stream));
    }
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (valid) for (int i = 0; i < m; ++i) valid[i] = v[size_t(i) * size_t(per)];
    if (n_features) *n_features = cnt;
    return MLH_OK;
}

int evaluate_run(mlh_ctx *ctx, const double *T_match, const double *pose, const mlh_loop_opts &o, double *H, double *g, double *cost, int32_t *counts)
{
    { const int rc = loop_process_gate(ctx, "mlh_loop_evaluate"); if (rc) return rc; }
    int rc = loop_stage_maps(ctx, o);
    if (rc || (rc = loop_slots_ensure(ctx)) || (rc = loop_state_ensure(ctx, 1))) return rc;
    if ((rc = loop_match_enqueue(ctx, o, xf_of(T_match), 3)) || (rc = loop_eval_enqueue(ctx, o, 0, pose))) return rc;
    if ((rc = reduce_only_launch(ctx, 0))) return rc;                       // SolverState::ne <- the tiles' records in the LM launches' order
    double ne[NE_STRIDE];
    MLH_HIP(ctx, hipMemcpyAsync(ne, ctx->state.as<SolverState>()->ne, sizeof(ne), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (H) { int q = 0; for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { H[i * 6 + j] = ne[q]; H[j * 6 + i] = ne[q]; ++q; } }
    if (g) for (int i = 0; i < 6; ++i) g[i] = ne[NE_G + i];
    if (cost) *cost = ne[NE_COST];
    if (counts) { counts[0] = int(ne[NE_CNT + 1] + 0.5); counts[1] = int(ne[NE_CNT + 2] + 0.5); }
    return MLH_OK;
}

int register_run(mlh_ctx *ctx, const double *T_ini, const mlh_loop_opts &o, mlh_loop_result *res)
{
    LoopStore &L = ctx->loop;
    { const int rc = loop_process_gate(ctx, "mlh_loop_register"); if (rc) return rc; }
    int rc = loop_stage_maps(ctx, o);
    if (rc || (rc = loop_slots_ensure(ctx)) || (rc = loop_state_ensure(ctx, o.max_outer))) return rc;
    hipStream_t st = ctx->stream;
    std::memset(res, 0, sizeof(*res));
    double T[16], opti_cost = 1e7;                                          // cpp:114-116
    for (int i = 0; i < 16; ++i) T[i] = T_ini[i];
    loop_pose_of(T, res->para_pose);
    LoopPinned *pin = L.h_pin.as<LoopPinned>();
    const size_t surf_size = size_t(L.flt_n[MLH_LOOP_DATA_SURF]), corner_size = size_t(L.flt_n[MLH_LOOP_DATA_CORNER]);
    for (int outer = 0; outer < o.max_outer; ++outer) {
        double para_pose[7];
        loop_pose_of(T, para_pose);                                         // cpp:124-132
        if ((rc = loop_match_enqueue(ctx, o, xf_of(T), 3))) return rc;      // cpp:142-155
        // the solve, enqueued behind the matches before the host knows their counts (cpp:165-189)
        if ((rc = loop_eval_enqueue(ctx, o, 0, para_pose))) return rc;
        if ((rc = lm_begin_launch(ctx, -1.0, o.max_lm_iterations, outer, 0, para_pose))) return rc;
        for (int it = 0; it < o.max_lm_iterations; ++it) {
            if ((rc = loop_eval_enqueue(ctx, o, 1, nullptr)) || (rc = lm_step_launch(ctx, o.max_lm_iterations, outer))) return rc;
        }
        if ((rc = lm_finish_launch(ctx, outer))) return rc;
        // the ONE wait of this outer iteration: counts, LM summary and pose together
        MLH_HIP(ctx, hipMemcpyAsync(&pin->stat, ctx->stats.as<IterStatDev>() + outer, sizeof(IterStatDev), hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipMemcpyAsync(pin->counts, L.counts.as<int>(), sizeof(int) * 2, hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, stream_wait_spin(ctx));
        { const int drc = device_error_check(ctx); if (drc) return drc; }
        mlh_loop_outer_stat &os = res->outer[outer];
        os.entered = 1;
        os.surf_num = pin->counts[0]; os.corner_num = pin->counts[1];
        res->n_outer = outer + 1;
        if (loop_too_few_matches(size_t(os.surf_num), surf_size, size_t(os.corner_num), corner_size, o.min_match_ratio)) break;      // cpp:158-163
        os.ran = 1;
        os.lm_iterations = pin->stat.lm_iterations; os.successful_steps = pin->stat.successful_steps; os.termination = pin->stat.termination;
        os.initial_cost = pin->stat.cost; os.final_cost = pin->stat.final_cost;
        opti_cost = std::min(os.final_cost, opti_cost);                     // cpp:192
        for (int i = 0; i < 7; ++i) res->para_pose[i] = pin->stat.pose_after[i];
        loop_mat_of(res->para_pose, T);                                     // cpp:194-197
    }
    for (int i = 0; i < 16; ++i) res->T_relative[i] = T[i];
    res->opti_cost = opti_cost;
    res->accepted = loop_accepted(opti_cost, o.local_registration_threshold) ? 1 : 0;
    if (ctx->prof.mask) prof_collect(ctx);
    return MLH_OK;
}

}  // namespace

int loop_process_gate(mlh_ctx *ctx, const char *entry)
{
    if (ctx->solves.pending()) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": a solve submitted with mlh_*_begin has not been collected").c_str());
    if (distributed(ctx)) return fail(ctx, MLH_ERR_UNSUPPORTED, (std::string(entry) + ": not under a communicator (a loop process uses a context of its own)").c_str());
    return gn_flush_pending(ctx);
}

}  // namespace mlh

using namespace mlh;

extern "C" {

void mlh_loop_opts_default(mlh_loop_opts *o)
{
    if (o) loop_opts_defaults(*o);
}

int mlh_loop_build_clouds(mlh_ctx *ctx, const int32_t *data_keys, const float *data_T, int n_data, const int32_t *model_keys, const float *model_T, int n_model,
                          const mlh_loop_opts *opts, int32_t *n_pre, int32_t *n_ds)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_loop_opts o;
    { const int rc = loop_opts_take(ctx, "mlh_loop_build_clouds", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return build_clouds_run(ctx, data_keys, data_T, n_data, model_keys, model_T, n_model, o, n_pre, n_ds);
}

int mlh_loop_set_clouds(mlh_ctx *ctx, const void *const *clouds, const int32_t *n, int stride_bytes, int intensity_offset_bytes, int mem)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return set_clouds_run(ctx, clouds, n, stride_bytes, intensity_offset_bytes, mem);
}

int mlh_loop_cloud(mlh_ctx *ctx, int which, int filtered, const void **device_points, int32_t *n)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (which < 0 || which > 3 || (filtered != 0 && filtered != 1) || !device_points || !n) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_cloud: bad arguments");
    const LoopStore &L = ctx->loop;
    *n = filtered ? L.flt_n[which] : L.pre_n[which];
    *device_points = *n == 0 ? nullptr : (filtered ? L.flt : L.pre).as<float4>() + L.off[which];
    return MLH_OK;
}

int mlh_loop_info_get(mlh_ctx *ctx, mlh_loop_info *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_info_get: null output");
    const LoopStore &L = ctx->loop;
    for (int c = 0; c < 4; ++c) { out->n_pre[c] = L.pre_n[c]; out->n_ds[c] = L.flt_n[c]; }
    out->allocations = L.allocations;
    out->bytes_hbm = int64_t(L.pre.cap + L.flt.cap + L.tab.cap + L.slots.cap + L.valid.cap + L.counts.cap);
    return MLH_OK;
}

int mlh_loop_match(mlh_ctx *ctx, int kind, const double *T, const mlh_loop_opts *opts, uint8_t *valid, double *coeffs, int32_t *n_features)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (kind < 0 || kind > 1 || !T || !finite16(T)) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_match: bad kind or T");
    mlh_loop_opts o;
    { const int rc = loop_opts_take(ctx, "mlh_loop_match", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return match_run(ctx, kind, T, o, valid, coeffs, n_features);
}

int mlh_loop_evaluate(mlh_ctx *ctx, const double *T_match, const double *pose, const mlh_loop_opts *opts, double *H, double *g, double *cost, int32_t *counts)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!T_match || !pose || !finite16(T_match)) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_evaluate: bad T_match or pose");
    for (int i = 0; i < 7; ++i) if (!std::isfinite(pose[i])) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_evaluate: non-finite pose");
    mlh_loop_opts o;
    { const int rc = loop_opts_take(ctx, "mlh_loop_evaluate", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return evaluate_run(ctx, T_match, pose, o, H, g, cost, counts);
}

int mlh_loop_register(mlh_ctx *ctx, const double *T_ini, const mlh_loop_opts *opts, mlh_loop_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!T_ini || !result || !finite16(T_ini)) return fail(ctx, MLH_ERR_INVALID, "mlh_loop_register: bad T_ini or result");
    mlh_loop_opts o;
    { const int rc = loop_opts_take(ctx, "mlh_loop_register", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return register_run(ctx, T_ini, o, result);
}

}  // extern "C"
