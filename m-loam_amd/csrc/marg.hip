// The odometry window's marginalisation prior on gfx950 (estimator.cpp:658-665, 871-1063; marginalization_factor.cpp:16-82, 126-144, 189-319, 321-410;
// prior_factor.hpp:27-72). A context holds at most one prior -- n_keep kept blocks of the window layout [pivot | frames | extrinsics], their linearisation
// points x0, linearized_jacobians J0 (n x n, n = 6 n_keep), linearized_residuals r0 and the cached J0^T J0 -- and at most one set of extrinsic PriorFactor rows.
// Everything is f64 and lives in HBM between the call that makes it (mlh_window_marginalize / mlh_window_prior_set) and the solves that read it:
//   window_prior_term_kernel   one workgroup: dx = x [-] x0, res = r0 + J0 dx, then J0^T J0 / J0^T res / 0.5 |res|^2 added into the window's D x D normal
//                              equations through the block map (MarginalizationFactor::Evaluate), and the PriorFactor rows of the extrinsics when asked for.
//                              Fixed summation order, no atomics.
//   window_marg_kernel         one workgroup: Amm = 0.5 (Amm + Amm^T), its pseudo-inverse through an eigen-decomposition (eigenvalues > 1e-8), the Schur
//                              complement on the kept blocks, a second eigen-decomposition, J0 = sqrt(S) V^T, r0 = sqrt(S^-1) V^T b (MarginalizationInfo::marginalize).
// The eigen-decompositions are a parallel cyclic Jacobi iteration (n / 2 disjoint rotations per step in round-robin order, sweeps until the largest off-diagonal
// entry is below 1e-18 of the matrix's scale). The matrix being diagonalised stays in LDS (n <= 126: 124 KiB); its eigenvectors sit beside it while both fit
// (n <= 90) and in HBM beyond that.
#include "ctx.hpp"
#include "dev_math.hpp"
#include "wg_dev.hpp"

namespace mlh {

constexpr int MARG_MAX_KEEP = 21;                 // 22 window blocks, the pivot marginalised
constexpr int MARG_MAX_N = 6 * MARG_MAX_KEEP;     // 126
constexpr int MARG_V_LDS_MAX_N = 90;              // the eigenvectors share LDS with the matrix up to this size
constexpr double MARG_EPS = 1e-8;                 // marginalization_factor.h: eps
constexpr int MARG_MAX_SWEEPS = 60;

struct MargInfoDev {
    int kept[2], sweeps[2];                       // [0]: Amm, [1]: the Schur complement
    double min_kept[2], max_dropped[2];
};

// ---- the prior's term (and the extrinsics' PriorFactor rows) added into a window's normal equations
struct PriorTermArgs {
    const double *poses;    // 7 per block of the window layout
    int D;                  // 6 * window blocks
    int n_keep;             // 0: no prior term
    const int *ids;         // kept block -> window block
    const double *x0, *J0, *r0, *JtJ;
    int n_ext_rows;         // 0: no PriorFactor rows
    int ext_block0;         // window block of extrinsic 0
    const double *ext_rows; // 9 per extrinsic: t[3], q[4] (xyzw), pos_scale, rot_scale
    double *ne;             // D*D + D + 2 (J^T J | J^T r | cost, count): added to
    double *res_out;        // the n residuals, or null
};

// Eigen's Quaterniond::inverse(): conjugate / squaredNorm (zero for the zero quaternion)
__device__ __forceinline__ q4 qinverse(const q4 &q)
{
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (!(n2 > 0.0)) return q4{0.0, 0.0, 0.0, 0.0};
    return q4{-q.x / n2, -q.y / n2, -q.z / n2, q.w / n2};
}

__global__ __launch_bounds__(256) void window_prior_term_kernel(PriorTermArgs P)
{
    __shared__ double s_dx[MARG_MAX_N], s_res[MARG_MAX_N], s_ecost[MARG_MAX_KEEP + 1];
    const int t = threadIdx.x, n = 6 * P.n_keep, D = P.D;
    if (n > 0) {
        if (t < P.n_keep) {
            // marginalization_factor.cpp:381-386: translation x - x0; rotation 2 (q0^-1 q).vec(), negated when that product's w is negative (positify returns its
            // argument unchanged, utility.h:198-205, so the sign lives in the `if` alone)
            const double *x = P.poses + 7 * P.ids[t], *x0 = P.x0 + 7 * t;
            const q4 dq = qmul(qinverse(q4{x0[3], x0[4], x0[5], x0[6]}), q4{x[3], x[4], x[5], x[6]});
            double *d = s_dx + 6 * t;
            d[0] = x[0] - x0[0]; d[1] = x[1] - x0[1]; d[2] = x[2] - x0[2];
            d[3] = 2.0 * dq.x; d[4] = 2.0 * dq.y; d[5] = 2.0 * dq.z;
            if (!(dq.w >= 0.0)) { d[3] = 2.0 * -dq.x; d[4] = 2.0 * -dq.y; d[5] = 2.0 * -dq.z; }
        }
        __syncthreads();
        for (int i = t; i < n; i += 256) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) acc += P.J0[size_t(i) * n + j] * s_dx[j];
            const double r = P.r0[i] + acc;
            s_res[i] = r;
            if (P.res_out) P.res_out[i] = r;
        }
        __syncthreads();
        for (int j = t; j < n; j += 256) {
            double acc = 0.0;
            for (int i = 0; i < n; ++i) acc += P.J0[size_t(i) * n + j] * s_res[i];
            P.ne[size_t(D) * D + 6 * P.ids[j / 6] + j % 6] += acc;
        }
        for (int q = t; q < n * n; q += 256) {
            const int i = q / n, j = q % n;
            const int row = 6 * P.ids[i / 6] + i % 6, col = 6 * P.ids[j / 6] + j % 6;     // the kept blocks are distinct: one thread per entry
            P.ne[size_t(row) * D + col] += P.JtJ[q];
        }
        if (t == 0) {
            double c = 0.0;
            for (int i = 0; i < n; ++i) c += s_res[i] * s_res[i];
            P.ne[size_t(D) * D + D] += 0.5 * c;
        }
        __syncthreads();
    }
    if (P.n_ext_rows > 0) {
        if (t < P.n_ext_rows) {
            // PriorFactor::Evaluate (prior_factor.hpp:36-72): residual sqrt_info [P - pos, 2 (rot^-1 Q).vec()]; Jacobian sqrt_info [I, 0; 0, LeftQuatMatrix(Q^-1 rot)
            // .topLeftCorner<3, 3>()] -- the one its own comment calls wrong, as written
            const double *x = P.poses + 7 * (P.ext_block0 + t), *row = P.ext_rows + 9 * t;
            const q4 Q{x[3], x[4], x[5], x[6]}, rot{row[3], row[4], row[5], row[6]};
            const double ps = row[7], rs = row[8];
            const q4 e = qmul(qinverse(rot), Q), l = qmul(qinverse(Q), rot);
            const double r[6] = {ps * (x[0] - row[0]), ps * (x[1] - row[1]), ps * (x[2] - row[2]), rs * (2.0 * e.x), rs * (2.0 * e.y), rs * (2.0 * e.z)};
            // LeftQuatMatrix (common/algos/math.hpp:77-87): w I + [v]x
            const double M[9] = {rs * l.w, rs * -l.z, rs * l.y, rs * l.z, rs * l.w, rs * -l.x, rs * -l.y, rs * l.x, rs * l.w};
            const int off = 6 * (P.ext_block0 + t);
            double c = 0.0;
            for (int a = 0; a < 3; ++a) {
                P.ne[size_t(off + a) * D + off + a] += ps * ps;
                P.ne[size_t(D) * D + off + a] += ps * r[a];
                double g = 0.0;
                for (int k = 0; k < 3; ++k) g += M[k * 3 + a] * r[3 + k];
                P.ne[size_t(D) * D + off + 3 + a] += g;
                for (int b = 0; b < 3; ++b) {
                    double h = 0.0;
                    for (int k = 0; k < 3; ++k) h += M[k * 3 + a] * M[k * 3 + b];
                    P.ne[size_t(off + 3 + a) * D + off + 3 + b] += h;
                }
            }
            for (int a = 0; a < 6; ++a) c += r[a] * r[a];
            s_ecost[t] = 0.5 * c;
        }
        __syncthreads();
        if (t == 0) {
            double c = 0.0;
            for (int e = 0; e < P.n_ext_rows; ++e) c += s_ecost[e];
            P.ne[size_t(D) * D + D] += c;
        }
    }
}

// J0^T J0 of an installed prior (mlh_window_prior_set), entry by entry in row order
__global__ __launch_bounds__(256) void window_prior_jtj_kernel(const double *J0, int n, double *JtJ)
{
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n * n; q += gridDim.x * 256) {
        const int i = q / n, j = q % n;
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += J0[size_t(k) * n + i] * J0[size_t(k) * n + j];
        JtJ[q] = acc;
    }
}

// ---- symmetric eigen-decomposition by parallel cyclic Jacobi, all threads of the workgroup
constexpr int MARG_THREADS = 1024;

__device__ __forceinline__ double block_max(double v, double *s_red)
{
    v = wave_max(v);
    __syncthreads();                                    // s_red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = s_red[0];
    for (int w = 1; w < MARG_THREADS / 64; ++w) m = fmax(m, s_red[w]);
    return m;
}

// A: n x n symmetric, both triangles (n even, <= MARG_MAX_N); on return its diagonal holds the eigenvalues and V's columns the eigenvectors. One step applies the
// n / 2 rotations of a round of the round-robin tournament (player n - 1 stays, the others rotate): columns of A and V, then rows of A, then the rotated entries
// are set to zero. s_cs: n doubles, s_pq: n ints, s_red: MARG_THREADS / 64 doubles. Returns the sweeps used.
__device__ int jacobi_eig(double *A, double *V, int n, double *s_cs, int *s_pq, double *s_red)
{
    const int t = threadIdx.x, half = n / 2;
    for (int q = t; q < n * n; q += MARG_THREADS) V[q] = (q / n == q % n) ? 1.0 : 0.0;
    double dmax = 0.0;
    for (int q = t; q < n * n; q += MARG_THREADS) dmax = fmax(dmax, fabs(A[q]));
    const double scale = block_max(dmax, s_red);
    if (!(scale > 0.0)) return 0;
    int sweeps = 0;
    while (sweeps < MARG_MAX_SWEEPS) {
        double off = 0.0;
        for (int q = t; q < n * n; q += MARG_THREADS) if (q / n != q % n) off = fmax(off, fabs(A[q]));
        off = block_max(off, s_red);
        if (off <= 1e-18 * scale) break;
        for (int r = 0; r < n - 1; ++r) {
            if (t < half) {
                int p, q;
                if (t == 0) { p = r; q = n - 1; }
                else { p = (r + t) % (n - 1); q = (r - t + (n - 1)) % (n - 1); }
                if (p > q) { const int x = p; p = q; q = x; }
                const double app = A[p * n + p], aqq = A[q * n + q], apq = A[p * n + q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > 1e-20 * scale) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(tt * tt + 1.0);
                    s = tt * c;
                }
                s_cs[2 * t] = c; s_cs[2 * t + 1] = s;
                s_pq[2 * t] = p; s_pq[2 * t + 1] = q;
            }
            __syncthreads();
            for (int it = t; it < half * n; it += MARG_THREADS) {       // A <- A J, V <- V J
                const int k = it / n, i = it % n, p = s_pq[2 * k], q = s_pq[2 * k + 1];
                const double c = s_cs[2 * k], s = s_cs[2 * k + 1];
                double x = A[i * n + p], y = A[i * n + q];
                A[i * n + p] = c * x - s * y; A[i * n + q] = s * x + c * y;
                x = V[i * n + p]; y = V[i * n + q];
                V[i * n + p] = c * x - s * y; V[i * n + q] = s * x + c * y;
            }
            __syncthreads();
            for (int it = t; it < half * n; it += MARG_THREADS) {       // A <- J^T A
                const int k = it / n, j = it % n, p = s_pq[2 * k], q = s_pq[2 * k + 1];
                const double c = s_cs[2 * k], s = s_cs[2 * k + 1];
                const double x = A[p * n + j], y = A[q * n + j];
                A[p * n + j] = c * x - s * y; A[q * n + j] = s * x + c * y;
            }
            __syncthreads();
            if (t < half && s_cs[2 * t + 1] != 0.0) { const int p = s_pq[2 * t], q = s_pq[2 * t + 1]; A[p * n + q] = 0.0; A[q * n + p] = 0.0; }
            __syncthreads();
        }
        ++sweeps;
    }
    return sweeps;
}

struct MargArgs {
    const double *ne;       // the assembled D*D + D normal equations, D = 6 + n
    int n;                  // 6 * kept blocks
    double *V_hbm;          // n*n, used when the eigenvectors do not fit beside the matrix
    double *J0, *r0, *JtJ;  // the new prior
    MargInfoDev *info;
};

__global__ __launch_bounds__(MARG_THREADS) void window_marg_kernel(MargArgs M)
{
    extern __shared__ double s_A[];                     // n*n (+ n*n eigenvectors while n <= MARG_V_LDS_MAX_N)
    __shared__ double s_T[6 * MARG_MAX_N], s_bs[MARG_MAX_N], s_cs[MARG_MAX_N], s_red[MARG_THREADS / 64];
    __shared__ double s_Am[36], s_Vm[36], s_Ainv[36], s_tb[6];
    __shared__ int s_pq[MARG_MAX_N];
    const int t = threadIdx.x, n = M.n, D = 6 + n;
    double *A = s_A, *V = n <= MARG_V_LDS_MAX_N ? s_A + size_t(n) * n : M.V_hbm;
    // Amm = 0.5 (Amm + Amm^T), cpp:286
    if (t < 36) { const int i = t / 6, j = t % 6; s_Am[t] = 0.5 * (M.ne[size_t(i) * D + j] + M.ne[size_t(j) * D + i]); }
    __syncthreads();
    const int sw_m = jacobi_eig(s_Am, s_Vm, 6, s_cs, s_pq, s_red);
    __syncthreads();
    // Amm^+ = V diag(lambda > eps ? 1 / lambda : 0) V^T, cpp:291
    if (t < 36) {
        const int i = t / 6, j = t % 6;
        double acc = 0.0;
        for (int k = 0; k < 6; ++k) { const double l = s_Am[k * 6 + k]; acc += s_Vm[i * 6 + k] * (l > MARG_EPS ? 1.0 / l : 0.0) * s_Vm[j * 6 + k]; }
        s_Ainv[t] = acc;
    }
    if (t == 0) {
        int kept = 0; double mk = 0.0, md = 0.0; bool any_d = false;
        for (int k = 0; k < 6; ++k) {
            const double l = s_Am[k * 6 + k];
            if (l > MARG_EPS) { mk = kept ? fmin(mk, l) : l; ++kept; } else { md = any_d ? fmax(md, l) : l; any_d = true; }
        }
        M.info->kept[0] = kept; M.info->sweeps[0] = sw_m; M.info->min_kept[0] = mk; M.info->max_dropped[0] = md;
    }
    __syncthreads();
    // T = Amm^+ Amr (6 x n), tb = Amm^+ bmm
    for (int q = t; q < 6 * n; q += MARG_THREADS) {
        const int a = q / n, j = q % n;
        double acc = 0.0;
        for (int b = 0; b < 6; ++b) acc += s_Ainv[a * 6 + b] * M.ne[size_t(b) * D + 6 + j];
        s_T[q] = acc;
    }
    if (t < 6) {
        double acc = 0.0;
        for (int b = 0; b < 6; ++b) acc += s_Ainv[t * 6 + b] * M.ne[size_t(D) * D + b];
        s_tb[t] = acc;
    }
    __syncthreads();
    // Arr - Arm Amm^+ Amr, brr - Arm Amm^+ bmm (cpp:294-301). SelfAdjointEigenSolver reads the lower triangle: it is computed and mirrored.
    for (int q = t; q < n * n; q += MARG_THREADS) {
        const int i = q / n, j = q % n;
        if (j > i) continue;
        double acc = 0.0;
        for (int a = 0; a < 6; ++a) acc += M.ne[size_t(6 + i) * D + a] * s_T[a * n + j];
        const double v = M.ne[size_t(6 + i) * D + 6 + j] - acc;
        A[i * n + j] = v; A[j * n + i] = v;
    }
    for (int i = t; i < n; i += MARG_THREADS) {
        double acc = 0.0;
        for (int a = 0; a < 6; ++a) acc += M.ne[size_t(6 + i) * D + a] * s_tb[a];
        s_bs[i] = M.ne[size_t(D) * D + 6 + i] - acc;
    }
    __syncthreads();
    const int sw_r = jacobi_eig(A, V, n, s_cs, s_pq, s_red);
    __syncthreads();
    // linearized_jacobians = sqrt(S) V^T, linearized_residuals = sqrt(S^-1) V^T b (cpp:305-313); rows of dropped eigenvalues are zero
    for (int q = t; q < n * n; q += MARG_THREADS) {
        const int k = q / n, j = q % n;
        const double l = A[k * n + k];
        M.J0[q] = l > MARG_EPS ? sqrt(l) * V[j * n + k] : 0.0;
    }
    for (int k = t; k < n; k += MARG_THREADS) {
        const double l = A[k * n + k];
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc += V[j * n + k] * s_bs[j];
        M.r0[k] = l > MARG_EPS ? sqrt(1.0 / l) * acc : 0.0;
    }
    if (t == 0) {
        int kept = 0; double mk = 0.0, md = 0.0; bool any_d = false;
        for (int k = 0; k < n; ++k) {
            const double l = A[k * n + k];
            if (l > MARG_EPS) { mk = kept ? fmin(mk, l) : l; ++kept; } else { md = any_d ? fmax(md, l) : l; any_d = true; }
        }
        M.info->kept[1] = kept; M.info->sweeps[1] = sw_r; M.info->min_kept[1] = mk; M.info->max_dropped[1] = md;
    }
    __syncthreads();
    for (int q = t; q < n * n; q += MARG_THREADS) {
        const int i = q / n, j = q % n;
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += M.J0[size_t(k) * n + i] * M.J0[size_t(k) * n + j];
        M.JtJ[q] = acc;
    }
}

// ---- host side
static int prior_buffers(mlh_ctx *ctx, int n_keep)
{
    // sized once for the largest prior: a marginalisation replaces the prior it has just read without an allocation in between
    MargPrior &P = ctx->marg;
    (void)n_keep;
    const size_t n = MARG_MAX_N;
    MLH_HIP(ctx, P.ids_dev.ensure(sizeof(int) * MARG_MAX_KEEP));
    MLH_HIP(ctx, P.x0.ensure(sizeof(double) * 7 * MARG_MAX_KEEP));
    MLH_HIP(ctx, P.J0.ensure(sizeof(double) * n * n));
    MLH_HIP(ctx, P.r0.ensure(sizeof(double) * n));
    MLH_HIP(ctx, P.JtJ.ensure(sizeof(double) * n * n));
    return MLH_OK;
}

static void prior_info_reset(MargPrior &P)
{
    std::memset(&P.info, 0, sizeof(P.info));
    P.info.valid = P.valid ? 1 : 0;
    P.info.n_keep = P.valid ? P.n_keep : 0;
    P.info.n = 6 * P.info.n_keep;
    P.info.kept_mm = P.info.kept_rr = P.info.sweeps_mm = P.info.sweeps_rr = -1;      // not the result of a marginalisation
}

extern "C" int mlh_window_prior_clear(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MargPrior &P = ctx->marg;
    P.valid = false; P.n_keep = 0; P.shape_frames = P.shape_ext = -1;
    prior_info_reset(P);
    return MLH_OK;
}

extern "C" int mlh_window_prior_set(mlh_ctx *ctx, int n_keep, const int32_t *block_ids, const double *x0, const double *J0, const double *r0)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    if (n_keep < 1 || !block_ids || !x0 || !J0 || !r0) return fail(ctx, MLH_ERR_INVALID, "mlh_window_prior_set: bad arguments");
    if (n_keep > MARG_MAX_KEEP) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_window_prior_set: at most 21 kept blocks");
    for (int k = 0; k < n_keep; ++k) {
        if (block_ids[k] < 0 || block_ids[k] > MARG_MAX_KEEP) return fail(ctx, MLH_ERR_INVALID, "mlh_window_prior_set: block id outside 0..21");
        for (int j = 0; j < k; ++j) if (block_ids[j] == block_ids[k]) return fail(ctx, MLH_ERR_INVALID, "mlh_window_prior_set: a block is kept twice");
    }
    MargPrior &P = ctx->marg;
    { const int rc = prior_buffers(ctx, n_keep); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    const int n = 6 * n_keep;
    MLH_HIP(ctx, hipMemcpyAsync(P.ids_dev.p, block_ids, sizeof(int) * n_keep, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(P.x0.p, x0, sizeof(double) * 7 * n_keep, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(P.J0.p, J0, sizeof(double) * size_t(n) * n, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(P.r0.p, r0, sizeof(double) * n, hipMemcpyHostToDevice, st));
    MLH_LAUNCH(window_prior_jtj_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, P.J0.as<double>(), n, P.JtJ.as<double>());
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipStreamSynchronize(st));                // the caller's buffers are pageable
    for (int k = 0; k < n_keep; ++k) P.ids[k] = block_ids[k];
    P.valid = true; P.n_keep = n_keep; P.shape_frames = P.shape_ext = -1;
    prior_info_reset(P);
    return MLH_OK;
}

extern "C" int mlh_window_prior_get(mlh_ctx *ctx, mlh_window_prior_info *info, int32_t *block_ids, double *x0, double *J0, double *r0)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MargPrior &P = ctx->marg;
    if (info) { *info = P.info; info->valid = P.valid ? 1 : 0; }
    if (!P.valid) {
        if (block_ids || x0 || J0 || r0) return fail(ctx, MLH_ERR_STATE, "mlh_window_prior_get: no prior is installed");
        return MLH_OK;
    }
    hipStream_t st = ctx->stream;
    const size_t n = 6 * size_t(P.n_keep);
    if (block_ids) for (int k = 0; k < P.n_keep; ++k) block_ids[k] = P.ids[k];
    if (x0) MLH_HIP(ctx, hipMemcpyAsync(x0, P.x0.p, sizeof(double) * 7 * P.n_keep, hipMemcpyDeviceToHost, st));
    if (J0) MLH_HIP(ctx, hipMemcpyAsync(J0, P.J0.p, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
    if (r0) MLH_HIP(ctx, hipMemcpyAsync(r0, P.r0.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (x0 || J0 || r0) MLH_HIP(ctx, hipStreamSynchronize(st));
    return MLH_OK;
}

extern "C" int mlh_window_ext_prior_set(mlh_ctx *ctx, int n_ext, const double *rows, uint32_t flags)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MargPrior &P = ctx->marg;
    if (n_ext < 0 || n_ext > MARG_MAX_KEEP || (n_ext > 0 && !rows) || (flags & ~3u)) return fail(ctx, MLH_ERR_INVALID, "mlh_window_ext_prior_set: bad arguments");
    if (n_ext == 0) { P.ext_n = 0; P.ext_flags = 0; return MLH_OK; }
    MLH_HIP(ctx, P.ext_rows.ensure(sizeof(double) * 9 * MARG_MAX_KEEP));
    MLH_HIP(ctx, hipMemcpyAsync(P.ext_rows.p, rows, sizeof(double) * 9 * n_ext, hipMemcpyHostToDevice, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    P.ext_n = n_ext; P.ext_flags = flags;
    return MLH_OK;
}

int window_prior_fits(mlh_ctx *ctx, const char *entry, int n_frames, int n_ext, uint32_t ext_bit)
{
    const MargPrior &P = ctx->marg;
    const int nb = 1 + n_frames + n_ext;
    if (P.valid) {
        bool ok = P.shape_frames < 0 || (P.shape_frames == n_frames && P.shape_ext == n_ext);
        for (int k = 0; k < P.n_keep; ++k) ok = ok && P.ids[k] < nb;
        if (!ok) { ctx->err = std::string(entry) + ": the installed window prior's block map does not fit this call's (n_frames, n_ext)"; return MLH_ERR_STATE; }
    }
    if (P.ext_n > 0 && (P.ext_flags & ext_bit) && P.ext_n != n_ext) {
        ctx->err = std::string(entry) + ": the extrinsic prior was installed for another number of extrinsics";
        return MLH_ERR_STATE;
    }
    return MLH_OK;
}

bool window_prior_in_solve(const mlh_ctx *ctx) { return ctx->marg.valid || (ctx->marg.ext_n > 0 && (ctx->marg.ext_flags & 2u)); }

void window_prior_term_enqueue(mlh_ctx *ctx, const double *poses_dev, int n_frames, int n_ext, double *ne_dev, uint32_t ext_bit, double *res_out)
{
    const MargPrior &P = ctx->marg;
    PriorTermArgs T;
    T.poses = poses_dev; T.D = 6 * (1 + n_frames + n_ext);
    T.n_keep = P.valid ? P.n_keep : 0;
    T.ids = P.ids_dev.as<int>(); T.x0 = P.x0.as<double>(); T.J0 = P.J0.as<double>(); T.r0 = P.r0.as<double>(); T.JtJ = P.JtJ.as<double>();
    T.n_ext_rows = (P.ext_n > 0 && (P.ext_flags & ext_bit)) ? P.ext_n : 0;
    T.ext_block0 = 1 + n_frames; T.ext_rows = P.ext_rows.as<double>();
    T.ne = ne_dev; T.res_out = res_out;
    if (T.n_keep == 0 && T.n_ext_rows == 0) return;
    MLH_LAUNCH(window_prior_term_kernel, dim3(1), dim3(256), 0, ctx->stream, T);
}

extern "C" int mlh_window_prior_evaluate(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext,
                                         double *residuals, double *H, double *g, double *cost)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MargPrior &P = ctx->marg;
    if (!pivot || n_frames < 0 || n_ext < 0 || (n_frames > 0 && !frames) || (n_ext > 0 && !exts)) return fail(ctx, MLH_ERR_INVALID, "mlh_window_prior_evaluate: bad arguments");
    if (!P.valid) return fail(ctx, MLH_ERR_STATE, "mlh_window_prior_evaluate: no prior is installed");
    const int nb = 1 + n_frames + n_ext, D = 6 * nb, n = 6 * P.n_keep;
    if (nb > MARG_MAX_KEEP + 1) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_window_prior_evaluate: at most 22 parameter blocks");
    { const int rc = window_prior_fits(ctx, "mlh_window_prior_evaluate", n_frames, n_ext, 0u); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    const size_t n_out = size_t(D) * D + D + 2, n_all = n_out + size_t(n) + 7 * size_t(nb);
    MLH_HIP(ctx, P.eval.ensure(sizeof(double) * n_all));
    std::vector<double> h(n_all, 0.0);
    double *hp = h.data() + n_out + n;
    for (int k = 0; k < 7; ++k) hp[k] = pivot[k];
    for (int k = 0; k < 7 * n_frames; ++k) hp[7 + k] = frames[k];
    for (int k = 0; k < 7 * n_ext; ++k) hp[7 + 7 * n_frames + k] = exts[k];
    MLH_HIP(ctx, hipMemcpyAsync(P.eval.p, h.data(), sizeof(double) * n_all, hipMemcpyHostToDevice, st));
    double *d = P.eval.as<double>();
    window_prior_term_enqueue(ctx, d + n_out + n, n_frames, n_ext, d, 0u, d + n_out);
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipMemcpyAsync(h.data(), d, sizeof(double) * (n_out + n), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipStreamSynchronize(st));
    if (H) std::memcpy(H, h.data(), sizeof(double) * size_t(D) * D);
    if (g) std::memcpy(g, h.data() + size_t(D) * D, sizeof(double) * D);
    if (cost) *cost = h[size_t(D) * D + D];
    if (residuals) std::memcpy(residuals, h.data() + n_out, sizeof(double) * n);
    return MLH_OK;
}

extern "C" int mlh_window_marginalize(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext, double huber_delta,
                                      mlh_window_prior_info *info_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    // as mlh_pure_odom_gn_solve: this rank's sums are not the job's
    if (distributed(ctx)) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_window_marginalize under a communicator: build the whole factor table on one rank");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MargPrior &P = ctx->marg;
    if (!pivot || !frames || !exts || n_frames < 1 || n_ext < 1) return fail(ctx, MLH_ERR_INVALID, "mlh_window_marginalize: bad arguments");
    const int nb = 1 + n_frames + n_ext, n_keep = nb - 1, n = 6 * n_keep;
    if (nb > MARG_MAX_KEEP + 1) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_window_marginalize: at most 22 parameter blocks");
    { const int rc = window_prior_fits(ctx, "mlh_window_marginalize", n_frames, n_ext, 1u); if (rc) return rc; }
    // every factor of the table touches the pivot; the prior does when its map names block 0 (cpp:877-889); the extrinsics' PriorFactor rows never do
    bool prior_on_pivot = false;
    for (int k = 0; P.valid && k < P.n_keep; ++k) prior_on_pivot = prior_on_pivot || P.ids[k] == 0;
    const bool table = ctx->odom.n > 0 && ctx->odom.n_tiles > 0;
    if (!table && !prior_on_pivot) {                       // MarginalizationInfo::marginalize with m == 0 (cpp:210-215): no prior comes out
        mlh_window_prior_clear(ctx);
        if (info_out) *info_out = P.info;
        return MLH_OK;
    }
    { const int rc = window_assemble(ctx, pivot, frames, n_frames, exts, n_ext, huber_delta); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    double *ne = ctx->odom.ne_out.as<double>(), *poses = ctx->odom.poses.as<double>();
    window_prior_term_enqueue(ctx, poses, n_frames, n_ext, ne, 1u, nullptr);
    // the old prior has been read: the new one takes its place
    { const int rc = prior_buffers(ctx, n_keep); if (rc) return rc; }
    MLH_HIP(ctx, P.work.ensure(sizeof(double) * size_t(n) * n + sizeof(MargInfoDev)));
    MLH_HIP(ctx, P.h_info.ensure(sizeof(MargInfoDev) + sizeof(int) * (MARG_MAX_KEEP + 1)));
    MargInfoDev *d_info = reinterpret_cast<MargInfoDev *>(P.work.as<double>() + size_t(n) * n);
    MargInfoDev *h_info = P.h_info.as<MargInfoDev>();
    int *h_ids = reinterpret_cast<int *>(h_info + 1);
    // kept blocks [frames | extrinsics], already slid as addr_shift does (cpp:1042-1050): frame i -> block i, extrinsic e -> 1 + n_frames + e
    for (int i = 0; i < n_frames; ++i) h_ids[i] = i;
    for (int e = 0; e < n_ext; ++e) h_ids[n_frames + e] = 1 + n_frames + e;
    MargArgs M;
    M.ne = ne; M.n = n; M.V_hbm = P.work.as<double>(); M.J0 = P.J0.as<double>(); M.r0 = P.r0.as<double>(); M.JtJ = P.JtJ.as<double>(); M.info = d_info;
    const size_t lds = sizeof(double) * size_t(n) * n * (n <= MARG_V_LDS_MAX_N ? 2 : 1);
    MLH_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(window_marg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    MLH_LAUNCH(window_marg_kernel, dim3(1), dim3(MARG_THREADS), lds, st, M);
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipMemcpyAsync(P.x0.p, poses + 7, sizeof(double) * 7 * n_keep, hipMemcpyDeviceToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(P.ids_dev.p, h_ids, sizeof(int) * n_keep, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(h_info, d_info, sizeof(MargInfoDev), hipMemcpyDeviceToHost, st));
    for (int k = 0; k < n_keep; ++k) P.ids[k] = h_ids[k];
    P.valid = true; P.n_keep = n_keep; P.shape_frames = n_frames; P.shape_ext = n_ext;
    MLH_HIP(ctx, hipStreamSynchronize(st));                // info_out is read here
    prior_info_reset(P);
    P.info.kept_mm = h_info->kept[0]; P.info.kept_rr = h_info->kept[1]; P.info.sweeps_mm = h_info->sweeps[0]; P.info.sweeps_rr = h_info->sweeps[1];
    P.info.min_kept_mm = h_info->min_kept[0]; P.info.max_dropped_mm = h_info->max_dropped[0];
    P.info.min_kept_rr = h_info->min_kept[1]; P.info.max_dropped_rr = h_info->max_dropped[1];
    if (info_out) *info_out = P.info;
    return MLH_OK;
}

}  // namespace mlh
