// Pose-graph optimisation for the loop closure on the device (gfx950): PoseGraph::addKeyFrame's bookkeeping (mloam_loop/src/pose_graph.cpp:94-96, 140-142) and one
// pass of PoseGraph::optimizePoseGraph (cpp:505-642). include/mloam_hip.h, section (f14), has the contract and every CHOSEN / DEPARTURE; pg_host.hpp the arithmetic
// of one edge (residual, Jacobians, Plus, pose compose / inverse), shared with the host.
// One optimisation over M keyframes (block 0 constant, NB = M - 1 free 6-dof blocks, n = 6 NB) and L loop edges is a FIXED list of launches, each of which returns at
// once when the state record says the solve has terminated (or, inside an iteration, that its linear solve failed):
//   pg_begin_kernel      poses -> both slots of x, the sequential edges' measurements from the current poses, the current keyframe's old pose
//   pg_linearize_kernel  one thread per edge slot (4 sequential + 1 loop per keyframe): residual and the two 6 x 6 local Jacobians, Huber-corrected, the edge's cost;
//                        at a candidate also |J delta|^2 of the CURRENT linearisation (the model cost change's quadratic term)
//   pg_decide_kernel     one workgroup, every decision of the Levenberg-Marquardt policy (the one the library's other solves follow: solver_dev.hpp); sums in a fixed order
//   per iteration:
//   pg_assemble_kernel   per free block: the band's block column (unscaled), the full diagonal, g; the Jacobi scaling (iteration 0), the clamped LM diagonal (unless
//                        reused), S g, and the block's share of the gradient's max norm
//   pg_factor_kernel     one workgroup: the loop's head (iteration limit, gradient tolerance, minimum radius), then B = L L^T by block columns: 6 x 6 factor, 24 x 6
//                        panel solve, 24 x 24 symmetric update on a 5 x 5-block circular window in LDS; the next block row is fetched while a step computes
//   pg_forward_kernel    [Y | y_b] = L^-1 [W^T | S g]: one lane per column, each workgroup starts at the first non-zero block of its columns, L's block row is
//                        staged once per step in LDS (double-buffered) for all lanes; Y stored with the column index fastest
//   pg_gram_kernel       Y^T Y by v_mfma_f64_16x16x4_f64 on 32 x 32 macro-tiles of the lower triangle, K (= n) split over workgroups, partials to HBM
//   pg_dense_kernel      L <= 128: one workgroup: the partials summed in split order, C = I + Y^T Y factored and C z = Y^T y_b solved -- in LDS up to 84 rows, in HBM beyond
//   L > 128 (chosen by the problem's L, never by the context's capacity): the blocked dense stage over the whole device, 3 ceil(6 L / 64) launches in the order of
//   pg_host.hpp's pg_dense_step -- see "the blocked dense stage" below
//   pg_yz_kernel         y_b - Y z
//   pg_back_kernel       one workgroup: L^T x = y_b - Y z in one sweep from the last block to the first; step = -x
//   pg_candidate_kernel  x (+) S step, and the per-keyframe terms of step . S g, |x - candidate|^2, |x|^2
//   pg_linearize_kernel  (at the candidate, into the other slot), pg_decide_kernel
//   pg_writeback_kernel  updatePose on first..cur, the drift onto every later keyframe
// No floating-point atomics: every sum has one order, two runs give the same bits.
// The marginal covariances of section (f18) -- mlh_pg_marginals: these kernels on the undamped system, then four of its own -- are pgcov.inc, included at the end of
// this file's namespace.
#include "ctx.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "pg_host.hpp"
#include "pg_marg_host.hpp"
#include "wg_dev.hpp"

namespace mlh {

namespace {

constexpr int PG_TPB = 256;
constexpr int PG_WAVE = 64;
constexpr int PG_DENSE_LDS = 84;             // rows of C that fit the dense stage's LDS image (84 x 84 f64 = 55 KiB, beside the 6 KiB right-hand side)
constexpr int PG_DENSE_H_MAX = 128;          // mlh_pg_linearize hands out the dense H up to this many keyframes

struct PgState {
    int done, termination, iteration, n_succ, slot, reuse_diag, have_S, lin_ok, n_invalid, max_it;
    double radius, decrease, initial_cost, final_cost, cost;
    double cur_old[7], drift[7];
    double model_cost_change, relative_decrease, gmax;       // of the last iteration that computed them (diagnosis)
    double solve_radius;                                     // the radius the last linear solve ran with
};

struct PgDev {
    PgKeyframe *kf;
    int first, cur, count, M, NB, L, n, m, ncol, ncp, ks, rows_per;
    int T, Tb, ld;                           // the blocked dense stage (L > PG_MAX_LOOPS): column panels, row tiles, the factor's leading dimension 64 Tb; else 0
    double t_var, q_var, huber;
    double *x, *meas, *lr, *lJi, *lJj, *cost_e, *sas_e, *Bb, *hd, *g, *S, *diag, *gs, *gm, *Lrow, *Linv, *Y, *Gpart, *C, *Dg, *z, *zw, *rvec, *step, *red;
    int *loops;
    PgState *st;
};

enum { DECIDE_INIT = 0, DECIDE_STEP = 1 };

// sum of a[0..n) in a fixed order: 256 strided chains, then a tree
__device__ double pg_block_sum(const double *a, int n, double *sh)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += PG_TPB) s += a[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = PG_TPB / 2; w > 0; w >>= 1) {
        if (int(threadIdx.x) < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(PG_TPB) void pg_begin_kernel(PgDev P)
{
    const int k = blockIdx.x * PG_TPB + threadIdx.x;
    if (k >= P.M) return;
    const PgKeyframe &K = P.kf[P.first + k];
    for (int c = 0; c < 7; ++c) { P.x[size_t(k) * 7 + c] = K.pose[c]; P.x[(size_t(P.M) + k) * 7 + c] = K.pose[c]; }
    for (int s = 0; s < PG_SEQ; ++s)
        if (k - 1 - s >= 0) pg_sequential_measurement(P.kf[P.first + k - 1 - s].pose, K.pose, P.meas + (size_t(k) * PG_SEQ + s) * 7);
    if (k == P.M - 1)
        for (int c = 0; c < 7; ++c) P.st->cur_old[c] = K.pose[c];
}

__global__ __launch_bounds__(PG_TPB) void pg_linearize_kernel(PgDev P, int at_candidate)
{
    const PgState &S = *P.st;
    if (at_candidate && (S.done || !S.lin_ok)) return;
    const int e = blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= P.M * PG_SLOTS) return;
    const int cur_slot = at_candidate ? S.slot : 0, slot = at_candidate ? 1 - S.slot : 0;
    const int k = e / PG_SLOTS, s = e % PG_SLOTS;
    const PgKeyframe &K = P.kf[P.first + k];
    const int i = s < PG_SEQ ? k - 1 - s : (K.loop_index >= 0 ? K.loop_index - P.first : -1);
    const size_t E = size_t(P.M) * PG_SLOTS;
    double *cost_out = P.cost_e + size_t(slot) * E + e;
    if (i < 0) {
        *cost_out = 0.0;
        if (at_candidate) P.sas_e[e] = 0.0;
        return;
    }
    const double *xs = P.x + size_t(slot) * P.M * 7;
    const double *meas = s < PG_SEQ ? P.meas + (size_t(k) * PG_SEQ + s) * 7 : K.loop_rel;
    double r[6], Ji[36], Jj[36];
    pg_edge_eval(xs + size_t(i) * 7, xs + size_t(k) * 7, meas, P.t_var, P.q_var, r, Ji, Jj);
    double sq = 0.0;
    for (int c = 0; c < 6; ++c) sq += r[c] * r[c];
    double rho = sq;
    if (s == PG_SEQ) {
        const double sc = pg_huber(sq, P.huber, &rho);
        for (int c = 0; c < 6; ++c) r[c] *= sc;
        for (int c = 0; c < 36; ++c) { Ji[c] *= sc; Jj[c] *= sc; }
    }
    *cost_out = 0.5 * rho;
    double *ro = P.lr + (size_t(slot) * E + e) * 6, *io = P.lJi + (size_t(slot) * E + e) * 36, *jo = P.lJj + (size_t(slot) * E + e) * 36;
    for (int c = 0; c < 6; ++c) ro[c] = r[c];
    for (int c = 0; c < 36; ++c) { io[c] = Ji[c]; jo[c] = Jj[c]; }
    if (at_candidate) {
        const double *ci = P.lJi + (size_t(cur_slot) * E + e) * 36, *cj = P.lJj + (size_t(cur_slot) * E + e) * 36;
        double di[6], dj[6];
        for (int c = 0; c < 6; ++c) {
            di[c] = i >= 1 ? P.step[size_t(i - 1) * 6 + c] * P.S[size_t(i - 1) * 6 + c] : 0.0;
            dj[c] = k >= 1 ? P.step[size_t(k - 1) * 6 + c] * P.S[size_t(k - 1) * 6 + c] : 0.0;
        }
        double uu = 0.0;
        for (int a = 0; a < 6; ++a) {
            double u = 0.0;
            for (int c = 0; c < 6; ++c) u += ci[a * 6 + c] * di[c];
            for (int c = 0; c < 6; ++c) u += cj[a * 6 + c] * dj[c];
            uu += u * u;
        }
        P.sas_e[e] = uu;
    }
}

// thread (b, d): d = 0 the diagonal block, the full diagonal, g and the scalings; d = 1..4 the block (b + d, b) of the band
__global__ __launch_bounds__(PG_TPB) void pg_assemble_kernel(PgDev P, int raw)
{
    const PgState &S = *P.st;
    if (!raw && S.done) return;
    const int tid = blockIdx.x * PG_TPB + threadIdx.x;
    if (tid >= P.NB * PG_SLOTS) return;
    const int b = tid / PG_SLOTS, d = tid % PG_SLOTS, k = b + 1;
    const size_t E = size_t(P.M) * PG_SLOTS;
    const size_t so = size_t(S.slot) * E;
    double *out = P.Bb + size_t(tid) * 36;
    if (d >= 1) {
        const int kk = k + d;
        if (kk < P.M) {
            const size_t e = so + size_t(kk) * PG_SLOTS + (d - 1);
            const double *Ji = P.lJi + e * 36, *Jj = P.lJj + e * 36;
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 6; ++c) {
                    double v = 0.0;
                    for (int r = 0; r < 6; ++r) v += Jj[r * 6 + a] * Ji[r * 6 + c];
                    out[a * 6 + c] = v;
                }
        } else {
            for (int c = 0; c < 36; ++c) out[c] = 0.0;
        }
        return;
    }
    double H[36], hl[6], gv[6];
    for (int c = 0; c < 36; ++c) H[c] = 0.0;
    for (int c = 0; c < 6; ++c) { hl[c] = 0.0; gv[c] = 0.0; }
    const auto add_seq = [&](const double *J, const double *r) {
        for (int a = 0; a < 6; ++a) {
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
                for (int q = 0; q < 6; ++q) v += J[q * 6 + a] * J[q * 6 + c];
                H[a * 6 + c] += v;
            }
            double w = 0.0;
            for (int q = 0; q < 6; ++q) w += J[q * 6 + a] * r[q];
            gv[a] += w;
        }
    };
    const auto add_loop = [&](const double *J, const double *r) {
        for (int a = 0; a < 6; ++a) {
            double v = 0.0, w = 0.0;
            for (int q = 0; q < 6; ++q) { v += J[q * 6 + a] * J[q * 6 + a]; w += J[q * 6 + a] * r[q]; }
            hl[a] += v; gv[a] += w;
        }
    };
    for (int s = 0; s < PG_SEQ; ++s)
        if (k - 1 - s >= 0) { const size_t e = so + size_t(k) * PG_SLOTS + s; add_seq(P.lJj + e * 36, P.lr + e * 6); }
    for (int dd = 1; dd <= PG_SEQ; ++dd)
        if (k + dd < P.M) { const size_t e = so + size_t(k + dd) * PG_SLOTS + (dd - 1); add_seq(P.lJi + e * 36, P.lr + e * 6); }
    if (P.kf[P.first + k].loop_index >= 0) { const size_t e = so + size_t(k) * PG_SLOTS + PG_SEQ; add_loop(P.lJj + e * 36, P.lr + e * 6); }
    for (int l = 0; l < P.L; ++l) {
        const int kl = P.loops[l];
        if (P.kf[P.first + kl].loop_index - P.first == k) { const size_t e = so + size_t(kl) * PG_SLOTS + PG_SEQ; add_loop(P.lJi + e * 36, P.lr + e * 6); }
    }
    for (int c = 0; c < 36; ++c) out[c] = H[c];
    double hd[6];
    for (int c = 0; c < 6; ++c) { hd[c] = H[c * 6 + c] + hl[c]; P.hd[size_t(b) * 6 + c] = hd[c]; P.g[size_t(b) * 6 + c] = gv[c]; }
    if (raw) return;
    double ng[6], xp[7];
    for (int c = 0; c < 6; ++c) {
        double sv;
        if (!S.have_S) { sv = 1.0 / (1.0 + sqrt(hd[c])); P.S[size_t(b) * 6 + c] = sv; }
        else sv = P.S[size_t(b) * 6 + c];
        if (!S.reuse_diag) P.diag[size_t(b) * 6 + c] = fmin(fmax((sv * hd[c]) * sv, 1e-6), 1e32);
        P.gs[size_t(b) * 6 + c] = sv * gv[c];
        ng[c] = -gv[c];
    }
    const double *x = P.x + (size_t(S.slot) * P.M + k) * 7;
    pg_plus(x, ng, xp);
    double mx = 0.0;
    for (int c = 0; c < 7; ++c) mx = fmax(mx, fabs(x[c] - xp[c]));
    P.gm[b] = mx;
}

// the (i, j) entry of block (rb, cb), rb >= cb, of S H_band S + D / radius
__device__ __forceinline__ double pg_band_entry(const PgDev &P, double radius, int rb, int cb, int i, int j)
{
    double v = (P.S[size_t(rb) * 6 + i] * P.Bb[(size_t(cb) * PG_SLOTS + (rb - cb)) * 36 + i * 6 + j]) * P.S[size_t(cb) * 6 + j];
    if (rb == cb && i == j) v += P.diag[size_t(rb) * 6 + i] / radius;
    return v;
}

// force_fail: the solve is declared failed whatever its pivots (mlh_pg_optimize_forced: the invalid-step branch of the policy under test)
__global__ __launch_bounds__(PG_WAVE) void pg_factor_kernel(PgDev P, int loop_head, int force_fail)
{
    __shared__ double Wn[25 * 36];
    __shared__ double Ld[36], rinv[6], Pn[24 * 6];
    __shared__ int sh_run, sh_fail;
    __shared__ double sh_gm[PG_WAVE];
    const int t = threadIdx.x;
    PgState &S = *P.st;
    if (loop_head) {            // the gradient's max norm over the blocks' shares: a maximum has no order
        double m = 0.0;
        for (int b = t; b < P.NB; b += PG_WAVE) m = fmax(m, P.gm[b]);
        sh_gm[t] = m;
    }
    __syncthreads();
    if (t == 0) {
        int run = 1;
        if (loop_head) {
            if (S.done) run = 0;
            else {
                double gmax = 0.0;
                for (int l = 0; l < PG_WAVE; ++l) gmax = fmax(gmax, sh_gm[l]);
                S.gmax = gmax;
                if (S.iteration >= S.max_it) { S.termination = 0; S.done = 1; run = 0; }
                else if (gmax <= 1e-10) { S.termination = 1; S.done = 1; run = 0; }
                else if (S.radius <= 1e-32) { S.termination = 4; S.done = 1; run = 0; }
                else { S.iteration++; S.have_S = 1; }
            }
        }
        sh_run = run; sh_fail = 0;
    }
    __syncthreads();
    if (!sh_run) return;
    const int NB = P.NB;
    const double radius = S.radius;
    if (t == 0) S.solve_radius = radius;
    for (int idx = t; idx < 25 * 36; idx += PG_WAVE) {
        const int rb = idx / 180, cb = (idx / 36) % 5, i = (idx % 36) / 6, j = idx % 6;
        if (rb >= cb && rb < NB) Wn[idx] = pg_band_entry(P, radius, rb, cb, i, j);
    }
    __syncthreads();
    for (int b = 0; b < NB; ++b) {
        double nv[3] = {0.0, 0.0, 0.0};
        if (b + 5 < NB) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int idx = t + q * PG_WAVE;
                if (idx < 180) { const int d = idx / 36; nv[q] = pg_band_entry(P, radius, b + 5, b + 5 - d, (idx % 36) / 6, idx % 6); }
            }
        }
        const int sb = b % 5;
        if (t == 0) {
            const double *D = Wn + (sb * 5 + sb) * 36;
            for (int c = 0; c < 36; ++c) Ld[c] = 0.0;
            for (int j = 0; j < 6; ++j) {
                double p = D[j * 6 + j];
                for (int q = 0; q < j; ++q) p -= Ld[j * 6 + q] * Ld[j * 6 + q];
                if (!(p > 0.0)) { sh_fail = 1; p = 1.0; }
                const double dj = sqrt(p), ri = 1.0 / dj;
                Ld[j * 6 + j] = dj; rinv[j] = ri;
                for (int i = j + 1; i < 6; ++i) {
                    double v = D[i * 6 + j];
                    for (int q = 0; q < j; ++q) v -= Ld[i * 6 + q] * Ld[j * 6 + q];
                    Ld[i * 6 + j] = v * ri;
                }
            }
        }
        __syncthreads();
        if (t < 24) {
            const int d = 1 + t / 6, i = t % 6;
            double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (b + d < NB) {
                const double *A = Wn + (((b + d) % 5) * 5 + sb) * 36 + i * 6;
                for (int c = 0; c < 6; ++c) {
                    double v = A[c];
                    for (int q = 0; q < c; ++q) v -= p[q] * Ld[c * 6 + q];
                    p[c] = v * rinv[c];
                }
            }
            for (int c = 0; c < 6; ++c) Pn[t * 6 + c] = p[c];
        }
        __syncthreads();
        for (int idx = t; idx < 180; idx += PG_WAVE) {
            const int d = idx / 36, e = idx % 36;
            if (d == 0) P.Lrow[(size_t(b) * PG_SLOTS) * 36 + e] = Ld[e];
            else if (b + d < NB) P.Lrow[(size_t(b + d) * PG_SLOTS + d) * 36 + e] = Pn[(d - 1) * 36 + e];
        }
        if (t < 6) P.Linv[size_t(b) * 6 + t] = rinv[t];
        for (int idx = t; idx < 360; idx += PG_WAVE) {
            const int pr = idx / 36, i = (idx % 36) / 6, j = idx % 6;
            // the ten block pairs dr >= dc of 1..4
            const int dr = pr < 1 ? 1 : pr < 3 ? 2 : pr < 6 ? 3 : 4;
            const int dc = 1 + pr - (dr * (dr - 1)) / 2;
            if (b + dr < NB) {
                double v = 0.0;
                for (int q = 0; q < 6; ++q) v += Pn[((dr - 1) * 6 + i) * 6 + q] * Pn[((dc - 1) * 6 + j) * 6 + q];
                Wn[(((b + dr) % 5) * 5 + (b + dc) % 5) * 36 + i * 6 + j] -= v;
            }
        }
        __syncthreads();
        if (b + 5 < NB) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int idx = t + q * PG_WAVE;
                if (idx < 180) { const int d = idx / 36; Wn[(sb * 5 + (b + 5 - d) % 5) * 36 + idx % 36] = nv[q]; }
            }
        }
        __syncthreads();
    }
    if (t == 0) S.lin_ok = (sh_fail || force_fail) ? 0 : 1;
}

__global__ __launch_bounds__(PG_WAVE) void pg_forward_kernel(PgDev P)
{
    __shared__ double Lb[2][192];
    __shared__ int sh_start;
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, col = blockIdx.x * PG_WAVE + t;
    const int NB = P.NB, ncp = P.ncp;
    const bool active = col < ncp;
    const size_t E = size_t(P.M) * PG_SLOTS;
    int bi = -1, bj = -1, fb = NB;
    const double *rowi = nullptr, *rowj = nullptr;
    const bool is_b = col == 6 * P.L;
    if (col < 6 * P.L) {
        const int l = col / 6, r = col % 6, kl = P.loops[l];
        const size_t e = size_t(S.slot) * E + size_t(kl) * PG_SLOTS + PG_SEQ;
        bi = P.kf[P.first + kl].loop_index - P.first - 1;
        bj = kl - 1;
        rowi = P.lJi + e * 36 + r * 6; rowj = P.lJj + e * 36 + r * 6;
        fb = bi >= 0 ? min(bi, bj) : bj;
    } else if (is_b) fb = 0;
    if (t == 0) sh_start = NB;
    __syncthreads();
    atomicMin(&sh_start, fb);
    __syncthreads();
    const int b0 = sh_start;
    if (active)
        for (int row = 0; row < 6 * b0; ++row) P.Y[size_t(row) * ncp + col] = 0.0;
    if (b0 >= NB) return;
    double yp[4][6];
    for (int d = 0; d < 4; ++d)
        for (int c = 0; c < 6; ++c) yp[d][c] = 0.0;
    const auto fetch = [&](int b, int idx) { return idx < 180 ? P.Lrow[size_t(b) * 180 + idx] : P.Linv[size_t(b) * 6 + (idx - 180)]; };
    for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) Lb[0][idx] = fetch(b0, idx); }
    __syncthreads();
    for (int b = b0; b < NB; ++b) {
        const int buf = (b - b0) & 1;
        double pre[3] = {0.0, 0.0, 0.0};
        if (b + 1 < NB) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) pre[q] = fetch(b + 1, idx); }
        }
        const double *Lq = Lb[buf];
        double acc[6], y[6];
        for (int r = 0; r < 6; ++r) {
            double w = 0.0;
            if (is_b) w = P.gs[size_t(b) * 6 + r];
            else if (b == bi) w = rowi[r] * P.S[size_t(b) * 6 + r];
            else if (b == bj) w = rowj[r] * P.S[size_t(b) * 6 + r];
            acc[r] = w;
        }
#pragma unroll
        for (int d = 1; d <= 4; ++d)
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) acc[r] -= Lq[d * 36 + r * 6 + c] * yp[d - 1][c];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = acc[r];
#pragma unroll
            for (int c = 0; c < r; ++c) v -= Lq[r * 6 + c] * y[c];
            y[r] = v * Lq[180 + r];
        }
        if (active)
            for (int r = 0; r < 6; ++r) P.Y[(size_t(b) * 6 + r) * ncp + col] = y[r];
#pragma unroll
        for (int d = 3; d >= 1; --d)
#pragma unroll
            for (int c = 0; c < 6; ++c) yp[d][c] = yp[d - 1][c];
#pragma unroll
        for (int c = 0; c < 6; ++c) yp[0][c] = y[c];
        if (b + 1 < NB) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) Lb[buf ^ 1][idx] = pre[q]; }
        }
        __syncthreads();
    }
}

typedef double pg_d4 __attribute__((ext_vector_type(4)));

// blockIdx.x: the macro-tile pair (mI >= nI) of 32 x 32 outputs; blockIdx.y: the K split. One wavefront.
// v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register q of lane l is D[row (l >> 4) + 4 q][col l & 15].
// With A[m][k] = Y[k][m0 + m] and B[k][c] = Y[k][n0 + c] both operands are 16 consecutive columns of one row of Y per quarter wavefront.
__global__ __launch_bounds__(PG_WAVE) void pg_gram_kernel(PgDev P)
{
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    int mI = 0, rest = blockIdx.x;
    while (rest > mI) { rest -= mI + 1; ++mI; }
    const int nI = rest;
    const int t = threadIdx.x, lr = t >> 4, lc = t & 15, ncp = P.ncp;
    const int k0 = blockIdx.y * P.rows_per, k1 = min(P.n, k0 + P.rows_per);
    pg_d4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c) acc[a][c] = pg_d4{0.0, 0.0, 0.0, 0.0};
    for (int k = k0; k < k1; k += 4) {
        const int row = k + lr;
        double a0 = 0.0, a1 = 0.0, c0 = 0.0, c1 = 0.0;
        if (row < k1) {
            const double *yr = P.Y + size_t(row) * ncp;
            a0 = yr[mI * 32 + lc]; a1 = yr[mI * 32 + 16 + lc];
            c0 = yr[nI * 32 + lc]; c1 = yr[nI * 32 + 16 + lc];
        }
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c1, acc[1][1], 0, 0, 0);
    }
    double *G = P.Gpart + size_t(blockIdx.y) * ncp * ncp;
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c)
            for (int q = 0; q < 4; ++q) G[size_t(mI * 32 + a * 16 + lr + 4 * q) * ncp + nI * 32 + c * 16 + lc] = acc[a][c][q];
}

// keep_factor: the factor is left in P.C also when it was computed in LDS (mlh_pg_marginals reads it; an optimise does not)
__global__ __launch_bounds__(PG_TPB) void pg_dense_kernel(PgDev P, int keep_factor)
{
    __shared__ double Cl[PG_DENSE_LDS * PG_DENSE_LDS];
    __shared__ double rhs[6 * PG_MAX_LOOPS];
    __shared__ double sh_d;
    __shared__ int sh_fail;
    PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, m = P.m, ncp = P.ncp;
    if (m == 0) return;
    double *Cm = m <= PG_DENSE_LDS ? Cl : P.C;
    const size_t gs = size_t(ncp) * ncp;
    if (t == 0) sh_fail = 0;
    for (int idx = t; idx < m * m; idx += PG_TPB) {
        const int r = idx / m, c = idx % m;
        if (c > r) continue;
        double v = 0.0;
        for (int kz = 0; kz < P.ks; ++kz) v += P.Gpart[kz * gs + size_t(r) * ncp + c];
        Cm[idx] = r == c ? 1.0 + v : v;
    }
    for (int r = t; r < m; r += PG_TPB) {
        double v = 0.0;
        for (int kz = 0; kz < P.ks; ++kz) v += P.Gpart[kz * gs + size_t(m) * ncp + r];
        rhs[r] = v;
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
        if (t == 0) {
            double p = Cm[j * m + j];
            if (!(p > 0.0)) { sh_fail = 1; p = 1.0; }
            const double dj = sqrt(p);
            Cm[j * m + j] = dj; sh_d = dj;
        }
        __syncthreads();
        const double dj = sh_d;
        for (int r = j + 1 + t; r < m; r += PG_TPB) Cm[r * m + j] /= dj;
        __syncthreads();
        // the lower triangle of the trailing block, 16 x 16 threads striding rows and columns (every entry takes one product: no order to keep)
        for (int r = j + 1 + (t >> 4); r < m; r += 16) {
            const double lr = Cm[r * m + j];
            for (int c = j + 1 + (t & 15); c <= r; c += 16) Cm[r * m + c] -= lr * Cm[c * m + j];
        }
        __syncthreads();
    }
    for (int j = 0; j < m; ++j) {
        if (t == 0) rhs[j] /= Cm[j * m + j];
        __syncthreads();
        const double u = rhs[j];
        for (int r = j + 1 + t; r < m; r += PG_TPB) rhs[r] -= Cm[r * m + j] * u;
        __syncthreads();
    }
    for (int j = m - 1; j >= 0; --j) {
        if (t == 0) rhs[j] /= Cm[j * m + j];
        __syncthreads();
        const double u = rhs[j];
        for (int r = t; r < j; r += PG_TPB) rhs[r] -= Cm[j * m + r] * u;
        __syncthreads();
    }
    for (int r = t; r < m; r += PG_TPB) P.z[r] = rhs[r];
    if (keep_factor && Cm == Cl)
        for (int idx = t; idx < m * m; idx += PG_TPB) P.C[idx] = Cl[idx];
    if (t == 0 && sh_fail) S.lin_ok = 0;
}

// ---------------------------------------------------------------- the blocked dense stage (L > PG_MAX_LOOPS; m = 6 L up to 6144)
// The bordered matrix [C; r^T] -- C = I + Y^T Y (m x m), r = Y^T y_b as row m, which the Gram image already holds -- is factored by a blocked Cholesky over
// PG_PANEL = 64-wide tiles, T = ceil(m / 64) column panels and Tb = ceil((m + 1) / 64) row tiles. Carrying r along as one more row of the panel solves leaves
// L^-1 r in that row: the forward substitution is free. Only the TRANSPOSED factor is stored: U[j][r] = L[r][j] in P.C, row-major with leading dimension
// ld = 64 Tb, the contraction index j slow. Then both operands of a v_mfma_f64_16x16x4_f64 step of the update are 16 consecutive doubles of one row of U per quarter
// wavefront (the layout pg_gram_kernel documents) with no LDS transpose, the tile stores are 16 consecutive doubles too, and the backward substitution U z = w reads
// rows of U. Columns >= m of the last panel and rows > m are padding: zeros, a pivot of 1, never flagged.
// The factored DIAGONAL tiles live in P.Dg (T x 64 x 64), not in P.C: within a panel's launch every workgroup reads tile (k, k) of P.C, so the one that stores the
// factor must not store it there -- no address is written by one workgroup and read by another inside a launch.
// LEFT-looking: tile (k, i) is written once by the summation, once by the update of panel k (minus the products of ALL earlier panels, j ascending in one
// accumulator chain) and once by the panel solve. Right-looking would rewrite the whole trailing matrix once per panel (m^2 / 2 doubles x T: 14 GB of stores at
// m = 6144) and take three launches per panel (factor, solve, trailing update) where this takes two; the price is that panel k's update has only Tb - k workgroups
// with a contraction of 64 k -- the reads (about T^3 / 3 tiles) are served from rows of U that stay in L2 / MALL.
// Launches (pg_host.hpp: pg_dense_step), synchronised by kernel boundaries only:
//   pg_csum_kernel     one workgroup per tile: the Gram partials summed in split order, 1 added on the diagonal, stored transposed through LDS. 256 threads,
//                      33 KiB LDS, 18 VGPRs
//   pg_cupdate_kernel  k = 1 .. T - 1, workgroup i - k for tile (k, i): 4 wavefronts, each a 32 x 32 quadrant = 2 x 2 MFMA accumulators (32 AccVGPRs), four steps'
//                      operands in flight (56 VGPRs), straight from HBM / L2, no LDS
//   pg_cpanel_kernel   k = 0 .. T - 1, workgroup i - k: EVERY workgroup factors the diagonal tile (k, k) for itself in LDS (the same operations in the same order:
//                      the same bits; 64 column steps, two barriers each) -- that spares a launch per panel; workgroup 0 stores it, into P.Dg (T tiles of 64 x 64, a
//                      buffer of its own: tile (k, k) of P.C is READ by every workgroup of the launch, so none may write it), and reports a non-positive pivot
//                      (lin_ok = 0, the factorisation goes on with 1 in its place, as pg_dense_kernel does); the others solve X L_kk^T = tile for their tile, 16
//                      rows of it in registers per thread, one barrier per column. 256 threads, 33 KiB LDS, 91 VGPRs
//   pg_cback_kernel    k = T - 1 .. 0, workgroup jt <= k: every workgroup solves the 64 x 64 triangle of panel k for z_k (one wavefront, shuffles); workgroup k stores
//                      z_k, workgroup jt < k subtracts U[tile jt][panel k] z_k from its 64 entries of w (a wavefront per row, a fixed xor-tree). 33 KiB LDS, 24 VGPRs.
//                      Blocked over launches rather than one wide workgroup, which streams the whole factor (151 MB at m = 6144) through one compute unit:
//                      measured with a 1024-thread variant (equal bits), the dense stage of five iterations took 9.18 / 21.2 / 195.8 ms at L = 129 / 256 / 1024
//                      against 9.14 / 18.9 / 131.6 ms this way, both before the diagonal factors got their own buffer
// Every sum has one order; no atomics; every kernel returns at once when the solve is over or the band's factorisation failed (force_fail included).

__global__ __launch_bounds__(PG_TPB) void pg_csum_kernel(PgDev P)
{
    __shared__ double Tl[PG_PANEL * (PG_PANEL + 1)];
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    int k, i;
    pg_dense_sum_tile(int(blockIdx.x), P.Tb, &k, &i);
    const int t = threadIdx.x, m = P.m, ncp = P.ncp;
    const size_t gs = size_t(ncp) * ncp;
    for (int idx = t; idx < PG_PANEL * PG_PANEL; idx += PG_TPB) {
        const int rr = idx >> 6, cc = idx & 63, r = i * PG_PANEL + rr, c = k * PG_PANEL + cc;
        double v = 0.0;
        if (r <= m && c < m && c <= r) {
            for (int kz = 0; kz < P.ks; ++kz) v += P.Gpart[kz * gs + size_t(r) * ncp + c];
            if (r == c) v = 1.0 + v;
        }
        Tl[cc * (PG_PANEL + 1) + rr] = v;
    }
    __syncthreads();
    for (int idx = t; idx < PG_PANEL * PG_PANEL; idx += PG_TPB) {
        const int cc = idx >> 6, rr = idx & 63;
        P.C[(size_t(k) * PG_PANEL + cc) * P.ld + size_t(i) * PG_PANEL + rr] = Tl[cc * (PG_PANEL + 1) + rr];
    }
}

// tile (k, i) -= sum over j < 64 k of U[j][64 k + c] U[j][64 i + r]; the result's row is c (the slow index of U), its column r
__global__ __launch_bounds__(PG_TPB) void pg_cupdate_kernel(PgDev P, int k)
{
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int i = k + int(blockIdx.x);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lr = l >> 4, lc = l & 15;
    const int a0 = (w >> 1) * 32, b0 = (w & 1) * 32;
    const size_t ld = size_t(P.ld);
    const double *Uk = P.C + size_t(k) * PG_PANEL + a0 + lc, *Ui = P.C + size_t(i) * PG_PANEL + b0 + lc;
    pg_d4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c) acc[a][c] = pg_d4{0.0, 0.0, 0.0, 0.0};
    const int K = k * PG_PANEL;
    for (int j0 = 0; j0 < K; j0 += 16) {                 // (K is a multiple of 64) four steps' operands in flight
        double av[4][2], cv[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t ro = size_t(j0 + 4 * u + lr) * ld;
            av[u][0] = Uk[ro]; av[u][1] = Uk[ro + 16]; cv[u][0] = Ui[ro]; cv[u][1] = Ui[ro + 16];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][0], cv[u][0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][0], cv[u][1], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][1], cv[u][0], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][1], cv[u][1], acc[1][1], 0, 0, 0);
        }
    }
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c)
            for (int q = 0; q < 4; ++q) {
                double *o = P.C + (size_t(k) * PG_PANEL + a0 + a * 16 + lr + 4 * q) * ld + size_t(i) * PG_PANEL + b0 + c * 16 + lc;
                *o = *o - acc[a][c][q];
            }
}

__global__ __launch_bounds__(PG_TPB) void pg_cpanel_kernel(PgDev P, int k)
{
    __shared__ double Dl[PG_PANEL * PG_PANEL];           // Dl[c * 64 + r] = L_kk[r][c], r >= c
    __shared__ double xs[2][PG_PANEL];
    PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, m = P.m, i = k + int(blockIdx.x);
    const size_t ld = size_t(P.ld);
    const double *Ukk = P.C + size_t(k) * PG_PANEL * ld + size_t(k) * PG_PANEL;
    for (int idx = t; idx < PG_PANEL * PG_PANEL; idx += PG_TPB) Dl[idx] = Ukk[size_t(idx >> 6) * ld + (idx & 63)];
    __syncthreads();
    int fail = 0;
    const int r = t & 63, q = t >> 6;
    for (int j = 0; j < PG_PANEL; ++j) {
        double p = Dl[j * PG_PANEL + j];
        if (k * PG_PANEL + j >= m) p = 1.0;              // padding
        else if (!(p > 0.0)) { fail = 1; p = 1.0; }
        const double dj = sqrt(p);
        if (t > j && t < PG_PANEL) Dl[j * PG_PANEL + t] /= dj;
        __syncthreads();
        if (t == 0) Dl[j * PG_PANEL + j] = dj;           // (read by no one before the next barrier: lrj below is taken for r > j only)
        const double lrj = r > j ? Dl[j * PG_PANEL + r] : 0.0;
        for (int c = j + 1 + q; c < PG_PANEL; c += 4)
            if (r >= c) Dl[c * PG_PANEL + r] -= Dl[j * PG_PANEL + c] * lrj;
        __syncthreads();
    }
    if (i == k) {
        // the factor goes to a buffer of its own: the other workgroups of this launch read tile (k, k) of P.C, which therefore nobody writes here
        double *out = P.Dg + size_t(k) * PG_PANEL * PG_PANEL;
        for (int idx = t; idx < PG_PANEL * PG_PANEL; idx += PG_TPB) out[idx] = Dl[idx];
        if (t == 0 && fail) S.lin_ok = 0;
        return;
    }
    // thread (r, q): column r of the tile, its rows c = 4 u + q
    double *Tki = P.C + size_t(k) * PG_PANEL * ld + size_t(i) * PG_PANEL + r;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = Tki[size_t(4 * u + q) * ld];
#pragma unroll
    for (int c = 0; c < PG_PANEL; ++c) {
        if (q == (c & 3)) {
            const double x = v[c >> 2] / Dl[c * PG_PANEL + c];
            xs[c & 1][r] = x;
            Tki[size_t(c) * ld] = x;
        }
        __syncthreads();
        const double x = xs[c & 1][r];
#pragma unroll
        for (int u = c >> 2; u < 16; ++u)
            if (4 * u + q > c) v[u] -= Dl[c * PG_PANEL + 4 * u + q] * x;
    }
}

// panel k of U z = w, w = L^-1 r (column m of U): z_k from the panel's triangle, then w -= U[.][panel k] z_k on the row tiles above
__global__ __launch_bounds__(PG_TPB) void pg_cback_kernel(PgDev P, int k)
{
    __shared__ double Dl[PG_PANEL * (PG_PANEL + 1)];
    __shared__ double zs[PG_PANEL];
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, m = P.m, jt = int(blockIdx.x);
    const size_t ld = size_t(P.ld);
    const bool first = k == P.T - 1;                     // w still lies in the factor's bordering row
    const double *Dkk = P.Dg + size_t(k) * PG_PANEL * PG_PANEL;
    for (int idx = t; idx < PG_PANEL * PG_PANEL; idx += PG_TPB) Dl[(idx >> 6) * (PG_PANEL + 1) + (idx & 63)] = Dkk[idx];
    __syncthreads();
    if (t < PG_PANEL) {
        const int c = t, gc = k * PG_PANEL + c;
        // the last panel's share of the bordering row lies in its diagonal tile when m is no multiple of 64, in a row tile of its own otherwise
        double wv = !first ? P.zw[gc] : m < P.T * PG_PANEL ? Dl[c * (PG_PANEL + 1) + (m - k * PG_PANEL)] : P.C[size_t(gc) * ld + m];
        double mine = 0.0;
        for (int r = PG_PANEL - 1; r >= 0; --r) {
            double zr = __shfl(wv / Dl[r * (PG_PANEL + 1) + r], r);
            if (k * PG_PANEL + r >= m) zr = 0.0;
            if (c < r) wv -= Dl[c * (PG_PANEL + 1) + r] * zr;
            if (c == r) mine = zr;
        }
        zs[c] = mine;
    }
    __syncthreads();
    if (jt == k) {
        if (t < PG_PANEL) P.z[k * PG_PANEL + t] = zs[t];
        return;
    }
    const int w = t >> 6, l = t & 63;
    const double zl = zs[l];
    for (int rr = 0; rr < 16; ++rr) {
        const int j = jt * PG_PANEL + w * 16 + rr;
        const double v = wave_sum(P.C[size_t(j) * ld + size_t(k) * PG_PANEL + l] * zl);
        if (l == 0) P.zw[j] = (first ? P.C[size_t(j) * ld + m] : P.zw[j]) - v;
    }
}

__global__ __launch_bounds__(PG_TPB) void pg_yz_kernel(PgDev P)
{
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int i = blockIdx.x * PG_TPB + threadIdx.x;
    if (i >= P.n) return;
    const double *yr = P.Y + size_t(i) * P.ncp;
    double v = yr[P.m];
    for (int c = 0; c < P.m; ++c) v -= yr[c] * P.z[c];
    P.rvec[i] = v;
}

__global__ __launch_bounds__(PG_WAVE) void pg_back_kernel(PgDev P)
{
    __shared__ double Lb[2][192];
    __shared__ double xw[5 * 6], acc[6];
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, NB = P.NB;
    // what step b reads: L[b + d][b] (d = 0..4), 1 / diag(L[b][b]), r_b
    const auto fetch = [&](int b, int idx) {
        if (idx < 180) { const int d = idx / 36; return b + d < NB ? P.Lrow[(size_t(b + d) * PG_SLOTS + d) * 36 + idx % 36] : 0.0; }
        if (idx < 186) return P.Linv[size_t(b) * 6 + (idx - 180)];
        return P.rvec[size_t(b) * 6 + (idx - 186)];
    };
    if (t < 30) xw[t] = 0.0;
    for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 192) Lb[0][idx] = fetch(NB - 1, idx); }
    __syncthreads();
    for (int b = NB - 1; b >= 0; --b) {
        const int buf = (NB - 1 - b) & 1;
        double pre[3] = {0.0, 0.0, 0.0};
        if (b > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 192) pre[q] = fetch(b - 1, idx); }
        }
        const double *Lq = Lb[buf];
        if (t < 6) {
            double a = Lq[186 + t];
            for (int d = 1; d <= 4; ++d)
                for (int r = 0; r < 6; ++r) a -= Lq[d * 36 + r * 6 + t] * xw[((b + d) % 5) * 6 + r];
            acc[t] = a;
        }
        __syncthreads();
        if (t == 0) {
            double xn[6];
            for (int c = 5; c >= 0; --c) {
                double v = acc[c];
                for (int r = c + 1; r < 6; ++r) v -= Lq[r * 6 + c] * xn[r];
                xn[c] = v * Lq[180 + c];
            }
            for (int c = 0; c < 6; ++c) { xw[(b % 5) * 6 + c] = xn[c]; P.step[size_t(b) * 6 + c] = -xn[c]; }
        }
        if (b > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 192) Lb[buf ^ 1][idx] = pre[q]; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PG_TPB) void pg_candidate_kernel(PgDev P)
{
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int k = blockIdx.x * PG_TPB + threadIdx.x;
    if (k >= P.M) return;
    const double *x = P.x + (size_t(S.slot) * P.M + k) * 7;
    double *cand = P.x + (size_t(1 - S.slot) * P.M + k) * 7;
    double sg = 0.0, sn = 0.0, xn = 0.0;
    if (k == 0) {
        for (int c = 0; c < 7; ++c) cand[c] = x[c];
    } else {
        const int b = k - 1;
        double delta[6], out[7];
        for (int c = 0; c < 6; ++c) {
            const double s = P.step[size_t(b) * 6 + c];
            sg += s * P.gs[size_t(b) * 6 + c];
            delta[c] = s * P.S[size_t(b) * 6 + c];
        }
        pg_plus(x, delta, out);
        for (int c = 0; c < 7; ++c) { cand[c] = out[c]; sn += (x[c] - out[c]) * (x[c] - out[c]); xn += x[c] * x[c]; }
    }
    P.red[k] = sg; P.red[size_t(P.M) + k] = sn; P.red[2 * size_t(P.M) + k] = xn;
}

__global__ __launch_bounds__(PG_TPB) void pg_decide_kernel(PgDev P, int mode, int max_it, double radius0)
{
    __shared__ double sh[PG_TPB];
    PgState &S = *P.st;
    const int E = P.M * PG_SLOTS;
    if (mode == DECIDE_INIT) {
        const double cost = pg_block_sum(P.cost_e, E, sh);
        if (threadIdx.x == 0) {
            S.done = 0; S.termination = 0; S.iteration = 0; S.n_succ = 0; S.slot = 0; S.reuse_diag = 0; S.have_S = 0; S.lin_ok = 1; S.n_invalid = 0; S.max_it = max_it;
            S.radius = radius0; S.decrease = 2.0; S.initial_cost = S.final_cost = S.cost = cost;
            S.model_cost_change = 0.0; S.relative_decrease = 0.0; S.gmax = 0.0; S.solve_radius = radius0;
            for (int c = 0; c < 7; ++c) S.drift[c] = c == 6 ? 1.0 : 0.0;
            if (max_it <= 0) S.done = 1;                 // the loop's head at iteration 0 with no iteration allowed: termination 0
        }
        return;
    }
    if (S.done) return;
    const bool lin_ok = S.lin_ok != 0;
    const int slot = S.slot;
    __syncthreads();
    double sg = 0.0, sas = 0.0, sn = 0.0, xn = 0.0, cost_c = 0.0;
    if (lin_ok) {
        sg = pg_block_sum(P.red, P.M, sh);
        sn = pg_block_sum(P.red + P.M, P.M, sh);
        xn = pg_block_sum(P.red + 2 * size_t(P.M), P.M, sh);
        sas = pg_block_sum(P.sas_e, E, sh);
        cost_c = pg_block_sum(P.cost_e + size_t(1 - slot) * E, E, sh);
    }
    if (threadIdx.x != 0) return;
    S.reuse_diag = 1;
    const double mcc = -(sg + 0.5 * sas);
    S.model_cost_change = lin_ok ? mcc : 0.0;
    const bool valid = lin_ok && mcc > 0.0;
    if (!valid) {
        if (++S.n_invalid >= 5) { S.termination = 4; S.done = 1; }
        else { S.radius /= S.decrease; S.decrease *= 2.0; }
    } else {
        S.n_invalid = 0;
        const double step_norm = sqrt(sn), x_norm = sqrt(xn);
        const double cost_change = S.cost - cost_c;
        if (step_norm <= 1e-8 * (x_norm + 1e-8)) { S.termination = 2; S.done = 1; }
        else if (fabs(cost_change) <= 1e-6 * S.cost) { S.termination = 3; S.done = 1; }
        else {
            const double rd = cost_change / mcc;
            S.relative_decrease = rd;
            if (rd > 1e-3) {
                S.slot = 1 - slot; S.cost = cost_c; S.n_succ++; S.final_cost = cost_c;
                const double w = 2.0 * rd - 1.0;
                S.radius = fmin(1e16, S.radius / fmax(1.0 / 3.0, 1.0 - w * w * w));
                S.decrease = 2.0; S.reuse_diag = 0;
            } else { S.radius /= S.decrease; S.decrease *= 2.0; }
        }
    }
    S.lin_ok = 1;
    if (!S.done && S.iteration >= S.max_it) { S.termination = 0; S.done = 1; }
}

// first..cur: updatePose(Pose(q, t)) with the solve's values; cur + 1 .. count - 1: updatePose(pose_drift * pose)
__global__ __launch_bounds__(PG_TPB) void pg_writeback_kernel(PgDev P)
{
    const int k = blockIdx.x * PG_TPB + threadIdx.x;
    if (P.first + k >= P.count) return;
    PgState &S = *P.st;
    PgKeyframe &K = P.kf[P.first + k];
    const double *xs = P.x + size_t(S.slot) * P.M * 7;
    double old[7], nw[7];
    for (int c = 0; c < 7; ++c) old[c] = K.pose[c];
    if (k < P.M) {
        double q[4];
        pg_q_of_pose(xs + size_t(k) * 7, q);
        pg_pose_make(q, xs + size_t(k) * 7, nw);
    }
    if (k >= P.M - 1) {
        double q[4], cur_new[7], inv[7], drift[7];
        pg_q_of_pose(xs + size_t(P.M - 1) * 7, q);
        pg_pose_make(q, xs + size_t(P.M - 1) * 7, cur_new);
        pg_pose_inverse(S.cur_old, inv);
        pg_pose_mul(cur_new, inv, drift);
        if (k == P.M - 1) { for (int c = 0; c < 7; ++c) S.drift[c] = drift[c]; }
        else pg_pose_mul(drift, old, nw);
    }
    for (int c = 0; c < 7; ++c) { K.last[c] = old[c]; K.pose[c] = nw[c]; }
}

// ---------------------------------------------------------------- host

int pg_gate(mlh_ctx *ctx, const char *entry)
{
    { const int rc = loop_process_gate(ctx, entry); if (rc) return rc; }
    ctx->pg.launches = 0; ctx->pg.host_waits = 0;          // (a refused call leaves the previous call's counts)
    return MLH_OK;
}

int pg_opts_take(mlh_ctx *ctx, const char *entry, const mlh_pg_opts *opts, mlh_pg_opts &o)
{
    if (opts) o = *opts; else pg_opts_defaults(o);
    if (const char *f = pg_opts_fault(o)) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": bad option " + f).c_str());
    return MLH_OK;
}

inline int pg_blocks(size_t n) { return int((n + PG_TPB - 1) / PG_TPB); }

// the problem first..cur: checks, sizes, the work buffers carved out of one allocation, the loop list uploaded
int pg_problem(mlh_ctx *ctx, const char *entry, int cur_index, const mlh_pg_opts &o, PgDev &P)
{
    PgStore &G = ctx->pg;
    if (cur_index < 0 || cur_index >= G.count) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": cur_index names no keyframe").c_str());
    if (G.earliest_loop < 0) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": no loop has been set yet").c_str());
    if (cur_index < G.earliest_loop) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": cur_index lies before the earliest looped keyframe").c_str());
    std::memset(&P, 0, sizeof(P));
    P.first = G.earliest_loop; P.cur = cur_index; P.count = G.count;
    P.M = cur_index - P.first + 1; P.NB = P.M - 1; P.n = 6 * P.NB;
    std::vector<int> &loops = G.h_loops;         // (a member: the copy below reads it after this function has returned)
    loops.clear();
    for (int k = 0; k < P.M; ++k)
        if (G.loop_index[size_t(P.first + k)] >= 0) loops.push_back(k);
    if (int(loops.size()) > G.max_loops)
        return fail(ctx, MLH_ERR_UNSUPPORTED, (std::string(entry) + ": " + std::to_string(loops.size()) + " loop edges between the earliest looped keyframe and cur_index; at most " +
                                               std::to_string(G.max_loops) + " are supported (mlh_pg_info::max_loops; mlh_pg_reserve raises it up to " +
                                               std::to_string(int(MLH_PG_LOOPS_LIMIT)) + ")").c_str());
    P.L = int(loops.size()); P.m = 6 * P.L; P.ncol = P.m + 1; P.ncp = ((P.ncol + 31) / 32) * 32;
    const bool blocked = P.L > PG_MAX_LOOPS;
    if (blocked) { P.T = pg_dense_panels(P.m); P.Tb = pg_dense_row_tiles(P.m); P.ld = P.Tb * PG_PANEL; }
    const size_t gbytes = size_t(P.ncp) * P.ncp * sizeof(double);
    const int ks_max = int(std::max<size_t>(1, (size_t(128) << 20) / gbytes));
    int rows_per = std::max(256, (P.n + 63) / 64);
    rows_per = std::max(rows_per, (P.n + ks_max - 1) / ks_max);
    rows_per = ((rows_per + 3) / 4) * 4;
    P.rows_per = rows_per; P.ks = std::max(1, (P.n + rows_per - 1) / rows_per);
    P.t_var = o.t_var; P.q_var = o.q_var; P.huber = o.huber_delta;
    const size_t M = size_t(P.M), NB = size_t(P.NB), E = M * PG_SLOTS, n = size_t(P.n), m = size_t(P.m);
    size_t off = 0;
    const auto take = [&](size_t doubles) { const size_t at = off; off += ((doubles + 1 + 15) / 16) * 16; return at; };
    const size_t o_x = take(2 * M * 7), o_meas = take(M * PG_SEQ * 7), o_lr = take(2 * E * 6), o_Ji = take(2 * E * 36), o_Jj = take(2 * E * 36), o_ce = take(2 * E),
                 o_sas = take(E), o_Bb = take(NB * 180), o_hd = take(NB * 6), o_g = take(NB * 6), o_S = take(NB * 6), o_diag = take(NB * 6), o_gs = take(NB * 6),
                 o_gm = take(NB), o_Lrow = take(NB * 180), o_Linv = take(NB * 6), o_Y = take(n * P.ncp), o_G = take(size_t(P.ks) * P.ncp * P.ncp),
                 o_C = take(blocked ? size_t(P.T) * PG_PANEL * P.ld : m * m), o_z = take(blocked ? size_t(P.T) * PG_PANEL : m), o_rv = take(n), o_step = take(n),
                 o_red = take(3 * M), o_loops = take((size_t(P.L) + 1) / 2 + 1), o_zw = take(blocked ? size_t(P.T) * PG_PANEL : 0),
                 o_Dg = take(blocked ? size_t(P.T) * PG_PANEL * PG_PANEL : 0);
    const size_t before = G.work.cap + G.state.cap + G.h_pin.cap;
    {   // (ensure frees before it allocates: after a failure the work buffer is empty and the next call allocates again; the keyframe store is not touched)
        const hipError_t e = G.work.ensure(off * sizeof(double));
        if (e != hipSuccess) {
            G.work.p = nullptr; G.work.cap = 0;
            (void)hipGetLastError();
            return fail(ctx, MLH_ERR_HIP, (std::string(entry) + ": the work buffers of " + std::to_string(off * sizeof(double)) + " bytes could not be allocated").c_str(), e);
        }
    }
    MLH_HIP(ctx, G.state.ensure(sizeof(PgState)));
    MLH_HIP(ctx, G.h_pin.ensure(sizeof(PgState), 0, true));
    if (G.work.cap + G.state.cap + G.h_pin.cap != before) ++G.allocations;
    double *w = G.work.as<double>();
    P.kf = G.kf.as<PgKeyframe>();
    P.x = w + o_x; P.meas = w + o_meas; P.lr = w + o_lr; P.lJi = w + o_Ji; P.lJj = w + o_Jj; P.cost_e = w + o_ce; P.sas_e = w + o_sas; P.Bb = w + o_Bb; P.hd = w + o_hd;
    P.g = w + o_g; P.S = w + o_S; P.diag = w + o_diag; P.gs = w + o_gs; P.gm = w + o_gm; P.Lrow = w + o_Lrow; P.Linv = w + o_Linv; P.Y = w + o_Y; P.Gpart = w + o_G;
    P.C = w + o_C; P.z = w + o_z; P.zw = w + o_zw; P.Dg = w + o_Dg; P.rvec = w + o_rv; P.step = w + o_step; P.red = w + o_red; P.loops = reinterpret_cast<int *>(w + o_loops);
    P.st = G.state.as<PgState>();
    hipStream_t st = ctx->stream;
    if (P.L) MLH_HIP(ctx, hipMemcpyAsync(P.loops, loops.data(), sizeof(int) * loops.size(), hipMemcpyHostToDevice, st));
    if (NB) MLH_HIP(ctx, hipMemsetAsync(P.Lrow, 0, NB * 180 * sizeof(double), st));       // the blocks left of the first column are read as zeros
    return MLH_OK;
}

// mlh_pg_time_stages: an event behind every stage of the launch list; the time between two marks goes to the stage of the later one
enum { PG_T_LINEARIZE = 0, PG_T_ASSEMBLE, PG_T_FACTOR, PG_T_FORWARD, PG_T_GRAM, PG_T_DENSE, PG_T_BACK, PG_T_LM, PG_T_COUNT };
struct PgTimer {
    hipStream_t st = nullptr;
    std::vector<std::pair<int, hipEvent_t>> marks;
    hipError_t err = hipSuccess;
    void mark(int stage)
    {
        hipEvent_t e = nullptr;
        if (err == hipSuccess) err = hipEventCreate(&e);
        if (err == hipSuccess) err = hipEventRecord(e, st);
        if (e) marks.emplace_back(stage, e);
    }
    // ms[stage] += the spans; call once the stream has been waited for
    void collect(double *ms)
    {
        for (size_t i = 1; i < marks.size(); ++i) {
            float t = 0.f;
            if (err == hipSuccess) err = hipEventElapsedTime(&t, marks[i - 1].second, marks[i].second);
            if (err == hipSuccess) ms[marks[i].first] += double(t);
        }
        release();
    }
    void release()
    {
        for (auto &m : marks) (void)hipEventDestroy(m.second);
        marks.clear();
    }
    PgTimer() = default;
    PgTimer(const PgTimer &) = delete;
    PgTimer &operator=(const PgTimer &) = delete;
    ~PgTimer() { release(); }          // (an early return on a failed launch must not leak the events recorded so far)
};
inline void pg_mark(PgTimer *T, int stage) { if (T) T->mark(stage); }

// begin + the linearisation at the stored poses + the state record
int pg_enqueue_begin(mlh_ctx *ctx, const PgDev &P, int max_it, double radius0)
{
    hipStream_t st = ctx->stream;
    MLH_LAUNCH(pg_begin_kernel, dim3(pg_blocks(P.M)), dim3(PG_TPB), 0, st, P);
    MLH_LAUNCH(pg_linearize_kernel, dim3(pg_blocks(size_t(P.M) * PG_SLOTS)), dim3(PG_TPB), 0, st, P, 0);
    MLH_LAUNCH(pg_decide_kernel, dim3(1), dim3(PG_TPB), 0, st, P, int(DECIDE_INIT), max_it, radius0);
    ctx->pg.launches += 3;
    return MLH_OK;
}

// [Y | y_b] = L^-1 [W^T | S g], the Gram image and the dense stage (P.NB > 0): the launches between the band's factorisation and y_b - Y z
int pg_enqueue_reduce(mlh_ctx *ctx, const PgDev &P, PgTimer *T, int keep_factor)
{
    hipStream_t st = ctx->stream;
    PgStore &G = ctx->pg;
    const int nmt = P.ncp / 32;
    MLH_LAUNCH(pg_forward_kernel, dim3((P.ncp + PG_WAVE - 1) / PG_WAVE), dim3(PG_WAVE), 0, st, P);
    pg_mark(T, PG_T_FORWARD);
    MLH_LAUNCH(pg_gram_kernel, dim3(nmt * (nmt + 1) / 2, P.ks), dim3(PG_WAVE), 0, st, P);
    pg_mark(T, PG_T_GRAM);
    G.launches += 2;
    if (P.L <= PG_MAX_LOOPS) {
        MLH_LAUNCH(pg_dense_kernel, dim3(1), dim3(PG_TPB), 0, st, P, keep_factor);
        ++G.launches;
    } else {
        const int ns = pg_dense_launches(P.m);
        for (int s = 0; s < ns; ++s) {
            const PgDenseStep d = pg_dense_step(P.m, s);
            const dim3 grid(unsigned(d.hi - d.lo));
            if (d.kind == PG_STEP_SUM) MLH_LAUNCH(pg_csum_kernel, grid, dim3(PG_TPB), 0, st, P);
            else if (d.kind == PG_STEP_UPDATE) MLH_LAUNCH(pg_cupdate_kernel, grid, dim3(PG_TPB), 0, st, P, d.k);
            else if (d.kind == PG_STEP_PANEL) MLH_LAUNCH(pg_cpanel_kernel, grid, dim3(PG_TPB), 0, st, P, d.k);
            else MLH_LAUNCH(pg_cback_kernel, grid, dim3(PG_TPB), 0, st, P, d.k);
        }
        G.launches += ns;
    }
    pg_mark(T, PG_T_DENSE);
    return MLH_OK;
}

// assemble + the linear solve of one iteration (the launches between the loop's head and the candidate)
int pg_enqueue_solve(mlh_ctx *ctx, const PgDev &P, int loop_head, PgTimer *T = nullptr, int force_fail = 0)
{
    hipStream_t st = ctx->stream;
    PgStore &G = ctx->pg;
    if (P.NB > 0) { MLH_LAUNCH(pg_assemble_kernel, dim3(pg_blocks(size_t(P.NB) * PG_SLOTS)), dim3(PG_TPB), 0, st, P, 0); ++G.launches; }
    pg_mark(T, PG_T_ASSEMBLE);
    MLH_LAUNCH(pg_factor_kernel, dim3(1), dim3(PG_WAVE), 0, st, P, loop_head, force_fail);
    ++G.launches;
    pg_mark(T, PG_T_FACTOR);
    if (P.NB > 0) {
        { const int rc = pg_enqueue_reduce(ctx, P, T, 0); if (rc) return rc; }
        MLH_LAUNCH(pg_yz_kernel, dim3(pg_blocks(P.n)), dim3(PG_TPB), 0, st, P);
        MLH_LAUNCH(pg_back_kernel, dim3(1), dim3(PG_WAVE), 0, st, P);
        pg_mark(T, PG_T_BACK);
        G.launches += 2;
    }
    return MLH_OK;
}

int pg_fetch_state(mlh_ctx *ctx, PgState &out)
{
    PgStore &G = ctx->pg;
    MLH_HIP(ctx, hipMemcpyAsync(G.h_pin.p, G.state.p, sizeof(PgState), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    ++G.host_waits;
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    std::memcpy(&out, G.h_pin.p, sizeof(PgState));
    return MLH_OK;
}

// mlh_pg_optimize, and (stage_ms != nullptr) mlh_pg_time_stages: the same launches without the write-back, an event behind every stage
int optimize_run(mlh_ctx *ctx, const char *entry, int cur_index, const mlh_pg_opts &o, mlh_pg_result *res, double *stage_ms, uint32_t fail_mask = 0u)
{
    PgStore &G = ctx->pg;
    { const int rc = pg_gate(ctx, entry); if (rc) return rc; }
    PgDev P;
    { const int rc = pg_problem(ctx, entry, cur_index, o, P); if (rc) return rc; }
    if (!stage_ms) G.invalidate_marginals();                 // (f18): the poses they were computed at are about to move
    hipStream_t st = ctx->stream;
    PgTimer timer;
    timer.st = st;
    PgTimer *T = stage_ms ? &timer : nullptr;
    pg_mark(T, PG_T_LINEARIZE);
    { const int rc = pg_enqueue_begin(ctx, P, o.max_num_iterations, 1e4); if (rc) return rc; }
    pg_mark(T, PG_T_LINEARIZE);
    for (int it = 0; it < o.max_num_iterations; ++it) {
        { const int rc = pg_enqueue_solve(ctx, P, 1, T, it < 32 && ((fail_mask >> it) & 1u) ? 1 : 0); if (rc) return rc; }
        if (P.NB > 0) {
            MLH_LAUNCH(pg_candidate_kernel, dim3(pg_blocks(P.M)), dim3(PG_TPB), 0, st, P);
            pg_mark(T, PG_T_LM);
            MLH_LAUNCH(pg_linearize_kernel, dim3(pg_blocks(size_t(P.M) * PG_SLOTS)), dim3(PG_TPB), 0, st, P, 1);
            pg_mark(T, PG_T_LINEARIZE);
            MLH_LAUNCH(pg_decide_kernel, dim3(1), dim3(PG_TPB), 0, st, P, int(DECIDE_STEP), o.max_num_iterations, 0.0);
            pg_mark(T, PG_T_LM);
            G.launches += 3;
        }
    }
    if (!stage_ms) {
        MLH_LAUNCH(pg_writeback_kernel, dim3(pg_blocks(size_t(P.count - P.first))), dim3(PG_TPB), 0, st, P);
        ++G.launches;
    }
    MLH_HIP(ctx, hipGetLastError());
    PgState S;
    { const int rc = pg_fetch_state(ctx, S); if (rc) return rc; }
    if (stage_ms) {
        MLH_HIP(ctx, hipStreamSynchronize(st));
        for (int k = 0; k < PG_T_COUNT; ++k) stage_ms[k] = 0.0;
        timer.collect(stage_ms);
        MLH_HIP(ctx, timer.err);
    }
    std::memset(res, 0, sizeof(*res));
    res->num_iterations = S.iteration; res->num_successful_steps = S.n_succ; res->termination = S.termination;
    res->n_keyframes = P.M; res->n_loops = P.L; res->first_index = P.first;
    res->launches = G.launches; res->host_waits = G.host_waits;
    res->initial_cost = S.initial_cost; res->final_cost = S.final_cost; res->final_radius = S.radius; res->solve_radius = S.solve_radius;
    std::memcpy(res->drift, S.drift, sizeof(S.drift));
    if (ctx->prof.mask) prof_collect(ctx);
    return MLH_OK;
}

int linearize_run(mlh_ctx *ctx, int cur_index, const mlh_pg_opts &o, int32_t *n_edges, int32_t *edge_ij, double *residuals, double *Ji, double *Jj, double *cost,
                  double *H, double *g)
{
    PgStore &G = ctx->pg;
    { const int rc = pg_gate(ctx, "mlh_pg_linearize"); if (rc) return rc; }
    PgDev P;
    { const int rc = pg_problem(ctx, "mlh_pg_linearize", cur_index, o, P); if (rc) return rc; }
    if ((H || g) && P.M > PG_DENSE_H_MAX) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_pg_linearize: the dense H, g are handed out for at most 128 keyframes");
    hipStream_t st = ctx->stream;
    { const int rc = pg_enqueue_begin(ctx, P, 0, 1e4); if (rc) return rc; }
    if (P.NB > 0) { MLH_LAUNCH(pg_assemble_kernel, dim3(pg_blocks(size_t(P.NB) * PG_SLOTS)), dim3(PG_TPB), 0, st, P, 1); ++G.launches; }
    MLH_HIP(ctx, hipGetLastError());
    const size_t E = size_t(P.M) * PG_SLOTS, NB = size_t(P.NB);
    std::vector<double> r(E * 6), ji(E * 36), jj(E * 36), bb(NB * 180 + 1), gv(NB * 6 + 1);
    MLH_HIP(ctx, hipMemcpyAsync(r.data(), P.lr, sizeof(double) * r.size(), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipMemcpyAsync(ji.data(), P.lJi, sizeof(double) * ji.size(), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipMemcpyAsync(jj.data(), P.lJj, sizeof(double) * jj.size(), hipMemcpyDeviceToHost, st));
    if (NB) {
        MLH_HIP(ctx, hipMemcpyAsync(bb.data(), P.Bb, sizeof(double) * NB * 180, hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipMemcpyAsync(gv.data(), P.g, sizeof(double) * NB * 6, hipMemcpyDeviceToHost, st));
    }
    PgState S;
    { const int rc = pg_fetch_state(ctx, S); if (rc) return rc; }
    MLH_HIP(ctx, hipStreamSynchronize(st));
    if (cost) *cost = S.cost;
    // the edges in the reference's order: per keyframe its sequential edges to i - 1 .. i - 4, then its loop edge
    int ne = 0;
    const size_t nn = size_t(P.n);
    if (H) std::fill(H, H + nn * nn, 0.0);
    for (int k = 0; k < P.M; ++k)
        for (int s = 0; s < PG_SLOTS; ++s) {
            const int i = s < PG_SEQ ? k - 1 - s : (G.loop_index[size_t(P.first + k)] >= 0 ? G.loop_index[size_t(P.first + k)] - P.first : -1);
            if (i < 0) continue;
            const size_t e = size_t(k) * PG_SLOTS + s;
            if (edge_ij) { edge_ij[2 * ne] = i; edge_ij[2 * ne + 1] = k; }
            if (residuals) std::memcpy(residuals + size_t(ne) * 6, &r[e * 6], sizeof(double) * 6);
            if (Ji) std::memcpy(Ji + size_t(ne) * 36, &ji[e * 36], sizeof(double) * 36);
            if (Jj) std::memcpy(Jj + size_t(ne) * 36, &jj[e * 36], sizeof(double) * 36);
            if (H && s == PG_SEQ) {
                // W^T W of this loop edge: the part of H the device keeps as 6 rows of W
                const double *J[2] = {&ji[e * 36], &jj[e * 36]};
                const int blk[2] = {i - 1, k - 1};
                for (int u = 0; u < 2; ++u)
                    for (int v = 0; v < 2; ++v) {
                        if (blk[u] < 0 || blk[v] < 0) continue;
                        for (int a = 0; a < 6; ++a)
                            for (int c = 0; c < 6; ++c) {
                                double acc = 0.0;
                                for (int q = 0; q < 6; ++q) acc += J[u][q * 6 + a] * J[v][q * 6 + c];
                                H[(size_t(blk[u]) * 6 + a) * nn + size_t(blk[v]) * 6 + c] += acc;
                            }
                    }
            }
            ++ne;
        }
    if (n_edges) *n_edges = ne;
    if (H)
        for (size_t b = 0; b < NB; ++b)
            for (size_t d = 0; d < size_t(PG_SLOTS) && b + d < NB; ++d)
                for (int a = 0; a < 6; ++a)
                    for (int c = 0; c < 6; ++c) {
                        const double v = bb[(b * PG_SLOTS + d) * 36 + a * 6 + c];
                        H[((b + d) * 6 + a) * nn + b * 6 + c] += v;
                        if (d) H[(b * 6 + c) * nn + (b + d) * 6 + a] += v;
                    }
    if (g) std::memcpy(g, gv.data(), sizeof(double) * nn);
    return MLH_OK;
}

int solve_step_run(mlh_ctx *ctx, int cur_index, const mlh_pg_opts &o, double radius, double *step, double *delta, int32_t *ok)
{
    { const int rc = pg_gate(ctx, "mlh_pg_solve_step"); if (rc) return rc; }
    PgDev P;
    { const int rc = pg_problem(ctx, "mlh_pg_solve_step", cur_index, o, P); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    { const int rc = pg_enqueue_begin(ctx, P, 1, radius); if (rc) return rc; }
    { const int rc = pg_enqueue_solve(ctx, P, 0); if (rc) return rc; }
    MLH_HIP(ctx, hipGetLastError());
    const size_t n = size_t(P.n);
    std::vector<double> sv(n + 1), Sv(n + 1);
    if (n) {
        MLH_HIP(ctx, hipMemcpyAsync(sv.data(), P.step, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipMemcpyAsync(Sv.data(), P.S, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    PgState S;
    { const int rc = pg_fetch_state(ctx, S); if (rc) return rc; }
    MLH_HIP(ctx, hipStreamSynchronize(st));
    if (ok) *ok = S.lin_ok;
    for (size_t i = 0; i < n; ++i) {
        if (step) step[i] = sv[i];
        if (delta) delta[i] = sv[i] * Sv[i];
    }
    return MLH_OK;
}

#include "pgcov.inc"

}  // namespace

}  // namespace mlh

using namespace mlh;

extern "C" {

void mlh_pg_opts_default(mlh_pg_opts *o)
{
    if (o) pg_opts_defaults(*o);
}

int mlh_pg_reset(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    PgStore &G = ctx->pg;
    G.count = 0; G.earliest_loop = -1; G.loop_index.clear();
    G.invalidate_marginals();
    return MLH_OK;
}

int mlh_pg_reserve(mlh_ctx *ctx, int32_t max_loops)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (max_loops < PG_MAX_LOOPS || max_loops > MLH_PG_LOOPS_LIMIT)
        return fail(ctx, MLH_ERR_INVALID, ("mlh_pg_reserve: max_loops must lie in " + std::to_string(PG_MAX_LOOPS) + " .. " + std::to_string(int(MLH_PG_LOOPS_LIMIT))).c_str());
    ctx->pg.max_loops = max_loops;
    return MLH_OK;
}

int mlh_pg_info(mlh_ctx *ctx, mlh_pg_info_t *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_info: null output");
    const PgStore &G = ctx->pg;
    std::memset(out, 0, sizeof(*out));
    out->n_keyframes = G.count;
    for (int v : G.loop_index) out->n_loops += v >= 0;
    out->earliest_loop_index = G.earliest_loop;
    out->max_loops = G.max_loops;
    out->allocations = G.allocations;
    out->bytes_hbm = int64_t(G.kf.cap + G.work.cap + G.state.cap + G.marg_out.cap + G.marg_work.cap);
    return MLH_OK;
}

int mlh_pg_add_keyframe(mlh_ctx *ctx, const double *pose, int32_t *index_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!pose) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_add_keyframe: null pose");
    for (int c = 0; c < 7; ++c)
        if (!std::isfinite(pose[c])) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_add_keyframe: non-finite pose");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    PgStore &G = ctx->pg;
    const size_t before = G.kf.cap;
    MLH_HIP(ctx, G.kf.grow(sizeof(PgKeyframe) * (size_t(G.count) + 1), sizeof(PgKeyframe) * size_t(G.count), ctx->stream));
    if (G.kf.cap != before) ++G.allocations;
    PgKeyframe K;
    std::memset(&K, 0, sizeof(K));
    std::memcpy(K.pose, pose, sizeof(K.pose));
    K.last[6] = 1.0; K.loop_rel[6] = 1.0;          // Pose(): identity
    K.loop_index = -1;
    MLH_HIP(ctx, hipMemcpyAsync(G.kf.as<PgKeyframe>() + G.count, &K, sizeof(K), hipMemcpyHostToDevice, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (index_out) *index_out = G.count;
    G.loop_index.push_back(-1);
    ++G.count;
    return MLH_OK;
}

int mlh_pg_set_loop(mlh_ctx *ctx, int32_t index, int32_t loop_index, const double *rel_pose)
{
    if (!ctx) return MLH_ERR_INVALID;
    PgStore &G = ctx->pg;
    if (!rel_pose || index < 0 || index >= G.count || loop_index < 0 || loop_index >= index)
        return fail(ctx, MLH_ERR_INVALID, "mlh_pg_set_loop: needs 0 <= loop_index < index < the number of keyframes and a relative pose");
    for (int c = 0; c < 7; ++c)
        if (!std::isfinite(rel_pose[c])) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_set_loop: non-finite relative pose");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    struct { double rel[7]; int loop_index, pad; } rec;
    std::memcpy(rec.rel, rel_pose, sizeof(rec.rel));
    rec.loop_index = loop_index; rec.pad = 0;
    static_assert(sizeof(rec) == sizeof(PgKeyframe) - offsetof(PgKeyframe, loop_rel), "loop_rel and loop_index are the record's tail");
    MLH_HIP(ctx, hipMemcpyAsync(reinterpret_cast<char *>(G.kf.as<PgKeyframe>() + index) + offsetof(PgKeyframe, loop_rel), &rec, sizeof(rec), hipMemcpyHostToDevice, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    G.loop_index[size_t(index)] = loop_index;
    G.invalidate_marginals();
    if (G.earliest_loop > loop_index || G.earliest_loop == -1) G.earliest_loop = loop_index;      // pose_graph.cpp:141-142
    return MLH_OK;
}

int mlh_pg_optimize(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, mlh_pg_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!result) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_optimize: null result");
    mlh_pg_opts o;
    { const int rc = pg_opts_take(ctx, "mlh_pg_optimize", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return optimize_run(ctx, "mlh_pg_optimize", cur_index, o, result, nullptr);
}

int mlh_pg_optimize_forced(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, uint32_t fail_mask, mlh_pg_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!result) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_optimize_forced: null result");
    mlh_pg_opts o;
    { const int rc = pg_opts_take(ctx, "mlh_pg_optimize_forced", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return optimize_run(ctx, "mlh_pg_optimize_forced", cur_index, o, result, nullptr, fail_mask);
}

int mlh_pg_time_stages(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, mlh_pg_result *result, double *stage_ms)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!result || !stage_ms) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_time_stages: null output");
    mlh_pg_opts o;
    { const int rc = pg_opts_take(ctx, "mlh_pg_time_stages", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return optimize_run(ctx, "mlh_pg_time_stages", cur_index, o, result, stage_ms);
}

int mlh_pg_poses(mlh_ctx *ctx, int32_t first, int32_t n, double *poses, double *last_poses)
{
    if (!ctx) return MLH_ERR_INVALID;
    PgStore &G = ctx->pg;
    if (first < 0 || n < 0 || first + n > G.count || (n > 0 && !poses)) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_poses: bad range or null output");
    if (n == 0) return MLH_OK;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<PgKeyframe> rec;
    rec.resize(size_t(n));
    MLH_HIP(ctx, hipMemcpyAsync(rec.data(), G.kf.as<PgKeyframe>() + first, sizeof(PgKeyframe) * size_t(n), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < size_t(n); ++i) {
        std::memcpy(poses + 7 * i, rec[i].pose, sizeof(double) * 7);
        if (last_poses) std::memcpy(last_poses + 7 * i, rec[i].last, sizeof(double) * 7);
    }
    return MLH_OK;
}

int mlh_pg_device_poses(mlh_ctx *ctx, const void **records, int32_t *stride_bytes, int32_t *count)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!records) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_device_poses: null output");
    *records = ctx->pg.count ? ctx->pg.kf.p : nullptr;
    if (stride_bytes) *stride_bytes = int32_t(sizeof(PgKeyframe));
    if (count) *count = ctx->pg.count;
    return MLH_OK;
}

int mlh_pg_linearize(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, int32_t *n_edges, int32_t *edge_ij, double *residuals, double *Ji, double *Jj,
                     double *cost, double *H, double *g)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_pg_opts o;
    { const int rc = pg_opts_take(ctx, "mlh_pg_linearize", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return linearize_run(ctx, cur_index, o, n_edges, edge_ij, residuals, Ji, Jj, cost, H, g);
}

int mlh_pg_solve_step(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, double radius, double *step, double *delta, int32_t *ok)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_pg_opts o;
    { const int rc = pg_opts_take(ctx, "mlh_pg_solve_step", opts, o); if (rc) return rc; }
    if (!std::isfinite(radius) || !(radius > 0.0)) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_solve_step: the radius must be finite and > 0");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return solve_step_run(ctx, cur_index, o, radius, step, delta, ok);
}

int mlh_pg_marginals(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, int32_t form, double *covs, mlh_pg_marginals_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!result) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_marginals: null result");
    if (form != MLH_PG_COV_LOCAL && form != MLH_PG_COV_STORE) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_marginals: form must be MLH_PG_COV_LOCAL or MLH_PG_COV_STORE");
    mlh_pg_opts o;
    { const int rc = pg_opts_take(ctx, "mlh_pg_marginals", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return marginals_run(ctx, cur_index, o, form, covs, result);
}

int mlh_pg_device_marginals(mlh_ctx *ctx, const double **cov_local, const double **cov_store, int32_t *first_index, int32_t *n_keyframes)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!cov_local || !cov_store) return fail(ctx, MLH_ERR_INVALID, "mlh_pg_device_marginals: null output");
    const PgStore &G = ctx->pg;
    const int M = G.marg_valid ? G.marg_cur - G.marg_first + 1 : 0;
    *cov_local = M ? G.marg_out.as<double>() : nullptr;
    *cov_store = M ? G.marg_out.as<double>() + size_t(36) * size_t(M) : nullptr;
    if (first_index) *first_index = M ? G.marg_first : -1;
    if (n_keyframes) *n_keyframes = M;
    return MLH_OK;
}

}  // extern "C"
