// The initial extrinsic calibration on the device (include/mloam_hip.h section (f16); estimator/src/initial/initial_extrinsics.cpp:79-309 as estimator.cpp:437-467
// drives it). State in HBM: Q_ (n_lidar x 1200 x 4 f64), v_pose_ (300 x n_lidar x 7 f64), one IeRecord per LiDAR; the bookkeeping (heap, pose_laser_add_, cov
// states) is initext_host.hpp's IeBook on the host.
//   initext_store_kernel   one accepted pose set, a kernel argument, into its slot of v_pose_ (mlh_initext_add_pose: no copy, no wait)
//   initext_solve_kernel   one workgroup of 256 per listed LiDAR, one launch for all of them:
//     rotation     the new 4 x 4 block (a kernel argument) into Q_; each thread takes its rows (<= 5) of the 1200 x 4 matrix into registers; one-sided Jacobi
//                  (svd_dev.hpp), the three sums of a column pair reduced per wavefront by a __shfl_xor butterfly and the four wavefront results combined in
//                  wavefront order, so every lane holds the same bits, takes the same decisions and keeps the same V; the null vector under the sign rule; the
//                  decision rot_cov(1) > rot_cov_thre_
//     translation  (asked for, and the rotation of this launch converged or no rotation was asked for) the rows of A | b (3N x 3) or G | w (2N x 4) built from
//                  the stored sets, the same Jacobi, x = V Sigma^+ U^T b with U^T b = (a_j . b) / sigma_j and Eigen's rank rule, then Pose(q_zyx, x) or the planar tail
//   No float atomics, fixed summation order: two runs give the same bits. Per calibration: one launch, one device-to-pinned copy of the records, one host wait.
#include "ctx.hpp"
#include "initext_host.hpp"
#include "wg_dev.hpp"

namespace mlh {

namespace {

constexpr int IE_TPB = 256;
constexpr int IE_WAVES = IE_TPB / 64;

struct IeSetArg { double p[IE_MAX_LIDAR * 7]; };

struct IeSolveArgs {
    double *Q;                   // n_lidar x IE_Q_ROWS x 4
    const double *sets;          // IE_N_POSE x n_lidar x 7
    IeRecord *rec;               // n_lidar
    int n_lidar, idx_ref, planar, n_sets;
    int slot, do_rot, do_trans;
    double thre;
    int lidar[IE_MAX_LIDAR];
    double block[IE_MAX_LIDAR][16];
};

// all rows' sums to every thread, the same bits everywhere: butterfly per wavefront, the wavefronts' results added in wavefront order. Two buffers used in turn, so
// that one barrier per sum is enough (a buffer is written again only behind the barrier of the sum in between, which every reader of its old values has reached).
struct IeBlockRed {
    double (*s_w)[IE_WAVES][4];
    int turn;
    template <int N> __device__ __forceinline__ void sum(double (&v)[N])
    {
        static_assert(N <= 4, "at most four sums at a time");
        wave_sum(v);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < N; ++i) s_w[turn][wave][i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = ((s_w[turn][0][i] + s_w[turn][1][i]) + s_w[turn][2][i]) + s_w[turn][3][i];
        turn ^= 1;
    }
};

__global__ __launch_bounds__(64) void initext_store_kernel(double *sets, int slot, int n_lidar, IeSetArg S)
{
    const int k = threadIdx.x;
    if (k < 7 * n_lidar) sets[size_t(slot) * n_lidar * 7 + k] = S.p[k];
}

// the translation system of NC columns with ROWS_PER_SET rows per stored set; every thread returns the same x and sigma
template <int NC, int RPS, int RPT>
__device__ __forceinline__ void ie_translation_solve(const double *sets, int n_sets, int n_lidar, int idx_ref, int lidar, const double q[4], IeBlockRed &red, double *sigma,
                                                     double *x, int *rank, int *sweeps)
{
    static_assert(RPT * IE_TPB >= RPS * IE_N_POSE, "every row has a thread");
    SvdRegRows<NC, RPT> rows;
    double b[RPT];
    const int n_rows = RPS * n_sets;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int r = int(threadIdx.x) + IE_TPB * j;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        b[j] = 0.0;
        if (r < n_rows) {
            const int set = r / RPS, comp = r % RPS;
            const double *pr = sets + size_t(set * n_lidar + idx_ref) * 7, *pd = sets + size_t(set * n_lidar + lidar) * 7;
            if (NC == 3) ie_row_nonplanar(pr, pd, q, comp, a, &b[j]);
            else ie_row_planar(pr, pd, q, comp, a, &b[j]);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) rows.at(j, c) = a[c];
    }
    double V[NC * NC];
    int perm[NC];
    *sweeps = svd_onesided_jacobi<NC>(rows, red, IE_SVD_TOL, sigma, V, perm);
    double dots[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) dots[c] = 0.0;
#pragma unroll
    for (int j = 0; j < RPT; ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) dots[c] += rows.at(j, c) * b[j];
    red.template sum<NC>(dots);
    double utb[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        double d = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) d = (perm[j] == c) ? dots[c] : d;
        utb[j] = d;
    }
    *rank = svd_solve<NC>(sigma, V, utb, x);
}

__global__ __launch_bounds__(IE_TPB) void initext_solve_kernel(IeSolveArgs G)
{
    __shared__ double s_w[2][IE_WAVES][4];
    __shared__ double s_blk[16];
    IeBlockRed red{s_w, 0};
    const int k = threadIdx.x;
    // this workgroup's entry of the argument's lists, picked by comparison: a run-time index would make the compiler copy the whole argument to scratch
    int lidar = 0;
    double blk_k = 0.0;
#pragma unroll
    for (int i = 0; i < IE_MAX_LIDAR; ++i) {
        const bool mine = int(blockIdx.x) == i;
        lidar = mine ? G.lidar[i] : lidar;
#pragma unroll
        for (int e = 0; e < 16; ++e) blk_k = (mine && k == e) ? G.block[i][e] : blk_k;
    }
    double *Q = G.Q + size_t(lidar) * IE_Q_ROWS * 4;
    IeRecord *R = G.rec + lidar;
    // calib_ext_'s rotation before this call (read by every thread before thread 0 writes the record at the very end)
    double q_xyzw[4] = {R->q[0], R->q[1], R->q[2], R->q[3]};
    double rot_sv[4] = {R->rot_sv[0], R->rot_sv[1], R->rot_sv[2], R->rot_sv[3]};
    int rot_ran = 0, converged = 0, rot_sweeps = 0;
    if (G.do_rot) {
        if (k < 16) { Q[size_t(G.slot) * 16 + k] = blk_k; s_blk[k] = blk_k; }
        __syncthreads();
        SvdRegRows<4, 5> rows;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int r = k + IE_TPB * j;
            const bool in_new = (r >> 2) == G.slot;          // (the block just stored is taken from the argument, not read back)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double v = 0.0;
                if (r < IE_Q_ROWS) v = in_new ? s_blk[4 * (r & 3) + c] : Q[size_t(r) * 4 + c];
                rows.at(j, c) = v;
            }
        }
        double V[16];
        int perm[4];
        rot_sweeps = svd_onesided_jacobi<4>(rows, red, IE_SVD_TOL, rot_sv, V, perm);
        ie_null_vector(V, q_xyzw);
        rot_ran = 1;
        converged = rot_sv[2] > G.thre ? 1 : 0;            // cpp:198-201: the second-smallest singular value
    }
    double t[3] = {R->t[0], R->t[1], R->t[2]};
    double trans_sv[4] = {0.0, 0.0, 0.0, 0.0};
    int solved = 0, rank = 0, trans_sweeps = 0;
    if (G.do_trans && (!G.do_rot || converged)) {
        const double q[4] = {q_xyzw[3], q_xyzw[0], q_xyzw[1], q_xyzw[2]};
        double pose[7];
        if (!G.planar) {
            double x[3];
            ie_translation_solve<3, 3, 4>(G.sets, G.n_sets, G.n_lidar, G.idx_ref, lidar, q, red, trans_sv, x, &rank, &trans_sweeps);
            ie_tail_nonplanar(q, x, pose);
        } else {
            double m[4];
            ie_translation_solve<4, 2, 3>(G.sets, G.n_sets, G.n_lidar, G.idx_ref, lidar, q, red, trans_sv, m, &rank, &trans_sweeps);
            ie_tail_planar(q, m, pose);
        }
        q_xyzw[0] = pose[3]; q_xyzw[1] = pose[4]; q_xyzw[2] = pose[5]; q_xyzw[3] = pose[6];
        t[0] = pose[0]; t[1] = pose[1]; t[2] = pose[2];
        solved = 1;
    }
    __syncthreads();          // (every thread has read the old record)
    if (k == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { R->q[c] = q_xyzw[c]; R->rot_sv[c] = rot_sv[c]; R->trans_sv[c] = trans_sv[c]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) R->t[c] = t[c];
        R->rot_ran = rot_ran; R->rot_converged = converged; R->trans_solved = solved; R->trans_rank = rank; R->rot_sweeps = rot_sweeps; R->trans_sweeps = trans_sweeps;
    }
}

int ie_book(mlh_ctx *ctx, const char *entry, IeBook **B)
{
    if (!ctx->ie.book) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": mlh_initext_reset has not been called").c_str());
    if (ctx->solves.pending()) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": a solve submitted with mlh_*_begin has not been collected").c_str());
    *B = ctx->ie.book.get();
    return MLH_OK;
}

void ie_records_from_book(const IeBook &B, IeRecord *rec)
{
    std::memset(rec, 0, sizeof(IeRecord) * size_t(B.opts.n_lidar));
    for (int l = 0; l < B.opts.n_lidar; ++l) {
        const double *p = B.calib_ext + 7 * l;
        rec[l].q[0] = p[3]; rec[l].q[1] = p[4]; rec[l].q[2] = p[5]; rec[l].q[3] = p[6];
        rec[l].t[0] = p[0]; rec[l].t[1] = p[1]; rec[l].t[2] = p[2];
    }
}

}  // namespace

}  // namespace mlh

using namespace mlh;

extern "C" {

void mlh_initext_opts_default(mlh_initext_opts *o)
{
    if (o) ie_opts_defaults(*o);
}

int mlh_initext_reset(mlh_ctx *ctx, const mlh_initext_opts *opts)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_initext_opts o;
    if (opts) o = *opts; else ie_opts_defaults(o);
    if (const char *f = ie_opts_fault(o)) return fail(ctx, MLH_ERR_INVALID, (std::string("mlh_initext_reset: bad option ") + f).c_str());
    if (ctx->solves.pending()) return fail(ctx, MLH_ERR_STATE, "mlh_initext_reset: a solve submitted with mlh_*_begin has not been collected");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    InitExtStore &S = ctx->ie;
    const size_t nl = size_t(o.n_lidar), q_bytes = nl * IE_Q_ROWS * 4 * sizeof(double), set_bytes = size_t(IE_N_POSE) * nl * 7 * sizeof(double);
    MLH_HIP(ctx, ensure_counted(S.Q, q_bytes, S.allocations));
    MLH_HIP(ctx, ensure_counted(S.sets, set_bytes, S.allocations));
    MLH_HIP(ctx, ensure_counted(S.rec, sizeof(IeRecord) * IE_MAX_LIDAR, S.allocations));
    if (S.h_rec.cap < sizeof(IeRecord) * IE_MAX_LIDAR) ++S.allocations;
    MLH_HIP(ctx, S.h_rec.ensure(sizeof(IeRecord) * IE_MAX_LIDAR, 0, true));
    if (!S.book) S.book = std::make_shared<IeBook>();
    S.book->reset(o);
    hipStream_t st = ctx->stream;
    MLH_HIP(ctx, hipMemsetAsync(S.Q.p, 0, q_bytes, st));
    MLH_HIP(ctx, hipMemsetAsync(S.sets.p, 0, set_bytes, st));
    ie_records_from_book(*S.book, S.h_rec.as<IeRecord>());
    MLH_HIP(ctx, hipMemcpyAsync(S.rec.p, S.h_rec.p, sizeof(IeRecord) * nl, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipStreamSynchronize(st));
    S.launches = 0; S.host_waits = 0;
    return MLH_OK;
}

int mlh_initext_add_pose(mlh_ctx *ctx, const double *poses, int32_t *accepted)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!poses || !accepted) return fail(ctx, MLH_ERR_INVALID, "mlh_initext_add_pose: null argument");
    IeBook *B = nullptr;
    { const int rc = ie_book(ctx, "mlh_initext_add_pose", &B); if (rc) return rc; }
    for (int c = 0; c < 7 * B->opts.n_lidar; ++c)
        if (!std::isfinite(poses[c])) return fail(ctx, MLH_ERR_INVALID, "mlh_initext_add_pose: non-finite pose");
    InitExtStore &S = ctx->ie;
    S.launches = 0; S.host_waits = 0;
    if (!B->screw_ok(poses)) { *accepted = 0; return MLH_OK; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    // (the launch is prepared before the bookkeeping moves, so that a failure leaves the heap as it was)
    const bool fill = B->pq.size() < size_t(B->opts.n_pose);
    const size_t slot = fill ? B->pq.size() : B->pq.top().first;
    if (slot >= size_t(IE_N_POSE)) return fail(ctx, MLH_ERR_STATE, "mlh_initext_add_pose: slot out of range");
    IeSetArg A;
    std::memset(&A, 0, sizeof(A));
    std::memcpy(A.p, poses, sizeof(double) * 7 * size_t(B->opts.n_lidar));
    MLH_LAUNCH(initext_store_kernel, dim3(1), dim3(64), 0, ctx->stream, S.sets.as<double>(), int(slot), B->opts.n_lidar, A);
    MLH_HIP(ctx, hipGetLastError());
    ++S.launches;
    B->accept(poses);
    *accepted = 1;
    return MLH_OK;
}

int mlh_initext_calibrate(mlh_ctx *ctx, const int32_t *lidars, int32_t n, int32_t stages, mlh_initext_result *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!lidars || !out) return fail(ctx, MLH_ERR_INVALID, "mlh_initext_calibrate: null argument");
    IeBook *B = nullptr;
    { const int rc = ie_book(ctx, "mlh_initext_calibrate", &B); if (rc) return rc; }
    if (n < 1 || n > B->opts.n_lidar) return fail(ctx, MLH_ERR_INVALID, "mlh_initext_calibrate: needs 1 <= n <= n_lidar LiDARs");
    if (stages < 1 || stages > (MLH_INITEXT_ROT | MLH_INITEXT_TRANS)) return fail(ctx, MLH_ERR_INVALID, "mlh_initext_calibrate: stages is MLH_INITEXT_ROT, MLH_INITEXT_TRANS or both");
    unsigned seen = 0;
    for (int i = 0; i < n; ++i) {
        const int l = lidars[i];
        if (l < 0 || l >= B->opts.n_lidar || l == B->opts.idx_ref || ((seen >> l) & 1u))
            return fail(ctx, MLH_ERR_INVALID, "mlh_initext_calibrate: a listed LiDAR is out of range, the reference LiDAR, or listed twice");
        seen |= 1u << l;
    }
    InitExtStore &S = ctx->ie;
    S.launches = 0; S.host_waits = 0;
    const bool want_rot = (stages & MLH_INITEXT_ROT) != 0, want_trans = (stages & MLH_INITEXT_TRANS) != 0;
    const bool do_rot = want_rot && B->window_full() && B->add_first >= 0;         // cpp:125
    const bool launch = do_rot || (want_trans && !want_rot);
    IeSolveArgs A;
    std::memset(&A, 0, sizeof(A));
    if (launch) {
        MLH_HIP(ctx, hipSetDevice(ctx->device));
        A.Q = S.Q.as<double>(); A.sets = S.sets.as<double>(); A.rec = S.rec.as<IeRecord>();
        A.n_lidar = B->opts.n_lidar; A.idx_ref = B->opts.idx_ref; A.planar = B->opts.planar_movement ? 1 : 0; A.n_sets = int(B->n_sets);
        A.slot = do_rot ? int(B->add_first) : -1; A.do_rot = do_rot ? 1 : 0; A.do_trans = want_trans ? 1 : 0;
        A.thre = B->rot_cov_thre;
        for (int i = 0; i < n; ++i) {
            A.lidar[i] = lidars[i];
            if (do_rot) ie_rot_block(B->add_poses + 7 * B->opts.idx_ref, B->add_poses + 7 * lidars[i], B->calib_ext + 7 * lidars[i], A.block[i]);
        }
        hipStream_t st = ctx->stream;
        MLH_LAUNCH(initext_solve_kernel, dim3(unsigned(n)), dim3(IE_TPB), 0, st, A);
        MLH_HIP(ctx, hipGetLastError());
        ++S.launches;
        MLH_HIP(ctx, hipMemcpyAsync(S.h_rec.p, S.rec.p, sizeof(IeRecord) * size_t(B->opts.n_lidar), hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, stream_wait_spin(ctx));
        ++S.host_waits;
        { const int rc = device_error_check(ctx); if (rc) return rc; }
    }
    const IeRecord *rec = S.h_rec.as<IeRecord>();
    for (int i = 0; i < n; ++i) {
        const int l = lidars[i];
        mlh_initext_result &r = out[i];
        std::memset(&r, 0, sizeof(r));
        r.lidar = l; r.slot = -1;
        double *ext = B->calib_ext + 7 * l;
        if (launch) {
            const IeRecord &d = rec[l];
            ext[0] = d.t[0]; ext[1] = d.t[1]; ext[2] = d.t[2]; ext[3] = d.q[0]; ext[4] = d.q[1]; ext[5] = d.q[2]; ext[6] = d.q[3];
            std::memcpy(r.rot_sv, d.rot_sv, sizeof(r.rot_sv));
            std::memcpy(r.trans_sv, d.trans_sv, sizeof(r.trans_sv));
            r.rot_ran = d.rot_ran; r.rot_converged = d.rot_converged; r.trans_solved = d.trans_solved; r.trans_rank = d.trans_rank;
            r.rot_sweeps = d.rot_sweeps; r.trans_sweeps = d.trans_sweeps;
            if (d.rot_ran) r.slot = A.slot;
            if (d.rot_converged) B->set_cov_rotation(l);
            if (d.trans_solved) B->set_cov_translation(l);
        }
        r.q[0] = ext[3]; r.q[1] = ext[4]; r.q[2] = ext[5]; r.q[3] = ext[6];
        r.t[0] = ext[0]; r.t[1] = ext[1]; r.t[2] = ext[2];
    }
    if (ctx->prof.mask) prof_collect(ctx);
    return MLH_OK;
}

int mlh_initext_info(mlh_ctx *ctx, mlh_initext_info_t *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_initext_info: null output");
    const InitExtStore &S = ctx->ie;
    std::memset(out, 0, sizeof(*out));
    out->last_slot = -1;
    out->allocations = S.allocations;
    out->bytes_hbm = int64_t(S.Q.cap + S.sets.cap + S.rec.cap);
    out->launches = S.launches; out->host_waits = S.host_waits;
    if (!S.book) return MLH_OK;
    const IeBook &B = *S.book;
    out->configured = 1; out->n_lidar = B.opts.n_lidar;
    out->n_sets = int32_t(B.n_sets); out->heap_size = int32_t(B.pq.size()); out->last_slot = int32_t(B.add_first);
    for (int l = 0; l < B.opts.n_lidar; ++l) { out->cov_rot_mask |= int32_t(B.cov_rot[l]) << l; out->cov_pos_mask |= int32_t(B.cov_pos[l]) << l; }
    out->full_cov_rot = B.full_cov_rot; out->full_cov_pos = B.full_cov_pos;
    out->rot_cov_thre = B.rot_cov_thre;
    return MLH_OK;
}

int mlh_initext_read_state(mlh_ctx *ctx, double *Q, double *sets, double *calib_ext)
{
    if (!ctx) return MLH_ERR_INVALID;
    IeBook *B = nullptr;
    { const int rc = ie_book(ctx, "mlh_initext_read_state", &B); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const InitExtStore &S = ctx->ie;
    const size_t nl = size_t(B->opts.n_lidar);
    if (Q) MLH_HIP(ctx, hipMemcpyAsync(Q, S.Q.p, nl * IE_Q_ROWS * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sets) MLH_HIP(ctx, hipMemcpyAsync(sets, S.sets.p, size_t(IE_N_POSE) * nl * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (calib_ext) std::memcpy(calib_ext, B->calib_ext, sizeof(double) * 7 * nl);
    return MLH_OK;
}

}  // extern "C"
