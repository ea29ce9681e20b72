// The host side of the solvers: staging of the feature sets, the pose's way in and out of the solver state, and the launch schedules of the Gauss-Newton solves
// and of scan2MapOptimization (the kernels: match.hip, solver.hip, select.hip). Host logic only, apart from the one-wavefront kernels that carry a pose.
#include "ctx.hpp"
#include "solve_host.hpp"
#include "dev_math.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <random>

namespace mlh {

int ensure_state(mlh_ctx *ctx, int n_stats)
{
    if (!ctx->state.p) {
        MLH_HIP(ctx, ctx->state.ensure(sizeof(SolverState)));
        MLH_HIP(ctx, hipMemsetAsync(ctx->state.p, 0, sizeof(SolverState), ctx->stream));
    }
    if (n_stats > 0) MLH_HIP(ctx, ctx->stats.ensure(sizeof(IterStatDev) * size_t(n_stats)));
    return MLH_OK;
}

// ---- host <-> device hand-over of the pose without copy engines or blocking waits
// In: the pose travels in the kernel-argument segment of a one-wavefront launch that also resets the solver state (no staging
// buffer, no hipMemcpyAsync set-up latency, nothing for the host to wait on). Out: a one-wavefront launch writes the pose(s) into
// pinned host memory and then stores a sequence number with system-scope release; the host spins on that word (acquire) --
// microseconds instead of the tens of microseconds an interrupt-driven hipStreamSynchronize wake-up costs per frame.
struct PoseArg { double p[7]; };
static void pose_copy(double dst[7], const double src[7]) { for (int i = 0; i < 7; ++i) dst[i] = src[i]; }
__global__ void init_state_kernel(SolverState *S, PoseArg pose)
{
    double *w = reinterpret_cast<double *>(S);
    for (int i = threadIdx.x; i < int(sizeof(SolverState) / sizeof(double)); i += blockDim.x) w[i] = 0.0;
    __syncthreads();
    if (threadIdx.x < 7) { S->x[threadIdx.x] = pose.p[threadIdx.x]; S->cand[threadIdx.x] = pose.p[threadIdx.x]; }
    if (threadIdx.x < 6) S->V[threadIdx.x * 7] = 1.0;
}

// The pose the mapper starts frame k+1 from, computed where frame k's result lives (dev_math.hpp: chain_start_pose). One lane; the solve enqueued behind it reads S->x.
__global__ void chain_pose_kernel(SolverState *S, PoseArg wodom_prev, PoseArg wodom_cur, HostPublish *start_out)
{
    if (threadIdx.x != 0) return;
    double xc[7], out[7];
    for (int i = 0; i < 7; ++i) xc[i] = S->x[i];
    chain_start_pose(xc, wodom_prev.p, wodom_cur.p, out);
    for (int i = 0; i < 7; ++i) { S->x[i] = out[i]; S->cand[i] = out[i]; }
    if (start_out) for (int i = 0; i < 7; ++i) start_out->xb[1][i] = out[i];      // the frame's start pose, for a host that may have to solve the frame again
}

__global__ void set_block_pose_kernel(SolverState *S, int b, PoseArg pose)
{
    if (threadIdx.x < 7) S->xb[b][threadIdx.x] = pose.p[threadIdx.x];
}

__global__ void publish_kernel(const SolverState *S, HostPublish *h, unsigned long long seq)
{
    if (threadIdx.x < 7) h->x[threadIdx.x] = S->x[threadIdx.x];
    if (threadIdx.x < 56) h->xb[threadIdx.x / 7][threadIdx.x % 7] = S->xb[threadIdx.x / 7][threadIdx.x % 7];
    if (threadIdx.x == 63) h->done = S->done;
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&h->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int upload_pose(mlh_ctx *ctx, const double pose[7])
{
    static_assert(sizeof(SolverState) % sizeof(double) == 0, "SolverState is cleared in doubles");
    // a solve submitted with mlh_gn_solve_begin* may have left its last iteration as tile records and its pose in SolverState::xi[slot]: this launch zeroes the whole
    // state, so that solve has to be completed (and published to ITS host record) before, not by the match launch that follows
    { const int frc = gn_flush_pending(ctx); if (frc) return frc; }
    PoseArg a;
    pose_copy(a.p, pose);
    MLH_LAUNCH(init_state_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->state.as<SolverState>(), a);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

static int upload_block_pose(mlh_ctx *ctx, int b, const double pose[7])
{
    PoseArg a;
    pose_copy(a.p, pose);
    MLH_LAUNCH(set_block_pose_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->state.as<SolverState>(), b, a);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// The chained start pose, made on the device from the pose the previous solve left there; start_out (may be null): see chain_pose_kernel
static int enqueue_chain_pose(mlh_ctx *ctx, const double *wodom_prev, const double *wodom_cur, HostPublish *start_out)
{
    PoseArg pa, pb;
    pose_copy(pa.p, wodom_prev); pose_copy(pb.p, wodom_cur);
    MLH_LAUNCH(chain_pose_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->state.as<SolverState>(), pa, pb, start_out);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// What a solver entry point begins with: the last iteration a solve submitted with mlh_gn_solve_begin* may have left as records, and the state (+ n_stats records)
int solver_begin(mlh_ctx *ctx, int n_stats)
{
    const int rc = gn_flush_pending(ctx);
    return rc ? rc : ensure_state(ctx, n_stats);
}

__global__ void stream_flag_kernel(unsigned long long *h, unsigned long long seq)
{
    if (threadIdx.x == 0) __hip_atomic_store(h, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t stream_flag_post(mlh_ctx *ctx, unsigned long long *seq_out)
{
    const hipError_t e = ctx->h_sync.ensure(64, 0, true);
    if (e != hipSuccess) return e;
    const unsigned long long seq = ++ctx->sync_seq;
    MLH_LAUNCH(stream_flag_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->h_sync.as<unsigned long long>(), seq);
    *seq_out = seq;
    return hipGetLastError();
}

// the word only grows (one stream, launches in order): anything at or past `seq` means the work enqueued before that post is done
hipError_t stream_flag_wait(mlh_ctx *ctx, unsigned long long seq)
{
    const unsigned long long *word = ctx->h_sync.as<unsigned long long>();
    return host_spin([=] { return __atomic_load_n(word, __ATOMIC_ACQUIRE) >= seq; }) ? hipSuccess : hipStreamSynchronize(ctx->stream);
}

hipError_t stream_wait_spin(mlh_ctx *ctx)
{
    unsigned long long seq = 0;
    hipError_t e = stream_flag_post(ctx, &seq);
    if (e != hipSuccess) { (void)hipGetLastError(); return hipStreamSynchronize(ctx->stream); }
    return stream_flag_wait(ctx, seq);
}

// the pinned record and the next sequence number (allocated on first use)
// Three pinned records. Record 0 is everybody's; records 1 and 2 belong to scan2map's LM driver, which has one publication being read and the next chunk's
// already enqueued -- and may return with that one still to arrive: it must not land in a record some later call (a map staging on the other stream, say)
// is polling. which < 0: record 0; otherwise record 1 + (which & 1).
int publish_slot(mlh_ctx *ctx, HostPublish **h, unsigned long long *seq, int which)
{
    MLH_HIP(ctx, ctx->h_state.ensure(3 * sizeof(HostPublish), 0, true));
    *h = ctx->h_state.as<HostPublish>() + (which < 0 ? 0 : 1 + (which & 1));
    *seq = ++ctx->publish_seq;
    return MLH_OK;
}

// spin until the device has stored `seq`; every kernel enqueued before the publishing one has completed when this returns
int wait_published(mlh_ctx *ctx, unsigned long long seq, HostPublish &out, void *record)
{
    HostPublish *h = static_cast<HostPublish *>(record ? record : ctx->h_state.p);
    { const int rc = host_wait_seq(ctx, &h->seq, seq, ctx->stream, "pose publication did not arrive"); if (rc) return rc; }
    out = *h;
    // several ranks joined by the mailbox communicator: the launches behind this publication exchanged records with the peers inside their finish. A peer that
    // never arrived leaves the error word set (p2p_dev.hpp): no solve entry point returns a pose built on partial sums as if it were the job's
    if (ctx->p2p.active) return device_error_check(ctx);
    return MLH_OK;
}

// enqueue a stand-alone publication of the pose(s) and wait for it
static int fetch_published(mlh_ctx *ctx, HostPublish &out)
{
    HostPublish *h;
    unsigned long long seq;
    int rc = publish_slot(ctx, &h, &seq);
    if (rc) return rc;
    MLH_LAUNCH(publish_kernel, dim3(1), dim3(64), 0, ctx->stream, (const SolverState *)ctx->state.as<SolverState>(), h, seq);
    MLH_HIP(ctx, hipGetLastError());
    return wait_published(ctx, seq, out);
}

static void copy_stat(const IterStatDev &d, mlh_iter_stat &o)
{
    o.n_surf = d.n_surf; o.n_corner = d.n_corner; o.is_degenerate = d.is_degenerate; o.lm_iterations = d.lm_iterations;
    o.successful_steps = d.successful_steps; o.termination = d.termination; o.cost = d.cost; o.final_cost = d.final_cost;
    std::memcpy(o.eigval, d.eigval, sizeof(o.eigval));
    std::memcpy(o.H, d.H, sizeof(o.H));
    std::memcpy(o.g, d.g, sizeof(o.g));
    std::memcpy(o.pose_after, d.pose_after, sizeof(o.pose_after));
}

// The profiler's events of a collected solve: the kernel that published may still be retiring, so where one of the `retiring` kernels is profiled its own stop
// event needs the stream to drain first
static int prof_drain(mlh_ctx *ctx, uint32_t retiring = ~0u)
{
    if (ctx->prof.pending.empty()) return MLH_OK;
    if (ctx->prof.mask & retiring) MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return MLH_OK;
}

int fetch_pose_and_stats(mlh_ctx *ctx, double pose[7], mlh_iter_stat *stats, int n_stats)
{
    if (!stats || n_stats <= 0) {
        HostPublish hp;
        int rc = fetch_published(ctx, hp);
        if (rc) return rc;
        if (!ctx->prof.pending.empty()) prof_collect(ctx);     // their events precede the publication in stream order: complete
        pose_copy(pose, hp.x);
        return MLH_OK;
    }
    SolverState hs;
    std::vector<IterStatDev> hd(n_stats);
    MLH_HIP(ctx, hipMemcpyAsync(&hs, ctx->state.p, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipMemcpyAsync(hd.data(), ctx->stats.p, sizeof(IterStatDev) * size_t(n_stats), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    if (ctx->p2p.active) { const int erc = device_error_check(ctx); if (erc) return erc; }      // (see wait_published)
    pose_copy(pose, hs.x);
    for (int i = 0; i < n_stats; ++i) copy_stat(hd[i], stats[i]);
    return MLH_OK;
}

// The pose a one-launch loop published to rec / seq, into pose_out (hp_out, nullable: the whole publication -- a scan2map caller collects its matrices from it once the call is known to succeed). *given_up: DONE_GIVEN_UP -- pose_out is left as it was (note_loop_given_up)
int collect_loop_pose(mlh_ctx *ctx, unsigned long long seq, HostPublish *rec, double pose_out[7], bool *given_up, HostPublish *hp_out)
{
    HostPublish hp;
    int rc = wait_published(ctx, seq, hp, rec);
    if (rc) return rc;
    *given_up = (hp.done & DONE_GIVEN_UP) != 0;
    if (*given_up || (rc = prof_drain(ctx))) return rc;
    pose_copy(pose_out, hp.x);
    if (hp_out) *hp_out = hp;
    return MLH_OK;
}

int match_for_factors(mlh_ctx *ctx, int kind, const double rel_pose[7], int k_neigh, uint32_t flags, float min_match_sq_dis, float min_plane_dis)
{
    int rc = ensure_state(ctx, 0);
    if (rc) return rc;
    if ((rc = upload_pose(ctx, rel_pose))) return rc;
    MatchArgs a;
    a.kind_mask = 1 << kind; a.flags = flags & MLH_FLAG_CHECK_FOV; a.min_match_sq_dis = min_match_sq_dis; a.min_plane_dis = min_plane_dis;
    a.huber_delta = 0.0; a.cov_measurement_trace = 0.0; a.dense = false; a.pose_sel = 0; a.k_neigh[0] = k_neigh;
    return match_launch(ctx, a);
}

}  // namespace mlh

using namespace mlh;

extern "C" {

// ---------------------------------------------------------------- features
// marks the padding slots between two pose blocks (intensity < 0 = "not a feature")
__global__ void pad_fill_kernel(float4 *pts, float4 *covd, int from, int to)
{
    const int i = from + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < to) { pts[i] = make_float4(0.f, 0.f, 0.f, -1.f); covd[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
}

int mlh_features_set_block(mlh_ctx *ctx, int kind, int block, const void *points, int stride_bytes, int n, int cov_offset_bytes, int mem)
{
    if (ctx) ++ctx->stage_epoch;
    if (!ctx || kind < 0 || kind > 1 || block < 0 || block >= 8) return MLH_ERR_INVALID;
    // (n == 0: a LiDAR without features of this kind in this frame -- the block exists, holds nothing, contributes no residuals; `points` may be null then)
    const Records r = records_of(points, stride_bytes, n, mem, -1, cov_offset_bytes);
    { const int rc = records_check(ctx, "mlh_features_set_block", r, true); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    FeatSet &f = ctx->feat[kind];
    if (block == 0) { f.m = 0; f.n_blocks = 0; f.has_cov = false; }
    if (block != f.n_blocks) return fail(ctx, MLH_ERR_STATE, "pose blocks must be staged in ascending order starting at 0");
    f.matched = false;
    const int start = block == 0 ? 0 : ((f.m + 255) / 256) * 256;     // blocks begin on fit-tile boundaries
    const size_t total = size_t(start) + size_t(n);
    MLH_HIP(ctx, f.pts.grow(sizeof(float4) * total, sizeof(float4) * size_t(f.m), ctx->stream));
    MLH_HIP(ctx, f.covd.grow(sizeof(float4) * total, sizeof(float4) * size_t(f.m), ctx->stream));
    if (start > f.m)
        MLH_LAUNCH(pad_fill_kernel, dim3((start - f.m + 255) / 256), dim3(256), 0, ctx->stream, f.pts.as<float4>(), f.covd.as<float4>(), f.m, start);
    const unsigned char *src;
    { const int rc = records_stage(ctx, r, ctx->tmp, ctx->stream, &src); if (rc) return rc; }
    // the stored w is the pose-block id (>= 0; the padding's is < 0)
    if (n > 0) pack_points_launch(ctx->stream, src, stride_bytes, n, PACK_W_VALUE, float(block), cov_offset_bytes, f.pts.as<float4>() + start, f.covd.as<float4>() + start);
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    f.blk_start[block] = start;
    f.blk_real[block] = n;
    f.m = int(total);
    f.n_blocks = block + 1;
    for (int b = f.n_blocks; b <= 8; ++b) f.blk_start[b] = f.m;
    f.has_cov = f.has_cov || cov_offset_bytes >= 0;
    return MLH_OK;
}

int mlh_features_set(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, int intensity_offset_bytes,
                     int cov_offset_bytes, int mem)
{
    if (ctx) ++ctx->stage_epoch;
    if (!ctx || kind < 0 || kind > 1) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    FeatSet &f = ctx->feat[kind];
    f.matched = false;
    f.m = 0;
    const Records r = records_of(points, stride_bytes, n, mem, intensity_offset_bytes, cov_offset_bytes);
    int rc = records_check(ctx, "mlh_features_set", r);
    // (w stays 0: the LiDAR index is not needed by the single-pose path; the slot marks padding in block mode)
    if (rc || (rc = stage_points(ctx, r, PACK_W_ZERO, f.pts, &f.covd, ctx->tmp))) return rc;
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    f.single_block(n, cov_offset_bytes >= 0);
    return MLH_OK;
}

// The staged feature set of `kind` handed from one context to another on the same GPU, device to device: how an estimator-side context (extraction, fusion,
// thinning) feeds a mapper-side context (index, scan2MapOptimization) when the two run as separate pipelines, as the reference's estimator and mapper nodes do
// (there: a ROS message through host memory). Ordered after everything `src` has enqueued (waited for here); the copies run on dst's stream.
int mlh_features_copy(mlh_ctx *dst, mlh_ctx *src, int kind)
{
    if (dst) ++dst->stage_epoch;
    if (!dst || !src || dst == src || kind < 0 || kind > 1) return MLH_ERR_INVALID;
    if (dst->device != src->device) return fail(dst, MLH_ERR_UNSUPPORTED, "mlh_features_copy: both contexts must be on the same device");
    MLH_HIP(dst, hipSetDevice(dst->device));
    const FeatSet &a = src->feat[kind];
    FeatSet &f = dst->feat[kind];
    f.matched = false;
    f.m = 0;
    if (a.m <= 0) return fail(dst, MLH_ERR_STATE, "mlh_features_copy: the source context has no staged features of this kind");
    // ordered behind the source's producers ON THE DEVICE (an event of dst's, recorded on src's stream): the caller is typically another thread than the one
    // driving src, and nothing of src's host-side state is touched here (its feature set must simply not be restaged before this call returns)
    { const int hrc = dst->handoff.borrow_begin(dst, src); if (hrc) return hrc; }
    MLH_HIP(dst, f.pts.ensure(sizeof(float4) * size_t(a.m)));
    MLH_HIP(dst, f.covd.ensure(sizeof(float4) * size_t(a.m)));
    MLH_HIP(dst, hipMemcpyAsync(f.pts.p, a.pts.p, sizeof(float4) * size_t(a.m), hipMemcpyDeviceToDevice, dst->stream));
    MLH_HIP(dst, hipMemcpyAsync(f.covd.p, a.covd.p, sizeof(float4) * size_t(a.m), hipMemcpyDeviceToDevice, dst->stream));
    MLH_HIP(dst, stream_wait_spin(dst));                           // the source may overwrite its set as soon as this returns
    f.m = a.m; f.n_blocks = a.n_blocks; f.nbr_stride = a.nbr_stride; f.has_cov = a.has_cov;
    for (int b = 0; b < 9; ++b) f.blk_start[b] = a.blk_start[b];
    for (int b = 0; b < 8; ++b) f.blk_real[b] = a.blk_real[b];
    return MLH_OK;
}

// The staged feature set of `kind`, read only (include/mloam_hip.h): FeatSet::pts and the diagonal FeatSet::covd side by side, 7 floats per record
int mlh_features_fetch(mlh_ctx *ctx, int kind, float *out, int capacity, int32_t *n)
{
    if (n) *n = 0;
    if (!ctx || kind < 0 || kind > 1 || !n) return MLH_ERR_INVALID;
    const FeatSet &f = ctx->feat[kind];
    *n = f.m;
    if (f.m > 0 && f.n_blocks > 1) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_features_fetch: the set was staged in several pose blocks");
    if (capacity < f.m || (f.m > 0 && !out)) return fail(ctx, MLH_ERR_INVALID, "mlh_features_fetch: room for fewer records than are staged");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t m = size_t(f.m > 0 ? f.m : 0);
    std::vector<float4> h(2 * m);
    if (m > 0) {
        MLH_HIP(ctx, hipMemcpyAsync(h.data(), f.pts.p, sizeof(float4) * m, hipMemcpyDeviceToHost, ctx->stream));
        if (f.has_cov) MLH_HIP(ctx, hipMemcpyAsync(h.data() + m, f.covd.p, sizeof(float4) * m, hipMemcpyDeviceToHost, ctx->stream));
    }
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < m; ++i) {
        float *o = out + 7 * i;
        const float4 p = h[i], c = f.has_cov ? h[m + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = p.w; o[4] = c.x; o[5] = c.y; o[6] = c.z;
    }
    return MLH_OK;
}

int mlh_thin_info(mlh_ctx *ctx, mlh_thin_info_t *out)
{
    if (!ctx || !out) return MLH_ERR_INVALID;
    out->path = ctx->thin_note.path;
    out->n_in[0] = ctx->thin_note.n_in[0]; out->n_in[1] = ctx->thin_note.n_in[1];
    out->reserved = 0;
    return MLH_OK;
}

// are these records this context's own fused cloud of `kind` (mlh_fused_cloud: device float4 records whose exact bounding box is known)?
static bool is_fused_cloud(const mlh_ctx *ctx, int kind, const void *points, int n, int stride_bytes, int mem)
{
    return mem == MLH_MEM_DEVICE && !ctx->fused.dirty && n > 0 && points == ctx->fused.pts[kind].p && n == ctx->fused.n[kind] && stride_bytes == 16;
}
// ... and the pair both fused clouds, read with the intensity where mlh_fused_cloud puts it: they go through ONE thinning pipeline
static bool is_fused_pair(const mlh_ctx *ctx, const void *surf, int n_surf, const void *corner, int n_corner, int stride_bytes, int intensity_offset_bytes, int mem)
{
    return intensity_offset_bytes == 12 && is_fused_cloud(ctx, MLH_SURF, surf, n_surf, stride_bytes, mem) && is_fused_cloud(ctx, MLH_CORNER, corner, n_corner, stride_bytes, mem);
}

// downsampleCurrentScan for one feature kind, device-resident: the result IS the kind's feature set
int mlh_downsample_current_scan(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, int intensity_offset_bytes, int mem,
                                float leaf, const double *ext_poses, const double *ext_covs, int n_lidar, const double cov_measurement[9],
                                int with_ua, double trace_threshold, float *features_out, int32_t *n_features)
{
    if (ctx) ++ctx->stage_epoch;
    if (!ctx || kind < 0 || kind > 1 || !n_features) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    FeatSet &f = ctx->feat[kind];
    f.matched = false;
    f.m = 0;
    { const int rc = records_check(ctx, "mlh_downsample_current_scan", records_of(points, stride_bytes, n, mem, intensity_offset_bytes)); if (rc) return rc; }
    float *d_out = nullptr;
    if (features_out) {
        MLH_HIP(ctx, ctx->tmp.ensure(sizeof(float) * 11 * size_t(n)));
        d_out = ctx->tmp.as<float>();
    }
    int m = 0;
    // a fused cloud of this context brings its exact bounding box along (mlh_fused_cloud): no bounds pass
    const float *known_bounds = nullptr;
    for (int k = 0; k < 2; ++k)
        if (is_fused_cloud(ctx, k, points, n, stride_bytes, mem)) known_bounds = ctx->fused.minmax[k];
    int rc = downsample_current_scan_run(ctx, points, stride_bytes, n, intensity_offset_bytes, mem, leaf, ext_poses, ext_covs, n_lidar, cov_measurement,
                                         with_ua, trace_threshold, f.pts, f.covd, d_out, &m, known_bounds);
    if (rc) return rc;
    if (features_out && m > 0) {
        MLH_HIP(ctx, hipMemcpyAsync(features_out, d_out, sizeof(float) * 11 * size_t(m), hipMemcpyDeviceToHost, ctx->stream));
        MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *n_features = m;
    f.single_block(m, true);
    return MLH_OK;
}

// downsampleCurrentScan for BOTH feature kinds (lidar_mapper_keyframe.cpp:359-368 thins the surf and the corner cloud back to back).
// When both clouds are this context's fused clouds (device-resident, bounding boxes known) they go through ONE thinning pipeline --
// the chains are dispatch-bound, so one chain for both halves the time; otherwise the two single calls are made.
int mlh_downsample_current_scan_pair(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                                     int intensity_offset_bytes, int mem, float leaf_surf, float leaf_corner, const double *ext_poses, const double *ext_covs,
                                     int n_lidar, const double cov_measurement[9], int with_ua, double trace_threshold, int32_t *n_surf_features,
                                     int32_t *n_corner_features)
{
    if (ctx) ++ctx->stage_epoch;
    if (!ctx || !n_surf_features || !n_corner_features) return MLH_ERR_INVALID;
    ctx->thin_note.begin(n_surf, n_corner);
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const bool fused_pair = is_fused_pair(ctx, surf_points, n_surf, corner_points, n_corner, stride_bytes, intensity_offset_bytes, mem);
    if (fused_pair) {
        for (int k = 0; k < 2; ++k) { ctx->feat[k].matched = false; ctx->feat[k].m = 0; }
        int m[2] = {0, 0};
        int rc = downsample_current_scan_pair_run(ctx, surf_points, n_surf, ctx->fused.minmax[MLH_SURF], leaf_surf, corner_points, n_corner,
                                                  ctx->fused.minmax[MLH_CORNER], leaf_corner, stride_bytes, intensity_offset_bytes, ext_poses, ext_covs, n_lidar,
                                                  cov_measurement, with_ua, trace_threshold, &m[0], &m[1]);
        if (rc == MLH_OK) {
            for (int k = 0; k < 2; ++k) ctx->feat[k].single_block(m[k], true);
            *n_surf_features = m[0];
            *n_corner_features = m[1];
            return MLH_OK;
        }
        if (rc != MLH_ERR_UNSUPPORTED) return rc;            // a grid too large for the shared index space: one by one below
    }
    ctx->thin_note.path = MLH_THIN_SINGLE_CALLS;
    int rc = mlh_downsample_current_scan(ctx, MLH_SURF, surf_points, stride_bytes, n_surf, intensity_offset_bytes, mem, leaf_surf, ext_poses, ext_covs, n_lidar,
                                         cov_measurement, with_ua, trace_threshold, nullptr, n_surf_features);
    if (rc) return rc;
    return mlh_downsample_current_scan(ctx, MLH_CORNER, corner_points, stride_bytes, n_corner, intensity_offset_bytes, mem, leaf_corner, ext_poses, ext_covs, n_lidar,
                                       cov_measurement, with_ua, trace_threshold, nullptr, n_corner_features);
}

// ---------------------------------------------------------------- host-driven match / linearise
static int fetch_dense_and_reduced(mlh_ctx *ctx, int kind, bool want_corr, uint8_t *valid, double *coeffs, double *r, double *J,
                                   double *JtJ, double *Jtr, double *cost, int32_t *n_valid)
{
    FeatSet &f = ctx->feat[kind];
    hipStream_t st = ctx->stream;
    std::vector<Corr> hc;
    if (want_corr && (valid || coeffs)) {
        hc.resize(f.m);
        MLH_HIP(ctx, hipMemcpyAsync(hc.data(), f.corr.p, sizeof(Corr) * size_t(f.m), hipMemcpyDeviceToHost, st));
    }
    if (r) MLH_HIP(ctx, hipMemcpyAsync(r, f.r.p, sizeof(double) * size_t(f.m), hipMemcpyDeviceToHost, st));
    if (J) MLH_HIP(ctx, hipMemcpyAsync(J, f.J.p, sizeof(double) * 6 * size_t(f.m), hipMemcpyDeviceToHost, st));
    SolverState hs;
    MLH_HIP(ctx, hipMemcpyAsync(&hs, ctx->state.p, sizeof(hs), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipStreamSynchronize(st));
    prof_collect(ctx);
    if (!hc.empty()) {
        for (int i = 0; i < f.m; ++i) {
            if (valid) valid[i] = hc[i].valid ? 1 : 0;
            if (coeffs) for (int k = 0; k < 6; ++k) coeffs[size_t(i) * 6 + k] = double(hc[i].c[k]);
        }
    }
    if (JtJ) {
        int q = 0;
        for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { JtJ[i * 6 + j] = hs.ne[q]; JtJ[j * 6 + i] = hs.ne[q]; ++q; }
    }
    if (Jtr) for (int i = 0; i < 6; ++i) Jtr[i] = hs.ne[NE_G + i];
    if (cost) *cost = hs.ne[NE_COST];
    if (n_valid) *n_valid = int(hs.ne[NE_CNT] + 0.5);
    return MLH_OK;
}

int mlh_match_coeffs(mlh_ctx *ctx, int kind, uint8_t *valid, double *coeffs, int32_t *n_valid)
{
    if (!ctx || kind < 0 || kind > 1) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    FeatSet &f = ctx->feat[kind];
    if (!f.matched || f.m <= 0 || !f.corr.p) return fail(ctx, MLH_ERR_STATE, "no correspondences of this kind on the device (match first)");
    std::vector<Corr> hc(size_t(f.m));
    MLH_HIP(ctx, hipMemcpyAsync(hc.data(), f.corr.p, sizeof(Corr) * size_t(f.m), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (int i = 0; i < f.m; ++i) {
        if (valid) valid[i] = hc[i].valid ? 1 : 0;
        if (coeffs) for (int k = 0; k < 6; ++k) coeffs[size_t(i) * 6 + k] = double(hc[i].c[k]);
        n += hc[i].valid ? 1 : 0;
    }
    if (n_valid) *n_valid = n;
    return MLH_OK;
}

int mlh_match_neighbours(mlh_ctx *ctx, int kind, float *records_out, int32_t *k_stride_out)
{
    if (!ctx || kind < 0 || kind > 1) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    FeatSet &f = ctx->feat[kind];
    if (!f.matched || f.m <= 0 || !f.nbr.p) return fail(ctx, MLH_ERR_STATE, "no neighbour records of this kind on the device (match first)");
    if (k_stride_out) *k_stride_out = f.nbr_stride;
    if (!records_out) return MLH_OK;
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MLH_HIP(ctx, hipMemcpy(records_out, f.nbr.p, sizeof(float4) * size_t(f.nbr_stride) * size_t(f.m), hipMemcpyDeviceToHost));
    return MLH_OK;
}

int mlh_match_linearize(mlh_ctx *ctx, int kind, const double pose[7], int k_neigh, uint32_t flags,
                        float min_match_sq_dis, float min_plane_dis, double huber_delta, double cov_measurement_trace,
                        uint8_t *valid, double *coeffs, double *r, double *J,
                        double *JtJ, double *Jtr, double *cost, int32_t *n_valid)
{
    if (!ctx || kind < 0 || kind > 1 || !pose) return MLH_ERR_INVALID;
    if (k_neigh != 5 && k_neigh != 10) return fail(ctx, MLH_ERR_UNSUPPORTED, "N_NEIGH is 5 (the mapper, the reference LiDAR) or 10 (buildCalibMap's other LiDARs, estimator.cpp:1135)");
    if ((r == nullptr) != (J == nullptr)) return fail(ctx, MLH_ERR_INVALID, "r and J must be requested together");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_state(ctx, 0);
    if (rc) return rc;
    if ((rc = upload_pose(ctx, pose))) return rc;
    MatchArgs a;
    a.kind_mask = 1 << kind; a.flags = flags; a.min_match_sq_dis = min_match_sq_dis; a.min_plane_dis = min_plane_dis;
    a.huber_delta = huber_delta; a.cov_measurement_trace = cov_measurement_trace; a.dense = (r != nullptr); a.pose_sel = 0;
    a.k_neigh[0] = k_neigh;
    if ((rc = match_launch(ctx, a))) return rc;
    if ((rc = reduce_only_launch(ctx, 0))) return rc;
    return fetch_dense_and_reduced(ctx, kind, true, valid, coeffs, r, J, JtJ, Jtr, cost, n_valid);
}

int mlh_linearize(mlh_ctx *ctx, int kind, const double pose[7], uint32_t flags, double huber_delta, double cov_measurement_trace,
                  double *r, double *J, double *JtJ, double *Jtr, double *cost, int32_t *n_valid)
{
    if (!ctx || kind < 0 || kind > 1 || !pose) return MLH_ERR_INVALID;
    if ((r == nullptr) != (J == nullptr)) return fail(ctx, MLH_ERR_INVALID, "r and J must be requested together");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_state(ctx, 0);
    if (rc) return rc;
    if ((rc = upload_pose(ctx, pose))) return rc;
    MatchArgs a;
    a.kind_mask = 1 << kind; a.flags = flags; a.min_match_sq_dis = 0.f; a.min_plane_dis = 0.f;
    a.huber_delta = huber_delta; a.cov_measurement_trace = cov_measurement_trace; a.dense = (r != nullptr); a.pose_sel = 0;
    if ((rc = linearize_launch(ctx, a))) return rc;
    if ((rc = reduce_only_launch(ctx, 0))) return rc;
    return fetch_dense_and_reduced(ctx, kind, false, nullptr, nullptr, r, J, JtJ, Jtr, cost, n_valid);
}

static MatchArgs args_from_opts(const mlh_solver_opts *o, int kind_mask, int pose_sel)
{
    MatchArgs a;
    a.kind_mask = kind_mask; a.eig_thre[0] = o->map_eig_thre; a.flags = o->flags & (MLH_FLAG_CHECK_FOV | MLH_FLAG_WITH_UA | MLH_FLAG_POSE_COV);      // (POSE_COV: read by the LM launchers of scan2map only, match.hip: pose_cov_launch)
    a.min_match_sq_dis = o->min_match_sq_dis; a.min_plane_dis = o->min_plane_dis;
    a.huber_delta = o->huber_delta; a.cov_measurement_trace = o->cov_measurement_trace; a.dense = false; a.pose_sel = pose_sel;
    return a;
}

// the kinds a solve covers: bit k when kind k has features staged and its map built
static int solve_kind_mask(const mlh_ctx *ctx)
{
    return ((ctx->feat[0].m > 0 && ctx->map[0].built) ? 1 : 0) | ((ctx->feat[1].m > 0 && ctx->map[1].built) ? 2 : 0);
}
static int feature_tiles(const mlh_ctx *ctx, int kind_mask = 3)
{
    return ((kind_mask & 1) ? tiles_of(ctx->feat[0].m) : 0) + ((kind_mask & 2) ? tiles_of(ctx->feat[1].m) : 0);
}
// scan2MapOptimization runs only when the map has > 50 surf and > 10 corner points (lidar_mapper_keyframe.cpp:429)
static bool scan2map_has_maps(const mlh_ctx *ctx)
{
    return ctx->map[MLH_SURF].built && ctx->map[MLH_CORNER].built && ctx->map[MLH_SURF].n > 50 && ctx->map[MLH_CORNER].n > 10;
}

// The deferred finish makes EVERY workgroup of the next correspondence launch sum the fit tiles' records: cheap for a mapper frame (88 records, ~1 000
// workgroups: +3.5 us against the 5 us the fit kernel's serial tail costs), quadratic in the launch size beyond it -- measured (profiles/r04_feature_sweep.txt):
// even at 27-34 k features (108-133 tiles), a loss from ~100 k features on (447 tiles: +14 us), 4x the launch at 450 k. Launches with more tiles than this keep the
// classic finish, whose one serial tail is noise next to a 100 us kernel.
static bool gn_defer_applies(const mlh_ctx *ctx, int kind_mask)
{
    return ctx->gn_defer && !distributed(ctx) && feature_tiles(ctx, kind_mask) <= GN_DEFER_MAX_TILES;
}

// The arguments of Gauss-Newton iteration `it` of `n_iters` (the start pose goes in with iteration 0's). Iterations >= 1 re-find the neighbours of the same features
// in the same map: the previous iteration's five bound the search (not with ownership planes: a feature that changes hands between iterations would bring another
// frame's records). `defer`: one GPU, no per-iteration statistics -- the fit launch of every iteration but the last (or every one, `leave_final`) only leaves its
// tiles' records, and the next iteration's correspondence launch, whose every workgroup sums and solves for itself (match.hip: knn_features_kernel<.., PRE>), finishes
// it. Which iterations the start pose goes in with is the pose plan's rule (solve_plan_host.hpp).
static MatchArgs gn_iter_args(const mlh_ctx *ctx, const mlh_solver_opts *opts, int mask, int it, int n_iters, const double *pose, bool defer, bool leave_final = false)
{
    MatchArgs a = args_from_opts(opts, mask, 0);
    if (gn_start_pose_goes_in(it, defer)) a.init_pose = pose;
    a.warm = it >= 1 && ctx->knn_warm && !ctx->shard_lo && !ctx->shard_hi;
    a.finish = TAIL_GN;
    if (defer) {
        a.gn_iter = it; a.gn_iters = n_iters;
        if (it < n_iters - 1 || leave_final) a.finish = TAIL_RECORDS;
    }
    return a;
}

int mlh_gn_solve(mlh_ctx *ctx, double pose_inout[7], int n_iters, const mlh_solver_opts *opts, mlh_iter_stat *stats)
{
    if (!ctx || !pose_inout || !opts || n_iters <= 0) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = solver_begin(ctx, n_iters);
    if (rc) return rc;
    const int mask = solve_kind_mask(ctx);
    if (!mask) return fail(ctx, MLH_ERR_STATE, "no map/features staged");
    // the pose goes in with the first iteration's kernel arguments and (single GPU, no statistics wanted) comes back through
    // pinned host memory written by the last iteration's finish: 2 launches per iteration and nothing else
    unsigned long long seq = 0;
    const bool fused_publish = !stats && (!distributed(ctx) || ctx->p2p.active);
    const bool defer = !stats && n_iters >= 2 && gn_defer_applies(ctx, mask);
    ctx->gn_fused_launches = 0;
    for (int it = 0; it < n_iters; ++it) {
        MatchArgs a = gn_iter_args(ctx, opts, mask, it, n_iters, pose_inout, defer);
        if (!distributed(ctx) || ctx->p2p.active) {
            // single GPU: two launches per iteration; the fit kernel's last workgroup reduces, solves and updates the pose. Several ranks joined by the
            // mailbox communicator: the same two launches -- that workgroup exchanges the summed record with the peers (one hop) before it solves
            a.stat_slot = stats ? it : -1;
            if (it == n_iters - 1 && fused_publish) {
                if ((rc = publish_slot(ctx, &a.publish, &seq))) return rc;
                a.publish_seq = seq;
            }
            if ((rc = match_launch(ctx, a))) return rc;
        } else {
            // multi-GPU: the fit kernel's last workgroup leaves this rank's sums in the solver state, then ONE all-reduce of
            // 32 doubles, then every rank runs the identical solve
            a.finish = TAIL_REDUCE;
            if ((rc = match_launch(ctx, a))) return rc;
            if ((rc = comm_allreduce_state(ctx, 0))) return rc;
            if ((rc = gn_update_prereduced_launch(ctx, opts->map_eig_thre, stats ? it : -1))) return rc;
        }
    }
    if (fused_publish) {
        HostPublish hp;
        if ((rc = wait_published(ctx, seq, hp))) return rc;
        if ((rc = prof_drain(ctx, (1u << MLH_K_FIT) | (1u << MLH_K_SOLVE)))) return rc;
        pose_copy(pose_inout, hp.x);
        return MLH_OK;
    }
    return fetch_pose_and_stats(ctx, pose_inout, stats, n_iters);
}

// ---- the same solve, submitted and collected separately: mlh_gn_solve_begin enqueues the iterations and returns; mlh_gn_solve_end waits for the pose. A caller that
// stages the NEXT frame's maps between the two (mlh_map_set_pair: its launches queue up behind this solve on the context's stream) keeps the GPU busy across
// the frame boundary -- the ~16 us of host turn-around between "pose published" and "next frame's first launch" (profiles/r03_step_timeline.txt) disappear.
// Up to TWO solves may be in flight (frame k + 1 submitted before frame k's pose is collected: the GPU starts it the moment frame k is done instead of after the
// host has seen the pose and enqueued ten launches); each publishes into its own pinned record, apart from the one the staging hand-shake uses.
static int gn_solve_submit(mlh_ctx *ctx, const double *pose_in, const double *wodom_prev, const double *wodom_cur, int n_iters, const mlh_solver_opts *opts)
{
    // several ranks: fine with the mailbox communicator (the exchange happens inside the launches, the host is not involved); not over RCCL
    if (ctx->comm) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_gn_solve_begin under an RCCL communicator: the sharded solve there is a host-driven sequence of launches and collectives (use the mailbox communicator)");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long seq = 0;
    HostPublish *rec = nullptr;
    mlh_ctx::SolveSlot *slot = nullptr;
    int rc = ctx->solves.admit(ctx, "two solves are already in flight: collect the older one with mlh_gn_solve_end first", &seq, &rec, &slot);
    if (rc) return rc;
    if ((rc = ensure_state(ctx, 0))) return rc;
    const int mask = solve_kind_mask(ctx);
    if (!mask) return fail(ctx, MLH_ERR_STATE, "no map/features staged");
    slot->kind = mlh_ctx::SolveSlot::GN;
    const bool defer = n_iters >= 2 && gn_defer_applies(ctx, mask);
    // The previous solve may have left its LAST iteration as tile records (GnChain::pending). A chained, deferred solve completes it in its own first launch -- unless this
    // frame needs a larger record buffer (the records would not survive the reallocation); everything else completes it now, before the chain launch reads the pose.
    // A predecessor that left wavefront rows (a fused last iteration) needs a successor whose first launch reads rows (the planner says) and whose own rows fit the
    // buffer the pending set lies in.
    const mlh_ctx::GnPending pend = ctx->gn.pending;
    const bool rows_ok = pend.recs.rows != 4 || (gn_first_launch_takes_rows(ctx, mask) && ctx->gn.rows_hold(feature_tiles(ctx, mask)));
    const bool consume = !pose_in && defer && pend.active && sizeof(double) * NE_STRIDE * size_t(feature_tiles(ctx, mask)) <= ctx->partials.cap && rows_ok;
    ctx->gn_fused_launches = 0;
    if (!consume && (rc = gn_flush_pending(ctx))) return rc;
    if (!pose_in && !consume && (rc = enqueue_chain_pose(ctx, wodom_prev, wodom_cur, nullptr))) return rc;
    // this solve's own last iteration: left to a successor (or to mlh_gn_solve_end) when the schedule says so
    const bool leave_final = defer && ctx->gn_final_defer;
    const int base = ctx->gn.solve_begins();
    for (int it = 0; it < n_iters; ++it) {
        // (pose_in is null when chained: the kernels read the state's pose, or compute it: `consume`)
        MatchArgs a = gn_iter_args(ctx, opts, mask, it, n_iters, pose_in, defer, leave_final);
        if (defer) a.gn_slot_base = base;
        if (consume) {
            a.pre_final = &pend;               // iteration 0: complete the predecessor, publish its pose, chain; iterations >= 1: pose 0 sits in its slot
            if (it == 0) { a.chain_prev = wodom_prev; a.chain_cur = wodom_cur; }
        }
        if (it == n_iters - 1 && !leave_final) {
            a.publish = rec;
            a.publish_seq = seq;
        }
        if ((rc = match_launch(ctx, a))) return rc;
        if (it == 0 && consume) ctx->gn.take_pending();       // consumed by the launch just enqueued
    }
    if (leave_final) ctx->gn.solve_left_last(base, n_iters, opts->map_eig_thre, rec, seq);      // (tile records in `partials`, or a fused last iteration's set of wavefront rows)
    ctx->solves.commit(seq, ctx->map_set_cur);
    return MLH_OK;
}

int mlh_gn_solve_begin(mlh_ctx *ctx, const double pose_in[7], int n_iters, const mlh_solver_opts *opts)
{
    if (!ctx || !pose_in || !opts || n_iters <= 0) return MLH_ERR_INVALID;
    return gn_solve_submit(ctx, pose_in, nullptr, nullptr, n_iters, opts);
}

int mlh_gn_solve_begin_chained(mlh_ctx *ctx, const double wodom_prev[7], const double wodom_cur[7], int n_iters, const mlh_solver_opts *opts)
{
    if (!ctx || !wodom_prev || !wodom_cur || !opts || n_iters <= 0) return MLH_ERR_INVALID;
    if (ctx->solves.submitted == 0) return fail(ctx, MLH_ERR_STATE, "mlh_gn_solve_begin_chained continues from the pose a previous solve left on the device: submit the first frame with mlh_gn_solve_begin");
    return gn_solve_submit(ctx, nullptr, wodom_prev, wodom_cur, n_iters, opts);
}

int mlh_gn_solve_end(mlh_ctx *ctx, double pose_out[7])
{
    if (!ctx || !pose_out) return MLH_ERR_INVALID;
    if (!ctx->solves.pending()) return fail(ctx, MLH_ERR_STATE, "no solve in flight (mlh_gn_solve_begin)");
    const unsigned long long seq = ctx->solves.oldest();
    if (ctx->solves.slot[seq & 1].kind != mlh_ctx::SolveSlot::GN) return fail(ctx, MLH_ERR_STATE, "the oldest solve in flight was submitted with mlh_scan2map_begin: collect it with mlh_scan2map_end");
    if (ctx->gn.pending.active && ctx->gn.pending.seq == seq) {      // nobody chained a successor behind it: its last iteration is completed here
        const int frc = gn_flush_pending(ctx);
        if (frc) return frc;
    }
    HostPublish hp;
    int rc = wait_published(ctx, seq, hp, ctx->solves.record(seq));
    ctx->solves.retire(seq);
    if (rc) return rc;
    if (!ctx->solves.pending() && (rc = prof_drain(ctx, (1u << MLH_K_FIT) | (1u << MLH_K_SOLVE)))) return rc;
    pose_copy(pose_out, hp.x);
    return MLH_OK;
}

int mlh_gn_solve_blocks(mlh_ctx *ctx, double *poses_inout, int n_iters, const mlh_solver_opts *opts, const mlh_block_opts *bo,
                        mlh_iter_stat *stats)
{
    if (!ctx || !poses_inout || !opts || !bo || n_iters <= 0 || bo->n_blocks <= 0 || bo->n_blocks > 8) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const int nb = bo->n_blocks;
    int rc = solver_begin(ctx, n_iters * nb);
    if (rc) return rc;
    ctx->gn_fused_launches = 0;
    if ((rc = upload_pose(ctx, poses_inout))) return rc;
    for (int b = 1; b < nb; ++b) if ((rc = upload_block_pose(ctx, b, poses_inout + 7 * b))) return rc;
    const int mask = solve_kind_mask(ctx);
    if (!mask) return fail(ctx, MLH_ERR_STATE, "no map/features staged");
    // The finish in the consumer, per pose block (one GPU, no statistics): a correspondence workgroup serves features of ONE block, so its prologue sums that block's
    // records only and solves that block only -- the four serial finishes of the classic last workgroup (20 us of a 40 us fit launch on config 4's frame) become one
    // parallel prologue, and the redundancy is per block (at most 160 tiles each). Together with the bounded search (N_NEIGH 5 or 10); every block needs surf features
    // (its first surf tile's workgroup is the one that leaves the block's pose in HBM).
    bool defer_blocks = !distributed(ctx) && !stats && n_iters >= 2 && ctx->gn_defer && ctx->knn_warm && !ctx->shard_lo && !ctx->shard_hi;
    for (int b = 0; b < nb && defer_blocks; ++b) {
        int tiles = 0;
        for (int k = 0; k < 2; ++k) if (mask & (1 << k)) tiles += (ctx->feat[k].blk_start[b + 1] - ctx->feat[k].blk_start[b] + 255) / 256;
        if (!(mask & 1) || ctx->feat[0].n_blocks != nb || ctx->feat[0].blk_real[b] <= 0 || tiles > GN_DEFER_MAX_TILES) defer_blocks = false;
    }
    for (int it = 0; it < n_iters; ++it) {
        MatchArgs a = args_from_opts(opts, mask, 0);
        a.n_blocks = nb;
        for (int b = 0; b < nb; ++b) { a.k_neigh[b] = bo->k_neigh[b]; a.eig_thre[b] = bo->eig_thre[b]; a.freeze[b] = bo->freeze[b]; }
        if (!distributed(ctx) || ctx->p2p.active) {      // (mailbox communicator: the blocks' records are exchanged inside the finish, one after the other)
            a.finish = TAIL_GN;
            a.stat_slot = stats ? it * nb : -1;
            if (defer_blocks) {
                a.gn_iter = it; a.gn_iters = n_iters; a.gn_blocks = true;
                a.warm = it >= 1;
                if (it < n_iters - 1) a.finish = TAIL_RECORDS;
            }
            if ((rc = match_launch(ctx, a))) return rc;
        } else {
            // multi-GPU: per-block local sums in the fit kernel's last workgroup, ONE all-reduce of nb x 32 doubles, identical updates
            a.finish = TAIL_REDUCE;
            if ((rc = match_launch(ctx, a))) return rc;
            if ((rc = comm_allreduce_blocks(ctx, nb))) return rc;
            if ((rc = gn_update_blocks_prereduced_launch(ctx, nb, bo->eig_thre, bo->freeze, stats ? it * nb : -1))) return rc;
        }
    }
    HostPublish hs;
    std::vector<IterStatDev> hd(stats ? size_t(n_iters) * nb : 0);
    if (stats) MLH_HIP(ctx, hipMemcpyAsync(hd.data(), ctx->stats.p, sizeof(IterStatDev) * hd.size(), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = fetch_published(ctx, hs))) return rc;
    if (stats) MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    pose_copy(poses_inout, hs.x);
    for (int b = 1; b < nb; ++b) pose_copy(poses_inout + 7 * b, hs.xb[b]);
    for (size_t i = 0; stats && i < hd.size(); ++i) copy_stat(hd[i], stats[i]);
    return MLH_OK;
}

// ---------------------------------------------------------------- scan2MapOptimization: the forms a frame's launches take
enum class S2mForm {   // per outer iteration: correspondences (+ a good-feature selection), then a Levenberg-Marquardt loop on them -- where that loop runs:
    HOST_STEPPED,      // stand-alone kernels: lm_begin_launch, then linearize_launch + lm_step_launch per iteration, the verdict fetched between chunks of them
    FUSED_CHUNKS,      // the classic launches: the begin / step in the last workgroup of the launch that evaluated (TAIL_LM_BEGIN / _STEP), polled between chunks
    CONSUMER_CHUNKS,   // the consumer-side launches: the begin / step in every workgroup of the NEXT launch (LMC_BEGIN / _STEP) -- one launch more per loop
    LOOP               // an outer iteration's whole loop as ONE launch whose workgroups synchronise among themselves (LMC_LOOP); the frame is enqueued at once
};
static bool s2m_selects(const mlh_solver_opts *opts) { return opts->gf_method != MLH_GF_WO; }

// ---- MLH_FLAG_POSE_COV: H at the returned pose and its inverse ride in the publication that carries the pose (reduce_dev.hpp: publish_pose_cov); what
// mlh_scan2map_cov hands out is copied from that record when the solve is collected
static bool wants_pose_cov(const mlh_solver_opts *opts) { return (opts->flags & MLH_FLAG_POSE_COV) != 0; }
// a scan2map solve is being collected: until it has produced a result there is nothing for the getter
static void pose_cov_open(mlh_ctx *ctx, const mlh_solver_opts *opts)
{
    ctx->pose_cov.state = wants_pose_cov(opts) ? mlh_ctx::PoseCov::NOT_A_RESULT : mlh_ctx::PoseCov::UNFLAGGED;
}
// ... and has: hp = the publication its pose came with, or null -- nothing was optimised (a local map below cpp:429's minimum): both matrices zero (cpp:637)
static void pose_cov_collect(mlh_ctx *ctx, const mlh_solver_opts *opts, const HostPublish *hp)
{
    if (!wants_pose_cov(opts)) { ctx->pose_cov.state = mlh_ctx::PoseCov::UNFLAGGED; return; }
    for (int i = 0; i < 36; ++i) { ctx->pose_cov.H[i] = hp ? hp->H_final[i] : 0.0; ctx->pose_cov.cov[i] = hp ? hp->cov[i] : 0.0; }
    ctx->pose_cov.state = mlh_ctx::PoseCov::VALID;
}
// the multi-rank forms exchange records inside their launches or step through them on the host: they publish no covariance, so the flag is refused up front
static int pose_cov_refuse_distributed(mlh_ctx *ctx, const mlh_solver_opts *opts)
{
    if (wants_pose_cov(opts) && distributed(ctx))
        return fail(ctx, MLH_ERR_UNSUPPORTED, "MLH_FLAG_POSE_COV under an RCCL or mailbox communicator: the pose covariance is delivered by the single-GPU forms of scan2map only");
    return MLH_OK;
}

// THE decision: mlh_scan2map, mlh_scan2map_begin* and mlh_downsample_scan2map all ask here (DESIGN.md section 5 has it as a table). allow_loop: the caller has not
// ruled the one-launch loop out; gate / tiles: the residency gate the loop launch would pass (mlh_ctx::caps::loop_max_tiles) and the workgroups it would have.
static S2mForm s2m_form(const mlh_ctx *ctx, const mlh_solver_opts *opts, bool want_stats, bool allow_loop, int gate, int tiles)
{
    const bool one_gpu = !distributed(ctx);
    // the mailbox communicator's exchange rides in the fused finish; under RCCL, and for a selection's rows on several ranks, the host steps through the iterations
    if (!one_gpu && !(ctx->p2p.active && !s2m_selects(opts))) return S2mForm::HOST_STEPPED;
    // Consumer-side: one GPU, nobody reading per-iteration statistics, few enough tiles that every workgroup summing every tile's record pays (the Gauss-Newton
    // path's limit). Gate 1 -- the fused thinning + solve call, which sizes its launches for the UN-thinned clouds -- deliberately tests that bound against its own
    // gate only (FUSED_LOOP_MAX_TILES, set_loop_gates): the thinned frame it solves is far below the limit.
    if (!one_gpu || want_stats || !schedule_on(Schedule::LM_CONSUMER) || (gate != 1 && tiles > GN_DEFER_MAX_TILES)) return S2mForm::FUSED_CHUNKS;
    if (allow_loop && schedule_on(Schedule::LM_LOOP) && loop_tiles_ok(ctx, gate, tiles, wants_pose_cov(opts))) return S2mForm::LOOP;      // (every tile's workgroup resident at once)
    return s2m_selects(opts) ? S2mForm::FUSED_CHUNKS : S2mForm::CONSUMER_CHUNKS;      // (linearize_launch's LM begin has no consumer-side chunk form)
}

static bool s2m_warm_applies(const mlh_ctx *ctx) { return ctx->knn_warm && !ctx->shard_lo && !ctx->shard_hi && ctx->own_mod <= 1; }

// scan2MapOptimization matches through ActiveFeatureSelection::goodFeatureMatching, which passes n_neigh = 5 and CHECK_FOV = false to match*PointFromMap whatever
// the caller's configuration says (lidar_mapper.h:256-283, every gf_method): MLH_FLAG_CHECK_FOV does not apply to the scan2map entry points. (The flag is for
// mlh_gn_solve*, mlh_match_linearize and the odometry's matches, where the reference does pass CHECK_FOV: estimator.cpp:1142, 1149. Found by the "hard" scene
// family of round 6: tall poles put corner features outside the +-60 degree cone, and a scan2map that honoured the flag dropped what the reference keeps.)
static mlh_solver_opts scan2map_opts(const mlh_solver_opts *o)
{
    mlh_solver_opts c = *o;
    c.flags &= ~uint32_t(MLH_FLAG_CHECK_FOV);
    return c;
}

// The match launch of an outer iteration (records_only: a consumer-side launch runs the LM begin). Outer iterations behind the first search the same map for the
// same features from a pose a few centimetres away: bounded by the neighbours the previous one left (knn_feature_warm: still the exact 5-NN). `unpolled`
// (scan2map_submit): the host has not read the previous LM loop's verdict.
static MatchArgs s2m_begin_args(const mlh_ctx *ctx, const mlh_solver_opts *opts, bool records_only, int outer, const double *pose, bool unpolled)
{
    MatchArgs a = args_from_opts(opts, 3, 0);
    a.finish = records_only ? TAIL_RECORDS : TAIL_LM_BEGIN; a.lm_max_it = opts->max_lm_iterations;
    if (outer == 0) { a.init_pose = pose; a.lm_expect_done = LM_FIRST_OF_SOLVE; }
    else if (unpolled) a.lm_expect_done = LM_VERDICT_UNREAD;
    a.warm = outer >= 1 && s2m_warm_applies(ctx);
    return a;
}

// The j-th (from 0) LM launch behind that match launch, consumer-side (lmc) or classic. `unpolled` as above.
static MatchArgs s2m_lm_args(const mlh_solver_opts *opts, bool lmc, int outer, int j, const double *pose, bool unpolled)
{
    MatchArgs a = args_from_opts(opts, 3, 1);
    a.finish = TAIL_LM_STEP; a.lm_max_it = opts->max_lm_iterations;
    if (outer != opts->max_outer - 1) a.flags &= ~uint32_t(MLH_FLAG_POSE_COV);      // (the covariance belongs to the LAST outer iteration's loop: earlier chunks publish the default way)
    if (lmc) {
        a.finish = TAIL_RECORDS; a.lmc = j == 0 ? LMC_BEGIN : LMC_STEP; a.lmc_j = j + 1;
        if (j == 0 && outer == 0) { a.init_pose = pose; a.lm_expect_done = LM_FIRST_OF_SOLVE; }
        else if (j == 0 && unpolled) a.lm_expect_done = LM_VERDICT_UNREAD;
    }
    return a;
}

// The launch that runs outer iteration `outer`'s whole LM loop on the device. The start pose goes in with the first one (pose null: the state holds it), the last
// one publishes pose and verdict to rec / seq. `match_in_front`: the match launch enqueued in front of it, whose fit moves into the loop launch where
// loop_fit_fusable says so -- no_fit and fit_in_loop leave here as a pair -- or null: a linearise launch over a selection's rows is in front.
static MatchArgs s2m_loop_args(const mlh_solver_opts *opts, int outer, const double *pose, HostPublish *rec, unsigned long long seq, MatchArgs *match_in_front)
{
    MatchArgs b = args_from_opts(opts, 3, 1);
    b.lmc = LMC_LOOP; b.lmc_j = 1; b.lm_max_it = opts->max_lm_iterations;
    b.lm_expect_done = outer == 0 ? LM_FIRST_OF_SOLVE : LM_VERDICT_UNREAD;
    if (outer == 0) b.init_pose = pose;
    if (outer == opts->max_outer - 1) { b.publish = rec; b.publish_seq = seq; }
    if (match_in_front) { b.m_dev = match_in_front->m_dev; match_in_front->no_fit = b.fit_in_loop = loop_fit_fusable(*match_in_front); }
    return b;
}

// The selection step of an outer iteration: goodFeatureMatching for corners, then surfs (cpp:503-533), each against a fresh 1e-6 * I. Both kinds' dense passes and
// their copies to the host are enqueued first: the corner selection loop runs on the host while the surf pass and its copies are still in flight, and each kind's
// flags go back without a wait (the linearise launch that evaluates the selected rows -- problem.Evaluate, cpp:575-581 -- is behind them on the stream)
static int s2m_select(mlh_ctx *ctx, const mlh_solver_opts *opts, std::mt19937 &rng)
{
    int rc;
    std::vector<int32_t> sel;
    for (int kind : {MLH_CORNER, MLH_SURF})
        if ((rc = good_feature_stage(ctx, kind, opts->gf_method, opts->gf_ratio, rng, opts->min_match_sq_dis, opts->min_plane_dis, true))) return rc;
    if ((rc = good_feature_fps_flush(ctx))) return rc;      // ('fps': the two kinds' loops side by side in one launch; nothing pending otherwise)
    for (int kind : {MLH_CORNER, MLH_SURF}) {
        double Hsel[36];
        for (int i = 0; i < 36; ++i) Hsel[i] = (i % 7 == 0) ? 1e-6 : 0.0;
        if ((rc = good_feature_finish(ctx, kind, opts->gf_method, opts->gf_ratio, rng, sel, Hsel, nullptr))) return rc;
    }
    return MLH_OK;
}

// A whole frame in the LOOP form, enqueued: per outer iteration the match launch -- or the selection and the linearisation of the rows it kept, which leaves records;
// the pose then stays on the device, each selection starts from it -- and the loop launch. m_dev: the feature counts on the device (mlh_downsample_scan2map), or null.
static int enqueue_s2m_loop_frame(mlh_ctx *ctx, const mlh_solver_opts *opts, const double *pose, const int *m_dev, HostPublish *rec, unsigned long long seq)
{
    int rc = s2m_selects(opts) ? upload_pose(ctx, pose) : MLH_OK;
    std::mt19937 rng((uint32_t)opts->gf_seed);
    for (int outer = 0; outer < opts->max_outer && !rc; ++outer) {
        MatchArgs a = args_from_opts(opts, 3, 0), b;
        a.lm_max_it = opts->max_lm_iterations; a.m_dev = m_dev;
        if (s2m_selects(opts)) {
            if ((rc = s2m_select(ctx, opts, rng)) || (rc = linearize_launch(ctx, a))) return rc;
            b = s2m_loop_args(opts, outer, nullptr, rec, seq, nullptr);
        } else {
            if (outer == 0) a.init_pose = pose;
            a.warm = outer >= 1 && s2m_warm_applies(ctx);
            b = s2m_loop_args(opts, outer, pose, rec, seq, &a);
            if ((rc = match_launch(ctx, a))) return rc;
        }
        rc = lm_consume_launch(ctx, b);
    }
    return rc;
}

// LM iterations enqueued between two looks at the device-side verdict: six first (the mapper's solves converge in 5-7), then two at a time -- launches enqueued
// after convergence are no-ops, but each still costs a dispatch (profiles/r03_frame_timeline.txt: five of them behind a 7-iteration solve)
constexpr int S2M_FIRST_CHUNK = 6, S2M_NEXT_CHUNK = 2;

// One outer iteration's LM launches (FUSED_CHUNKS, or CONSUMER_CHUNKS: lmc) in chunks, each ending in a launch that publishes pose + `done` itself. The chunk
// after the one whose verdict the host is waiting for is already enqueued (into the other of the two pinned records: *chunk_idx counts on through the frame): when
// the verdict is "not yet" the GPU has gone on without the host's round trip (~15 us of idle stream per poll in profiles/r03_frame_cpp_timeline_*.txt), when it
// is "done" the chunk ahead is two launches that find `done` set and leave. *verdict: the last publication read.
static int s2m_lm_chunks(mlh_ctx *ctx, const mlh_solver_opts *opts, bool lmc, int outer, const double *pose, int *chunk_idx, HostPublish *verdict)
{
    struct Pending { unsigned long long seq; HostPublish *rec; } pend[2];
    int rc, n_pend = 0, enq = 0, lm_j = 0;
    const int lm_cap = opts->max_lm_iterations + (lmc ? 1 : 0);     // launches after which the loop has terminated by itself
    auto enqueue_chunk = [&](int count) -> int {
        for (int j = 0; j < count; ++j) {
            MatchArgs a = s2m_lm_args(opts, lmc, outer, lm_j++, pose, false);
            if (j == count - 1) {                   // the chunk's last launch publishes (no publication launch)
                if ((rc = publish_slot(ctx, &a.publish, &a.publish_seq, *chunk_idx))) return rc;
                pend[n_pend++] = Pending{a.publish_seq, a.publish};
            }
            if ((rc = lmc ? lm_consume_launch(ctx, a) : linearize_launch(ctx, a))) return rc;
        }
        ++*chunk_idx;
        enq += count;
        return MLH_OK;
    };
    if ((rc = enqueue_chunk(std::min(S2M_FIRST_CHUNK + (lmc ? 1 : 0), lm_cap)))) return rc;
    for (;;) {
        if (enq < lm_cap && n_pend < 2 && (rc = enqueue_chunk(std::min(S2M_NEXT_CHUNK, lm_cap - enq)))) return rc;
        // pinned-memory poll of the device-side `done` flag (no copy engine, no blocking wait)
        if ((rc = wait_published(ctx, pend[0].seq, *verdict, pend[0].rec))) return rc;
        pend[0] = pend[1]; --n_pend;
        if ((verdict->done & DONE_TERMINATED) || n_pend == 0) return MLH_OK;
    }
}

// One outer iteration's LM loop in the HOST_STEPPED form, behind a launch that left the rows' sums in the state
static int s2m_lm_host_stepped(mlh_ctx *ctx, const mlh_solver_opts *opts, int stat_slot)
{
    int rc = lm_begin_launch(ctx, opts->map_eig_thre, opts->max_lm_iterations, stat_slot);
    for (int it = 0, j_end = 0; !rc && it < opts->max_lm_iterations; it = j_end) {
        j_end = std::min(it + (it == 0 ? S2M_FIRST_CHUNK : S2M_NEXT_CHUNK), opts->max_lm_iterations);
        for (int j = it; j < j_end; ++j) {
            if ((rc = linearize_launch(ctx, args_from_opts(opts, 3, 1)))) return rc;
            if ((rc = lm_step_launch(ctx, opts->max_lm_iterations, -1))) return rc;
        }
        HostPublish hp;
        if ((rc = fetch_published(ctx, hp))) return rc;
        if (hp.done) break;      // (publish_kernel: SolverState::done)
    }
    return rc;
}

// A frame in a form with a launch per LM iteration (statistics, RCCL ranks, frames beyond the loop's gates, the re-solve of a frame whose loop was given up or
// outgrew its look-ahead): the host reads each loop's verdict before it enqueues the next outer iteration
static int s2m_polled_frame(mlh_ctx *ctx, double pose_inout[7], const mlh_solver_opts *opts, mlh_iter_stat *stats, S2mForm form)
{
    const bool in_launch = form != S2mForm::HOST_STEPPED, lmc = form == S2mForm::CONSUMER_CHUNKS;
    int rc;
    if (!in_launch && (rc = pose_cov_refuse_distributed(ctx, opts))) return rc;      // (HOST_STEPPED is a multi-rank form: s2m_form)
    // (every feature used, the LM begin in the match launch's own tail or its consumer: the pose goes in with the first launch's kernel arguments instead)
    if ((!in_launch || s2m_selects(opts)) && (rc = upload_pose(ctx, pose_inout))) return rc;
    HostPublish verdict;       // in_launch: the last chunk's publication already carries the pose
    int chunk_idx = 0;
    std::mt19937 rng((uint32_t)opts->gf_seed);
    for (int outer = 0; outer < opts->max_outer; ++outer) {
        const int stat_slot = stats ? outer : -1;
        if (s2m_selects(opts)) {
            if ((rc = s2m_select(ctx, opts, rng))) return rc;
            MatchArgs a = args_from_opts(opts, 3, 0);      // the evaluation of the rows it kept: the LM begin rides in its tail, or lm_begin_launch follows
            if (in_launch) { a.finish = TAIL_LM_BEGIN; a.stat_slot = stat_slot; a.lm_max_it = opts->max_lm_iterations; }
            rc = linearize_launch(ctx, a);
        } else if (in_launch) {
            MatchArgs a = s2m_begin_args(ctx, opts, lmc, outer, pose_inout, false);
            a.stat_slot = stat_slot;
            rc = match_launch(ctx, a);
        } else rc = match_launch(ctx, args_from_opts(opts, 3, 0));
        if (rc) return rc;
        if ((rc = in_launch ? s2m_lm_chunks(ctx, opts, lmc, outer, pose_inout, &chunk_idx, &verdict) : s2m_lm_host_stepped(ctx, opts, stat_slot))) return rc;
        if (stats && (rc = lm_finish_launch(ctx, outer))) return rc;     // fills the record's LM summary
    }
    if (in_launch && !stats) {
        if ((rc = prof_drain(ctx))) return rc;
        pose_copy(pose_inout, verdict.x);
        pose_cov_collect(ctx, opts, &verdict);
        return MLH_OK;
    }
    if ((rc = fetch_pose_and_stats(ctx, pose_inout, stats, opts->max_outer))) return rc;
    if (in_launch) pose_cov_collect(ctx, opts, &verdict);      // (the last chunk's publication: the loop's last launch, statistics or not)
    return MLH_OK;
}

// The synchronous solve. allow_loop = false (mlh_scan2map_end / mlh_downsample_scan2map, behind a loop that was given up): a launch-per-iteration form
static int scan2map_polled(mlh_ctx *ctx, double pose_inout[7], const mlh_solver_opts *opts_in, mlh_iter_stat *stats, bool allow_loop = true)
{
    if (!ctx || !pose_inout || !opts_in || opts_in->max_outer <= 0) return MLH_ERR_INVALID;
    const mlh_solver_opts opts_v = scan2map_opts(opts_in), *opts = &opts_v;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = pose_cov_refuse_distributed(ctx, opts);
    if (rc) return rc;
    pose_cov_open(ctx, opts);
    if ((rc = solver_begin(ctx, opts->max_outer))) return rc;
    if (!scan2map_has_maps(ctx)) {
        if (stats) std::memset(stats, 0, sizeof(mlh_iter_stat) * size_t(opts->max_outer));
        pose_cov_collect(ctx, opts, nullptr);
        return MLH_OK;
    }
    if (ctx->feat[0].m <= 0 || ctx->feat[1].m <= 0) return fail(ctx, MLH_ERR_STATE, "features_set is required for both kinds");
    const int tiles = feature_tiles(ctx);
    const S2mForm form = s2m_form(ctx, opts, stats != nullptr, allow_loop, 0, tiles);
    if (form != S2mForm::LOOP) return s2m_polled_frame(ctx, pose_inout, opts, stats, form);
    HostPublish *rec = nullptr;       // the whole frame is enqueued at once, the last loop launch publishes
    unsigned long long seq = 0;
    bool given_up = false;
    if ((rc = publish_slot(ctx, &rec, &seq, 0)) || (rc = enqueue_s2m_loop_frame(ctx, opts, pose_inout, nullptr, rec, seq))) return rc;
    HostPublish hp;
    if ((rc = collect_loop_pose(ctx, seq, rec, pose_inout, &given_up, &hp))) return rc;
    if (!given_up) { pose_cov_collect(ctx, opts, &hp); return MLH_OK; }
    // (a selection's draws start from opts->gf_seed again: the same frame)
    note_loop_given_up(ctx, 0, tiles);
    return s2m_polled_frame(ctx, pose_inout, opts, stats, s2m_form(ctx, opts, stats != nullptr, false, 0, tiles));
}

// ---- scan2MapOptimization, submitted and collected separately (the call the reference makes once per frame, pipelined like mlh_gn_solve_begin / _end).
// The host does not read the Levenberg-Marquardt loop's verdict between launches: per outer iteration the match launch (LM begin in its finish) and `lm_lookahead`
// LM launches are enqueued at once; launches behind the loop's termination find `done` on the device and leave (~3 us each). The last launch publishes pose and
// verdict. A frame whose LM loop needs MORE than the look-ahead is detected on the device (the next outer iteration finds the loop unterminated: lm_overflow; or the
// last loop is unterminated at the publication) -- its result is then not scan2MapOptimization's and is never returned as such: mlh_scan2map_end solves the frame
// again synchronously when that is sound (nothing restaged since the submission, no younger solve chained behind it), and says so otherwise.
static int scan2map_submit(mlh_ctx *ctx, const double *pose_in, const double *wodom_prev, const double *wodom_cur, const mlh_solver_opts *opts_in, int lm_lookahead)
{
    const mlh_solver_opts opts_v = scan2map_opts(opts_in), *opts = &opts_v;
    if (ctx->comm) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_scan2map_begin under an RCCL communicator: the sharded LM iteration there is a host-driven sequence of launches and collectives (use the mailbox communicator)");
    if (opts->gf_method != MLH_GF_WO) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_scan2map_begin with a good-feature selection: the selection loops run on the host between the launches (use mlh_scan2map)");
    if (opts->max_outer <= 0) return fail(ctx, MLH_ERR_INVALID, "max_outer must be positive");
    { const int crc = pose_cov_refuse_distributed(ctx, opts); if (crc) return crc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long seq = 0;
    HostPublish *rec = nullptr;
    mlh_ctx::SolveSlot *slot_p = nullptr;
    int rc = ctx->solves.admit(ctx, "two solves are already in flight: collect the older one first", &seq, &rec, &slot_p);
    if (rc) return rc;
    mlh_ctx::SolveSlot &slot = *slot_p;
    if ((rc = solver_begin(ctx, 0))) return rc;
    // everything that can refuse the frame is checked BEFORE the chain launch below rewrites the device pose: a refused mlh_scan2map_begin_chained leaves the
    // state as it found it, so the caller's retry does not apply transformUpdate / transformAssociateToMap twice
    const bool have_maps = scan2map_has_maps(ctx);
    if (have_maps && (ctx->feat[0].m <= 0 || ctx->feat[1].m <= 0)) return fail(ctx, MLH_ERR_STATE, "features_set is required for both kinds");
    slot.kind = mlh_ctx::SolveSlot::SCAN2MAP; slot.chained = pose_in == nullptr; slot.opts = *opts; slot.epoch = ctx->stage_epoch; slot.tainted = false;
    if (pose_in) pose_copy(slot.start, pose_in);
    else if ((rc = enqueue_chain_pose(ctx, wodom_prev, wodom_cur, rec))) return rc;
    // scan2MapOptimization runs only where scan2map_has_maps: otherwise the start pose is the result
    if (!have_maps) {
        slot.kind = mlh_ctx::SolveSlot::SCAN2MAP_NO_MAP;
        if (!pose_in) {          // chained: the start pose exists on the device only
            MLH_LAUNCH(publish_kernel, dim3(1), dim3(64), 0, ctx->stream, (const SolverState *)ctx->state.as<SolverState>(), rec, seq);
            MLH_HIP(ctx, hipGetLastError());
        }
        ctx->solves.commit(seq, -1);      // (nothing of it reads a map)
        return MLH_OK;
    }
    const int budget = std::max(1, std::min(lm_lookahead > 0 ? lm_lookahead : ctx->solves.lm_lookahead_auto, opts->max_lm_iterations));
    // Consumer-side (`budget + 1` launches run `budget` LM steps) unless the mailbox communicator is active -- or one launch per LM loop, which ends on the device
    // when the loop does: no budget, nothing to overflow. An explicit lm_lookahead keeps the launches it counts: it rules the loop out.
    const int tiles = feature_tiles(ctx);
    const S2mForm form = s2m_form(ctx, opts, false, lm_lookahead <= 0, 0, tiles);
    const bool loop = form == S2mForm::LOOP, lmc = form == S2mForm::CONSUMER_CHUNKS;
    slot.loop_tiles = loop ? tiles : 0;
    if (loop && (rc = enqueue_s2m_loop_frame(ctx, opts, pose_in, nullptr, rec, seq))) return rc;
    for (int outer = 0; !loop && outer < opts->max_outer; ++outer) {
        if ((rc = match_launch(ctx, s2m_begin_args(ctx, opts, lmc, outer, pose_in, true)))) return rc;
        const int n_launch = budget + (lmc ? 1 : 0);
        for (int j = 0; j < n_launch; ++j) {
            MatchArgs b = s2m_lm_args(opts, lmc, outer, j, pose_in, true);
            if (outer == opts->max_outer - 1 && j == n_launch - 1) { b.publish = rec; b.publish_seq = seq; }
            if ((rc = lmc ? lm_consume_launch(ctx, b) : linearize_launch(ctx, b))) return rc;
        }
    }
    ctx->solves.commit(seq, ctx->map_set_cur);
    return MLH_OK;
}

int mlh_scan2map_begin(mlh_ctx *ctx, const double pose_in[7], const mlh_solver_opts *opts, int lm_lookahead)
{
    if (!ctx || !pose_in || !opts) return MLH_ERR_INVALID;
    return scan2map_submit(ctx, pose_in, nullptr, nullptr, opts, lm_lookahead);
}

int mlh_scan2map_begin_chained(mlh_ctx *ctx, const double wodom_prev[7], const double wodom_cur[7], const mlh_solver_opts *opts, int lm_lookahead)
{
    if (!ctx || !wodom_prev || !wodom_cur || !opts) return MLH_ERR_INVALID;
    if (ctx->solves.submitted == 0) return fail(ctx, MLH_ERR_STATE, "mlh_scan2map_begin_chained continues from the pose a previous solve left on the device: submit the first frame with mlh_scan2map_begin");
    return scan2map_submit(ctx, nullptr, wodom_prev, wodom_cur, opts, lm_lookahead);
}

int mlh_scan2map_end(mlh_ctx *ctx, double pose_out[7], int32_t *status_out)
{
    if (!ctx || !pose_out) return MLH_ERR_INVALID;
    if (status_out) *status_out = 0;
    if (!ctx->solves.pending()) return fail(ctx, MLH_ERR_STATE, "no solve in flight (mlh_scan2map_begin)");
    const unsigned long long seq = ctx->solves.oldest();
    mlh_ctx::SolveSlot slot = ctx->solves.slot[seq & 1];
    if (slot.kind == mlh_ctx::SolveSlot::GN) return fail(ctx, MLH_ERR_STATE, "the oldest solve in flight was submitted with mlh_gn_solve_begin: collect it with mlh_gn_solve_end");
    HostPublish hp;
    int rc = MLH_OK;
    const bool solved = slot.kind == mlh_ctx::SolveSlot::SCAN2MAP;       // (otherwise the maps were too small to optimise against: the start pose is the result)
    if (solved || slot.chained) rc = wait_published(ctx, seq, hp, ctx->solves.record(seq));
    else { pose_copy(hp.x, slot.start); hp.done = DONE_TERMINATED; }
    ctx->solves.retire(seq);
    pose_cov_open(ctx, &slot.opts);
    if (rc) { ctx->solves.taint_successor(seq); return rc; }
    if (!ctx->solves.pending() && (rc = prof_drain(ctx))) return rc;
    const bool barrier_given_up = solved && (hp.done & DONE_GIVEN_UP);       // (a one-launch LM loop whose workgroups were not all resident: lm_loop_kernel)
    if (barrier_given_up) demote_loop_gate(ctx, 0, slot.loop_tiles);
    if (solved && !barrier_given_up) {
        // the next frame's automatic look-ahead: what this frame's longest LM loop used, plus two (consecutive mapper frames need about the same); a frame that
        // overflowed doubles it
        const int used = int(hp.xb[2][0]);
        const bool ok = (hp.done & DONE_TERMINATED) && !(hp.done & DONE_OVERFLOWED);
        ctx->solves.lm_lookahead_auto = ok ? std::max(3, used + 2) : std::min(2 * std::max(ctx->solves.lm_lookahead_auto, 4), slot.opts.max_lm_iterations);
    }
    if (!solved || ((hp.done & DONE_TERMINATED) && !(hp.done & (DONE_OVERFLOWED | DONE_GIVEN_UP)))) {
        pose_copy(pose_out, hp.x);
        if (slot.tainted) {
            // this frame was chained behind one whose LM loop outgrew its look-ahead: it began from that frame's UNFINISHED pose. Its own loops terminated, but the
            // result is not the mapper's; a solve chained behind THIS one inherits the mark.
            ctx->solves.taint_successor(seq);
            if (status_out) { *status_out = 3; return MLH_OK; }
            return fail(ctx, MLH_ERR_INCOMPLETE, "mlh_scan2map_end: the frame was chained behind one that did not finish inside its look-ahead (status 3) and status_out is NULL");
        }
        pose_cov_collect(ctx, &slot.opts, solved ? &hp : nullptr);
        return MLH_OK;
    }
    // the look-ahead was too short for this frame -- or its one-launch loop gave its barrier up
    pose_copy(pose_out, slot.chained ? hp.xb[1] : slot.start);
    if (!ctx->solves.pending() && ctx->stage_epoch == slot.epoch && !slot.tainted) {
        // nothing younger is chained behind it and the frame's maps and features are still the staged ones: solve it as mlh_scan2map would have (after a barrier
        // given up on: the second half of note_loop_given_up -- the gate came down above)
        if (status_out) *status_out = 2;
        if (barrier_given_up) ++ctx->caps.loop_fallbacks;
        return scan2map_polled(ctx, pose_out, &slot.opts, nullptr, !barrier_given_up);
    }
    // a younger solve chained behind this frame started from its unfinished pose: marked, and reported at ITS end (status 3)
    ctx->solves.taint_successor(seq);
    if (status_out) { *status_out = slot.tainted ? 3 : 1; return MLH_OK; }
    // the pose handed back is NOT a result, and this caller has no way to see that: a distinct return code instead of success
    return fail(ctx, MLH_ERR_INCOMPLETE, "mlh_scan2map_end: the frame did not finish inside its look-ahead and cannot be solved again here (status 1); status_out is NULL");
}

int mlh_scan2map(mlh_ctx *ctx, double pose_inout[7], const mlh_solver_opts *opts, mlh_iter_stat *stats)
{
    return scan2map_polled(ctx, pose_inout, opts, stats);
}

int mlh_scan2map_cov(mlh_ctx *ctx, double cov_out[36], double H_final_out[36])
{
    if (!ctx || !cov_out) return MLH_ERR_INVALID;
    switch (ctx->pose_cov.state) {
    case mlh_ctx::PoseCov::NONE: return fail(ctx, MLH_ERR_STATE, "mlh_scan2map_cov: no scan2map solve has been collected yet");
    case mlh_ctx::PoseCov::UNFLAGGED: return fail(ctx, MLH_ERR_STATE, "mlh_scan2map_cov: the most recently collected scan2map solve did not set MLH_FLAG_POSE_COV");
    case mlh_ctx::PoseCov::NOT_A_RESULT: return fail(ctx, MLH_ERR_STATE, "mlh_scan2map_cov: the most recently collected scan2map solve did not return a result (an error, or mlh_scan2map_end status 1 / 3)");
    case mlh_ctx::PoseCov::VALID: break;
    }
    std::memcpy(cov_out, ctx->pose_cov.cov, sizeof(ctx->pose_cov.cov));
    if (H_final_out) std::memcpy(H_final_out, ctx->pose_cov.H, sizeof(ctx->pose_cov.H));
    return MLH_OK;
}

// downsampleCurrentScan + scan2MapOptimization with no host read between them (include/mloam_hip.h)
int mlh_downsample_scan2map(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                            int intensity_offset_bytes, int mem, float leaf_surf, float leaf_corner, const double *ext_poses, const double *ext_covs,
                            int n_lidar, const double cov_measurement[9], int with_ua, double trace_threshold, double pose_inout[7],
                            const mlh_solver_opts *opts_in, int32_t *n_surf_features, int32_t *n_corner_features)
{
    if (!ctx || !pose_inout || !opts_in || !n_surf_features || !n_corner_features || opts_in->max_outer <= 0) return MLH_ERR_INVALID;
    const mlh_solver_opts opts_v = scan2map_opts(opts_in), *opts = &opts_v;      // (CHECK_FOV does not apply to scan2map: see scan2map_opts)
    ctx->thin_note.begin(n_surf, n_corner);
    { const int crc = pose_cov_refuse_distributed(ctx, opts); if (crc) return crc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    auto two_calls = [&]() -> int {
        int rc = mlh_downsample_current_scan_pair(ctx, surf_points, n_surf, corner_points, n_corner, stride_bytes, intensity_offset_bytes, mem, leaf_surf, leaf_corner,
                                                  ext_poses, ext_covs, n_lidar, cov_measurement, with_ua, trace_threshold, n_surf_features, n_corner_features);
        if (rc) return rc;
        return mlh_scan2map(ctx, pose_inout, opts, nullptr);
    };
    const bool fused_pair = is_fused_pair(ctx, surf_points, n_surf, corner_points, n_corner, stride_bytes, intensity_offset_bytes, mem);
    // the loop kernel's barrier wants every tile's workgroup resident: the BOUND's tiles, since the real count is not known here
    const int bound_tiles = tiles_of(n_surf) + tiles_of(n_corner);
    // The one-call form exists as a frame of loop launches only (gate 1: see s2m_form), for device-resident clouds thinned by the one pipeline that publishes its
    // counts from a kernel (the reference's member order on the device), every feature used, nothing in flight
    if (!fused_pair || !scan2map_has_maps(ctx) || s2m_selects(opts) || s2m_form(ctx, opts, false, true, 1, bound_tiles) != S2mForm::LOOP || ctx->solves.pending() ||
        ctx->vox_member_order != 1)
        return two_calls();
    int rc = solver_begin(ctx, 0);
    if (rc) return rc;
    pose_cov_open(ctx, opts);
    ++ctx->stage_epoch;
    for (int k = 0; k < 2; ++k) { ctx->feat[k].matched = false; ctx->feat[k].m = 0; }
    int m[2] = {0, 0};
    rc = downsample_current_scan_pair_run(ctx, surf_points, n_surf, ctx->fused.minmax[MLH_SURF], leaf_surf, corner_points, n_corner, ctx->fused.minmax[MLH_CORNER],
                                          leaf_corner, stride_bytes, intensity_offset_bytes, ext_poses, ext_covs, n_lidar, cov_measurement, with_ua, trace_threshold,
                                          &m[0], &m[1], true);
    if (rc == MLH_ERR_UNSUPPORTED) return two_calls();
    if (rc) return rc;
    auto stage_counts = [&](const int cnt[2]) { for (int k = 0; k < 2; ++k) ctx->feat[k].single_block(cnt[k], true); };
    if (m[0] >= 0) {                       // the thinning took a pipeline that waits for its counts anyway: the solve as usual
        stage_counts(m);
        *n_surf_features = m[0]; *n_corner_features = m[1];
        return mlh_scan2map(ctx, pose_inout, opts, nullptr);
    }
    const int bound[2] = {n_surf, n_corner};
    stage_counts(bound);                   // upper bounds: the launches' grids and the buffers; the kernels read the real counts
    HostPublish *rec = nullptr;
    unsigned long long seq = 0;
    if ((rc = publish_slot(ctx, &rec, &seq, 0))) return rc;
    rc = enqueue_s2m_loop_frame(ctx, opts, pose_inout, ctx->thin_counts_dev, rec, seq);
    double pose[7];
    bool given_up = false;
    HostPublish hp;
    if (!rc) rc = collect_loop_pose(ctx, seq, rec, pose, &given_up, &hp);
    // the counts were published by the thinning's last launch, long before the pose: no wait here in practice
    int real[2] = {0, 0};
    if (!rc && !(rc = host_wait_seq(ctx, ctx->thin_seq_host, ctx->thin_seq, ctx->stream, "the thinned feature counts did not arrive"))) {
        real[0] = ctx->thin_counts_host[0]; real[1] = ctx->thin_counts_host[1];
    }
    if (rc) { (void)hipStreamSynchronize(ctx->stream); for (int k = 0; k < 2; ++k) { ctx->feat[k].m = 0; ctx->feat[k].matched = false; } return rc; }
    stage_counts(real);
    *n_surf_features = real[0]; *n_corner_features = real[1];
    if ((rc = device_error_check(ctx))) return rc;
    if (real[0] <= 0 || real[1] <= 0) return fail(ctx, MLH_ERR_STATE, "features_set is required for both kinds");      // (what mlh_scan2map says of an empty kind)
    // given up (workgroups sized for the un-thinned clouds): the thinned sets are staged and counted by now -- the solve again, as the second of the two calls
    if (given_up) { note_loop_given_up(ctx, 1, bound_tiles); return scan2map_polled(ctx, pose_inout, opts, nullptr, false); }
    pose_copy(pose_inout, pose);
    pose_cov_collect(ctx, opts, &hp);      // (behind every error return: a call that failed leaves nothing for mlh_scan2map_cov)
    return MLH_OK;
}

int mlh_good_feature_matching(mlh_ctx *ctx, int kind, const double pose[7], int gf_method, double gf_ratio, uint64_t seed,
                              float min_match_sq_dis, float min_plane_dis, int32_t *sel_idx, int32_t *n_sel,
                              double sub_mat_H[36], uint8_t *matched)
{
    if (!ctx || kind < 0 || kind > 1 || !pose || !sel_idx || !n_sel || !sub_mat_H) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_state(ctx, 0);
    if (rc) return rc;
    if ((rc = upload_pose(ctx, pose))) return rc;
    std::mt19937 rng((uint32_t)seed);
    std::vector<int32_t> sel;
    if ((rc = good_feature_select(ctx, kind, gf_method, gf_ratio, rng, min_match_sq_dis, min_plane_dis, sel, sub_mat_H, matched))) return rc;
    *n_sel = (int32_t)sel.size();
    std::copy(sel.begin(), sel.end(), sel_idx);
    return MLH_OK;
}

}  // extern "C"
