// What belongs to the context itself (see include/mloam_hip.h for the contract): errors and the launch check, the profiler, the intake of a caller's records,
// what the device admits and the residency gates, create / destroy / synchronize, the setters and the context-free helpers. Every subsystem's entry points
// sit beside its kernels, in its own unit. Host logic only; no kernel is defined here.
#include "ctx.hpp"
#include "solve_host.hpp"
#include <cstdlib>
#include "dev_math.hpp"
#include <algorithm>
#include <cmath>
#include <new>
#include <random>

namespace mlh {

int fail(mlh_ctx *ctx, int code, const char *what, hipError_t e)
{
    if (ctx) {
        ctx->err = what ? what : "";
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}

bool launch_check_enabled()
{
    static const bool on = std::getenv("MLH_CHECK_LAUNCH") && std::atoi(std::getenv("MLH_CHECK_LAUNCH")) != 0;
    return on;
}
namespace { thread_local hipError_t t_launch_err = hipSuccess; thread_local const char *t_launch_kernel = nullptr; }
void launch_check(const char *kernel)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess && t_launch_err == hipSuccess) { t_launch_err = e; t_launch_kernel = kernel; }     // the FIRST failing launch is the one to name
}
hipError_t launch_check_take(const char **kernel)
{
    const hipError_t e = t_launch_err;
    if (kernel) *kernel = t_launch_kernel;
    t_launch_err = hipSuccess; t_launch_kernel = nullptr;
    return e;
}
int fail_launch(mlh_ctx *ctx, const char *kernel, hipError_t e)
{
    if (ctx) { ctx->err = "launch of "; ctx->err += kernel ? kernel : "?"; ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    return MLH_ERR_HIP;
}

static hipEvent_t prof_event(mlh_ctx *ctx)
{
    Profile &p = ctx->prof;
    if (!p.pool.empty()) { hipEvent_t e = p.pool.back(); p.pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void prof_begin(mlh_ctx *ctx, int id)
{
    if (!(ctx->prof.mask & (1u << id))) return;
    Profile::Pending pd;
    pd.id = id; pd.a = prof_event(ctx); pd.b = nullptr;
    (void)hipEventRecord(pd.a, ctx->stream);
    ctx->prof.pending.push_back(pd);
}

void prof_end(mlh_ctx *ctx, int id)
{
    if (!(ctx->prof.mask & (1u << id)) || ctx->prof.pending.empty()) return;
    Profile::Pending &pd = ctx->prof.pending.back();
    if (pd.id != id || pd.b) return;
    pd.b = prof_event(ctx);
    (void)hipEventRecord(pd.b, ctx->stream);
}

bool prof_kernel_events(mlh_ctx *ctx, int id, hipEvent_t *start, hipEvent_t *stop)
{
    if (!(ctx->prof.mask & (1u << id))) return false;
    if ((ctx->prof.seen[id]++ % ctx->prof.every) != 0) return false;
    Profile::Pending pd;
    pd.id = id; pd.a = prof_event(ctx); pd.b = prof_event(ctx);
    if (!pd.a || !pd.b) return false;
    ctx->prof.pending.push_back(pd);
    *start = pd.a; *stop = pd.b;
    return true;
}

void prof_collect(mlh_ctx *ctx)
{
    Profile &p = ctx->prof;
    for (auto &pd : p.pending) {
        if (pd.a && pd.b) {
            float ms = 0.f;
            if (hipEventSynchronize(pd.b) == hipSuccess && hipEventElapsedTime(&ms, pd.a, pd.b) == hipSuccess) {
                p.total_ms[pd.id] += ms;
                p.launches[pd.id] += 1;
            }
        }
        if (pd.a) p.pool.push_back(pd.a);
        if (pd.b) p.pool.push_back(pd.b);
    }
    p.pending.clear();
}

int records_check(mlh_ctx *ctx, const char *entry, const Records &r, bool allow_empty)
{
    const char *fault = records_fault(r, allow_empty);
    return fault ? fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": bad " + fault + " (records: stride a multiple of 4 >= 12, every field inside it)").c_str()) : MLH_OK;
}

int records_stage(mlh_ctx *ctx, const Records &r, DevBuf &staging, hipStream_t st, const unsigned char **dev, size_t at)
{
    *dev = r.p;
    if (r.mem != MLH_MEM_HOST || r.n == 0) return MLH_OK;
    MLH_HIP(ctx, staging.ensure(at + r.bytes()));
    *dev = staging.as<unsigned char>() + at;
    MLH_HIP(ctx, hipMemcpyAsync(staging.as<unsigned char>() + at, r.p, r.bytes(), hipMemcpyHostToDevice, st));
    return MLH_OK;
}

// validated records -> dst (float4, w as w_off says) and, with covd, the covariance diagonals; *dev_src (optional) = where the records were read from
int stage_points(mlh_ctx *ctx, const Records &r, int w_off, DevBuf &dst, DevBuf *covd, DevBuf &tmp, const unsigned char **dev_src)
{
    MLH_HIP(ctx, dst.ensure(sizeof(float4) * size_t(r.n)));
    if (covd) MLH_HIP(ctx, covd->ensure(sizeof(float4) * size_t(r.n)));
    const unsigned char *src;
    { const int rc = records_stage(ctx, r, tmp, ctx->stream, &src); if (rc) return rc; }
    pack_points_launch(ctx->stream, src, r.stride, r.n, w_off, 0.f, r.cov_off, dst.as<float4>(), covd ? covd->as<float4>() : nullptr);
    MLH_HIP(ctx, hipGetLastError());
    if (dev_src) *dev_src = src;
    return MLH_OK;
}

// ---------------------------------------------------------------- what the device admits (mlh_ctx::caps)
// "hex[,hex...]" -> CU-mask words (32 compute units each), cut to the device's size; an empty vector = no mask
std::vector<uint32_t> parse_cu_mask(const char *text, int cu_count)
{
    const int n_words = (cu_count + 31) / 32;
    std::vector<uint32_t> w(size_t(n_words), 0u);
    const char *p = text;
    bool any = false;
    for (int i = 0; i < n_words && p && *p; ++i) {
        char *rest = nullptr;
        w[size_t(i)] = uint32_t(std::strtoul(p, &rest, 16));
        any = any || rest != p;
        p = (rest && *rest == ',') ? rest + 1 : nullptr;
    }
    if (!any) return {};
    if (cu_count % 32) w.back() &= (1u << (cu_count % 32)) - 1u;      // (no bits beyond the device's last compute unit)
    return w;
}

// The first half of the device's compute units as mask words: the default of the staging stream (mlh_map_set_pair_overlapped)
std::vector<uint32_t> lower_half_cu_mask(int cu_count)
{
    std::vector<uint32_t> w(size_t((cu_count + 31) / 32), 0u);
    for (int cu = 0; cu < cu_count / 2; ++cu) w[size_t(cu / 32)] |= 1u << (cu % 32);
    return w;
}

static int query_device_caps(mlh_ctx *c)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return MLH_ERR_HIP;
    c->caps.cu_count = prop.multiProcessorCount;
    c->caps.cu_solver = prop.multiProcessorCount;
    int occ[2] = {0, 0}, occ_cov[2] = {0, 0}, occ_t = 0;
    if (lm_loop_occupancy(occ, occ_cov) != MLH_OK || track_loop_occupancy(&occ_t) != MLH_OK) return MLH_ERR_HIP;
    c->caps.blocks_per_cu[0] = occ[0]; c->caps.blocks_per_cu[1] = occ[1]; c->caps.blocks_per_cu[2] = occ_t;
    c->caps.blocks_per_cu_cov[0] = occ_cov[0]; c->caps.blocks_per_cu_cov[1] = occ_cov[1];
    unsigned long long us = 20000;                // a completed barrier takes ~2 us; another context's longest kernel in the way, < 1 ms
    if (const char *e = std::getenv("MLH_LOOP_TIMEOUT_US")) { const long long v = std::atoll(e); if (v > 0) us = (unsigned long long)v; }
    c->caps.loop_timeout_ticks = us * 100ull;     // wall_clock64(): 100 MHz
    return MLH_OK;
}

// Workgroups of the loop kernels that may stand behind one in-kernel barrier. Residency: blocks per compute unit = min(occupancy query, 8, 6) -- the query is
// known to answer one too many where the SCALAR registers bind (MI355X_MICROARCH.md "Residency and cooperative launch": admitted = min(API, 8,
// floor(800 / (ceil(sgpr / 16) * 16 + 16)))); the runtime does not report a kernel's scalar register count, so the rule is applied for the most a wavefront can
// have (112 -> 6; these kernels: 106 SGPRs, 218 VGPRs -> the query's 2 is the vector registers' and exact) -- x the compute units the solver's stream may use,
// less a margin of an eighth of them (at least 8 workgroups). What ELSE runs on those compute units -- the staging stream's index builds, other contexts'
// kernels -- is not subtracted: such kernels end by themselves, so they can delay an arrival by their own duration (tens of microseconds, far inside the
// barrier's time limit) but cannot keep a workgroup of ours out for good; only our own grid exceeding the device could (tests/test_gpu_residency.py: four
// contexts' whole frames at once, 1 024-thread sort workgroups in every wave slot, no barrier given up on). Redundancy: every workgroup sums every tile's record, which
// stops paying beyond GN_DEFER_MAX_TILES (measured, profiles/r04_feature_sweep.txt; the fused thinning + solve call sizes its grid for the un-thinned clouds and
// accepts up to FUSED_LOOP_MAX_TILES). The smaller of the two; MLH_LOOP_MAX_TILES lowers it further (0: never).
static void set_loop_gates(mlh_ctx *c)
{
    const int by_size[3] = {GN_DEFER_MAX_TILES, FUSED_LOOP_MAX_TILES, GN_DEFER_MAX_TILES};
    int by_hand = -1;
    if (const char *e = std::getenv("MLH_LOOP_MAX_TILES")) by_hand = std::max(0, std::atoi(e));
    auto gate_of = [&](int i, int blocks_per_cu) {
        const int per_cu = std::max(0, std::min(blocks_per_cu, 6));
        long long resident = (long long)per_cu * c->caps.cu_solver;
        resident = std::max(0ll, resident - std::max<long long>(c->caps.cu_solver / 8, 8));
        int gate = int(std::min<long long>(resident, by_size[i]));
        if (by_hand >= 0) gate = std::min(gate, by_hand);
        if (c->caps.loop_demoted[i] >= 0) gate = std::min(gate, c->caps.loop_demoted[i]);
        return gate;
    };
    for (int i = 0; i < 3; ++i) c->caps.loop_max_tiles[i] = gate_of(i, c->caps.blocks_per_cu[i]);
    // a frame that carries MLH_FLAG_POSE_COV ends in the loop kernel's covariance instantiation: both instantiations' workgroups have to be resident
    for (int i = 0; i < 2; ++i) c->caps.loop_max_tiles_cov[i] = std::min(c->caps.loop_max_tiles[i], gate_of(i, c->caps.blocks_per_cu_cov[i]));
}

// A loop kernel of kind `which` came back with its barrier given up on at `tiles` workgroups: that many are evidently not resident together here. Half of it from
// now on (a second failure halves again; 0 = the launch-per-iteration forms for good).
void demote_loop_gate(mlh_ctx *c, int which, int tiles)
{
    ++c->caps.loop_timeouts;
    const int cur = c->caps.loop_max_tiles[which];
    c->caps.loop_demoted[which] = std::min(cur, tiles) / 2;
    set_loop_gates(c);
}
bool loop_tiles_ok(const mlh_ctx *c, int which, int tiles, bool cov)
{
    return tiles > 0 && tiles <= ((cov && which < 2) ? c->caps.loop_max_tiles_cov : c->caps.loop_max_tiles)[which];
}
// The barrier of a one-launch loop was given up on (DONE_GIVEN_UP: its workgroups were not all resident at once beside whatever else runs here). Counted and the
// gate lowered; the caller then solves the frame again from the start pose it still holds through a launch-per-iteration form: same arithmetic, same pose bits, no
// residency requirement. (mlh_scan2map_end, which may have to hand the frame back instead, uses the pieces separately.)
void note_loop_given_up(mlh_ctx *ctx, int gate, int tiles) { demote_loop_gate(ctx, gate, tiles); ++ctx->caps.loop_fallbacks; }

}  // namespace mlh

using namespace mlh;

extern "C" {

const char *mlh_version(void) { return "mloam_hip 0.1 (gfx950)"; }

int mlh_create(mlh_ctx **out, int device_id)
{
    if (!out) return MLH_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return MLH_ERR_HIP;
    if (device_id < 0 || device_id >= count) return MLH_ERR_INVALID;
    if (hipSetDevice(device_id) != hipSuccess) return MLH_ERR_HIP;
    mlh_ctx *c = new (std::nothrow) mlh_ctx;
    if (!c) return MLH_ERR_NOMEM;
    c->device = device_id;
    if (const char *e = std::getenv("MLH_KNN_LANES")) c->knn_lanes_override = std::atoi(e);
    if (const char *e = std::getenv("MLH_KNN_WG_THREADS")) {
        const int v = std::atoi(e);
        if (v != 256 && v != 512 && v != 1024) { delete c; return MLH_ERR_INVALID; }
        c->knn_wg_override = v;
    }
    if (const char *e = std::getenv("MLH_GN_FIT_IN_SEARCH")) {
        if ((e[0] != '0' && e[0] != '1') || e[1] != '\0') { delete c; return MLH_ERR_INVALID; }
        c->gn_fit_in_search = e[0] - '0';
    }
    if (query_device_caps(c) != MLH_OK) { delete c; return MLH_ERR_HIP; }
    // the solver's stream: the whole device, or -- MLH_SOLVER_CU_MASK=<hex word>[,<hex word>...], bit i of word w = compute unit 32 w + i -- a part of it (a
    // deployment that keeps compute units for other work; the tests of the residency gates)
    std::vector<uint32_t> mask;
    if (const char *m = std::getenv("MLH_SOLVER_CU_MASK")) mask = parse_cu_mask(m, c->caps.cu_count);
    hipError_t se;
    if (!mask.empty()) {
        int bits = 0;
        for (uint32_t w : mask) bits += __builtin_popcount(w);
        if (bits <= 0) { delete c; return MLH_ERR_INVALID; }
        se = hipExtStreamCreateWithCUMask(&c->stream, uint32_t(mask.size()), mask.data());
        c->caps.cu_solver = bits; c->caps.solver_masked = true;
    } else se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) { delete c; return MLH_ERR_HIP; }
    set_loop_gates(c);
    *out = c;
    return MLH_OK;
}

int mlh_get_info(mlh_ctx *ctx, mlh_device_info *out)
{
    if (!ctx || !out) return MLH_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->cu_count = ctx->caps.cu_count; out->cu_solver = ctx->caps.cu_solver;
    for (int i = 0; i < 3; ++i) { out->loop_blocks_per_cu[i] = ctx->caps.blocks_per_cu[i]; out->loop_max_tiles[i] = ctx->caps.loop_max_tiles[i]; }
    out->scan_uploads_from_ahead = int32_t(ctx->ahead.used & 0x7fffffffull);
    out->loop_launches = ctx->caps.loop_launches; out->loop_timeouts = ctx->caps.loop_timeouts; out->loop_fallbacks = ctx->caps.loop_fallbacks;
    return MLH_OK;
}

void mlh_destroy(mlh_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // every stream runs dry before anything it may still use is let go of
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->ahead.cs) (void)hipStreamSynchronize(ctx->ahead.cs);
    prof_collect(ctx);
    for (auto e : ctx->prof.pool) (void)hipEventDestroy(e);
    comm_destroy(ctx);
    keyframes_release(ctx);
    if (ctx->handoff.ev_handover) (void)hipEventDestroy(ctx->handoff.ev_handover);
    for (int i = 0; i < 2; ++i) if (ctx->ev_set_built[i]) (void)hipEventDestroy(ctx->ev_set_built[i]);
    if (ctx->handoff.ev_reader) (void)hipEventDestroy(ctx->handoff.ev_reader);
    if (ctx->ahead.ev_arrived) (void)hipEventDestroy(ctx->ahead.ev_arrived);
    if (ctx->ahead.ev_consumed) (void)hipEventDestroy(ctx->ahead.ev_consumed);
    // The device and pinned blocks: every DevBuf / PinnedBuf member frees its own -- the device is set and every stream drained. The streams themselves go LAST, behind
    // the frees, as they always did for most of the memory. (With them destroyed first, the two programs that hold no other stream on the device -- the C++
    // framebench, scripts/soak_schedule.py -- did not end on the MI355X; in this order a process that creates, uses and destroys two contexts does.)
    hipStream_t streams[3] = {ctx->ahead.cs, ctx->stream2, ctx->stream};
    delete ctx;
    for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
}

const char *mlh_last_error(const mlh_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
void *mlh_stream(mlh_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int mlh_synchronize(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return device_error_check(ctx);
}

int mlh_profile_enable(mlh_ctx *ctx, int kernel_mask)
{
    if (!ctx) return MLH_ERR_INVALID;
    ctx->prof.mask = unsigned(kernel_mask) & ((1u << MLH_K_COUNT) - 1u);
    return MLH_OK;
}

int mlh_profile_sample(mlh_ctx *ctx, int every_n)
{
    if (!ctx || every_n < 1) return MLH_ERR_INVALID;
    ctx->prof.every = every_n;
    for (int i = 0; i < MLH_K_COUNT; ++i) ctx->prof.seen[i] = 0;
    return MLH_OK;
}

int mlh_profile_reset(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    for (int i = 0; i < MLH_K_COUNT; ++i) { ctx->prof.total_ms[i] = 0; ctx->prof.launches[i] = 0; }
    return MLH_OK;
}

int mlh_profile_get(mlh_ctx *ctx, int kernel_id, double *total_ms, long long *launches)
{
    if (!ctx || kernel_id < 0 || kernel_id >= MLH_K_COUNT) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    if (total_ms) *total_ms = ctx->prof.total_ms[kernel_id];
    if (launches) *launches = ctx->prof.launches[kernel_id];
    return MLH_OK;
}

void mlh_segment_params_default(mlh_segment_params *p)
{
    if (!p) return;
    p->vertical_scans = 16; p->horizon_scans = 1800; p->min_cluster_size = 30; p->segment_valid_point_num = 5; p->segment_valid_line_num = 3;
    p->segment_theta = 1.047f; p->roi_range = 1.0; p->segment_flag = 1;
}

int mlh_compound_pose_with_cov(const double pose_1[7], const double cov_1[36], const double pose_2[7], const double cov_2[36],
                               double pose_cp[7], double cov_cp[36])
{
    if (!pose_1 || !cov_1 || !pose_2 || !cov_2 || !pose_cp || !cov_cp) return MLH_ERR_INVALID;
    compound_pose_with_cov(pose_1, cov_1, pose_2, cov_2, pose_cp, cov_cp);
    return MLH_OK;
}

int mlh_set_extract_tie_order(mlh_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return MLH_ERR_INVALID;
    ctx->extract_tie_ref = mode;
    return MLH_OK;
}

int mlh_set_gn_schedule(mlh_ctx *ctx, int deferred_finish, int knn_warm_start, int final_in_successor)
{
    if (!ctx) return MLH_ERR_INVALID;
    if ((deferred_finish != 0 && deferred_finish != 1) || (knn_warm_start != 0 && knn_warm_start != 1) || (final_in_successor != 0 && final_in_successor != 1))
        return fail(ctx, MLH_ERR_INVALID, "schedule switches are 0 or 1");
    { const int frc = gn_flush_pending(ctx); if (frc) return frc; }
    ctx->gn_defer = deferred_finish;
    ctx->knn_warm = knn_warm_start;
    ctx->gn_final_defer = final_in_successor;
    return MLH_OK;
}

int mlh_set_voxel_member_order(mlh_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return MLH_ERR_INVALID;
    ctx->vox_member_order = mode;
    return MLH_OK;
}

int mlh_std_sort_permutation(mlh_ctx *ctx, const int32_t *keys, int n0, int n, int32_t *perm_out, int mode)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!keys || !perm_out || n <= 0 || n0 < 0 || n0 > n || (mode != 1 && mode != 2)) return fail(ctx, MLH_ERR_INVALID, "bad arguments");
    if (mode == 2) {
        host_std_sort_permutation(keys, 0, n0, perm_out);
        host_std_sort_permutation(keys, n0, n, perm_out);
        return MLH_OK;
    }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MLH_HIP(ctx, ctx->tmp.ensure(sizeof(int) * size_t(n) * 2));
    int *d_keys = ctx->tmp.as<int>(), *d_perm = d_keys + n;
    MLH_HIP(ctx, hipMemcpyAsync(d_keys, keys, sizeof(int) * size_t(n), hipMemcpyHostToDevice, ctx->stream));
    int rc = device_std_sort_by_key(ctx, d_keys, n0, n, d_perm);
    if (rc) return rc;
    MLH_HIP(ctx, hipMemcpyAsync(perm_out, d_perm, sizeof(int) * size_t(n), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return device_error_check(ctx);
}

void mlh_solver_opts_default(mlh_solver_opts *o)
{
    if (!o) return;
    o->min_match_sq_dis = 1.0f;
    o->min_plane_dis = 0.2f;
    o->huber_delta = 0.1;
    o->map_eig_thre = 100.0;
    o->cov_measurement_trace = 0.0075;
    o->flags = 0;
    o->max_outer = 2;
    o->max_lm_iterations = 30;
    o->gf_method = MLH_GF_WO;
    o->gf_ratio = 1.0;
    o->gf_seed = 0;
}

// ---------------------------------------------------------------- small host helpers
int mlh_pose_plus(const double x[7], const double delta[6], const double *V_update, double x_plus_delta[7])
{
    if (!x || !delta || !x_plus_delta) return MLH_ERR_INVALID;
    pose_plus(x, delta, V_update, x_plus_delta);
    return MLH_OK;
}

int mlh_eval_degeneracy(const double H[36], double eig_thre, double eigval[6], double V_update[36])
{
    if (!H || !eigval || !V_update) return MLH_ERR_INVALID;
    // cyclic Jacobi on the host (same procedure as the device kernel)
    double a[36], V[36];
    for (int i = 0; i < 36; ++i) a[i] = H[i];
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) V[i * 6 + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int i = 0; i < 6; ++i) { dg += a[i * 6 + i] * a[i * 6 + i]; for (int j = i + 1; j < 6; ++j) off += a[i * 6 + j] * a[i * 6 + j]; }
        if (off <= 1e-32 * dg || off == 0.0) break;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                double apq = a[p * 6 + q];
                if (apq == 0.0) continue;
                double theta = (a[q * 6 + q] - a[p * 6 + p]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) { double u = a[k * 6 + p], v = a[k * 6 + q]; a[k * 6 + p] = c * u - s * v; a[k * 6 + q] = s * u + c * v; }
                for (int k = 0; k < 6; ++k) { double u = a[p * 6 + k], v = a[q * 6 + k]; a[p * 6 + k] = c * u - s * v; a[q * 6 + k] = s * u + c * v; }
                for (int k = 0; k < 6; ++k) { double u = V[k * 6 + p], v = V[k * 6 + q]; V[k * 6 + p] = c * u - s * v; V[k * 6 + q] = s * u + c * v; }
            }
    }
    int order[6] = {0, 1, 2, 3, 4, 5};
    for (int i = 0; i < 5; ++i) for (int j = i + 1; j < 6; ++j) if (a[order[j] * 7] < a[order[i] * 7]) std::swap(order[i], order[j]);
    bool deg = false, stop = false;
    bool keep[6];
    for (int j = 0; j < 6; ++j) {
        eigval[j] = a[order[j] * 7];
        if (!stop && eigval[j] < eig_thre) { keep[j] = false; deg = true; } else { keep[j] = true; stop = true; }
    }
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            double s = 0.0;
            if (deg) { for (int j = 0; j < 6; ++j) if (keep[j]) s += V[r * 6 + order[j]] * V[c * 6 + order[j]]; }
            else s = (r == c) ? 1.0 : 0.0;
            V_update[r * 6 + c] = s;
        }
    return deg ? 1 : 0;
}

}  // extern "C"
