// The accumulated calibration features of the online extrinsic calibration on gfx950: the one-block factors
//   LidarOnlineCalibPlaneNormFactor::Evaluate   estimator/src/factor/lidar_online_calib_factor.hpp:35-62
//   LidarOnlineCalibEdgeFactor::Evaluate        estimator/src/factor/lidar_online_calib_factor.hpp:135-165
// that Estimator::optimizeMap builds from cumu_surf_map_features_[n] / cumu_corner_map_features_[n] on every N_CUMU_FEATURE-th frame (estimator.cpp:714-735,
// 762-780) and hands to the marginalisation as well (cpp:921-938, 960-977). With ESTIMATE_EXTRINSIC == 1 they are the only feature terms on the extrinsic of a
// LiDAR other than the reference one. The store lives in HBM across windows: a record is the factor table's (point[3], coeff[6], sqrt_info, f64) plus a type;
// 256 records form a tile and every tile belongs to ONE extrinsic, so a workgroup computes R(Q_ext), t_ext once.
//   calib_append_kernel   the valid correspondences of a match pass, packed in feature order behind the store's last tile (no host round trip)
//   calib_ne_kernel       one workgroup per tile, one lane per factor: residual and 1x6 row, Huber correction, the tile's 29 sums (21 upper-triangle
//                         products, 6 J^T r, cost, count) reduced per wavefront in registers and combined in wavefront order
//   calib_ne_add_kernel   one workgroup behind the window's assembly: per extrinsic the tiles' sums in tile order into its diagonal block and gradient rows
//                         (the sums stream through LDS; 29 threads add them sequentially)
//   calib_eval_kernel     per-factor residual and 1x7 row (host-staged stores; the tests' view of the factor)
// Fixed summation order everywhere, no atomics: identical bits run to run.
#include "ctx.hpp"
#include "dev_math.hpp"
#include "factor_dev.hpp"
#include "tile_group.hpp"
#include "wg_dev.hpp"

namespace mlh {

constexpr int CAL_OUT = 32;       // 21 + 6 + cost + count = 29, padded
constexpr int CAL_NSUM = 29;

// the workgroup's extrinsic: R (9, row-major), t (3), q (4, xyzw) -- written by one thread, read by all
__device__ __forceinline__ void calib_stage_ext(const double *pe, double *s_ext)
{
    qtorot(q4{pe[3], pe[4], pe[5], pe[6]}, s_ext);
    s_ext[9] = pe[0]; s_ext[10] = pe[1]; s_ext[11] = pe[2];
    s_ext[12] = pe[3]; s_ext[13] = pe[4]; s_ext[14] = pe[5]; s_ext[15] = pe[6];
}

// one factor at the staged extrinsic: residual and the six columns of its row, both times sqrt_info (hpp:35-62 / 135-165 term by term)
__device__ __forceinline__ void calib_factor(const double *tb, int type, const double *s_ext, double &r_out, double *J6)
{
    const double *R = s_ext;
    const d3 p{tb[0], tb[1], tb[2]};
    const double s = tb[9];
    const d3 rp = qrot(q4{s_ext[12], s_ext[13], s_ext[14], s_ext[15]}, p);       // Q_ext * point_
    const d3 lp{rp.x + s_ext[9], rp.y + s_ext[10], rp.z + s_ext[11]};
    d3 jt, jr;
    double res;
    if (type == 0) {
        const d3 w{tb[3], tb[4], tb[5]};
        res = (w.x * lp.x + w.y * lp.y + w.z * lp.z) + tb[6];
        jt = w;
        const d3 k = row_skew(rowmul(w, R), p);                     // w^T R [p]x
        jr = d3{-k.x, -k.y, -k.z};
    } else {
        const LineFront F = point_to_line(lp, d3{tb[3], tb[4], tb[5]}, d3{tb[6], tb[7], tb[8]});
        res = F.res;
        const d3 ed = row_skew(F.eta, F.de);                        // eta [lpa - lpb]x
        jt = d3{-ed.x, -ed.y, -ed.z};
        jr = row_skew(rowmul(ed, R), p);                            // eta [lpa - lpb]x R [p]x
    }
    r_out = s * res;
    J6[0] = s * jt.x; J6[1] = s * jt.y; J6[2] = s * jt.z; J6[3] = s * jr.x; J6[4] = s * jr.y; J6[5] = s * jr.z;
}

struct CalibNeArgs {
    const double *tab;      // slots x 10
    const int *type, *perm; // slots
    const int *tile_ext;    // tiles
    const int *tile_pos;    // tiles: the tile's rank in (extrinsic, tile) order = its row of `partial`
    const double *exts;     // n_ext x 7
    int n_ext;
    double huber_delta;
    double *partial;        // tiles x CAL_OUT
};

__global__ __launch_bounds__(256) void calib_ne_kernel(CalibNeArgs G)
{
    __shared__ double s_ext[16];
    __shared__ double s_w[4][CAL_OUT];
    const int tile = blockIdx.x, k = threadIdx.x, lane = k & 63, wave = k >> 6;
    if (k == 0) calib_stage_ext(G.exts + 7 * min(max(G.tile_ext[tile], 0), G.n_ext - 1), s_ext);
    __syncthreads();
    const size_t slot = size_t(tile) * CALIB_TILE + k;
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // 6 corrected columns, corrected residual, cost, count: zeros for padding
    if (G.perm[slot] >= 0) {
        double r, J[6];
        calib_factor(G.tab + slot * 10, G.type[slot], s_ext, r, J);
        double rho0, rho1;
        huber_correct(r * r, G.huber_delta, rho0, rho1);
        const double sc = sqrt(rho1);
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = J[c] * sc;
        v[6] = r * sc; v[7] = 0.5 * rho0; v[8] = 1.0;
    }
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 7; ++b) {
            // row a of the upper triangle (b < 6), then its J^T r entry (b == 6): outputs 0..20 are the products in row-major order, 21..26 the gradient
            const double sum = wave_sum(v[a] * v[b]);
            const int dst = b < 6 ? o++ : 21 + a;
            if (lane == 0) s_w[wave][dst] = sum;
        }
    { const double sum = wave_sum(v[7]); if (lane == 0) s_w[wave][27] = sum; }
    { const double sum = wave_sum(v[8]); if (lane == 0) s_w[wave][28] = sum; }
    __syncthreads();
    if (k < CAL_OUT) G.partial[size_t(G.tile_pos[tile]) * CAL_OUT + k] = k < CAL_NSUM ? ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k] : 0.0;
}

struct CalibAddArgs {
    const double *partial;              // n_tiles x CAL_OUT, rows sorted by (extrinsic, tile): calib_ne_kernel writes a tile's sums to its rank in that order
    const int *ext_start;               // rows of extrinsic e: ext_start[e] .. ext_start[e + 1]
    int n_tiles, n_frames, n_ext;
    double *ne;                         // D*D + D + 2: added to
};

// One workgroup behind the window's assembly. A thread that owned an output and fetched its tiles from HBM one after the other spent a memory latency per tile
// (0.74 ms for 2 980 tiles); here all 1024 threads stream the rows through LDS, 256 rows at a time and the next 256 already on their way in registers, and
// threads 0..28 add them IN ROW ORDER -- per extrinsic in tile order, onto what the assembly left -- so the sums are the sequential ones, bit for bit.
constexpr int CAL_STAGE = 256;          // rows per LDS stage: 64 KiB
__global__ __launch_bounds__(1024) void calib_ne_add_kernel(CalibAddArgs F)
{
    __shared__ double s_p[CAL_STAGE * CAL_OUT];
    const int t = threadIdx.x, D = 6 * (1 + F.n_frames + F.n_ext);
    const size_t n_all = size_t(F.n_tiles) * CAL_OUT;
    constexpr int PER = CAL_STAGE * CAL_OUT / 1024;                 // 8 doubles per thread and stage
    double reg[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) { const size_t q = size_t(t) + 1024 * size_t(j); reg[j] = q < n_all ? F.partial[q] : 0.0; }
    // the walking threads: o < 27 owns output o of the current extrinsic's block, 27 / 28 the cost and the count
    int e = -1, next = 0, a = 0, b = 0;
    size_t at = 0;
    double acc = 0.0;
    if (t < 21) { int left = t; while (left >= 6 - a) { left -= 6 - a; ++a; } b = a + left; }
    if (t == 27 || t == 28) { at = size_t(D) * D + D + (t - 27); acc = F.ne[at]; }
    for (int row0 = 0; row0 < F.n_tiles; row0 += CAL_STAGE) {
        __syncthreads();                                            // the previous stage has been walked
#pragma unroll
        for (int j = 0; j < PER; ++j) s_p[t + 1024 * j] = reg[j];
        __syncthreads();
        if (row0 + CAL_STAGE < F.n_tiles) {
            const size_t base = size_t(row0 + CAL_STAGE) * CAL_OUT;
#pragma unroll
            for (int j = 0; j < PER; ++j) { const size_t q = base + size_t(t) + 1024 * size_t(j); reg[j] = q < n_all ? F.partial[q] : 0.0; }
        }
        if (t < CAL_NSUM) {
            const int rows = min(CAL_STAGE, F.n_tiles - row0);
            int r = 0;
            while (r < rows) {
                int end = rows;
                if (t < 27) {
                    if (row0 + r == next) {                         // the rows of the next extrinsic that has any begin here
                        if (e >= 0) { F.ne[at] = acc; if (t < 21 && a != b) F.ne[at + size_t(b - a) * (D - 1)] = acc; }
                        do { ++e; } while (e < F.n_ext - 1 && F.ext_start[e + 1] == F.ext_start[e]);
                        next = F.ext_start[e + 1];
                        const int off = 6 * (1 + F.n_frames + e);
                        at = t < 21 ? size_t(off + a) * D + off + b : size_t(D) * D + off + (t - 21);
                        acc = F.ne[at];                             // the assembly left both triangles with the same bits: the upper entry stands for both
                    }
                    end = min(rows, next - row0);
                    if (end <= r) end = rows;                       // (lists that do not add up to n_tiles: never loop in place)
                }
                // one extrinsic's rows of this stage: sixteen LDS reads in flight, the additions in row order
                for (; r + 16 <= end; r += 16) {
                    double x[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) x[j] = s_p[(r + j) * CAL_OUT + t];
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc += x[j];
                }
                for (; r < end; ++r) acc += s_p[r * CAL_OUT + t];
            }
        }
    }
    if (t < 27 && e >= 0) { F.ne[at] = acc; if (t < 21 && a != b) F.ne[at + size_t(b - a) * (D - 1)] = acc; }
    if (t == 27 || t == 28) F.ne[at] = acc;
}

struct CalibEvalArgs {
    const double *tab;
    const int *type, *perm, *tile_ext;
    const double *exts;
    int n_ext;
    double *r, *J;          // n_given, n_given x 7 (J may be null): in the order the factors were given
};
__global__ __launch_bounds__(256) void calib_eval_kernel(CalibEvalArgs E)
{
    __shared__ double s_ext[16];
    const int tile = blockIdx.x, k = threadIdx.x;
    if (k == 0) calib_stage_ext(E.exts + 7 * min(max(E.tile_ext[tile], 0), E.n_ext - 1), s_ext);
    __syncthreads();
    const size_t slot = size_t(tile) * CALIB_TILE + k;
    const int i = E.perm[slot];
    if (i < 0) return;
    double r, J[6];
    calib_factor(E.tab + slot * 10, E.type[slot], s_ext, r, J);
    E.r[i] = r;
    if (E.J) {
#pragma unroll
        for (int c = 0; c < 6; ++c) E.J[size_t(i) * 7 + c] = J[c];
        E.J[size_t(i) * 7 + 6] = 0.0;
    }
}

// the valid correspondences of a match pass -> records behind the store's last tile (factor_dev.hpp: append_valid_matches), so a device-built store has more
// slots than factors. n_valid (one word, this kernel its only writer while it runs) counts what was appended.
struct CalibAppend {
    const float4 *feat;
    const Corr *corr;
    int m, type, base_slot, cap_slots;
    double *tab;
    int *types, *perm, *n_valid;
};
__global__ __launch_bounds__(1024) void calib_append_kernel(CalibAppend P)
{
    const int n = append_valid_matches(P.feat, P.corr, P.m, P.base_slot, P.cap_slots, P.tab, P.perm, [&](int slot) { P.types[slot] = P.type; });
    if (threadIdx.x == 0) *P.n_valid += n;
}

// ---- host side
static int calib_grow(mlh_ctx *ctx, int n_tiles_new)
{
    CalibStore &S = ctx->calib;
    hipStream_t st = ctx->stream;
    const size_t have = size_t(S.n_tiles) * CALIB_TILE, want = size_t(n_tiles_new) * CALIB_TILE;
    const hipError_t e = grow_factor_slots(S.tab, S.type, sizeof(int), S.perm, want, have, st);
    if (e != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc calibration store", e);
    return MLH_OK;
}

extern "C" int mlh_calib_add(mlh_ctx *ctx, int n, const int32_t *type, const double *points, const double *coeffs, const double *sqrt_info, const int32_t *ext_idx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    if (n <= 0 || !type || !points || !coeffs || !ext_idx) return fail(ctx, MLH_ERR_INVALID, "mlh_calib_add: bad arguments");
    for (int i = 0; i < n; ++i) if (ext_idx[i] < 0) return fail(ctx, MLH_ERR_INVALID, "mlh_calib_add: negative extrinsic index");
    CalibStore &S = ctx->calib;
    const TileGrouping G = tile_group(n, ext_idx, S.n_given);
    const size_t slots = size_t(G.n_tiles) * CALIB_TILE, base = size_t(S.n_tiles) * CALIB_TILE;
    std::vector<double> tab(slots * 10, 0.0);
    std::vector<int> types(slots, 0);
    if (!pack_factor_rows(n, type, points, coeffs, sqrt_info, G.slot_of.data(), tab.data(), types.data(), 1))
        return fail(ctx, MLH_ERR_INVALID, "mlh_calib_add: factor type must be 0 (plane) or 1 (edge)");
    { const int rc = calib_grow(ctx, S.n_tiles + G.n_tiles); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    MLH_HIP(ctx, hipMemcpyAsync(S.tab.as<double>() + base * 10, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(S.type.as<int>() + base, types.data(), sizeof(int) * slots, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemcpyAsync(S.perm.as<int>() + base, G.perm.data(), sizeof(int) * slots, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipStreamSynchronize(st));                // the staging vectors end with this call
    S.h_tile_ext.insert(S.h_tile_ext.end(), G.tile_key.begin(), G.tile_key.end());
    S.n_tiles += G.n_tiles; S.n_appends += 1; S.n_given += n; S.max_ext = std::max(S.max_ext, G.max_key); S.lists_n_ext = -1;
    return MLH_OK;
}

int calib_accumulate(mlh_ctx *ctx, int kind, int ext_idx)
{
    if (ext_idx < 0) return fail(ctx, MLH_ERR_INVALID, "mlh_calib_accumulate: negative extrinsic index");
    FeatSet &f = ctx->feat[kind];
    if (f.m <= 0 || !f.matched || f.n_blocks != 1) return fail(ctx, MLH_ERR_STATE, "mlh_calib_accumulate: a single-block match pass must have run for this kind");
    CalibStore &S = ctx->calib;
    hipStream_t st = ctx->stream;
    const int cap_tiles = (f.m + CALIB_TILE - 1) / CALIB_TILE;
    { const int rc = calib_grow(ctx, S.n_tiles + cap_tiles); if (rc) return rc; }
    if (!S.n_valid_dev.p) {
        MLH_HIP(ctx, S.n_valid_dev.ensure(sizeof(int)));
        MLH_HIP(ctx, hipMemsetAsync(S.n_valid_dev.p, 0, sizeof(int), st));
    }
    CalibAppend P;
    P.feat = f.pts.as<float4>(); P.corr = f.corr.as<Corr>(); P.m = f.m; P.type = kind;
    P.base_slot = S.n_tiles * CALIB_TILE; P.cap_slots = cap_tiles * CALIB_TILE;
    P.tab = S.tab.as<double>(); P.types = S.type.as<int>(); P.perm = S.perm.as<int>(); P.n_valid = S.n_valid_dev.as<int>();
    MLH_LAUNCH(calib_append_kernel, dim3(1), dim3(1024), 0, st, P);
    MLH_HIP(ctx, hipGetLastError());
    for (int t = 0; t < cap_tiles; ++t) S.h_tile_ext.push_back(ext_idx);
    S.n_tiles += cap_tiles; S.n_appends += 1; S.max_ext = std::max(S.max_ext, ext_idx); S.lists_n_ext = -1; S.device_built = true;
    return MLH_OK;
}

extern "C" int mlh_calib_use(mlh_ctx *ctx, int on)
{
    if (!ctx) return MLH_ERR_INVALID;
    ctx->calib.in_use = on != 0;
    return MLH_OK;
}

extern "C" int mlh_calib_clear(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    CalibStore &S = ctx->calib;
    if (S.n_valid_dev.p) MLH_HIP(ctx, hipMemsetAsync(S.n_valid_dev.p, 0, sizeof(int), ctx->stream));
    S.h_tile_ext.clear();
    S.n_tiles = 0; S.n_appends = 0; S.n_given = 0; S.max_ext = -1; S.lists_n_ext = -1; S.in_use = false; S.device_built = false;
    return MLH_OK;
}

extern "C" int mlh_calib_info(mlh_ctx *ctx, mlh_calib_store_info *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_calib_info: null output");
    CalibStore &S = ctx->calib;
    int n_dev = 0;
    if (S.device_built && S.n_valid_dev.p) {
        MLH_HIP(ctx, hipMemcpyAsync(&n_dev, S.n_valid_dev.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    out->n_appends = S.n_appends; out->n_tiles = S.n_tiles; out->n_slots = S.n_tiles * CALIB_TILE; out->n_valid = S.n_given + n_dev;
    out->max_ext = S.max_ext; out->in_use = S.in_use ? 1 : 0;
    return MLH_OK;
}

bool calib_active(const mlh_ctx *ctx) { return ctx->calib.in_use && ctx->calib.n_tiles > 0; }

// the tile -> extrinsic keys and every extrinsic's tile list on the device, for this extrinsic count
static int calib_sync_lists(mlh_ctx *ctx, int n_ext)
{
    CalibStore &S = ctx->calib;
    if (S.lists_n_ext == n_ext) return MLH_OK;
    std::vector<int> start, tiles;
    calib_ext_lists(S.h_tile_ext, n_ext, start, tiles);
    std::vector<int> all(S.h_tile_ext);
    all.insert(all.end(), start.begin(), start.end());
    std::vector<int> pos(tiles.size(), 0);                 // n_ext covers the store (calib_ne_prepare): `tiles` is a permutation of all tiles
    for (size_t k = 0; k < tiles.size(); ++k) pos[size_t(tiles[k])] = int(k);
    all.insert(all.end(), pos.begin(), pos.end());
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));       // an earlier launch may still read the lists this replaces
    MLH_HIP(ctx, S.lists.ensure(sizeof(int) * all.size()));
    MLH_HIP(ctx, hipMemcpyAsync(S.lists.p, all.data(), sizeof(int) * all.size(), hipMemcpyHostToDevice, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    S.lists_n_ext = n_ext;
    return MLH_OK;
}

int calib_ne_prepare(mlh_ctx *ctx, int n_ext)
{
    CalibStore &S = ctx->calib;
    if (n_ext <= S.max_ext) return fail(ctx, MLH_ERR_INVALID, "the extrinsics do not cover the largest extrinsic index of the calibration store");
    { const int rc = calib_sync_lists(ctx, n_ext); if (rc) return rc; }
    MLH_HIP(ctx, S.partial.ensure(sizeof(double) * CAL_OUT * size_t(S.n_tiles)));
    return MLH_OK;
}

void calib_ne_enqueue(mlh_ctx *ctx, const double *poses_dev, int n_frames, int n_ext, double huber_delta, double *ne_dev)
{
    CalibStore &S = ctx->calib;
    const int *lists = S.lists.as<int>();
    CalibNeArgs G;
    G.tab = S.tab.as<double>(); G.type = S.type.as<int>(); G.perm = S.perm.as<int>(); G.tile_ext = lists; G.tile_pos = lists + S.n_tiles + n_ext + 1;
    G.exts = poses_dev + 7 * size_t(1 + n_frames); G.n_ext = n_ext; G.huber_delta = huber_delta; G.partial = S.partial.as<double>();
    MLH_LAUNCH(calib_ne_kernel, dim3(S.n_tiles), dim3(256), 0, ctx->stream, G);
    CalibAddArgs F;
    F.partial = S.partial.as<double>(); F.ext_start = lists + S.n_tiles;
    F.n_tiles = S.n_tiles; F.n_frames = n_frames; F.n_ext = n_ext; F.ne = ne_dev;
    MLH_LAUNCH(calib_ne_add_kernel, dim3(1), dim3(1024), 0, ctx->stream, F);
}

extern "C" int mlh_calib_evaluate(mlh_ctx *ctx, const double *exts, int n_ext, double *residuals, double *jacobians)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    CalibStore &S = ctx->calib;
    if (S.device_built) return fail(ctx, MLH_ERR_STATE, "mlh_calib_evaluate: per-factor outputs need a store made by mlh_calib_add alone: a device-built one is padded");
    if (S.n_given <= 0) return fail(ctx, MLH_ERR_STATE, "mlh_calib_evaluate: the store is empty");
    if (!exts || !residuals || n_ext <= S.max_ext) return fail(ctx, MLH_ERR_INVALID, "mlh_calib_evaluate: the extrinsics do not cover the store's largest extrinsic index");
    { const int rc = calib_sync_lists(ctx, n_ext); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    const size_t n = size_t(S.n_given), ne7 = 7 * size_t(n_ext);
    MLH_HIP(ctx, S.eval.ensure(sizeof(double) * (ne7 + n + 7 * n)));
    double *d = S.eval.as<double>();
    MLH_HIP(ctx, hipMemcpyAsync(d, exts, sizeof(double) * ne7, hipMemcpyHostToDevice, st));
    CalibEvalArgs E;
    E.tab = S.tab.as<double>(); E.type = S.type.as<int>(); E.perm = S.perm.as<int>(); E.tile_ext = S.lists.as<int>();
    E.exts = d; E.n_ext = n_ext; E.r = d + ne7; E.J = jacobians ? d + ne7 + n : nullptr;
    MLH_LAUNCH(calib_eval_kernel, dim3(S.n_tiles), dim3(256), 0, st, E);
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipMemcpyAsync(residuals, E.r, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (jacobians) MLH_HIP(ctx, hipMemcpyAsync(jacobians, E.J, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipStreamSynchronize(st));
    return MLH_OK;
}

}  // namespace mlh

using namespace mlh;

extern "C" {

int mlh_calib_accumulate(mlh_ctx *ctx, int kind, const double rel_pose[7], int k_neigh, uint32_t flags, float min_match_sq_dis, float min_plane_dis, int ext_idx)
{
    if (!ctx || kind < 0 || kind > 1 || !rel_pose) return MLH_ERR_INVALID;
    if (k_neigh != 5 && k_neigh != 10) return fail(ctx, MLH_ERR_UNSUPPORTED, "N_NEIGH is 5 or 10");
    if (ext_idx < 0) return fail(ctx, MLH_ERR_INVALID, "mlh_calib_accumulate: negative extrinsic index");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = match_for_factors(ctx, kind, rel_pose, k_neigh, flags, min_match_sq_dis, min_plane_dis);      // as mlh_pure_odom_add_matches: the correspondences stay in HBM
    if (rc) return rc;
    ctx->map_read_unsynced = true;
    return calib_accumulate(ctx, kind, ext_idx);
}

}  // extern "C"
