// The mapper's keyframe store and the local map built from it, on the device (gfx950).
//
// saveKeyframe (estimator/src/lidarMapper/lidar_mapper_keyframe.cpp:641-683) keeps a keyframe's pose and its surf / corner clouds; of a stored point only
// xyz and intensity (the LiDAR id) are ever read again -- cloudUCTAssociateToMap recomputes the covariance (cpp:1143-1155) -- so the store holds float4
// records, the layout of FeatSet::pts, and a staged feature set is saved device to device.
// extractSurroundingKeyFrames (cpp:254-354) is restated as one pipeline per call:
//   host    the early returns, the radius search over the keyframe positions, the cache's erase / append bookkeeping, and the thinning of the cached
//           keyframes' positions (VoxelGridCovarianceMLOAM<PointI>, plain branch: a few hundred points at most);
//   kf_uct_kernel        cloudUCTAssociateToMap for EVERY (entering keyframe x kind) segment in one launch: per-segment keyframe pose, extrinsics and
//                        compound poses from one table (compound poses: host f64, compound_pose_with_cov), per-point body shared with
//                        point_uncertainty_kernel (uct_dev.hpp), so both are bit-identical;
//   scan + kf_compact_kernel / kf_count_kernel   the keep flags, scanned once over all segments, compact each segment into the range it reserved in the
//                        cache arena; the kept counts stay on the device;
//   kf_prefix_kernel + kf_gather_kernel          the selected entries, in the order of the position filter, appended to the pre-filter clouds (`+=`): their
//                        offsets from a device prefix over the kept counts, the clouds' bounds folded on the way;
//   voxel_filter_run x 2 the two covariance filters (MAP_SURF_RES / MAP_CORNER_RES), bounds known, counts left on the device.
// Host waits per call: two (the pre-filter lengths + bounds; the filtered counts) plus one for an arena that has to grow. Launches do not depend on the
// number of keyframes.
#include "ctx.hpp"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <array>
#include <cstddef>
#include "dev_math.hpp"
#include "uct_dev.hpp"

namespace mlh {

namespace {

constexpr int REC = 48;          // PointIWithCov record: x y z intensity cov_vec[6] cov_trace pad
constexpr int REC_F4 = REC / 16;

struct KfSeg {                   // one (keyframe x kind) cloud on its way into the cache
    long long src;               // first record in the store (float4)
    long long dst;               // first reserved record in the cache
    int begin, n;                // its points' range in the launch
    int par;                     // offset (doubles) of its keyframe's pose / compound poses in the parameter table
    int slot2;                   // 2 * slot + kind: where its kept count goes
};
struct KfGat {                   // one cached cloud to copy (gather into the pre-filter cloud, or arena compaction)
    long long src, dst;          // first record in the cache; first record of the destination (compaction only)
    int ub_begin;                // prefix of the reserved counts: the launch's threads [ub_begin, ub_begin + reserved)
    int slot2;
};
struct Meas { double m[9]; };

__device__ __forceinline__ int enc_f(float f) { const int b = __float_as_int(f); return b >= 0 ? b : b ^ 0x7fffffff; }   // order-preserving as int
inline float dec_f(int b) { const int v = b >= 0 ? b : b ^ 0x7fffffff; float f; std::memcpy(&f, &v, 4); return f; }

template <class T>
__device__ __forceinline__ int seg_of(const T *s, int n, int i, int T::*key)
{
    int lo = 0, hi = n - 1;        // last entry whose key <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s[mid].*key <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void kf_uct_kernel(const float4 *__restrict__ store, const KfSeg *__restrict__ segs, int nseg, const double *__restrict__ par,
                                                     int n_lidar, Meas meas, int with_ua, double trace_thr, int N, float4 *__restrict__ stage,
                                                     int *__restrict__ keep, int *__restrict__ keep2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const KfSeg s = segs[seg_of(segs, nseg, i, &KfSeg::begin)];
    const float4 p = store[s.src + (i - s.begin)];
    const double *gpose = par + s.par;                    // [gpose 7 | compound poses n_lidar x 7 | their covariances n_lidar x 36]; extrinsics at par[0]
    const UctPoint u = uct_point(par, gpose + 7, gpose + 7 + 7 * n_lidar, n_lidar, meas.m, with_ua, trace_thr, p.x, p.y, p.z, p.w);
    keep[i] = u.keep;
    keep2[i] = u.keep;
    if (!u.keep) return;
    float xyz[3];
    uct_to_map(gpose, p.x, p.y, p.z, xyz);
    float4 *o = stage + size_t(i) * REC_F4;
    o[0] = make_float4(xyz[0], xyz[1], xyz[2], p.w);
    o[1] = make_float4(u.c6[0], u.c6[1], u.c6[2], u.c6[3]);
    o[2] = make_float4(u.c6[4], u.c6[5], float(u.tr), 0.f);
}

__global__ __launch_bounds__(256) void kf_compact_kernel(const float4 *__restrict__ stage, const int *__restrict__ keep, const int *__restrict__ scan,
                                                         const KfSeg *__restrict__ segs, int nseg, int N, float4 *__restrict__ cache)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || !keep[i]) return;
    const KfSeg s = segs[seg_of(segs, nseg, i, &KfSeg::begin)];
    const size_t d = size_t(s.dst + (scan[i] - scan[s.begin])) * REC_F4;
#pragma unroll
    for (int k = 0; k < REC_F4; ++k) cache[d + k] = stage[size_t(i) * REC_F4 + k];
}

__global__ __launch_bounds__(256) void kf_count_kernel(const KfSeg *__restrict__ segs, int nseg, const int *__restrict__ scan, const int *__restrict__ total, int N,
                                                       int *__restrict__ cnt)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nseg) return;
    const KfSeg s = segs[t];
    const int e = s.begin + s.n;
    cnt[s.slot2] = s.n == 0 ? 0 : (e < N ? scan[e] : *total) - scan[s.begin];
}

// the arena's live ranges moved to the front of a fresh arena (kept records only)
__global__ __launch_bounds__(256) void kf_move_kernel(const float4 *__restrict__ from, const KfGat *__restrict__ g, int ng, int ub, const int *__restrict__ cnt,
                                                      float4 *__restrict__ to)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ub) return;
    const KfGat e = g[seg_of(g, ng, i, &KfGat::ub_begin)];
    const int local = i - e.ub_begin;
    if (local >= cnt[e.slot2]) return;
#pragma unroll
    for (int k = 0; k < REC_F4; ++k) to[size_t(e.dst + local) * REC_F4 + k] = from[size_t(e.src + local) * REC_F4 + k];
}

// one thread per kind: the selected entries' destinations in the pre-filter cloud (`+=` behind what is there) and its new length; a cloud the host
// knows to be empty starts from length 0 and empty bounds
__global__ void kf_prefix_kernel(const KfGat *__restrict__ g, int n0, int n1, const int *__restrict__ cnt, int *__restrict__ dstate, int reset0, int reset1,
                                 long long *__restrict__ gofs)
{
    const int k = threadIdx.x;
    if (k > 1) return;
    if (k == 0 ? reset0 : reset1) {
        dstate[k] = 0;
        for (int d = 0; d < 3; ++d) { dstate[2 + 6 * k + d] = INT_MAX; dstate[2 + 6 * k + 3 + d] = INT_MIN; }
    }
    long long base = dstate[k];
    const int lo = k == 0 ? 0 : n0, hi = k == 0 ? n0 : n0 + n1;
    for (int e = lo; e < hi; ++e) { gofs[e] = base; base += cnt[g[e].slot2]; }
    dstate[k] = int(base);
}

__global__ __launch_bounds__(256) void kf_gather_kernel(const float4 *__restrict__ cache, const KfGat *__restrict__ g, int n0, int n1, int ub0, int ub1,
                                                        const int *__restrict__ cnt, const long long *__restrict__ gofs, float4 *__restrict__ pre0,
                                                        float4 *__restrict__ pre1, int *__restrict__ dstate)
{
    const int k = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ng = k == 0 ? n0 : n1, ub = k == 0 ? ub0 : ub1;
    const KfGat *gk = g + (k == 0 ? 0 : n0);
    const long long *ok = gofs + (k == 0 ? 0 : n0);
    float4 *pre = k == 0 ? pre0 : pre1;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool any = false;
    if (ng > 0 && i < ub) {
        const int e = seg_of(gk, ng, i, &KfGat::ub_begin);
        const int local = i - gk[e].ub_begin;
        if (local < cnt[gk[e].slot2]) {
            const size_t s = size_t(gk[e].src + local) * REC_F4, d = size_t(ok[e] + local) * REC_F4;
            const float4 r0 = cache[s];
            pre[d] = r0; pre[d + 1] = cache[s + 1]; pre[d + 2] = cache[s + 2];
            mn[0] = mx[0] = r0.x; mn[1] = mx[1] = r0.y; mn[2] = mx[2] = r0.z;
            any = true;
        }
    }
    // the bounds of what this workgroup appended, folded into the cloud's (min / max are exact: any order gives the same result)
    __shared__ float red[6][4];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn[d] = fminf(mn[d], __shfl_xor(mn[d], off)); mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off)); }
    }
    const int any_wg = __syncthreads_or(any ? 1 : 0);
    if ((threadIdx.x & 63) == 0) for (int d = 0; d < 3; ++d) { red[d][threadIdx.x >> 6] = mn[d]; red[3 + d][threadIdx.x >> 6] = mx[d]; }
    __syncthreads();
    if (threadIdx.x == 0 && any_wg) {
        for (int d = 0; d < 3; ++d) {
            const float a = fminf(fminf(red[d][0], red[d][1]), fminf(red[d][2], red[d][3]));
            const float b = fmaxf(fmaxf(red[3 + d][0], red[3 + d][1]), fmaxf(red[3 + d][2], red[3 + d][3]));
            atomicMin(dstate + 2 + 6 * k + d, enc_f(a));
            atomicMax(dstate + 2 + 6 * k + 3 + d, enc_f(b));
        }
    }
}

// VoxelGridCovarianceMLOAM<PointI>::filter, plain branch (voxel_grid_covariance_mloam_impl.hpp:68-130, 180-260, 392-420), over the cached keyframes'
// positions: which entry each output point names (the intensity of its voxel's last member in std::sort order), in output order (ascending voxel index)
std::vector<int> thin_positions(const std::vector<std::array<float, 3>> &pos, float leaf)
{
    const int m = int(pos.size());
    std::vector<int> out;
    if (m == 0) return out;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (const auto &p : pos) for (int d = 0; d < 3; ++d) { mn[d] = std::min(mn[d], p[d]); mx[d] = std::max(mx[d], p[d]); }
    const float inv = 1.0f / leaf;
    long long ext[3];
    for (int d = 0; d < 3; ++d) ext[d] = (long long)((mx[d] - mn[d]) * inv) + 1;
    if (ext[0] * ext[1] * ext[2] > (long long)INT_MAX) {           // "Leaf size is too small": the input comes back unchanged
        for (int j = 0; j < m; ++j) out.push_back(j);
        return out;
    }
    int min_b[3], div_b[3];
    for (int d = 0; d < 3; ++d) {
        min_b[d] = int(std::floor(mn[d] * inv));
        div_b[d] = int(std::floor(mx[d] * inv)) - min_b[d] + 1;
    }
    const int mul[3] = {1, div_b[0], div_b[0] * div_b[1]};
    struct IdxPt {
        unsigned int idx, cloud_point_index;
        bool operator<(const IdxPt &o) const { return idx < o.idx; }      // the voxel index only, as PCL's cloud_point_index_idx
    };
    std::vector<IdxPt> iv;
    iv.reserve(size_t(m));
    for (int j = 0; j < m; ++j) {
        int ijk[3];
        for (int d = 0; d < 3; ++d) ijk[d] = int(std::floor(pos[size_t(j)][d] * inv) - float(min_b[d]));
        iv.push_back(IdxPt{unsigned(ijk[0] * mul[0] + ijk[1] * mul[1] + ijk[2] * mul[2]), unsigned(j)});
    }
    std::sort(iv.begin(), iv.end());
    for (size_t a = 0; a < iv.size();) {
        size_t b = a + 1;
        while (b < iv.size() && iv[b].idx == iv[a].idx) ++b;
        out.push_back(int(iv[b - 1].cloud_point_index));          // centroid[3] = the last member's intensity = its position in the cache
        a = b;
    }
    return out;
}

template <class T> size_t put(std::vector<unsigned char> &h, const T *p, size_t n)
{
    size_t off = (h.size() + 15) & ~size_t(15);
    h.resize(off + sizeof(T) * n);
    if (n && p) std::memcpy(h.data() + off, p, sizeof(T) * n);
    return off;
}

bool bad_pose(const double *p) { for (int i = 0; i < 7; ++i) if (!std::isfinite(p[i])) return true; return false; }

}  // namespace

void keyframes_release(mlh_ctx *ctx)
{
    KfStore &K = ctx->kf;
    K.keys.clear(); K.entries.clear(); K.free_slots.clear(); K.n_slots = 0; K.pts_used = 0; K.cache_used = 0;
    K.pts.release(); K.cache.release(); K.cache_tmp.release(); K.cnt.release(); K.dstate.release(); K.tab.release();
    K.stage.release(); K.keep.release(); K.scan.release();
    for (int k = 0; k < 2; ++k) { K.pre[k].release(); K.flt[k].release(); K.pre_n[k] = K.flt_n[k] = 0; }
    std::vector<unsigned char>().swap(K.htab);
}

// saveKeyframe's store (cpp:664-681): the pose, the f32 position, the two clouds appended to the store. src[k] are device float4 records (staged) or
// caller records packed on the way in.
static int keyframe_store(mlh_ctx *ctx, const double pose[7], const double cov[36], const void *const src[2], const int n[2], int stride, int ioff, int mem,
                          bool packed, int32_t *key_out)
{
    KfStore &K = ctx->kf;
    hipStream_t st = ctx->stream;
    const size_t add = size_t(n[0]) + size_t(n[1]);
    if (K.pts_used + add > size_t(INT_MAX)) return fail(ctx, MLH_ERR_NOMEM, "keyframe store: more than 2^31 stored points");
    MLH_HIP(ctx, K.pts.grow(sizeof(float4) * (K.pts_used + add + 1), sizeof(float4) * K.pts_used, st));
    KfStore::Key key;
    for (int i = 0; i < 7; ++i) key.pose[i] = pose[i];
    for (int i = 0; i < 36; ++i) key.cov[i] = cov[i];
    for (int d = 0; d < 3; ++d) key.pos[d] = float(pose[d]);                 // pose_3d.x = pose_wmap_curr.t_[0] (PointI: f32)
    float4 *dst = K.pts.as<float4>();
    for (int k = 0; k < 2; ++k) {
        key.off[k] = K.pts_used; key.n[k] = n[k];
        if (n[k] > 0) {
            if (packed) {
                MLH_HIP(ctx, hipMemcpyAsync(dst + K.pts_used, src[k], sizeof(float4) * size_t(n[k]), hipMemcpyDeviceToDevice, st));
            } else {
                const unsigned char *s;
                { const int rc = records_stage(ctx, records_of(src[k], stride, n[k], mem), ctx->tmp, st, &s); if (rc) return rc; }
                pack_points_launch(st, s, stride, n[k], ioff, 0.f, -1, dst + K.pts_used, nullptr);
            }
            K.pts_used += size_t(n[k]);
        }
    }
    MLH_HIP(ctx, hipGetLastError());
    if (mem == MLH_MEM_HOST && !packed) MLH_HIP(ctx, hipStreamSynchronize(st));     // the caller's clouds have been read when the call returns
    K.keys.push_back(key);
    if (key_out) *key_out = int32_t(K.keys.size() - 1);
    return MLH_OK;
}

int keyframe_save_run(mlh_ctx *ctx, const double pose[7], const double cov[36], const void *surf, int n_surf, const void *corner, int n_corner, int stride,
                      int ioff, int mem, int32_t *key_out)
{
    if (!pose || !cov || ioff < 0 || bad_pose(pose)) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframe_save: bad arguments");
    const void *src[2] = {surf, corner};
    const int n[2] = {n_surf, n_corner};
    for (int k = 0; k < 2; ++k) { const int rc = records_check(ctx, "mlh_keyframe_save", records_of(src[k], stride, n[k], mem, ioff), true); if (rc) return rc; }
    return keyframe_store(ctx, pose, cov, src, n, stride, ioff, mem, false, key_out);
}

int keyframe_save_staged_run(mlh_ctx *ctx, const double pose[7], const double cov[36], int32_t *key_out)
{
    if (!pose || !cov || bad_pose(pose)) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframe_save_staged: bad arguments");
    const void *src[2];
    int n[2];
    for (int k = 0; k < 2; ++k) {
        const FeatSet &f = ctx->feat[k];
        if (f.n_blocks != 1) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_keyframe_save_staged: the staged feature set is split into pose blocks");
        src[k] = f.pts.p; n[k] = f.m;
    }
    return keyframe_store(ctx, pose, cov, src, n, 16, 12, MLH_MEM_DEVICE, true, key_out);
}

int keyframes_reset_run(mlh_ctx *ctx)
{
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    keyframes_release(ctx);
    return MLH_OK;
}

int local_map_clear_run(mlh_ctx *ctx)
{
    // clearCloud (cpp:921-927): the four map clouds only; the cache and the store stay
    KfStore &K = ctx->kf;
    for (int k = 0; k < 2; ++k) K.pre_n[k] = K.flt_n[k] = 0;
    return MLH_OK;
}

int local_map_assemble_run(mlh_ctx *ctx, const double pose_cur[7], const double *ext_poses, const double *ext_covs, int n_lidar, const mlh_local_map_opts *o,
                           int32_t *rebuilt, int32_t *n_surf_ds, int32_t *n_corner_ds, int32_t *kf_ids_out, int32_t *n_ids)
{
    if (!pose_cur || !ext_poses || !o || !rebuilt || !n_surf_ds || !n_corner_ds || n_lidar <= 0 || n_lidar > 16 || bad_pose(pose_cur))
        return fail(ctx, MLH_ERR_INVALID, "mlh_local_map_assemble: bad arguments");
    const auto pos_finite = [](float v) { return std::isfinite(v) && v > 0.f; };
    if (!std::isfinite(o->surrounding_kf_radius) || o->surrounding_kf_radius < 0.f || !pos_finite(o->map_sur_kf_res) || !pos_finite(o->leaf_surf) ||
        !pos_finite(o->leaf_corner) || std::isnan(o->trace_threshold))
        return fail(ctx, MLH_ERR_INVALID, "mlh_local_map_assemble: radius, resolutions and leaves must be finite (radius >= 0, the others > 0)");
    if (o->with_ua && !ext_covs) return fail(ctx, MLH_ERR_INVALID, "mlh_local_map_assemble: with_ua needs the extrinsic covariances");
    KfStore &K = ctx->kf;
    hipStream_t st = ctx->stream;
    *rebuilt = 0;
    if (n_ids) *n_ids = 0;
    *n_surf_ds = K.flt_n[0]; *n_corner_ds = K.flt_n[1];
    // cpp:256-261
    if (K.keys.empty()) return MLH_OK;
    if (K.flt_n[0] != 0 && K.flt_n[1] != 0) return MLH_OK;
    *rebuilt = 1;

    // radiusSearch around the f32 position (cpp:263-272): nearest first, equal distances by index
    const float cx = float(pose_cur[0]), cy = float(pose_cur[1]), cz = float(pose_cur[2]), r = o->surrounding_kf_radius;
    std::vector<std::pair<float, int>> hit;
    for (size_t i = 0; i < K.keys.size(); ++i) {
        const float dx = K.keys[i].pos[0] - cx, dy = K.keys[i].pos[1] - cy, dz = K.keys[i].pos[2] - cz, d2 = dx * dx + dy * dy + dz * dz;
        if (d2 <= r * r) hit.emplace_back(d2, int(i));
    }
    std::sort(hit.begin(), hit.end());
    std::vector<char> in_radius(K.keys.size(), 0);
    for (const auto &h : hit) in_radius[size_t(h.second)] = 1;
    // erase what left the radius, keeping the order of the rest (cpp:274-293)
    {
        std::vector<KfStore::Entry> kept;
        for (const auto &e : K.entries) {
            if (in_radius[size_t(e.id)]) kept.push_back(e);
            else K.free_slots.push_back(e.slot);
        }
        K.entries.swap(kept);
    }
    std::vector<char> cached(K.keys.size(), 0);
    for (const auto &e : K.entries) cached[size_t(e.id)] = 1;
    std::vector<int> entering;
    for (const auto &h : hit) if (!cached[size_t(h.second)]) entering.push_back(h.second);

    // reserve the entering clouds' ranges in the cache arena (compacting the live ranges into a fresh arena when the tail is out of room)
    size_t need = 0, live = 0;
    for (int id : entering) need += size_t(K.keys[size_t(id)].n[0]) + size_t(K.keys[size_t(id)].n[1]);
    for (const auto &e : K.entries) live += size_t(e.n[0]) + size_t(e.n[1]);
    if (K.cache_used + need > size_t(INT_MAX) / 2 || live + need > size_t(INT_MAX) / 2) return fail(ctx, MLH_ERR_NOMEM, "keyframe cache: too many points");
    std::vector<KfGat> moves;
    int ub_move = 0;
    const bool compact = (K.cache_used + need) * REC > K.cache.cap;
    if (compact) {
        for (auto &e : K.entries)
            for (int k = 0; k < 2; ++k) {
                if (e.n[k] > 0) { moves.push_back(KfGat{(long long)e.off[k], (long long)(ub_move), ub_move, 2 * e.slot + k}); }
                e.off[k] = size_t(ub_move);
                ub_move += e.n[k];
            }
        K.cache_used = size_t(ub_move);
    }
    // slots of the entering entries
    std::vector<KfSeg> segs;
    std::vector<double> par(size_t(n_lidar) * 7);
    for (int l = 0; l < 7 * n_lidar; ++l) par[size_t(l)] = ext_poses[l];
    int N = 0;
    for (int id : entering) {
        const KfStore::Key &key = K.keys[size_t(id)];
        KfStore::Entry e;
        e.id = id;
        if (!K.free_slots.empty()) { e.slot = K.free_slots.back(); K.free_slots.pop_back(); }
        else e.slot = K.n_slots++;
        const int p = int(par.size());
        par.resize(par.size() + 7 + size_t(n_lidar) * 43, 0.0);
        for (int i = 0; i < 7; ++i) par[size_t(p + i)] = key.pose[i];
        if (o->with_ua)
            for (int l = 0; l < n_lidar; ++l)       // compoundPoseWithCov(pose_global, pose_ext[n]) (cpp:1122-1126)
                compound_pose_with_cov(key.pose, key.cov, ext_poses + 7 * l, ext_covs + 36 * l, &par[size_t(p + 7 + 7 * l)], &par[size_t(p + 7 + 7 * n_lidar + 36 * l)]);
        for (int k = 0; k < 2; ++k) {
            e.off[k] = K.cache_used; e.n[k] = key.n[k];
            segs.push_back(KfSeg{(long long)key.off[k], (long long)K.cache_used, N, key.n[k], p, 2 * e.slot + k});
            K.cache_used += size_t(key.n[k]);
            N += key.n[k];
        }
        K.entries.push_back(e);
    }
    std::vector<KfSeg> segs_nz;
    for (const auto &s : segs) if (s.n > 0) segs_nz.push_back(s);

    // thinning of the cached keyframes' positions, intensity = position in the cache (cpp:312-327) -> the entries whose clouds are appended, in that order
    std::vector<std::array<float, 3>> pos;
    for (const auto &e : K.entries) pos.push_back({K.keys[size_t(e.id)].pos[0], K.keys[size_t(e.id)].pos[1], K.keys[size_t(e.id)].pos[2]});
    const std::vector<int> sel = thin_positions(pos, o->map_sur_kf_res);
    std::vector<KfGat> gat;
    int ub[2] = {0, 0}, ng[2] = {0, 0};
    for (int k = 0; k < 2; ++k)
        for (int j : sel) {
            const KfStore::Entry &e = K.entries[size_t(j)];
            if (e.n[k] == 0) continue;
            gat.push_back(KfGat{(long long)e.off[k], 0, ub[k], 2 * e.slot + k});
            ub[k] += e.n[k];
            ++ng[k];
        }
    if (kf_ids_out) for (size_t j = 0; j < sel.size(); ++j) kf_ids_out[j] = K.entries[size_t(sel[j])].id;
    if (n_ids) *n_ids = int32_t(sel.size());

    // buffers (growth of a store / arena / cloud that holds data waits for its copy: the one exception to the two waits)
    MLH_HIP(ctx, K.cnt.grow(sizeof(int) * size_t(2 * K.n_slots + 2), K.cnt.cap, st));
    MLH_HIP(ctx, K.dstate.ensure(sizeof(int) * 20));
    MLH_HIP(ctx, K.h_pin.ensure(sizeof(int) * 32));
    int *h_pin = K.h_pin.as<int>();
    if (compact) MLH_HIP(ctx, K.cache_tmp.ensure(size_t(REC) * std::max<size_t>(2 * K.cache_used, 1024)));   // live + entering, with room for turnover
    for (int k = 0; k < 2; ++k) MLH_HIP(ctx, K.pre[k].grow(size_t(REC) * (size_t(K.pre_n[k]) + size_t(ub[k]) + 1), size_t(REC) * size_t(K.pre_n[k]), st));
    if (N > 0) {
        MLH_HIP(ctx, K.stage.ensure(size_t(REC) * size_t(N)));
        MLH_HIP(ctx, K.keep.ensure(sizeof(int) * size_t(N)));
        MLH_HIP(ctx, K.scan.ensure(sizeof(int) * size_t(N + 1)));
    }
    // one upload of every table of the call
    std::vector<unsigned char> &h = K.htab;
    h.clear();
    const size_t o_par = put(h, par.data(), par.size());
    const size_t o_seg = put(h, segs.data(), segs.size());
    const size_t o_snz = put(h, segs_nz.data(), segs_nz.size());
    const size_t o_mov = put(h, moves.data(), moves.size());
    const size_t o_gat = put(h, gat.data(), gat.size());
    const size_t o_ofs = put(h, static_cast<const long long *>(nullptr), gat.size());
    MLH_HIP(ctx, K.tab.ensure(h.size() + 16));
    unsigned char *dt = K.tab.as<unsigned char>();
    MLH_HIP(ctx, hipMemcpyAsync(dt, h.data(), h.size(), hipMemcpyHostToDevice, st));
    const KfSeg *d_seg = reinterpret_cast<const KfSeg *>(dt + o_seg), *d_snz = reinterpret_cast<const KfSeg *>(dt + o_snz);
    const KfGat *d_mov = reinterpret_cast<const KfGat *>(dt + o_mov), *d_gat = reinterpret_cast<const KfGat *>(dt + o_gat);
    long long *d_ofs = reinterpret_cast<long long *>(dt + o_ofs);
    int *cnt = K.cnt.as<int>(), *ds = K.dstate.as<int>();

    if (compact) {
        if (ub_move > 0)
            MLH_LAUNCH(kf_move_kernel, dim3((ub_move + 255) / 256), dim3(256), 0, st, (const float4 *)K.cache.as<float4>(), d_mov, int(moves.size()), ub_move,
                       (const int *)cnt, K.cache_tmp.as<float4>());
        std::swap(K.cache.p, K.cache_tmp.p);
        std::swap(K.cache.cap, K.cache_tmp.cap);
    }
    if (N > 0) {
        Meas meas;
        for (int i = 0; i < 9; ++i) meas.m[i] = o->cov_measurement[i];
        const int nb = (N + 255) / 256;
        MLH_LAUNCH(kf_uct_kernel, dim3(nb), dim3(256), 0, st, (const float4 *)K.pts.as<float4>(), d_snz, int(segs_nz.size()),
                   (const double *)(dt + o_par), n_lidar, meas, o->with_ua ? 1 : 0, o->trace_threshold, N, K.stage.as<float4>(), K.keep.as<int>(), K.scan.as<int>());
        int rc = device_exclusive_scan(ctx, K.scan.as<int>(), N, ctx->vox.sums, ds + 16);
        if (rc) return rc;
        MLH_LAUNCH(kf_compact_kernel, dim3(nb), dim3(256), 0, st, (const float4 *)K.stage.as<float4>(), (const int *)K.keep.as<int>(),
                   (const int *)K.scan.as<int>(), d_snz, int(segs_nz.size()), N, K.cache.as<float4>());
    }
    if (!segs.empty())
        MLH_LAUNCH(kf_count_kernel, dim3((int(segs.size()) + 255) / 256), dim3(256), 0, st, d_seg, int(segs.size()), (const int *)K.scan.as<int>(),
                   (const int *)(ds + 16), N, cnt);
    MLH_LAUNCH(kf_prefix_kernel, dim3(1), dim3(64), 0, st, d_gat, ng[0], ng[1], (const int *)cnt, ds, K.pre_n[0] == 0 ? 1 : 0, K.pre_n[1] == 0 ? 1 : 0, d_ofs);
    const int ubm = std::max(ub[0], ub[1]);
    if (ubm > 0)
        MLH_LAUNCH(kf_gather_kernel, dim3((ubm + 255) / 256, 2), dim3(256), 0, st, (const float4 *)K.cache.as<float4>(), d_gat, ng[0], ng[1], ub[0], ub[1],
                   (const int *)cnt, (const long long *)d_ofs, K.pre[0].as<float4>(), K.pre[1].as<float4>(), ds);
    MLH_HIP(ctx, hipGetLastError());
    // wait 1: the pre-filter lengths and bounds
    MLH_HIP(ctx, hipMemcpyAsync(h_pin, ds, sizeof(int) * 14, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    float bounds[2][6];
    for (int k = 0; k < 2; ++k) {
        K.pre_n[k] = h_pin[k];
        for (int d = 0; d < 6; ++d) bounds[k][d] = dec_f(h_pin[2 + 6 * k + d]);
    }
    // the two covariance filters (cpp:343-346), results left in the context
    const float leaf[2] = {o->leaf_surf, o->leaf_corner};
    for (int k = 0; k < 2; ++k) {
        if (K.pre_n[k] == 0) { MLH_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ds + 14 + k), 0, 1, st)); continue; }
        int dummy = 0;
        int rc = voxel_filter_run(ctx, K.pre[k].p, REC, K.pre_n[k], 12, 16, 40, leaf[k], float(o->trace_threshold), nullptr, &dummy, MLH_MEM_DEVICE, bounds[k], false);
        if (rc) return rc;
        MLH_HIP(ctx, K.flt[k].ensure(size_t(REC) * size_t(K.pre_n[k])));
        MLH_HIP(ctx, hipMemcpyAsync(K.flt[k].p, ctx->vox.out.p, size_t(REC) * size_t(K.pre_n[k]), hipMemcpyDeviceToDevice, st));
        MLH_HIP(ctx, hipMemcpyAsync(ds + 14 + k, ctx->vox.total.p, sizeof(int), hipMemcpyDeviceToDevice, st));
    }
    // wait 2: the filtered counts
    MLH_HIP(ctx, hipMemcpyAsync(h_pin + 16, ds + 14, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    K.flt_n[0] = h_pin[16]; K.flt_n[1] = h_pin[17];
    *n_surf_ds = K.flt_n[0]; *n_corner_ds = K.flt_n[1];
    return device_error_check(ctx);
}

int local_map_cloud_run(mlh_ctx *ctx, int kind, int filtered, const void **device_points, int32_t *n)
{
    if (kind < 0 || kind > 1 || (filtered != 0 && filtered != 1) || !device_points || !n) return fail(ctx, MLH_ERR_INVALID, "mlh_local_map_cloud: bad arguments");
    const KfStore &K = ctx->kf;
    *device_points = filtered ? K.flt[kind].p : K.pre[kind].p;
    *n = filtered ? K.flt_n[kind] : K.pre_n[kind];
    return MLH_OK;
}

int local_map_info_run(mlh_ctx *ctx, int32_t *n_keyframes, int32_t *n_cached, int64_t *store_bytes, int64_t *cache_bytes)
{
    const KfStore &K = ctx->kf;
    if (n_keyframes) *n_keyframes = int32_t(K.keys.size());
    if (n_cached) *n_cached = int32_t(K.entries.size());
    if (store_bytes) *store_bytes = int64_t(K.pts.cap);
    if (cache_bytes) *cache_bytes = int64_t(K.cache.cap + K.cache_tmp.cap);
    return MLH_OK;
}

}  // namespace mlh

using namespace mlh;

extern "C" {

int mlh_keyframes_reset(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return keyframes_reset_run(ctx);
}

int mlh_keyframe_save(mlh_ctx *ctx, const double pose[7], const double cov[36], const void *surf, int n_surf, const void *corner, int n_corner,
                      int stride_bytes, int intensity_offset_bytes, int mem, int32_t *key_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return keyframe_save_run(ctx, pose, cov, surf, n_surf, corner, n_corner, stride_bytes, intensity_offset_bytes, mem, key_out);
}

int mlh_keyframe_save_staged(mlh_ctx *ctx, const double pose[7], const double cov[36], int32_t *key_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return keyframe_save_staged_run(ctx, pose, cov, key_out);
}

int mlh_local_map_assemble(mlh_ctx *ctx, const double pose_cur[7], const double *ext_poses, const double *ext_covs, int n_lidar, const mlh_local_map_opts *opts,
                           int32_t *rebuilt, int32_t *n_surf_ds, int32_t *n_corner_ds, int32_t *kf_ids_out, int32_t *n_ids)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return local_map_assemble_run(ctx, pose_cur, ext_poses, ext_covs, n_lidar, opts, rebuilt, n_surf_ds, n_corner_ds, kf_ids_out, n_ids);
}

int mlh_local_map_clear(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    return local_map_clear_run(ctx);
}

int mlh_local_map_cloud(mlh_ctx *ctx, int kind, int filtered, const void **device_points, int32_t *n)
{
    if (!ctx) return MLH_ERR_INVALID;
    return local_map_cloud_run(ctx, kind, filtered, device_points, n);
}

int mlh_local_map_info(mlh_ctx *ctx, int32_t *n_keyframes, int32_t *n_cached, int64_t *store_bytes, int64_t *cache_bytes)
{
    if (!ctx) return MLH_ERR_INVALID;
    return local_map_info_run(ctx, n_keyframes, n_cached, store_bytes, cache_bytes);
}

}  // extern "C"
