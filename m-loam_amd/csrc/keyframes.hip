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
//
// pubGlobalMap (cpp:796-849) and saveGlobalMap (cpp:853-901) -- the map itself -- are one more pipeline over the same store (global_map_assemble_run):
//   host    the radius search (or every keyframe, saveGlobalMap), the thinning of the hits' positions with intensity = the keyframe's own index, and a table
//           of 256-point TILES over the selected keyframes' (keyframe x kind) segments in destination order -- a tile never straddles a segment;
//   gm_uct_kernel        cloudUCTAssociateToMap of one tile per workgroup: the tile's keyframe pose, compound poses and covariances are uniform and are
//                        loaded ONCE per workgroup into LDS (no per-thread segment search, no per-thread table reads); the per-point body is uct_point /
//                        uct_to_map of uct_dev.hpp, so the bits are kf_uct_kernel's. It leaves the staged record, the waves' keep ballots and the
//                        tile's kept count (one LDS add per wave); without uncertainty nothing is dropped and it writes the destination and bounds itself;
//   scan + gm_place_kernel   the exclusive scan runs over the TILE counts (N / 256 entries); a kept record goes to tile offset + its rank inside the tile
//                        (popcounts of the ballots), the clouds' exact bounds folded once per workgroup;
//   voxel_filter_run x 1 or 2   the covariance filter per output cloud, bounds known.
// Nothing of it touches the local map's state: its state words travel in the per-call table, its clouds and pinned landing words are its own.
//
// updateKeyframe (cpp:685-688, a stub in the reference) -- loop-corrected poses into the store (keyframes_update_run, keyframes_update_from_pg_run) -- has no
// kernel of its own: the poses, the "changed" test, the drift and the cache's erase are host work (kf_update_host.hpp); the pose graph's records reach the host by
// one strided copy; the re-association a correction causes is the next local_map_assemble_run's ordinary batch over the erased keyframes.
#include "ctx.hpp"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <array>
#include <cstddef>
#include <string>
#include "bounds_dev.hpp"
#include "dev_math.hpp"
#include "kf_update_host.hpp"
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
struct GmTile {                  // up to 256 points of one (keyframe x kind) segment of the global map
    long long src;               // its first record in the store (float4)
    int begin;                   // its first point's place among the call's points in destination order (cloud 0's segments, then cloud 1's)
    int n;                       // 1 .. 256
    int par;                     // offset (doubles) of its keyframe's pose / compound poses in the parameter table
    int cloud;                   // the output cloud it belongs to
};
// the global map's state words (ints, in the per-call table): [0..1] pre-filter lengths, [2..13] their bounds (order-preserving int encoding),
// [14..15] filtered counts, [16] total of the tile scan
constexpr int GM_STATE_INTS = 20, GM_PIN = 32;      // GM_PIN: its first landing word in KfStore::h_pin
constexpr int GM_MAX_LIDAR = 16, GM_TAB = 7 * GM_MAX_LIDAR + 7 + 43 * GM_MAX_LIDAR;

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
    float p3[3] = {0.f, 0.f, 0.f};
    bool any = false;
    if (ng > 0 && i < ub) {
        const int e = seg_of(gk, ng, i, &KfGat::ub_begin);
        const int local = i - gk[e].ub_begin;
        if (local < cnt[gk[e].slot2]) {
            const size_t s = size_t(gk[e].src + local) * REC_F4, d = size_t(ok[e] + local) * REC_F4;
            const float4 r0 = cache[s];
            pre[d] = r0; pre[d + 1] = cache[s + 1]; pre[d + 2] = cache[s + 2];
            p3[0] = r0.x; p3[1] = r0.y; p3[2] = r0.z;
            any = true;
        }
    }
    wg_fold_bounds(any, p3[0], p3[1], p3[2], dstate + 2 + 6 * k);
}

// ---- the global map (pubGlobalMap / saveGlobalMap): one workgroup per tile
// cloudUCTAssociateToMap of a tile. The tile's tables -- the extrinsics and its keyframe's [gpose 7 | compound poses n_lidar x 7 | covariances n_lidar x 36] --
// are uniform over the workgroup: loaded once into LDS, from where uct_point reads them by the point's LiDAR id.
// DIRECT (with_ua == 0: nothing is ever dropped): the record goes straight to its destination and the bounds are folded here.
// otherwise: the record is staged at the point's place in destination order, each wave leaves its keep ballot (masks[4 tile + wave]) and the tile its kept count.
template <bool DIRECT>
__global__ __launch_bounds__(256) void gm_uct_kernel(const float4 *__restrict__ store, const GmTile *__restrict__ tiles, const double *__restrict__ par, int n_lidar,
                                                     Meas meas, int with_ua, double trace_thr, float4 *__restrict__ stage, unsigned long long *__restrict__ masks,
                                                     int *__restrict__ tile_cnt, float4 *__restrict__ pre0, float4 *__restrict__ pre1, int n_cloud0,
                                                     int *__restrict__ state)
{
    __shared__ double tab[GM_TAB];
    __shared__ int kept;
    const GmTile t = tiles[blockIdx.x];
    const int n_ext = 7 * n_lidar, n_all = n_ext + 7 + 43 * n_lidar;
    for (int j = threadIdx.x; j < n_all; j += 256) tab[j] = j < n_ext ? par[j] : par[t.par + (j - n_ext)];
    if (threadIdx.x == 0) kept = 0;
    __syncthreads();
    const double *gpose = tab + n_ext;
    int keep = 0;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    if (int(threadIdx.x) < t.n) {
        const float4 p = store[t.src + threadIdx.x];
        const UctPoint u = uct_point(tab, gpose + 7, gpose + 7 + 7 * n_lidar, n_lidar, meas.m, DIRECT ? 0 : with_ua, trace_thr, p.x, p.y, p.z, p.w);
        keep = u.keep;
        if (keep) {
            float xyz[3];
            uct_to_map(gpose, p.x, p.y, p.z, xyz);
            r0 = make_float4(xyz[0], xyz[1], xyz[2], p.w);
            r1 = make_float4(u.c6[0], u.c6[1], u.c6[2], u.c6[3]);
            r2 = make_float4(u.c6[4], u.c6[5], float(u.tr), 0.f);
        }
    }
    if (DIRECT) {
        if (keep) {
            float4 *o = (t.cloud ? pre1 : pre0) + size_t(t.begin - (t.cloud ? n_cloud0 : 0) + int(threadIdx.x)) * REC_F4;
            o[0] = r0; o[1] = r1; o[2] = r2;
        }
        wg_fold_bounds(keep != 0, r0.x, r0.y, r0.z, state + 2 + 6 * t.cloud);
    } else {
        if (keep) {
            float4 *o = stage + size_t(t.begin + int(threadIdx.x)) * REC_F4;
            o[0] = r0; o[1] = r1; o[2] = r2;
        }
        const unsigned long long b = __ballot(keep);
        if ((threadIdx.x & 63) == 0) {
            masks[size_t(blockIdx.x) * 4 + (threadIdx.x >> 6)] = b;
            atomicAdd(&kept, __popcll(b));
        }
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = kept;
    }
}

// a kept record of a tile -> its cloud, at the tile's offset (the scan over the tile counts; cloud 1's tiles come behind all of cloud 0's, so cloud 0's length
// is the offset of cloud 1's first tile) + its rank among the tile's kept records (popcounts of the keep ballots); the clouds' lengths and bounds on the way
__global__ __launch_bounds__(256) void gm_place_kernel(const float4 *__restrict__ stage, const GmTile *__restrict__ tiles, const unsigned long long *__restrict__ masks,
                                                       const int *__restrict__ tile_off, int n_tiles, int tiles0, const int *__restrict__ total,
                                                       float4 *__restrict__ pre0, float4 *__restrict__ pre1, int *__restrict__ state)
{
    const GmTile t = tiles[blockIdx.x];
    const int len0 = tiles0 < n_tiles ? tile_off[tiles0] : *total;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int rank = 0;
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long m = masks[size_t(blockIdx.x) * 4 + j];
        if (j < w) rank += __popcll(m);
        if (j == w) mine = m;
    }
    const bool keep = ((mine >> lane) & 1ull) != 0;
    rank += __popcll(mine & ((1ull << lane) - 1ull));
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (keep) {
        const float4 *s = stage + size_t(t.begin + int(threadIdx.x)) * REC_F4;
        float4 *o = (t.cloud ? pre1 : pre0) + size_t(tile_off[blockIdx.x] - (t.cloud ? len0 : 0) + rank) * REC_F4;
        r0 = s[0];
        o[0] = r0; o[1] = s[1]; o[2] = s[2];
    }
    wg_fold_bounds(keep, r0.x, r0.y, r0.z, state + 2 + 6 * t.cloud);
    if (blockIdx.x == 0 && threadIdx.x == 0) { state[0] = len0; state[1] = *total - len0; }
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

bool bad_pose(const double *p) { for (int i = 0; i < 7; ++i) if (!std::isfinite(p[i])) return true; return false; }

}  // namespace

void keyframes_release(mlh_ctx *ctx)
{
    KfStore &K = ctx->kf;
    K.keys.clear(); K.entries.clear(); K.free_slots.clear(); K.n_slots = 0; K.pts_used = 0; K.cache_used = 0;
    K.pts.release(); K.cache.release(); K.cache_tmp.release(); K.cnt.release(); K.dstate.release(); K.tab.release();
    K.stage.release(); K.keep.release(); K.scan.release();
    for (int k = 0; k < 2; ++k) { K.pre[k].release(); K.flt[k].release(); K.pre_n[k] = K.flt_n[k] = 0; }
    global_map_release_run(ctx);
    std::vector<unsigned char>().swap(K.htab);
    K.h_poses.release();
}

// one cloud appended to the store (which has room for it): device float4 records (`packed`), or a caller's records packed on the way in
static int store_append(mlh_ctx *ctx, const void *src, int n, int stride, int ioff, int mem, bool packed)
{
    KfStore &K = ctx->kf;
    hipStream_t st = ctx->stream;
    if (n <= 0) return MLH_OK;
    float4 *dst = K.pts.as<float4>() + K.pts_used;
    if (packed) {
        MLH_HIP(ctx, hipMemcpyAsync(dst, src, sizeof(float4) * size_t(n), hipMemcpyDeviceToDevice, st));
    } else {
        const unsigned char *s;
        { const int rc = records_stage(ctx, records_of(src, stride, n, mem), ctx->tmp, st, &s); if (rc) return rc; }
        pack_points_launch(st, s, stride, n, ioff, 0.f, -1, dst, nullptr);
    }
    K.pts_used += size_t(n);
    return MLH_OK;
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
    for (int k = 0; k < 2; ++k) {
        key.off[k] = K.pts_used; key.n[k] = n[k];
        const int rc = store_append(ctx, src[k], n[k], stride, ioff, mem, packed);
        if (rc) return rc;
    }
    key.off[2] = K.pts_used; key.n[2] = 0; key.has_outlier = false;       // the outlier cloud: mlh_keyframe_attach_outlier
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

// (f15) mlh_keyframes_update_poses: host memory only -- the rules are kf_update_host.hpp's; what a change costs is paid by the next mlh_local_map_assemble, whose
// kf_uct_kernel chain re-associates the erased keyframes in one batch
int keyframes_update_run(mlh_ctx *ctx, const char *entry, int32_t first_key, int32_t n, const double *poses, const double *covs, int drift_tail, int32_t *n_changed,
                         double *drift_out)
{
    KfStore &K = ctx->kf;
    if (!n_changed) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": null n_changed").c_str());
    if (const char *f = kf_update_fault(K.keys.size(), first_key, n, poses, covs)) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": " + f).c_str());
    std::vector<char> changed;
    double drift[7];
    *n_changed = kf_update_apply(K.keys, first_key, n, poses, covs, drift_tail, changed, drift);
    if (drift_out) std::memcpy(drift_out, drift, sizeof(drift));
    if (*n_changed > 0) {
        kf_erase_changed(K.entries, K.free_slots, changed);
        return local_map_clear_run(ctx);       // the next assemble rebuilds; the global clouds stay as they are until the next mlh_global_map_assemble
    }
    return MLH_OK;
}

int keyframes_update_from_pg_cov_run(mlh_ctx *ctx, mlh_ctx *pg, const char *entry, int32_t first_index, int32_t first_key, int32_t n, int drift_tail, int cov_mode,
                                     int32_t *n_changed, double *drift_out)
{
    const std::string e = std::string(entry) + ": ";
    if (cov_mode != MLH_KF_COV_RELATIVE && cov_mode != MLH_KF_COV_ABSOLUTE) return fail(ctx, MLH_ERR_INVALID, (e + "cov_mode must be MLH_KF_COV_RELATIVE or MLH_KF_COV_ABSOLUTE").c_str());
    if (ctx->device != pg->device) return fail(ctx, MLH_ERR_UNSUPPORTED, (e + "both contexts must be on the same device").c_str());
    { const int rc = loop_process_gate(pg, entry); if (rc) return pg == ctx ? rc : fail(ctx, rc, mlh_last_error(pg)); }
    const PgStore &G = pg->pg;
    KfStore &K = ctx->kf;
    if (!n_changed) return fail(ctx, MLH_ERR_INVALID, (e + "null n_changed").c_str());
    if (G.count == 0) return fail(ctx, MLH_ERR_INVALID, (e + "the pose graph is empty").c_str());
    if (first_index < 0 || first_index >= G.count) return fail(ctx, MLH_ERR_INVALID, (e + "first_index names no pose-graph keyframe").c_str());
    if (n < 0) n = G.count - first_index;
    if (n == 0 || (long long)first_index + n > (long long)G.count) return fail(ctx, MLH_ERR_INVALID, (e + "the range lies outside the pose graph").c_str());
    if (first_key < 0 || size_t(first_key) + size_t(n) > K.keys.size()) return fail(ctx, MLH_ERR_INVALID, (e + "the range lies outside the store").c_str());
    if (!G.marg_valid) return fail(ctx, MLH_ERR_STATE, (e + "the pose graph holds no valid marginal covariances (mlh_pg_marginals; an optimise, a new loop, a reset or an import made them stale)").c_str());
    if (first_index + n - 1 > G.marg_cur) return fail(ctx, MLH_ERR_STATE, (e + "the range reaches beyond the keyframes the marginal covariances were computed for").c_str());
    const long long anchor = (long long)first_key + ((long long)G.marg_first - first_index);     // the key `first` maps to
    if (cov_mode == MLH_KF_COV_ABSOLUTE && (anchor < 0 || anchor >= (long long)K.keys.size()))
        return fail(ctx, MLH_ERR_INVALID, (e + "MLH_KF_COV_ABSOLUTE: the problem's first keyframe maps to no key of the store").c_str());
    const size_t row = sizeof(double) * 7, blk = sizeof(double) * 36, N = size_t(n);
    const size_t cov_at = ((row * N + 63) / 64) * 64;
    MLH_HIP(ctx, K.h_poses.ensure(cov_at + blk * N, (cov_at + blk * N) / 4));
    const int lo = std::max(first_index, G.marg_first), n_blocks = first_index + n - lo;      // the pose-graph indices of the range that have a block
    const int Mm = G.marg_cur - G.marg_first + 1;
    hipStream_t st = ctx->stream;
    if (pg != ctx) { const int hrc = ctx->handoff.borrow_begin(ctx, pg); if (hrc) return hrc; }
    MLH_HIP(ctx, hipMemcpy2DAsync(K.h_poses.p, row, G.kf.as<PgKeyframe>() + first_index, sizeof(PgKeyframe), row, N, hipMemcpyDeviceToHost, st));
    double *hc = reinterpret_cast<double *>(static_cast<char *>(K.h_poses.p) + cov_at);
    if (n_blocks > 0)
        MLH_HIP(ctx, hipMemcpyAsync(hc + size_t(36) * size_t(lo - first_index), G.marg_out.as<double>() + size_t(36) * (size_t(Mm) + size_t(lo - G.marg_first)), blk * size_t(n_blocks),
                                    hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    double add[36];
    for (int c = 0; c < 36; ++c) add[c] = cov_mode == MLH_KF_COV_ABSOLUTE ? K.keys[size_t(anchor)].cov[c] : 0.0;
    for (int i = 0; i < n; ++i) {
        double *c = hc + size_t(36) * size_t(i);
        if (first_index + i <= G.marg_first) std::memcpy(c, K.keys[size_t(first_key) + size_t(i)].cov, blk);      // before `first`, and `first` itself
        else if (cov_mode == MLH_KF_COV_ABSOLUTE) for (int q = 0; q < 36; ++q) c[q] = c[q] + add[q];
    }
    return keyframes_update_run(ctx, entry, first_key, n, K.h_poses.as<double>(), hc, drift_tail, n_changed, drift_out);
}

// (f15) mlh_keyframes_update_from_pose_graph: the poses of pg's records (stride sizeof(PgKeyframe), pose at offset 0) through ONE strided copy into pinned memory
// on ctx's stream -- behind pg's work so far by an event when the contexts differ (as mlh_fuse_add_scan_from) --, one host wait, then the host rules
// (f18) cov_mode >= 0 (mlh_keyframes_update_from_pose_graph_cov): also ONE copy of the store-form marginal blocks of the range into the same pinned block, behind the
// pose copy and in front of the same wait; then covs per key by the mode's rule -- a key that keeps its covariance is handed its own bits
int keyframes_update_from_pg_run(mlh_ctx *ctx, mlh_ctx *pg, int32_t first_index, int32_t first_key, int32_t n, int drift_tail, int32_t *n_changed, double *drift_out,
                                 int cov_mode = -1)
{
    const char *entry = cov_mode >= 0 ? "mlh_keyframes_update_from_pose_graph_cov" : "mlh_keyframes_update_from_pose_graph";
    if (cov_mode >= 0) return keyframes_update_from_pg_cov_run(ctx, pg, entry, first_index, first_key, n, drift_tail, cov_mode, n_changed, drift_out);
    if (ctx->device != pg->device) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_keyframes_update_from_pose_graph: both contexts must be on the same device");
    { const int rc = loop_process_gate(pg, entry); if (rc) return pg == ctx ? rc : fail(ctx, rc, mlh_last_error(pg)); }
    const PgStore &G = pg->pg;
    KfStore &K = ctx->kf;
    if (!n_changed) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph: null n_changed");
    if (G.count == 0) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph: the pose graph is empty");
    if (first_index < 0 || first_index >= G.count) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph: first_index names no pose-graph keyframe");
    if (n < 0) n = G.count - first_index;
    if (n == 0 || (long long)first_index + n > (long long)G.count)
        return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph: the range lies outside the pose graph");
    if (first_key < 0 || size_t(first_key) + size_t(n) > K.keys.size())
        return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph: the range lies outside the store");
    static_assert(offsetof(PgKeyframe, pose) == 0, "the pose is the record's head");
    const size_t row = sizeof(double) * 7;
    MLH_HIP(ctx, K.h_poses.ensure(row * size_t(n), row * size_t(n) / 4));       // (no copy of an earlier call is in flight: every call waits for its own)
    hipStream_t st = ctx->stream;
    if (pg != ctx) { const int hrc = ctx->handoff.borrow_begin(ctx, pg); if (hrc) return hrc; }
    MLH_HIP(ctx, hipMemcpy2DAsync(K.h_poses.p, row, G.kf.as<PgKeyframe>() + first_index, sizeof(PgKeyframe), row, size_t(n), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));     // the copy has completed when the call returns: no reader event has to outlive it
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    return keyframes_update_run(ctx, entry, first_key, n, K.h_poses.as<double>(), nullptr, drift_tail, n_changed, drift_out);
}

int keyframe_poses_run(mlh_ctx *ctx, int32_t first_key, int32_t n, double *poses, double *covs, float *positions)
{
    const KfStore &K = ctx->kf;
    if (first_key < 0 || n < 0 || size_t(first_key) + size_t(n) > K.keys.size()) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframe_poses: the range lies outside the store");
    for (size_t i = 0; i < size_t(n); ++i) {
        const KfStore::Key &key = K.keys[size_t(first_key) + i];
        if (poses) std::memcpy(poses + 7 * i, key.pose, sizeof(key.pose));
        if (covs) std::memcpy(covs + 36 * i, key.cov, sizeof(key.cov));
        if (positions) std::memcpy(positions + 3 * i, key.pos, sizeof(key.pos));
    }
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
    MLH_HIP(ctx, K.h_pin.ensure(sizeof(int) * KfStore::KF_PIN_INTS));
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
    for (int k = 0; k < 2; ++k) K.pre_n[k] = h_pin[k];
    // the two covariance filters (cpp:343-346), results left in the context
    const float leaf[2] = {o->leaf_surf, o->leaf_corner};
    for (int k = 0; k < 2; ++k) {
        if (K.pre_n[k] == 0) { MLH_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ds + 14 + k), 0, 1, st)); continue; }
        MLH_HIP(ctx, K.flt[k].ensure(size_t(REC) * size_t(K.pre_n[k])));      // (ahead of the filter, which neither reads nor names this buffer: ensure enqueues nothing)
        const int rc = voxel_filter_collect(ctx, K.pre[k].p, REC, K.pre_n[k], 12, 16, 40, leaf[k], float(o->trace_threshold), h_pin + 2 + 6 * k, false, K.flt[k].p, ds + 14 + k);
        if (rc) return rc;
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

// saveKeyframe's third cloud (laser_cloud_outlier_cov, cpp:673, 677, 681), attached to a keyframe that is already in the store
int keyframe_attach_outlier_run(mlh_ctx *ctx, int32_t key, const void *points, int n, int stride, int ioff, int mem)
{
    KfStore &K = ctx->kf;
    if (key < 0 || size_t(key) >= K.keys.size()) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframe_attach_outlier: no such keyframe");
    if (ioff < 0) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframe_attach_outlier: bad arguments");
    { const int rc = records_check(ctx, "mlh_keyframe_attach_outlier", records_of(points, stride, n, mem, ioff), true); if (rc) return rc; }
    KfStore::Key &k = K.keys[size_t(key)];
    if (k.has_outlier) return fail(ctx, MLH_ERR_STATE, "mlh_keyframe_attach_outlier: the keyframe already has an outlier cloud");
    if (n == 0) return MLH_OK;
    if (K.pts_used + size_t(n) > size_t(INT_MAX)) return fail(ctx, MLH_ERR_NOMEM, "keyframe store: more than 2^31 stored points");
    MLH_HIP(ctx, K.pts.grow(sizeof(float4) * (K.pts_used + size_t(n) + 1), sizeof(float4) * K.pts_used, ctx->stream));
    const size_t off = K.pts_used;
    { const int rc = store_append(ctx, points, n, stride, ioff, mem, false); if (rc) return rc; }
    MLH_HIP(ctx, hipGetLastError());
    if (mem == MLH_MEM_HOST) MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the caller's cloud has been read when the call returns
    k.off[2] = off; k.n[2] = n; k.has_outlier = true;
    return MLH_OK;
}

// Which keyframes the global map is made of, in the order their clouds are appended (cpp:804-810 / cpp:865-868): radiusSearch around the f32 position
// (nearest first, equal distances by index; kf_radius < 0: every keyframe in index order), the hits in that order through the plain branch of
// VoxelGridCovarianceMLOAM<PointI> at kf_res with intensity = the keyframe's own index (cpp:666). Keyframes that share a position voxel contribute only
// the voxel's last member in std::sort order.
int global_map_select_host(const float *pos, int n, const float *center, float kf_radius, float kf_res, std::vector<int> &ids)
{
    ids.clear();
    if (n < 0 || (n > 0 && !pos) || !(kf_res > 0.f) || !std::isfinite(kf_res) || std::isnan(kf_radius) || (kf_radius >= 0.f && !std::isfinite(kf_radius)))
        return MLH_ERR_INVALID;
    std::vector<int> hits;
    if (kf_radius < 0.f) {
        for (int i = 0; i < n; ++i) hits.push_back(i);
    } else {
        if (!center || !std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2])) return MLH_ERR_INVALID;
        std::vector<std::pair<float, int>> hit;
        for (int i = 0; i < n; ++i) {
            const float dx = pos[3 * i] - center[0], dy = pos[3 * i + 1] - center[1], dz = pos[3 * i + 2] - center[2], d2 = dx * dx + dy * dy + dz * dz;
            if (d2 <= kf_radius * kf_radius) hit.emplace_back(d2, i);
        }
        std::sort(hit.begin(), hit.end());
        for (const auto &h : hit) hits.push_back(h.second);
    }
    std::vector<std::array<float, 3>> p;
    for (int i : hits) p.push_back({pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]});
    for (int j : thin_positions(p, kf_res)) ids.push_back(hits[size_t(j)]);
    return MLH_OK;
}

void global_map_release_run(mlh_ctx *ctx)
{
    KfStore &K = ctx->kf;
    for (int k = 0; k < 2; ++k) { K.gpre[k].release(); K.gflt[k].release(); K.gpre_n[k] = K.gflt_n[k] = 0; }
}

int global_map_assemble_run(mlh_ctx *ctx, const double *pose_cur, const double *ext_poses, const double *ext_covs, int n_lidar, const mlh_global_map_opts *o,
                            int32_t n_pre[2], int32_t n_ds[2], int32_t *kf_ids_out, int32_t *n_ids)
{
    if (!ext_poses || !o || !n_pre || !n_ds || n_lidar <= 0 || n_lidar > GM_MAX_LIDAR) return fail(ctx, MLH_ERR_INVALID, "mlh_global_map_assemble: bad arguments");
    const auto pos_finite = [](float v) { return std::isfinite(v) && v > 0.f; };
    if (std::isnan(o->kf_radius) || (o->kf_radius >= 0.f && !std::isfinite(o->kf_radius)) || !pos_finite(o->kf_res) || !pos_finite(o->leaf) ||
        std::isnan(o->trace_threshold) || (o->split != 0 && o->split != 1))
        return fail(ctx, MLH_ERR_INVALID, "mlh_global_map_assemble: radius, resolution and leaf must be finite (resolution and leaf > 0), split 0 or 1");
    if (o->kf_radius >= 0.f && (!pose_cur || bad_pose(pose_cur))) return fail(ctx, MLH_ERR_INVALID, "mlh_global_map_assemble: a radius search needs the current pose");
    if (o->with_ua && !ext_covs) return fail(ctx, MLH_ERR_INVALID, "mlh_global_map_assemble: with_ua needs the extrinsic covariances");
    KfStore &K = ctx->kf;
    hipStream_t st = ctx->stream;
    for (int k = 0; k < 2; ++k) { n_pre[k] = n_ds[k] = 0; K.gpre_n[k] = K.gflt_n[k] = 0; }
    if (n_ids) *n_ids = 0;
    if (K.keys.empty()) return MLH_OK;                                     // cpp:796

    // the selection (cpp:804-810 / 865-868)
    std::vector<float> pos(3 * K.keys.size());
    for (size_t i = 0; i < K.keys.size(); ++i) for (int d = 0; d < 3; ++d) pos[3 * i + size_t(d)] = K.keys[i].pos[d];
    float c[3] = {0.f, 0.f, 0.f};
    if (pose_cur) for (int d = 0; d < 3; ++d) c[d] = float(pose_cur[d]);
    std::vector<int> sel;
    if (global_map_select_host(pos.data(), int(K.keys.size()), c, o->kf_radius, o->kf_res, sel) != MLH_OK)
        return fail(ctx, MLH_ERR_INVALID, "mlh_global_map_assemble: bad selection arguments");
    if (kf_ids_out) for (size_t j = 0; j < sel.size(); ++j) kf_ids_out[j] = sel[j];
    if (n_ids) *n_ids = int32_t(sel.size());

    // the parameter table and the tiles, in destination order: split 0: per keyframe surf, corner, outlier (cpp:818-827) into one cloud;
    // split 1: cloud 0 = per keyframe surf, outlier, then cloud 1 = per keyframe corner (cpp:872-882)
    std::vector<double> par(size_t(n_lidar) * 7);
    for (int l = 0; l < 7 * n_lidar; ++l) par[size_t(l)] = ext_poses[l];
    std::vector<int> par_of(sel.size());
    for (size_t j = 0; j < sel.size(); ++j) {
        const KfStore::Key &key = K.keys[size_t(sel[j])];
        const int p = int(par.size());
        par_of[j] = p;
        par.resize(par.size() + 7 + size_t(n_lidar) * 43, 0.0);
        for (int i = 0; i < 7; ++i) par[size_t(p + i)] = key.pose[i];
        if (o->with_ua)
            for (int l = 0; l < n_lidar; ++l)       // compoundPoseWithCov(pose_global, pose_ext[n]) (cpp:1122-1126)
                compound_pose_with_cov(key.pose, key.cov, ext_poses + 7 * l, ext_covs + 36 * l, &par[size_t(p + 7 + 7 * l)], &par[size_t(p + 7 + 7 * n_lidar + 36 * l)]);
    }
    std::vector<GmTile> tiles;
    size_t total[2] = {0, 0}, N = 0;
    int tiles0 = 0;
    const auto add_segment = [&](size_t j, int kind, int cloud) {
        const KfStore::Key &key = K.keys[size_t(sel[j])];
        for (int at = 0; at < key.n[kind]; at += 256)
            tiles.push_back(GmTile{(long long)(key.off[kind] + size_t(at)), int(N) + at, std::min(256, key.n[kind] - at), par_of[j], cloud});
        total[cloud] += size_t(key.n[kind]);
        N += size_t(key.n[kind]);
    };
    static const int order0[3] = {0, 1, 2}, order1[2] = {0, 2};
    size_t need = 0;
    for (int id : sel) need += size_t(K.keys[size_t(id)].n[0]) + size_t(K.keys[size_t(id)].n[1]) + size_t(K.keys[size_t(id)].n[2]);
    if (need > size_t(INT_MAX) / 2) return fail(ctx, MLH_ERR_NOMEM, "global map: too many points");
    if (o->split == 0) {
        for (size_t j = 0; j < sel.size(); ++j) for (int kind : order0) add_segment(j, kind, 0);
        tiles0 = int(tiles.size());
    } else {
        for (size_t j = 0; j < sel.size(); ++j) for (int kind : order1) add_segment(j, kind, 0);
        tiles0 = int(tiles.size());
        for (size_t j = 0; j < sel.size(); ++j) add_segment(j, 1, 1);
    }
    const int n_tiles = int(tiles.size());
    if (n_tiles == 0) return MLH_OK;                                       // keyframes without a point
    const bool direct = !o->with_ua;                                       // nothing is ever dropped: no staging, no scan

    // buffers, and one upload of every table of the call (the state words start as: lengths known only on the direct path, empty bounds, no filtered records)
    for (int k = 0; k < 2; ++k) if (total[k] > 0) MLH_HIP(ctx, K.gpre[k].ensure(size_t(REC) * (total[k] + 1)));
    if (!direct) {
        MLH_HIP(ctx, K.stage.ensure(size_t(REC) * N));
        MLH_HIP(ctx, K.keep.ensure(sizeof(unsigned long long) * 4 * size_t(n_tiles)));
        MLH_HIP(ctx, K.scan.ensure(sizeof(int) * size_t(n_tiles + 1)));
    }
    MLH_HIP(ctx, K.h_pin.ensure(sizeof(int) * KfStore::KF_PIN_INTS));
    int *h_pin = K.h_pin.as<int>() + GM_PIN;
    int state0[GM_STATE_INTS] = {0};
    if (direct) { state0[0] = int(total[0]); state0[1] = int(total[1]); }
    for (int k = 0; k < 2; ++k) for (int d = 0; d < 3; ++d) { state0[2 + 6 * k + d] = INT_MAX; state0[2 + 6 * k + 3 + d] = INT_MIN; }
    std::vector<unsigned char> &h = K.htab;
    h.clear();
    const size_t o_par = put(h, par.data(), par.size());
    const size_t o_til = put(h, tiles.data(), tiles.size());
    const size_t o_sta = put(h, state0, size_t(GM_STATE_INTS));
    MLH_HIP(ctx, K.tab.ensure(h.size() + 16));
    unsigned char *dt = K.tab.as<unsigned char>();
    MLH_HIP(ctx, hipMemcpyAsync(dt, h.data(), h.size(), hipMemcpyHostToDevice, st));
    const GmTile *d_til = reinterpret_cast<const GmTile *>(dt + o_til);
    const double *d_par = reinterpret_cast<const double *>(dt + o_par);
    int *state = reinterpret_cast<int *>(dt + o_sta);

    Meas meas;
    for (int i = 0; i < 9; ++i) meas.m[i] = o->cov_measurement[i];
    if (direct) {
        MLH_LAUNCH(gm_uct_kernel<true>, dim3(n_tiles), dim3(256), 0, st, (const float4 *)K.pts.as<float4>(), d_til, d_par, n_lidar, meas, 0, o->trace_threshold,
                   (float4 *)nullptr, (unsigned long long *)nullptr, (int *)nullptr, K.gpre[0].as<float4>(), K.gpre[1].as<float4>(), int(total[0]), state);
    } else {
        MLH_LAUNCH(gm_uct_kernel<false>, dim3(n_tiles), dim3(256), 0, st, (const float4 *)K.pts.as<float4>(), d_til, d_par, n_lidar, meas, 1, o->trace_threshold,
                   K.stage.as<float4>(), K.keep.as<unsigned long long>(), K.scan.as<int>(), (float4 *)nullptr, (float4 *)nullptr, 0, state);
        const int rc = device_exclusive_scan(ctx, K.scan.as<int>(), n_tiles, ctx->vox.sums, state + 16);
        if (rc) return rc;
        MLH_LAUNCH(gm_place_kernel, dim3(n_tiles), dim3(256), 0, st, (const float4 *)K.stage.as<float4>(), d_til, (const unsigned long long *)K.keep.as<unsigned long long>(),
                   (const int *)K.scan.as<int>(), n_tiles, tiles0, (const int *)(state + 16), K.gpre[0].as<float4>(), K.gpre[1].as<float4>(), state);
    }
    MLH_HIP(ctx, hipGetLastError());
    // wait 1: the pre-filter lengths and bounds
    MLH_HIP(ctx, hipMemcpyAsync(h_pin, state, sizeof(int) * 14, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    for (int k = 0; k < 2; ++k) K.gpre_n[k] = h_pin[k];
    // one covariance filter per output cloud (cpp:839-842 / 896-901), results kept in buffers of the global map's own
    for (int k = 0; k < 2; ++k) {
        if (K.gpre_n[k] == 0) continue;                                    // (its filtered count stays at the 0 it was uploaded with)
        MLH_HIP(ctx, K.gflt[k].ensure(size_t(REC) * size_t(K.gpre_n[k])));    // (ahead of the filter, which neither reads nor names this buffer: ensure enqueues nothing)
        const int rc = voxel_filter_collect(ctx, K.gpre[k].p, REC, K.gpre_n[k], 12, 16, 40, o->leaf, float(o->trace_threshold), h_pin + 2 + 6 * k, false, K.gflt[k].p, state + 14 + k);
        if (rc) return rc;
    }
    // wait 2: the filtered counts
    MLH_HIP(ctx, hipMemcpyAsync(h_pin + 16, state + 14, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    for (int k = 0; k < 2; ++k) { K.gflt_n[k] = h_pin[16 + k]; n_pre[k] = K.gpre_n[k]; n_ds[k] = K.gflt_n[k]; }
    return device_error_check(ctx);
}

int global_map_cloud_run(mlh_ctx *ctx, int which, int filtered, const void **device_points, int32_t *n)
{
    if (which < 0 || which > 1 || (filtered != 0 && filtered != 1) || !device_points || !n) return fail(ctx, MLH_ERR_INVALID, "mlh_global_map_cloud: bad arguments");
    const KfStore &K = ctx->kf;
    *n = filtered ? K.gflt_n[which] : K.gpre_n[which];
    *device_points = *n == 0 ? nullptr : (filtered ? K.gflt[which].p : K.gpre[which].p);
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

int mlh_keyframes_update_poses(mlh_ctx *ctx, int32_t first_key, int32_t n, const double *poses, const double *covs, int drift_tail, int32_t *n_changed,
                               double drift_out[7])
{
    if (!ctx) return MLH_ERR_INVALID;
    return keyframes_update_run(ctx, "mlh_keyframes_update_poses", first_key, n, poses, covs, drift_tail, n_changed, drift_out);
}

int mlh_keyframes_update_from_pose_graph(mlh_ctx *ctx, mlh_ctx *pg_ctx, int32_t first_index, int32_t first_key, int32_t n, int drift_tail, int32_t *n_changed,
                                         double drift_out[7])
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!pg_ctx) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph: null pose-graph context");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return keyframes_update_from_pg_run(ctx, pg_ctx, first_index, first_key, n, drift_tail, n_changed, drift_out);
}

int mlh_keyframes_update_from_pose_graph_cov(mlh_ctx *ctx, mlh_ctx *pg_ctx, int32_t first_index, int32_t first_key, int32_t n, int drift_tail, int32_t cov_mode,
                                             int32_t *n_changed, double drift_out[7])
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!pg_ctx) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph_cov: null pose-graph context");
    if (cov_mode < 0) return fail(ctx, MLH_ERR_INVALID, "mlh_keyframes_update_from_pose_graph_cov: cov_mode must be MLH_KF_COV_RELATIVE or MLH_KF_COV_ABSOLUTE");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return keyframes_update_from_pg_run(ctx, pg_ctx, first_index, first_key, n, drift_tail, n_changed, drift_out, cov_mode);
}

int mlh_keyframe_poses(mlh_ctx *ctx, int32_t first_key, int32_t n, double *poses, double *covs, float *positions)
{
    if (!ctx) return MLH_ERR_INVALID;
    return keyframe_poses_run(ctx, first_key, n, poses, covs, positions);
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

int mlh_keyframe_attach_outlier(mlh_ctx *ctx, int32_t key, const void *points, int n, int stride_bytes, int intensity_offset_bytes, int mem)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return keyframe_attach_outlier_run(ctx, key, points, n, stride_bytes, intensity_offset_bytes, mem);
}

void mlh_global_map_opts_default(mlh_global_map_opts *o, int for_save)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->kf_radius = for_save ? -1.f : 1000.f;        // GLOBALMAP_KF_RADIUS (lidar_mapper.h:81); saveGlobalMap takes every keyframe (cpp:865-866)
    o->kf_res = 10.f;                               // down_size_filter_global_map_keyframes (cpp:1293)
    o->leaf = for_save ? 0.8f : 0.4f;               // MAP_SURF_RES (cpp:839), 2 * MAP_SURF_RES (cpp:896)
    o->split = for_save ? 1 : 0;
    o->trace_threshold = 0.6;
    o->with_ua = 1;
    o->cov_measurement[0] = o->cov_measurement[4] = o->cov_measurement[8] = 0.0025;
}

int mlh_global_map_assemble(mlh_ctx *ctx, const double pose_cur[7], const double *ext_poses, const double *ext_covs, int n_lidar, const mlh_global_map_opts *opts,
                            int32_t n_pre[2], int32_t n_ds[2], int32_t *kf_ids_out, int32_t *n_ids)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return global_map_assemble_run(ctx, pose_cur, ext_poses, ext_covs, n_lidar, opts, n_pre, n_ds, kf_ids_out, n_ids);
}

int mlh_global_map_cloud(mlh_ctx *ctx, int which, int filtered, const void **device_points, int32_t *n)
{
    if (!ctx) return MLH_ERR_INVALID;
    return global_map_cloud_run(ctx, which, filtered, device_points, n);
}

int mlh_global_map_release(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    global_map_release_run(ctx);
    return MLH_OK;
}

int mlh_global_map_select(const float *positions_xyz, int n, const float center[3], float kf_radius, float kf_res, int32_t *ids_out, int32_t *n_ids)
{
    if (!n_ids || (n > 0 && !ids_out)) return MLH_ERR_INVALID;
    std::vector<int> ids;
    const int rc = global_map_select_host(positions_xyz, n, center, kf_radius, kf_res, ids);
    if (rc) return rc;
    for (size_t j = 0; j < ids.size(); ++j) ids_out[j] = ids[j];
    *n_ids = int32_t(ids.size());
    return MLH_OK;
}

}  // extern "C"
