// Map clouds built from stored clouds on the device (gfx950): the one builder behind the odometry window's local maps (window.hip: buildLocalMap / buildCalibMap)
// and the loop closure's local maps (loopreg.hip: constructLocalMap). The caller names the stored clouds as SEGMENTS in destination order, each with a transform
// and an output cloud; here:
//   the tiles   host: every segment cut into TILES of up to 256 points (a tile never straddles a segment, an empty segment has none); transforms, tiles and the
//               state words go to the device in one table, one upload. State words: [6 c .. 6 c + 5] cloud c's bounds (order-preserving int encoding, bounds_dev.hpp),
//               [6 n_clouds + c] its filtered count.
//   wm_transform_kernel   pcl::transformPointCloud of one tile per workgroup: the tile's transform is uniform and is loaded ONCE per workgroup into LDS; the per-point
//               expression is transform_cloud_kernel's (frontend.hip), term for term, so the bits are mlh_transform_point_cloud's. The record goes straight to its
//               place in the pre-filter cloud, the intensity is copied, the source is left untouched, and the cloud's bounds are folded once per workgroup.
//   voxel_filter_collect x n_clouds   pcl::VoxelGrid per non-empty pre-filter cloud at its leaf, bounds known, counts left on the device.
// Per build: ONE transform launch and one upload, whatever the segments are; host waits: two (the clouds' bounds; the filtered counts), plus the one inside a voxel
// filter whose grid has more than 2^31 cells (the input comes back) and one for a buffer that has to grow.
#include "ctx.hpp"
#include <algorithm>
#include <climits>
#include "bounds_dev.hpp"
#include "tile_group.hpp"

namespace mlh {

struct WmTile {                             // up to 256 points of one segment
    long long src;                          // its first record in the arena of its kind
    int begin;                              // its first point's place among the call's points in destination order
    int n;                                  // 1 .. 256
    int xf;                                 // its transform in the table
    int cloud;                              // the output cloud it belongs to (its bounds are folded into bounds[6 cloud ..]); odd: read from the second arena
};

__global__ __launch_bounds__(256) void wm_transform_kernel(const float4 *__restrict__ arena_even, const float4 *__restrict__ arena_odd, const WmTile *__restrict__ tiles,
                                                           const FuseXf *__restrict__ xfs, float4 *__restrict__ pre, int *__restrict__ bounds)
{
    __shared__ FuseXf s_xf;
    const WmTile t = tiles[blockIdx.x];
    if (threadIdx.x < sizeof(FuseXf) / sizeof(float)) reinterpret_cast<float *>(&s_xf)[threadIdx.x] = reinterpret_cast<const float *>(xfs + t.xf)[threadIdx.x];
    __syncthreads();
    const FuseXf &xf = s_xf;
    const bool mine = int(threadIdx.x) < t.n;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mine) {
        const float4 p = ((t.cloud & 1) ? arena_odd : arena_even)[t.src + threadIdx.x];
        // transform_cloud_kernel's expression: products and sums kept separate (no contraction)
        o.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[0], p.x), __fmul_rn(xf.r[1], p.y)), __fmul_rn(xf.r[2], p.z)), xf.t[0]);
        o.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[3], p.x), __fmul_rn(xf.r[4], p.y)), __fmul_rn(xf.r[5], p.z)), xf.t[1]);
        o.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[6], p.x), __fmul_rn(xf.r[7], p.y)), __fmul_rn(xf.r[8], p.z)), xf.t[2]);
        o.w = p.w;
        pre[size_t(t.begin) + threadIdx.x] = o;
    }
    wg_fold_bounds(mine, o.x, o.y, o.z, bounds + 6 * t.cloud);
}

int stored_clouds_build(mlh_ctx *ctx, const float4 *arena_even, const float4 *arena_odd, const std::vector<FuseXf> &xfs, const std::vector<CloudSegment> &segs,
                        int n_clouds, const int *off, const int *len, const float *leaf, const CloudBuildBufs &B, int *flt_n)
{
    hipStream_t st = ctx->stream;
    std::vector<WmTile> tiles;
    size_t N = 0;
    for (const CloudSegment &s : segs) {
        segment_tiles(s.n, [&](int at, int len) { tiles.push_back(WmTile{(long long)(s.src + size_t(at)), int(N) + at, len, s.xf, s.cloud}); });
        N += size_t(s.n);
    }
    if (tiles.empty()) return MLH_OK;                       // every segment is empty

    // buffers, and one upload of every table of the call (the state words start as: empty bounds, no filtered records)
    MLH_HIP(ctx, ensure_counted(B.pre, sizeof(float4) * (N + 1), B.allocations));
    MLH_HIP(ctx, ensure_counted(B.flt, sizeof(float4) * (N + 1), B.allocations));
    std::vector<int> state0(size_t(7 * n_clouds), 0);
    for (int c = 0; c < n_clouds; ++c) for (int d = 0; d < 3; ++d) { state0[size_t(6 * c + d)] = INT_MAX; state0[size_t(6 * c + 3 + d)] = INT_MIN; }
    std::vector<unsigned char> &h = B.htab;
    h.clear();
    const size_t o_xf = put(h, xfs.data(), xfs.size());
    const size_t o_til = put(h, tiles.data(), tiles.size());
    const size_t o_sta = put(h, state0.data(), state0.size());
    MLH_HIP(ctx, ensure_counted(B.tab, h.size() + 16, B.allocations));
    unsigned char *dt = B.tab.as<unsigned char>();
    MLH_HIP(ctx, hipMemcpyAsync(dt, h.data(), h.size(), hipMemcpyHostToDevice, st));
    int *state = reinterpret_cast<int *>(dt + o_sta);
    float4 *pre = B.pre.as<float4>(), *flt = B.flt.as<float4>();

    MLH_LAUNCH(wm_transform_kernel, dim3(unsigned(tiles.size())), dim3(256), 0, st, arena_even, arena_odd, reinterpret_cast<const WmTile *>(dt + o_til),
               reinterpret_cast<const FuseXf *>(dt + o_xf), pre, state);
    MLH_HIP(ctx, hipGetLastError());
    // wait 1: the pre-filter clouds' bounds
    MLH_HIP(ctx, hipMemcpyAsync(B.h_pin, state, sizeof(int) * 6 * size_t(n_clouds), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    for (int c = 0; c < n_clouds; ++c) {
        if (len[c] == 0) continue;                          // (its filtered count stays at the 0 it was uploaded with)
        const int rc = voxel_filter_collect(ctx, pre + off[c], int(sizeof(float4)), len[c], 12, -1, -1, leaf[c], 0.f, B.h_pin + 6 * c, true, flt + off[c],
                                            state + 6 * n_clouds + c);
        if (rc) return rc;
    }
    // wait 2: the filtered counts
    MLH_HIP(ctx, hipMemcpyAsync(B.h_pin, state + 6 * n_clouds, sizeof(int) * size_t(n_clouds), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    for (int c = 0; c < n_clouds; ++c) flt_n[c] = B.h_pin[c];
    return device_error_check(ctx);
}

}  // namespace mlh
