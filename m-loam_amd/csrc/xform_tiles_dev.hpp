// The one-launch rigid transform of many cloud segments (pcl::transformPointCloud in f32, intensity carried), shared by the builders that concatenate stored clouds
// into map clouds: the odometry window's local maps (window.hip) and the loop closure's local maps (loopreg.hip). The host cuts every segment into TILES of up to 256
// points in destination order (a tile never straddles a segment, an empty segment has none) and uploads one FuseXf per segment; the launch has one workgroup per tile.
#pragma once
#include "ctx.hpp"
#include "bounds_dev.hpp"

namespace mlh {

struct WmTile {                             // up to 256 points of one segment (window.hip: LiDAR x kind x slot; loopreg.hip: cloud x keyframe)
    long long src;                          // its first record in the arena of its kind
    int begin;                              // its first point's place among the call's points in destination order
    int n;                                  // 1 .. 256
    int xf;                                 // its transform in the table
    int cloud;                              // the output cloud it belongs to (its bounds are folded into bounds[6 cloud ..]); odd: read from the corner arena
};

static __global__ __launch_bounds__(256) void wm_transform_kernel(const float4 *__restrict__ arena_surf, const float4 *__restrict__ arena_corner, const WmTile *__restrict__ tiles,
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
        const float4 p = ((t.cloud & 1) ? arena_corner : arena_surf)[t.src + threadIdx.x];
        // transform_cloud_kernel's expression: products and sums kept separate (no contraction)
        o.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[0], p.x), __fmul_rn(xf.r[1], p.y)), __fmul_rn(xf.r[2], p.z)), xf.t[0]);
        o.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[3], p.x), __fmul_rn(xf.r[4], p.y)), __fmul_rn(xf.r[5], p.z)), xf.t[1]);
        o.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[6], p.x), __fmul_rn(xf.r[7], p.y)), __fmul_rn(xf.r[8], p.z)), xf.t[2]);
        o.w = p.w;
        pre[size_t(t.begin) + threadIdx.x] = o;
    }
    wg_fold_bounds(mine, o.x, o.y, o.z, bounds + 6 * t.cloud);
}

}  // namespace mlh
