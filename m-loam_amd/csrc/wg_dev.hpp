// Workgroup-wide sums, scans and bounding boxes: the one copy of the shuffle ladders under the index build, the voxel filters, the segmenter and the small
// reductions beside them. Wavefronts are 64 lanes, workgroups whole wavefronts. Not for the solver's sums (reduce_dev.hpp: their DPP order fixes its bits), the
// group-width scan of the 5-NN walk (knn_dev.hpp) or the paired scans of stdsort.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace mlh {

__device__ __forceinline__ int wg_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int wg_max(int a, int b) { return max(a, b); }
__device__ __forceinline__ float wg_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float wg_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double wg_max(double a, double b) { return fmax(a, b); }

// sum / max over the 64 lanes, to every lane: the xor butterfly 32, 16, ..., 1. Both partners of a step add the same two values, so every lane ends with the
// same bits; a floating-point sum's order is this one wherever it is used.
template <typename T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// N sums side by side: the N shuffles of a step are independent of one another
template <typename T, int N> __device__ __forceinline__ void wave_sum(T (&v)[N])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], off);
}
template <typename T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = wg_max(v, __shfl_xor(v, off));
    return v;
}

// inclusive prefix sum over the wavefront, lanes in order
__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive prefix sum of one int per thread over a workgroup of WAVES wavefronts; total = the sum, to every thread. lds: WAVES ints. Two barriers: one behind
// the wavefronts' totals, one behind their last read, so the next call may reuse lds at once -- and whatever else the workgroup wrote to LDS before the call is
// visible to all of it after it: callers publish words of their own through these barriers (vscan_final_kernel's lds_off, scan_local_kernel's lds_occ).
template <int WAVES> __device__ __forceinline__ int block_excl_scan(int v, int *lds, int &total)
{
    static_assert(WAVES == 4, "256 threads");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (w < wave) base += lds[w];
    total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + incl - v;
}

// sum of one integer per thread over a workgroup of WAVES wavefronts, to every thread. lds: WAVES words. One barrier, behind the wavefronts' sums; NONE behind
// the reads: a caller that writes lds again (a second sum through the same words) puts a barrier of its own in between.
template <int WAVES, typename T> __device__ __forceinline__ T block_sum(T v, T *lds)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = lds[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += lds[w];
    return s;
}

// BOXES bounding boxes, each six running values {min x y z, max x y z}, over the wavefront (min / max are exact: any order gives the same result) ...
template <int BOXES, typename T> __device__ __forceinline__ void wave_fold_bounds(T (&m)[6 * BOXES])
{
#pragma unroll
    for (int b = 0; b < 6 * BOXES; b += 6) {
#pragma unroll
        for (int d = b; d < b + 3; ++d) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { m[d] = wg_min(m[d], __shfl_xor(m[d], off)); m[3 + d] = wg_max(m[3 + d], __shfl_xor(m[3 + d], off)); }
        }
    }
}
// ... and over a workgroup of four wavefronts: true for the threads 0 .. 6 BOXES - 1, thread d holding value d of the workgroup's boxes in r. One barrier.
template <int BOXES, typename T> __device__ __forceinline__ bool block_fold_bounds(T (&m)[6 * BOXES], T (*lds)[6 * BOXES], T &r)
{
    wave_fold_bounds<BOXES>(m);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 6 * BOXES; ++c) lds[threadIdx.x >> 6][c] = m[c];
    }
    __syncthreads();
    if (threadIdx.x >= 6 * BOXES) return false;
    const int d = threadIdx.x;
    const bool lo = (BOXES == 1 ? d : d % 6) < 3;
    r = lds[0][d];
    for (int w = 1; w < 4; ++w) r = lo ? wg_min(r, lds[w][d]) : wg_max(r, lds[w][d]);
    return true;
}

}  // namespace mlh
