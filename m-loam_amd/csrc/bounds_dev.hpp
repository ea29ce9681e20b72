// A cloud's bounding box folded on the device while a kernel writes the cloud (keyframes.hip, cloudbuild.hip): six state words per cloud in an order-preserving
// int encoding of the floats, so that atomicMin / atomicMax fold them; the host decodes them for the voxel filter that follows (known_bounds).
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstring>

namespace mlh {

__device__ __forceinline__ int enc_f(float f) { const int b = __float_as_int(f); return b >= 0 ? b : b ^ 0x7fffffff; }   // order-preserving as int
inline float dec_f(int b) { const int v = b >= 0 ? b : b ^ 0x7fffffff; float f; std::memcpy(&f, &v, 4); return f; }

// the bounds of what this workgroup wrote (`any`: this thread wrote the point x y z), folded into a cloud's six state words; all 256 threads call it.
// min / max are exact: any order gives the same result
__device__ __forceinline__ void wg_fold_bounds(bool any, float x, float y, float z, int *__restrict__ bnd)
{
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (any) { mn[0] = mx[0] = x; mn[1] = mx[1] = y; mn[2] = mx[2] = z; }
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
            atomicMin(bnd + d, enc_f(a));
            atomicMax(bnd + 3 + d, enc_f(b));
        }
    }
}

}  // namespace mlh
