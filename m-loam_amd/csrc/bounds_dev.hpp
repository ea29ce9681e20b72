// A cloud's bounding box folded on the device while a kernel writes the cloud (keyframes.hip, cloudbuild.hip): six state words per cloud in an order-preserving
// int encoding of the floats, so that atomicMin / atomicMax fold them; the host decodes them for the voxel filter that follows (known_bounds).
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstring>
#include "wg_dev.hpp"

namespace mlh {

__device__ __forceinline__ int enc_f(float f) { const int b = __float_as_int(f); return b >= 0 ? b : b ^ 0x7fffffff; }   // order-preserving as int
inline float dec_f(int b) { const int v = b >= 0 ? b : b ^ 0x7fffffff; float f; std::memcpy(&f, &v, 4); return f; }

// the bounds of what this workgroup wrote (`any`: this thread wrote the point x y z), folded into a cloud's six state words; all 256 threads call it.
// min / max are exact: any order gives the same result
__device__ __forceinline__ void wg_fold_bounds(bool any, float x, float y, float z, int *__restrict__ bnd)
{
    float m[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (any) { m[0] = m[3] = x; m[1] = m[4] = y; m[2] = m[5] = z; }
    __shared__ float red[4][6];
    const int any_wg = __syncthreads_or(any ? 1 : 0);
    float r;
    if (block_fold_bounds<1>(m, red, r) && any_wg) {
        if (threadIdx.x < 3) atomicMin(bnd + threadIdx.x, enc_f(r));
        else atomicMax(bnd + threadIdx.x, enc_f(r));
    }
}

}  // namespace mlh
