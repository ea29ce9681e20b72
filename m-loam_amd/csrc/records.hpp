// A caller's cloud as every entry point of the C-ABI takes it (include/mloam_hip.h: "Points are read through (base, stride_bytes)") and the one validation of
// it. Pure host C++, no HIP: tests/host/records_check.cpp compiles it with g++.
#pragma once
#include <cstddef>

namespace mlh {

struct Records {
    const unsigned char *p;                     // record 0; x, y, z are its first three floats
    int stride, n;                              // bytes per record, records
    int intensity_off, cov_off, trace_off;      // byte offsets of the f32 intensity, the six f32 of the covariance, the f32 trace; negative (-1): no such field
    int mem;                                    // MLH_MEM_HOST (0) or MLH_MEM_DEVICE (1)
    size_t bytes() const { return size_t(n) * size_t(stride); }
};

inline Records records_of(const void *p, int stride, int n, int mem, int intensity_off = -1, int cov_off = -1, int trace_off = -1)
{
    return Records{static_cast<const unsigned char *>(p), stride, n, intensity_off, cov_off, trace_off, mem};
}

// The argument at fault, or nullptr when every read `p + i * stride + off` of a present field stays inside record i: stride a multiple of 4 that is >= 12, each
// offset 4-byte aligned with its field ending inside the stride. allow_empty: n == 0 is a cloud (a pose block or a keyframe without features of a kind; `p` may be null).
inline const char *records_fault(const Records &r, bool allow_empty = false)
{
    if (r.n < 0 || (r.n == 0 && !allow_empty)) return "n";
    if (!r.p && r.n > 0) return "points";
    if (r.stride < 12 || (r.stride & 3)) return "stride_bytes";
    const int off[3] = {r.intensity_off, r.cov_off, r.trace_off}, size[3] = {4, 24, 4};
    const char *const name[3] = {"intensity_offset_bytes", "cov_offset_bytes", "trace_offset_bytes"};
    for (int f = 0; f < 3; ++f)
        if (off[f] >= 0 && ((off[f] & 3) || off[f] + size[f] > r.stride)) return name[f];
    return r.mem != 0 && r.mem != 1 ? "mem" : nullptr;
}

}  // namespace mlh
