// The host side of the Scan Context store (scancontext.hip), host arithmetic only: option validation, the searched-prefix / period bookkeeping of
// SCManager::detectLoopClosureID (mloam_loop/src/scan_context.cpp:246-267), the binning of one point (cpp:38-51, 165-175) as the device and the host both
// compute it -- the host with its own libm for the points the device leaves undecided -- and the yaw conversion (cpp:33-36, 319-321). Kept in a header of its
// own so that a stand-alone host program can run it under a sanitizer (tests/host/sc_host_main.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "../../include/mloam_hip.h"

#if defined(__HIPCC__)
#define MLH_SC_HD __host__ __device__
#else
#define MLH_SC_HD
#endif

namespace mlh {

constexpr int SC_MAX_BINS = 8192;            // num_ring * num_sector: the grid's image fits 32 KB of LDS
constexpr int SC_MAX_CANDIDATES = 256;
constexpr float SC_NO_POINT = -1000.f;       // cpp:157
// A point whose sector value lies within this many sectors of an integer is not binned on the device (segment.hip: SEG_EDGE_MARGIN_BINS): an f32 ulp of a
// 360-degree angle is 5e-6 sectors at 60 sectors, so the band is ~80 ulps -- it covers the device's atanf against the host's as well as the float / double question
constexpr double SC_EDGE_MARGIN_SECTORS = 4.0e-4;

// the argument at fault, or nullptr
inline const char *sc_opts_fault(const mlh_sc_opts &o)
{
    if (o.num_ring < 1) return "num_ring";
    if (o.num_sector < 1) return "num_sector";
    if (int64_t(o.num_ring) * int64_t(o.num_sector) > SC_MAX_BINS) return "num_ring * num_sector";
    if (o.num_candidates < 1 || o.num_candidates > SC_MAX_CANDIDATES) return "num_candidates";
    if (!std::isfinite(o.max_radius) || !(o.max_radius > 0.0)) return "max_radius";
    if (!std::isfinite(o.lidar_height)) return "lidar_height";
    if (o.tree_making_period < 1) return "tree_making_period";
    if (o.num_exclude_recent < 0) return "num_exclude_recent";
    if (!std::isfinite(o.search_ratio) || o.search_ratio < 0.0) return "search_ratio";
    if (std::isnan(o.dist_thres) || std::isnan(o.loop_distance_threshold)) return "dist_thres";
    return nullptr;
}

// f32 <-> an int whose order is the float's (the grid's cells are combined with integer max)
MLH_SC_HD inline int sc_encode(float v)
{
    int b;
    memcpy(&b, &v, 4);
    return b >= 0 ? b : int(unsigned(b) ^ 0x7fffffffu);
}
MLH_SC_HD inline float sc_decode(int e)
{
    const int b = e >= 0 ? e : int(unsigned(e) ^ 0x7fffffffu);
    float v;
    memcpy(&v, &b, 4);
    return v;
}

// pt.z = z + LIDAR_HEIGHT (cpp:167): float + double, stored in a float. (+ 0.f: -0 and +0 compare equal in std::max, so which of them a cell keeps depends on the
// point order in the reference; here it is +0.)
MLH_SC_HD inline float sc_height(float z, double lidar_height) { return float(double(z) + lidar_height) + 0.f; }

// azim_range (cpp:170), float arithmetic; the square root through f64 is the correctly rounded f32 one
MLH_SC_HD inline float sc_range(float x, float y)
{
    const float xx = x * x, yy = y * y, s = xx + yy;
    return float(sqrt(double(s)));
}

// xy2theta (cpp:38-51) with the float overloads of atan: the quotient and the arc tangent in float, (180 / M_PI) * ... in double, returned as float. The quotient
// through f64 is the correctly rounded f32 one. x and y are finite.
MLH_SC_HD inline float sc_xy2theta(float x, float y)
{
    const double k = 180 / 3.14159265358979323846;
    if ((x >= 0) & (y >= 0)) return float(k * double(atanf(float(double(y) / double(x)))));
    if ((x < 0) & (y >= 0)) return float(180 - (k * double(atanf(float(double(y) / double(-x))))));
    if ((x < 0) & (y < 0)) return float(180 + (k * double(atanf(float(double(y) / double(x))))));
    return float(360 - (k * double(atanf(float(double(-y) / double(x))))));
}

// ring_idx (cpp:174); range <= max_radius
MLH_SC_HD inline int sc_ring(float range, double max_radius, int R)
{
    const double c = ceil((double(range) / max_radius) * R);
    return c >= double(R) ? R : (c >= 1.0 ? int(c) : 1);
}

// (azim_angle / 360.0) * PC_NUM_SECTOR, and sctor_idx of it (cpp:175). A NaN angle (x = y = 0: atan(0 / 0)) converts to INT_MIN on x86 (cvttsd2si), which
// max(min(S, .), 1) turns into 1
MLH_SC_HD inline double sc_sector_value(float angle, int S) { return (double(angle) / 360.0) * S; }
MLH_SC_HD inline int sc_sector(double sv, int S)
{
    if (sv != sv) return 1;
    const double c = ceil(sv);
    return c >= double(S) ? S : (c >= 1.0 ? int(c) : 1);
}
MLH_SC_HD inline bool sc_in_band(double sv) { return fabs(sv - rint(sv)) < SC_EDGE_MARGIN_SECTORS; }

// the host's verdict on a point the device left undecided: its sector with this machine's libm
inline int sc_decide_sector(float x, float y, int S) { return sc_sector(sc_sector_value(sc_xy2theta(x, y), S), S); }

// cell of (ring, sector), both from 1, in Eigen's column-major order
MLH_SC_HD inline int sc_bin(int ring, int sector, int R) { return (sector - 1) * R + (ring - 1); }

// tree_making_period_conter_ and the prefix polarcontext_invkeys_to_search_ holds (cpp:246-267)
struct ScBook {
    int counter = 0;     // queries that got past the early return
    int prefix = 0;      // entries [0, prefix) are searched: que_index - NUM_EXCLUDE_RECENT as of the last rebuild
};
inline bool sc_early_return(int que_index, const mlh_sc_opts &o) { return que_index < o.num_exclude_recent + 1; }
// one query past the early return: rebuilds when the counter says so, counts, and returns the prefix this query searches
inline int sc_book_query(ScBook &b, int que_index, const mlh_sc_opts &o)
{
    if (b.counter % o.tree_making_period == 0) b.prefix = que_index - o.num_exclude_recent;
    b.counter++;
    return b.prefix;
}

// SEARCH_RADIUS (cpp:130)
inline int sc_search_radius(double search_ratio, int S)
{
    const double r = std::round(0.5 * search_ratio * S);
    return r >= double(S) ? S : int(r);
}

// The batched build (mlh_sc_add_keyframes): one workgroup of sc_desc_batch_kernel per chunk, a chunk being a run of one entry's points (its three clouds back to
// back). An entry is cut into as many chunks as bring the grid to `target_workgroups` when the entries alone do not -- at most SC_BATCH_MAX_CHUNKS per entry, and
// never chunks of fewer than SC_BATCH_CHUNK_POINTS points (one pass of the workgroup), so a small entry is one chunk and an empty one none. Every chunk but an
// entry's last holds a multiple of SC_BATCH_CHUNK_POINTS points.
constexpr int SC_BATCH_CHUNK_POINTS = 256;
constexpr int SC_BATCH_MAX_CHUNKS = 64;
struct ScChunk { int entry, first, count, pad; };      // points [first, first + count) of entry `entry` of the batch
inline int sc_batch_chunks_wanted(int n_entries, int target_workgroups)
{
    if (n_entries < 1) return 1;
    const long long w = ((long long)target_workgroups + n_entries - 1) / n_entries;
    return w < 1 ? 1 : (w > SC_BATCH_MAX_CHUNKS ? SC_BATCH_MAX_CHUNKS : int(w));
}
// chunks of entries 0..n_entries-1 with n_points[] points each, appended to out[] (room for sc_batch_chunk_bound of them) in entry order; their number
inline size_t sc_batch_chunk_bound(int n_entries, int target_workgroups) { return size_t(n_entries > 0 ? n_entries : 0) * size_t(sc_batch_chunks_wanted(n_entries, target_workgroups)); }
inline size_t sc_batch_plan(const int *n_points, int n_entries, int target_workgroups, ScChunk *out)
{
    const int wanted = sc_batch_chunks_wanted(n_entries, target_workgroups);
    size_t n_chunks = 0;
    for (int e = 0; e < n_entries; ++e) {
        const int n = n_points[e];
        if (n <= 0) continue;
        const int passes = (n - 1) / SC_BATCH_CHUNK_POINTS + 1;                    // <= 2^23
        const int chunks = passes < wanted ? passes : wanted;
        const long long per = (long long)((passes - 1) / chunks + 1) * SC_BATCH_CHUNK_POINTS;      // (2^31 for one chunk of 2^31 - 1 points)
        for (long long at = 0; at < n; at += per) {
            const long long left = (long long)n - at;
            out[n_chunks++] = ScChunk{e, int(at), int(left < per ? left : per), 0};
        }
    }
    return n_chunks;
}
// the store's room after growing for `more` entries at n entries and cap rooms: the doubling of the single add, repeated
inline long long sc_grown_cap(long long n, long long cap, long long more)
{
    while (n + more > cap) cap = cap * 2 > 64 ? cap * 2 : 64;
    return cap;
}

// deg2rad(nn_align * PC_UNIT_SECTORANGLE) (cpp:33-36, 319-321); PC_UNIT_SECTORANGLE = 360.0 / double(PC_NUM_SECTOR)
inline float sc_deg2rad(const float degrees) { return degrees * 3.14159265358979323846 / 180.0; }
inline float sc_yaw(int shift, int S) { return sc_deg2rad(float(shift * (360.0 / double(S)))); }

// (t_que - t_match).norm() > LOOP_DISTANCE_THRESHOLD (pose_graph.cpp:309); threshold < 0: off
inline bool sc_too_far(const double a[3], const double b[3], double threshold)
{
    if (threshold < 0.0) return false;
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz) > threshold;
}

}  // namespace mlh
