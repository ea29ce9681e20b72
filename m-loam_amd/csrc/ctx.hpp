// Internal definitions shared by the translation units of libmloam_hip.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cstddef>
#include <memory>
#include <string>
#include <vector>
#include <cstdlib>
#include <sched.h>
#include "../../include/mloam_hip.h"
#include "records.hpp"
#include "launch_modes.hpp"
#include "solve_plan_host.hpp"
#include "sc_host.hpp"

namespace mlh {

// ---------------------------------------------------------------- device-side records
// local-map cell grid (dense, x fastest). Cell edge h is a hair above sqrt(min_match_sq_dis) so that every map point
// within the acceptance radius of a query lies in the query's 27-cell neighbourhood.
struct GridDev {
    const float4 *sorted;     // cell-sorted points {x,y,z, original index (int bits)}
    const float4 *raw;        // the same points in original order
    const int *cell_start;    // ncell + 1 exclusive prefix of per-cell counts
    float ox, oy, oz, inv_h;
    int nx, ny, nz, n;
};

// what the match kernel keeps per feature for later re-linearisation (LM iterations on fixed correspondences)
struct __attribute__((aligned(16))) Corr {
    float c[6];        // surf: n_hat(3), d, 0, 0 ; corner: X1(3), X2(3)   (all exactly f32-valued in the reference)
    int valid;
    int pad;           // the f64 weight is recomputed from the feature's covariance diagonal on every evaluation
};

// packed normal equations: 21 upper-triangular J^T J entries, 6 J^T r, cost, count; padded to 32
constexpr int NE_H = 0, NE_G = 21, NE_COST = 27, NE_CNT = 28, NE_STRIDE = 32;

// device-resident optimiser state (one per context)
struct SolverState {
    double x[7];             // current pose [t, q(xyzw)]
    double cand[7];          // candidate pose (LM)
    double xb[8][7];         // poses of the additional blocks (config 4: extrinsics); xb[0] unused (block 0 is x)
    double V[36];            // PoseLocalParameterization::V_update_
    double ne[NE_STRIDE];    // normal equations at x
    double ce[NE_STRIDE];    // normal equations at cand (multi-GPU: all-reduced before lm_step consumes them)
    double neb[8][NE_STRIDE];   // multi-GPU pose-block mode: one record per block, all-reduced together
    double diag[6];          // LM diagonal (Jacobi-scaled)
    double S[6];             // Jacobi scaling 1/(1+sqrt(H_ii)) from iteration zero
    double radius, decrease_factor;
    double model_cost_change;
    double gmax;
    int reuse_diagonal;
    int iteration;
    int done;
    int termination;
    int num_successful;
    int num_invalid;
    int evaluations;
    int lm_overflow;         // split-submission scan2map: an outer iteration was begun while the previous one's LM loop had not terminated inside its look-ahead budget
    // Gauss-Newton with the finish deferred to the consumer (match.hip): the iteration poses of a solve, single-block (two pairs of slots) and over pose blocks (per
    // parity, per block). Which launch reads and writes which slot is ONE rule, solve_plan_host.hpp: pose_plan
    double xi[4][7];
    double xib[2][8][7];
    double lm_used_max;      // split-submission scan2map: the largest LM iteration count of the solve's outer iterations so far (the host sizes the next frame's look-ahead by it)
    double pad2[1];
};

// The Levenberg-Marquardt part of the solver state, in the form the consumer-side schedule keeps it (match.hip: lm_consume_kernel): two of these, launch g reads
// [(g - 1) & 1] and ONE workgroup of it writes [g & 1] -- the other workgroups of launch g may still be reading the first while that one stores the second
struct LmState {
    double x[7], cand[7];
    double V[36];
    double ne[NE_STRIDE];
    double diag[6], S[6];
    double radius, decrease_factor, model_cost_change, gmax, lm_used_max;
    int reuse_diagonal, iteration, done, termination, num_successful, num_invalid, evaluations, lm_overflow;
};

// pinned host record the device writes the result pose(s) into; seq is stored last with system-scope release
struct HostPublish {
    double x[7];
    double xb[8][7];
    long long done;          // DoneBits at publication (the LM driver polls it)
    unsigned long long seq;
    // MLH_FLAG_POSE_COV (reduce_dev.hpp: publish_pose_cov): the Hessian at the published pose -- the LM state's record at x, mirrored as IterStatDev::H is -- and its
    // inverse (lidar_mapper_keyframe.cpp:600-606), row-major in the tangent's order [t, theta]; stored in front of `seq` by a publication whose LM loop has terminated
    double H_final[36];
    double cov[36];
};
static_assert(offsetof(HostPublish, x) == 0 && offsetof(HostPublish, xb) == 56 && offsetof(HostPublish, done) == 504 && offsetof(HostPublish, seq) == 512 &&
              offsetof(HostPublish, H_final) == 520 && offsetof(HostPublish, cov) == 808 && sizeof(HostPublish) == 1096,
              "the publication record: pose, block poses, done word and sequence word where they have always been; the two matrices behind them");

// ---------------------------------------------------------------- the solver's launch modes: launch_modes.hpp (LaunchTail, LmConsumer, LmExpect, PreFinish)
enum : int { LM_OVERFLOW_BARRIER_GIVEN_UP = 4 };   // SolverState::lm_overflow: 0 / 1 = a loop outgrew its look-ahead; this value (the one-launch loops store it) = a barrier was given up on
// HostPublish::done (reduce_dev.hpp: publish_pose): the LM loop has terminated (a Gauss-Newton solve: the pose is final) | the look-ahead of launches overflowed, a
// loop had not ended where the host assumed it had | a one-launch loop gave a barrier up | the launch had no features
enum DoneBits : int { DONE_TERMINATED = 1, DONE_OVERFLOWED = 2, DONE_GIVEN_UP = 4, DONE_NO_FEATURES = 8 };

// The context's 256 pinned bytes of small read-backs (mlh_ctx::h_scratch). The kernels that publish the thinned feature counts receive the addresses of
// thin_counts and thin_seq (voxel.hip); a copy lands in read_back (read_back_int).
struct ScratchBlock {
    int pad0[8];
    int read_back;                     // one device int on its way to the host
    int pad1[7];
    int thin_counts[2];                // the thinned surf / corner feature counts ...
    int pad2[14];
    unsigned long long thin_seq;       // ... and the sequence number their publication stores last (system-scope release)
    unsigned char pad3[120];
};
static_assert(offsetof(ScratchBlock, read_back) == 32 && offsetof(ScratchBlock, thin_counts) == 64 && offsetof(ScratchBlock, thin_seq) == 128 &&
              sizeof(ScratchBlock) == 256, "the scratch block's layout is what the thinning kernels were handed pointers into");

// pinned record mlh_fused_cloud's publication launch fills (fused_publish_kernel gets the three addresses)
struct FusedPublish {
    int count[4];                      // the two record counts (padded to 4 ints)
    float box[12];                     // 2 x 6 bounds
    unsigned long long seq;            // stored last, with system-scope release
    unsigned char pad[56];
};
static_assert(offsetof(FusedPublish, count) == 0 && offsetof(FusedPublish, box) == 16 && offsetof(FusedPublish, seq) == 64 && sizeof(FusedPublish) == 128,
              "the fused-cloud publication: counts at 0, bounds at 16, sequence word at 64, 128 bytes");

struct IterStatDev {        // mirrors mlh_iter_stat, written by the device-side update kernels
    int n_surf, n_corner, is_degenerate, lm_iterations, successful_steps, termination;
    double cost, final_cost;
    double eigval[6];
    double H[36];
    double g[6];
    double pose_after[7];
};

// ---------------------------------------------------------------- host-side containers
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // owns its allocation: a buffer that is a member of the context (or of one of its sub-structures) is freed with it, so a new member
    // cannot be forgotten in mlh_destroy (which sets the device before `delete ctx`)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    // grow to `bytes`, preserving the first `keep` bytes (device-to-device copy on `st`)
    hipError_t grow(size_t bytes, size_t keep, hipStream_t st)
    {
        if (bytes <= cap) return hipSuccess;
        void *np = nullptr;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&np, want);
        if (e != hipSuccess) return e;
        if (p && keep) {
            e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
        }
        if (p) (void)hipFree(p);
        p = np; cap = want;
        return hipSuccess;
    }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
// a buffer of a store brought to `bytes` (contents dropped); counted in the store's `allocations` when it allocates
inline hipError_t ensure_counted(DevBuf &b, size_t bytes, long long &allocations)
{
    if (bytes > b.cap) ++allocations;
    return b.ensure(bytes);
}
// n records appended to a host table at the next 16-byte boundary (p == nullptr: room only); their offset. A call's tables go to the device in one upload.
template <class T> size_t put(std::vector<unsigned char> &h, const T *p, size_t n)
{
    size_t off = (h.size() + 15) & ~size_t(15);
    h.resize(off + sizeof(T) * n);
    if (n && p) std::memcpy(h.data() + off, p, sizeof(T) * n);
    return off;
}

// Page-locked host memory, owned the way DevBuf owns device memory: every pinned block of the library is one of these (the only place that allocates or frees one),
// a member of the context or of one of its sub-structures, and freed with it.
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    // A block of at least `bytes`. One that is too small is DROPPED, contents and all, for a new one of bytes + margin (`zeroed`: cleared; otherwise untouched, the
    // first touch of a large staging block is its user's). Never synchronises: a caller whose stream may still be copying into or out of the old block drains it first.
    hipError_t ensure(size_t bytes, size_t margin = 0, bool zeroed = false)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, bytes + margin, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes + margin;
        if (zeroed) std::memset(p, 0, cap);
        return hipSuccess;
    }
    void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; } }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// A pinned landing place in two halves used alternately, an event per half: what the host puts into a half goes to the device by a copy enqueued behind it, and the
// half is written again two turns later -- by then that copy has long run, and the event says so without a wait on the stream (mlh_scan_upload: points, ring tables).
struct PinnedHalves {
    PinnedBuf buf;
    size_t half_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    unsigned turn = 0;
    PinnedHalves() = default;
    PinnedHalves(const PinnedHalves &) = delete;
    PinnedHalves &operator=(const PinnedHalves &) = delete;
    ~PinnedHalves() { for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); }     // (with the context: its streams have been drained by then)
    // the next half, `bytes` of it usable, once the copy enqueued out of it two turns ago has run; growing (to halves of `half_cap` >= bytes) drains `st` first
    hipError_t take(size_t bytes, size_t half_cap, hipStream_t st, int *half, void **dst)
    {
        if (bytes > half_bytes) {
            hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
            half_bytes = 0;
            if ((e = buf.ensure(2 * half_cap)) != hipSuccess) return e;      // (half_cap >= bytes > half_bytes: always larger than the block it replaces)
            half_bytes = half_cap;
            for (int i = 0; i < 2; ++i) if (!ev[i] && (e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) return e;
            used[0] = used[1] = false;
        }
        *half = int(turn++ & 1);
        if (used[*half]) { const hipError_t e = hipEventSynchronize(ev[*half]); if (e != hipSuccess) return e; }
        *dst = buf.as<char>() + size_t(*half) * half_bytes;
        return hipSuccess;
    }
    // the copy out of `half` has been enqueued on `st`
    hipError_t record(int half, hipStream_t st)
    {
        const hipError_t e = hipEventRecord(ev[half], st);
        if (e == hipSuccess) used[half] = true;
        return e;
    }
};

struct MapGrid {
    DevBuf raw, sorted, cell_id, cell_start, cell_fill, block_sums, bounds, occ;
    int n = 0;
    bool want_occ = false;     // the index build also collects the occupancy statistics below (the mapper's two maps)
    int occ_parts = 0;         // per-workgroup partials in `occ`
    long long *occ_host = nullptr;   // pinned mirror of the totals (owned by the context)
    int occupied = 0;          // non-empty cells of the current index (0: not measured)
    long long pop_sq = 0;      // sum over the cells of population^2: pop_sq / n = the population of the cell an average map POINT lives in,
                               // which is what a query near the map sees (the density the query kernels tune to)
    float ox = 0, oy = 0, oz = 0, h = 1.f, inv_h = 1.f;
    int nx = 0, ny = 0, nz = 0;
    long long ncell = 0;
    float min_match_sq_dis = 1.0f;
    bool built = false;
    bool geom_valid = false;   // ox.. nz describe a box (with margin) laid out by a bounds pass; reusable while the clouds keep fitting
    float geom_sq_dis = 0.f;   // the acceptance radius that geometry was derived from
    int cur = 0;               // which of the two cell arrays (cell_start / cell_fill) holds the current index
    bool twin_clean = false;   // the other one has been cleared for the next build
    int *cells(int which) const { return (which ? cell_fill : cell_start).as<int>() + 3; }   // see grid.hip: cells + 1 is 16-byte aligned
    GridDev dev() const
    {
        GridDev g;
        g.sorted = sorted.as<float4>(); g.raw = raw.as<float4>(); g.cell_start = cells(cur);
        g.ox = ox; g.oy = oy; g.oz = oz; g.inv_h = inv_h; g.nx = nx; g.ny = ny; g.nz = nz; g.n = n;
        return g;
    }
};

struct FeatSet {
    DevBuf pts;        // float4 {x,y,z,intensity}
    DevBuf covd;       // float4 {cxx, cyy, czz, 0}  (diagonal of the f32 cov_vec)
    DevBuf corr;       // Corr per feature
    DevBuf nbr;        // 5 float4 per feature: the 5 nearest map points + squared distances
    DevBuf r, J;       // dense residual / Jacobian (double, double[6]) when requested
    DevBuf fps_order;  // 'fps' selection: [count][visiting order] (select.hip: fps_order_kernel)
    DevBuf fps_work;   // 'fps' selection: Morton keys, ranks, permutation of the pruned loop (select.hip: fps_order_pruned_kernel)
    DevBuf flag8;      // one byte per feature: Corr::valid on the way to the host, the selection's verdict on the way back (select.hip)
    int m = 0;             // feature slots (real + padding between pose blocks)
    int n_blocks = 1;
    int blk_start[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int blk_real[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // real features per block
    int nbr_stride = 5;
    bool has_cov = false;
    bool matched = false;
    // the set is one pose block of `count` features (mlh_features_set and the thinning calls; mlh_features_set_block is the several-block form)
    void single_block(int count, bool with_cov)
    {
        m = count; n_blocks = 1; blk_start[0] = 0; blk_real[0] = count; has_cov = with_cov;
        for (int b = 1; b <= 8; ++b) blk_start[b] = count;
    }
};

struct ScanBuf {
    DevBuf pts;            // float4 {x,y,z,intensity}
    DevBuf start, end;     // per ring
    int *end_alias = nullptr;   // mlh_scan_upload sends both tables in one copy: the end table then sits behind the start table in `start`
    int *end_ptr() { return end_alias ? end_alias : end.as<int>(); }
    DevBuf curvature, label, picked;
    DevBuf stage;          // per-ring staged picks
    DevBuf ring_counts;    // 4 counts per ring
    DevBuf ring_offsets;   // 4 exclusive offsets per ring (+ totals)
    DevBuf lists[4];
    DevBuf totals;         // 4 ints
    DevBuf vox_stage, vox_out, ring_vox;   // per-ring VoxelGrid of the less-flat points
    DevBuf tie_scratch;                    // label kernel: std::sort scratch of sectors with equal curvatures when it does not fit LDS
    DevBuf vox_keys, vox_perm;             // its voxel indices in list order and the order std::sort leaves them in (reference member order)
    bool voxelised = false;
    int n = 0, n_rings = 0;
    int max_ring_len = 0;  // max over rings of (scan_end - scan_start)
    bool extracted = false;
    int h_totals[5] = {0, 0, 0, 0, 0};   // host copy of the four list sizes + the thinned less-flat count, fetched once per scan
    bool h_lists_valid = false, h_vox_valid = false;
};

struct VoxBuf {   // scratch of mlh_voxel_filter
    DevBuf in, bounds, cell, wpre, cnt, vox_of, word_of, sorted_idx, members, leader, out, sums, total;
};

// The mapper's keyframe store and the local map extractSurroundingKeyFrames builds from it (keyframes.hip; lidar_mapper_keyframe.cpp:254-354, 641-683)
struct KfStore {
    // one saved keyframe: pose + cov_, f32 position, its clouds in `pts`: [0] surf, [1] corner, [2] outlier (attached later or empty; only the global map reads it)
    struct Key { double pose[7], cov[36]; float pos[3]; size_t off[3]; int n[3]; bool has_outlier; };
    struct Entry { int id; size_t off[2]; int n[2]; int slot; };                            // one cached keyframe: reserved records in `cache` (kept counts: cnt[2 slot + kind])
    std::vector<Key> keys;
    DevBuf pts;                  // float4 {x, y, z, lidar} of every saved cloud, appended
    size_t pts_used = 0;
    std::vector<Entry> entries;  // surrounding_existing_keyframes_id + the transformed clouds, in the reference's order
    std::vector<int> free_slots;
    int n_slots = 0;
    DevBuf cache, cache_tmp;     // 48-byte PointIWithCov records of the cached clouds (reserved ranges)
    size_t cache_used = 0;
    DevBuf cnt;                  // int per (slot, kind): kept records of a cached cloud (device only)
    DevBuf pre[2], flt[2];       // laser_cloud_{surf,corner}_from_map_cov and their _ds, 48-byte records
    int pre_n[2] = {0, 0}, flt_n[2] = {0, 0};
    DevBuf dstate;               // ints: [0..1] pre-filter lengths, [2..13] their bounds (order-preserving int encoding), [14..15] filtered counts, [16] scan total
    DevBuf tab;                  // per-call tables (segments, poses, gather lists)
    DevBuf stage, keep, scan;    // batched association: staged records, keep flags, their scan
    std::vector<unsigned char> htab;
    PinnedBuf h_pin;             // landing place of the read-backs (KF_PIN_INTS ints: [0..31] the local map's, [32..63] the global map's)
    static constexpr int KF_PIN_INTS = 64;
    PinnedBuf h_poses;           // landing place of the pose graph's poses on their way into `keys` (mlh_keyframes_update_from_pose_graph: 7 doubles per keyframe)
    // the global map (pubGlobalMap / saveGlobalMap, cpp:780-919): clouds and lengths of its own; its per-call state words travel in `tab`, never in `dstate`
    DevBuf gpre[2], gflt[2];     // pre-filter and filtered global clouds, 48-byte records
    int gpre_n[2] = {0, 0}, gflt_n[2] = {0, 0};
};

// a rigid transform in single precision (+ the LiDAR index of transformCloudFeature): what the per-point transform kernels of frontend.hip and cloudbuild.hip apply
struct FuseXf { float r[9], t[3], id; };
// rotation of the unit quaternion in double, rounded once to float: what Eigen::Matrix4f holds after `.cast<float>()`
inline FuseXf xf_from_pose(const double pose[7], float id)
{
    const double tx = pose[0], ty = pose[1], tz = pose[2], qx = pose[3], qy = pose[4], qz = pose[5], qw = pose[6];
    const double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                         2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                         2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)};
    FuseXf xf;
    for (int i = 0; i < 9; ++i) xf.r[i] = float(R[i]);
    xf.t[0] = float(tx); xf.t[1] = float(ty); xf.t[2] = float(tz);
    xf.id = id;
    return xf;
}

// The odometry's sliding window (window.hip; estimator.cpp:485-496, 1521-1536) and the local maps buildLocalMap / buildCalibMap make of it (cpp:1067-1110, 1159-1204)
struct WinStore {
    bool ready = false;          // mlh_window_reset has run
    int n_lidar = 0, window = 0; // NUM_OF_LASER, WINDOW_SIZE: every stack has window + 1 slots
    // CircularBuffer's three words (CircularBuffer.h:61-67, 134-137, 186-197); every stack is pushed together, so they share them
    int size = 0, start = 0;
    long long pushes = 0;
    // The clouds: float4 {x, y, z, intensity} in one arena per kind, cut into equal slabs of `slab` records (as many slabs as there are slots: a slot's cloud
    // is named by at most one slab, a slab by any number of slots). A slide moves names and counts, never points. A cloud larger than the slabs re-cuts the arena.
    DevBuf arena[2];
    size_t slab[2] = {0, 0};
    std::vector<int> slab_refs[2], slab_n[2];      // per slab: the slots that name it, its records
    std::vector<int> slot_slab[2];                 // per (lidar, PHYSICAL slot): its slab, -1 = the empty cloud
    long long allocations = 0;   // device allocations of the store and its maps since the reset
    // the local maps of the last build: every LiDAR's pre-filter clouds back to back in `pre` (cloud 2 n + kind at record map_off[2 n + kind]), the filtered
    // ones at the same offsets in `flt`
    DevBuf pre, flt, tab;
    std::vector<int> map_off, map_pre_n, map_flt_n;
    std::vector<unsigned char> htab;
    PinnedBuf h_pin;             // landing place of the two read-backs (bounds; filtered counts)
};

struct SegBuf {    // ImageSegmenter scratch (segment.hip)
    DevBuf raw, pix, owner, range, ground, keep;
    DevBuf edge;               // the cluster search's angle verdicts per pixel (seg_edge_kernel)
    DevBuf outmask, row_cnt;   // device row assembly: the outlier pixels' bit mask (from the host's cluster search), per-row counts of kept points (+ first kept index)
    PinnedBuf h_rows;      // [vs + 2] ints the row kernels leave for the host (kept points per row, total, first kept point index)
    DevBuf unc;            // points / ground pairs whose bin the device cannot decide (an angle within an ulp-scale margin of a bin edge): [counters 2 x int][records]
    DevBuf fix;            // the host's verdicts for the undecided points: {point index, pixel}
    PinnedBuf h_unc;       // mirror of `unc`
    PinnedBuf h_img;       // range / owner / ground images as the cluster search reads them, and the outlier mask it writes
    void *h_bfs = nullptr;     // plain: labels and the cluster search's queue / pushed-pixel arrays
    size_t h_bfs_cap = 0;
    ~SegBuf() { std::free(h_bfs); }
};

struct OdomSet {   // staged LidarPureOdom factor table (odom.hip)
    DevBuf tab, idx, poses, r, J;
    int n = 0, max_frame = 0, max_ext = 0;
    // normal equations of the coupled window problem: factor indices grouped by (frame, extrinsic) in 256-factor tiles
    DevBuf perm, tile_group, partial, ne_out, solve_aux;
    int n_tiles = 0, group_ext = 1;
    bool tile_group_keyed = true;
    std::vector<int> h_tile_frame, h_tile_ext;
    bool device_built = false;   // table appended from match passes on the device (padded regions): normal equations only
};

// The odometry window's marginalisation prior and the extrinsics' PriorFactor rows (marg.hip; estimator.cpp:658-685, 871-1063)
struct MargPrior {
    bool valid = false;
    int n_keep = 0;                       // kept blocks, 6 local parameters each
    int shape_frames = -1, shape_ext = -1;   // the window a marginalisation made it for (-1: installed by the caller, only the block ids are known)
    int ids[22] = {0};                    // kept block -> block of the window layout [pivot | frames | extrinsics]
    DevBuf ids_dev, x0, J0, r0, JtJ;      // the same map; 7 doubles per kept block; n x n; n; n x n (n = 6 n_keep)
    DevBuf work;                          // marginalisation: the eigenvectors when they do not fit in LDS, the device's info record
    DevBuf eval;                          // mlh_window_prior_evaluate: outputs and poses
    PinnedBuf h_info;                     // landing place of the info record; the new block map on its way to the device
    mlh_window_prior_info info = {};
    int ext_n = 0;                        // extrinsics with a PriorFactor (0: none installed)
    unsigned ext_flags = 0;               // bit 0: the rows enter the marginalisation, bit 1: the solve
    DevBuf ext_rows;                      // 9 doubles per extrinsic
};

// The accumulated calibration features (calib.hip): cumu_surf_map_features_ / cumu_corner_map_features_ of the estimator (estimator.cpp:714-735, 762-780) as
// one-block LidarOnlineCalib factors in HBM. Slot s of the store: tab[10 s ..] = point[3], coeff[6], sqrt_info; type[s]; perm[s] = -1 for padding, else the
// factor's index in the order the store was given it. 256 slots = one tile, every tile belongs to ONE extrinsic (h_tile_ext). Persists across windows.
struct CalibStore {
    DevBuf tab, type, perm;
    DevBuf lists;                         // [tile_ext (n_tiles) | ext_start (n_ext + 1) | tile_pos (n_tiles)]: a tile's extrinsic; the rows of extrinsic e in `partial`;
                                          // a tile's rank in (extrinsic, tile) order = its row of `partial`
    DevBuf partial;                       // n_tiles x 32: a tile's 21 + 6 + cost + count sums, rows sorted by (extrinsic, tile)
    DevBuf n_valid_dev;                   // one int: the correspondences mlh_calib_accumulate has appended
    DevBuf eval;                          // mlh_calib_evaluate: the extrinsics, residuals and Jacobian rows
    std::vector<int> h_tile_ext;
    int n_tiles = 0, n_appends = 0, n_given = 0, max_ext = -1;   // n_given: factors handed over by mlh_calib_add
    int lists_n_ext = -1;                 // the extrinsic count `lists` was made for (-1: stale)
    bool in_use = false, device_built = false;
};

// The Scan Context store (scancontext.hip; mloam_loop/src/scan_context.cpp:155-323): per entry the descriptor (f32, num_ring x num_sector, column-major), the ring
// key (f32 x num_ring), the sector key and the column norms (f64 x num_sector each), appended; the positions and the period bookkeeping on the host.
struct ScBatchStats {                      // the last mlh_sc_add_keyframes (mlh_sc_batch_info without the plan's constants)
    int n_entries = 0, n_chunks = 0, launches = 0, host_waits = 0, first_index = 0;
    long long n_points = 0, host_decided = 0, skipped = 0;
};
struct ScStore {
    mlh_sc_opts opts;
    bool configured = false;
    DevBuf desc, ring_key, sector_key, col_norm;
    int n = 0, cap = 0;                   // entries, entries the four buffers have room for
    std::vector<double> pos;              // 3 per entry
    std::vector<unsigned char> has_pos;
    ScBook book;
    DevBuf unc;                           // float4 {x, y, z', ring} of the points an add left undecided
    DevBuf counters;                      // ints: [0] undecided, [1] skipped (non-finite)
    DevBuf keys;                          // one u64 per searched entry: (f32 bits of the key distance) << 32 | index
    DevBuf work;                          // a query's small arrays (scancontext.hip: ScWork)
    PinnedBuf h_pin;                      // landing place of the counters, the undecided points, a query's result, a fetched entry
    int last_host_decided = 0, last_skipped = 0;
    long long points_host_decided = 0, points_skipped = 0;
    // the batched build (mlh_sc_add_keyframes)
    DevBuf unc_entry;                     // int per undecided point: its entry of the batch
    DevBuf batch_tab;                     // the call's tables: [ScBatchEntry per entry | ScChunk per chunk | n + 1 ints: the verdicts' range per entry]
    std::vector<unsigned char> htab;
    ScBatchStats batch;
};

// The loop closure's local registration (loopreg.hip; mloam_loop/src/pose_graph.cpp:364-419, loop_registration.cpp:104-211): the four clouds of constructLocalMap
// (model surf / corner, data surf / corner: float4 {x, y, z, intensity}, back to back at off[]), pre-filter and filtered, and the per-slot features of the matches.
struct LoopStore {
    DevBuf pre, flt, tab;
    int off[4] = {0, 0, 0, 0}, pre_n[4] = {0, 0, 0, 0}, flt_n[4] = {0, 0, 0, 0};
    std::vector<unsigned char> htab;
    DevBuf slots;                // double4 {w, d} per feature slot: one per surf data point, then two per corner data point
    DevBuf valid;                // one byte per feature slot
    DevBuf counts;               // ints: [0] surf, [1] corner features.size() of the last match
    PinnedBuf h_pin;             // landing place of the read-backs
    long long allocations = 0;
    unsigned long long cloud_gen = 0;                   // bumped by every build / set
    unsigned long long staged_gen = ~0ull, staged_epoch = ~0ull;   // the clouds and the stage_epoch the context's map indexes were staged from / left at
    float staged_sq[2] = {0.f, 0.f};
};

// FPFH + Fast Global Registration over the loop store's two filtered surf clouds (fgr.hip; mloam_loop/src/loop_registration.cpp:18-101, ThirdParty/
// FastGlobalRegistration/app.cpp). s = 0: the model surf cloud (pointcloud_[0]), s = 1: the data surf cloud. Everything per point is kept in the cloud's ORIGINAL order.
struct FgrStore {
    static constexpr unsigned long long NO_GEN = ~0ull;
    MapGrid grid[2];             // the self-index: grid.hip's build over {x, y, z, original index}, cell edge max(normal_radius, fpfh_radius)
    DevBuf ordered[2];           // the cell-sorted points with the order inside a cell fixed (ascending original index)
    DevBuf normals[2];           // float4 {nx, ny, nz, curvature}
    DevBuf spfh[2], nbr_k[2];    // int32 [n x 33] counts; int32 [n] fpfh_radius neighbours (the point itself included)
    DevBuf spfh_val[2];          // f32 [n x 33]: the counts as PCL's f32 bin values
    DevBuf feat[2];              // f32 [n x 33] FPFH (or a caller's descriptors)
    DevBuf npts[2];              // float4 normalised points (NormalizePoints)
    DevBuf nn[2];                // u64 (distance bits, row) keys: nn[s][r] = row r of cloud s's nearest row of the other cloud
    DevBuf scal;                 // 8 floats (per cloud: mean xyz, max norm) + 2 ints (pair count, pad)
    DevBuf pairs;                // FgrPair records
    PinnedBuf h_pin;
    int fn[2] = {0, 0};          // rows of feat[s]
    float index_edge[2] = {0.f, 0.f}, normals_radius[2] = {0.f, 0.f}, fpfh_radius[2] = {0.f, 0.f};
    unsigned long long index_gen[2] = {NO_GEN, NO_GEN}, normals_gen[2] = {NO_GEN, NO_GEN}, spfh_gen[2] = {NO_GEN, NO_GEN}, feat_gen[2] = {NO_GEN, NO_GEN};
    bool feat_user[2] = {false, false};      // feat[s] came through mlh_fgr_set_features / set_spfh / set_normals: mlh_fgr_register does not recompute it
    long long allocations = 0;
    int launches = 0, host_waits = 0;        // of the last call
    // the device tail (mlh_fgr_register_device; fgr.hip): the generator's jump table (uploaded once), the tuple test's per-segment counts and base ranks, the
    // correspondences, the tail's record and head words, the optimiser's working copy of (p, q) beyond the register-resident limit
    DevBuf rng_table, tt_counts, corres, tail, work;
    bool rng_table_ready = false;
};

// The loop closure's pose graph (posegraph.hip; mloam_loop/src/pose_graph.cpp:92-150, 491-653): one PgKeyframe record per keyframe in HBM, the work buffers of
// one optimisation (sized by its M keyframes and L loop edges), and the host's bookkeeping -- global_index_, earliest_loop_index_ and a mirror of the loop indices
// (what sizes a problem before anything is launched).
struct PgKeyframe {
    double pose[7], last[7], loop_rel[7];    // [t, q(xyzw)]: pose_w_, last_pose_w_, loop_info_
    int loop_index, pad;                     // -1: has_loop_ == false
};
static_assert(sizeof(PgKeyframe) == 176, "the pose graph's keyframe record: three poses and the loop index, 176 bytes");
struct PgStore {
    DevBuf kf;                   // PgKeyframe[count]
    DevBuf work;                 // one allocation carved into the buffers of an optimisation (posegraph.hip: pg_problem)
    DevBuf state;                // PgState
    PinnedBuf h_pin;
    std::vector<int> loop_index; // host mirror of PgKeyframe::loop_index
    std::vector<int> h_loops;    // the problem's loop list on its way to the device
    int count = 0, earliest_loop = -1;
    int max_loops = 128;                     // the capacity of loop edges of one problem (mlh_pg_reserve; pg_host.hpp: PG_MAX_LOOPS until then); mlh_pg_reset keeps it
    long long allocations = 0;
    int launches = 0, host_waits = 0;        // of the last call
    // the marginal covariances of (f18) (pgcov.inc): both forms (36 doubles per keyframe of marg_first .. marg_cur, the local form first), the buffers beyond an
    // optimise's, the blocks' landing place on the host. Allocated by the first mlh_pg_marginals only. marg_valid goes with the stored poses and loops it was
    // computed from (invalidate_marginals)
    DevBuf marg_out, marg_work;
    PinnedBuf h_marg;
    bool marg_valid = false;
    int marg_first = -1, marg_cur = -1;
    void invalidate_marginals() { marg_valid = false; marg_first = marg_cur = -1; }
};

// The session image (session.hip; session_host.hpp has the format): the staging image the pack kernel fills or checks, the call's tile table, the sections'
// checksum words, and what the last successful export / import did.
struct SessStore {
    DevBuf stage, tab, sums;
    PinnedBuf h_pin;             // the checksum words' landing place; the header on its way into a device dst
    std::vector<unsigned char> htab, himg;
    mlh_session_info last = {};
};

// The initial extrinsic calibration (initext.hip; estimator/src/initial/initial_extrinsics.cpp): Q_ and v_pose_ in HBM, one IeRecord per LiDAR (calib_ext_, the
// singular values and the flags of the last solve), and the host's bookkeeping (initext_host.hpp: IeBook -- options, the heap, pose_laser_add_, the cov states).
// Everything is made by mlh_initext_reset: a context that never calls it holds null pointers.
struct IeBook;
struct IeRecord {
    double q[4], t[3];                       // calib_ext_: q (x, y, z, w), t
    double rot_sv[4], trans_sv[4];           // descending
    int rot_ran, rot_converged, trans_solved, trans_rank, rot_sweeps, trans_sweeps;
};
static_assert(sizeof(IeRecord) == 144, "the initial-extrinsics record: 15 doubles and 6 ints");
struct InitExtStore {
    DevBuf Q;                    // n_lidar x 1200 x 4
    DevBuf sets;                 // 300 x n_lidar x 7
    DevBuf rec;                  // IeRecord[n_lidar]
    PinnedBuf h_rec;
    std::shared_ptr<IeBook> book;
    long long allocations = 0;
    int launches = 0, host_waits = 0;        // of the last call
};

constexpr int FUSE_BLOCKS = 64;          // workgroups per kind of the fusion kernel: each leaves one partial bounding box of what it appended (frontend.hip)
constexpr int TRACK_SHELLS = 4;          // the tracker's index cells are 1/4 of its acceptance radius (track.hip: nearest_in_radius)
constexpr int TRACK_MAX_RING = 255;      // ring ids 0..255 (mloam_hip.h; track.hip: track_rings_kernel refuses anything else)
constexpr int TRACK_RING_SLOTS = TRACK_MAX_RING + 3;   // ring_start[0 .. 256] + the slot the walks' upper bound is clamped to
struct TrackSet {   // scan-to-scan odometry (track.hip): previous frame's clouds + indices, current frame's features
    MapGrid grid[2];
    DevBuf ring[2], ring_start[2], walk[2], cur[2], corr[2];
    int m[2] = {0, 0};
};
struct TrackArgs {
    int pose_sel = 0;
    const double *init_pose = nullptr;
    float dist_sq_thr = 25.f, nearby_scan = 2.5f;
    double huber_delta = 0.1;
    LaunchTail finish = TAIL_RECORDS;        // track_linearize_launch: TAIL_LM_BEGIN / TAIL_LM_STEP (solver_dev.hpp has the bodies)
    int lm_max_it = 4, lm_min_blocks = 10, stat_slot = -1;
    HostPublish *publish = nullptr;          // an LM begin / step / loop launch: it hands pose + done bits to the host (pinned memory)
    unsigned long long publish_seq = 0;
};

// The body-frame union of the LiDARs' mapping features (mlh_fuse_* / mlh_fused_cloud, frontend.hip). Appends never wait for the host: the record counts and the
// appends' partial bounding boxes stay on the device while `dirty`; mlh_fused_cloud publishes them once. n[] and minmax[] are the clouds' while !dirty. Nothing
// but frontend.hip and the predicates that recognise a fused cloud among a caller's inputs (is_fused_cloud / is_fused_pair) reads or writes the members.
struct FusedClouds {
    DevBuf pts[2];             // float4 {x,y,z,lidar index}
    int n[2] = {0, 0};         // valid when !dirty
    float minmax[2][6];        // folded by mlh_fused_cloud: the voxel filter of a fused cloud needs no bounds pass of its own
    bool dirty = false;
    size_t bound[2] = {0, 0};  // host-side upper bounds of the counts (capacity)
    DevBuf cnt;                // the two record counts, device side: a prefix table, one pair per append
    DevBuf part;               // per-append, per-kind, per-workgroup partial bounds of the appended points
    int parts = 0;             // appends since the reset
    PinnedBuf host;            // one FusedPublish
    unsigned long long seq = 0;
    void mark_dirty() { dirty = true; }
    void publish_empty()       // no records, boxes that contain nothing
    {
        n[0] = n[1] = 0;
        for (int k = 0; k < 2; ++k) for (int d = 0; d < 6; ++d) minmax[k][d] = d < 3 ? FLT_MAX : -FLT_MAX;
        dirty = false;
    }
    void take_published()      // what the publication launch left in `host`
    {
        const FusedPublish *pub = host.as<FusedPublish>();
        n[0] = pub->count[0]; n[1] = pub->count[1];
        for (int k = 0; k < 2; ++k) for (int d = 0; d < 6; ++d) minmax[k][d] = pub->box[k * 6 + d];
        dirty = false;
    }
};

// Launches of one context that read what ANOTHER context of the same device holds (mlh_fuse_add_scan_from, mlh_window_set_from_scan: its scan buffers;
// mlh_features_copy, mlh_keyframes_update_from_pose_graph: copies the call itself waits for). Ordered on the device, in two halves: borrow_begin makes the
// reader's stream wait for the owner's work so far (an event of the reader's on the owner's stream); borrow_end leaves, behind the reading launches, an event of
// the OWNER's on the reader's stream, which wait_readers makes the owner's next rewrite of its scan wait for. ONE reader context per owner: a second reader
// would record over the first one's event. The owner is idle while another thread borrows from it: `reader_pending` is the only word both threads touch.
struct ScanHandoff {
    hipEvent_t ev_handover = nullptr;      // the reader's: recorded on the owner's stream, waited for on the reader's
    hipEvent_t ev_reader = nullptr;        // the owner's: recorded on the reader's stream behind its reading launches
    std::atomic<bool> reader_pending{false};
    int wait_readers(mlh_ctx *ctx);                   // ctx: the owner, in front of whatever rewrites its scan buffers
    int borrow_begin(mlh_ctx *ctx, mlh_ctx *src);     // ctx: the reader (this struct's context), src: the owner
    int borrow_end(mlh_ctx *ctx, mlh_ctx *src);
};

struct Profile {
    unsigned mask = 0;     // bit k: bracket launches of kernel id k
    int every = 1;         // bracket every n-th launch of a kernel id only (event pairs cost ~6 us of host/queue time each)
    long long seen[MLH_K_COUNT] = {0};
    double total_ms[MLH_K_COUNT] = {0};
    long long launches[MLH_K_COUNT] = {0};
    struct Pending { int id; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
};

int fail(mlh_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess);

}  // namespace mlh

struct mlh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // What the device (and the part of it the solver's stream may use) admits, asked once at mlh_create (capi.hip: query_device_caps) -- the kernels whose
    // workgroups synchronise among themselves inside one launch (match.hip: lm_loop_kernel, track.hip: track_lm_loop_kernel) need EVERY workgroup resident at
    // once, and a plain launch checks nothing: the hosts gates them on loop_max_tiles[] instead of on a literal sized for a whole 256-CU part.
    struct DeviceCaps {
        int cu_count = 0;                 // hipDeviceProp_t::multiProcessorCount
        int cu_solver = 0;                // compute units the solver's stream may use (MLH_SOLVER_CU_MASK; otherwise all of them)
        bool solver_masked = false;
        bool staging_masked = false;      // the staging stream (mlh_map_set_pair_overlapped) exists and is confined to a part of the compute units (informational)
        int loop_demoted[3] = {-1, -1, -1};   // >= 0: a barrier was given up on -- the gate this context keeps below from then on
        int blocks_per_cu[3] = {0, 0, 0}; // hipOccupancyMaxActiveBlocksPerMultiprocessor: lm_loop_kernel<false>, lm_loop_kernel<true>, track_lm_loop_kernel
        int loop_max_tiles[3] = {0, 0, 0};// workgroups of those kernels the host will put behind one in-kernel barrier (0: never -- the launch-per-iteration forms)
        int blocks_per_cu_cov[2] = {0, 0};   // the same two numbers for lm_loop_kernel's MLH_FLAG_POSE_COV instantiations, which a flagged frame's last loop launch is
        int loop_max_tiles_cov[2] = {0, 0};
        unsigned long long loop_timeout_ticks = 0;   // a barrier wait longer than this many 100 MHz ticks gives the loop up (MLH_LOOP_TIMEOUT_US, default 20 ms)
        unsigned long long loop_launches = 0;        // frames / rounds solved through the one-launch loop
        unsigned long long loop_timeouts = 0;        // ... that came back with the barrier given up on
        unsigned long long loop_fallbacks = 0;       // ... and were solved again through the launch-per-iteration form (the caller got a pose, later)
    } caps;
    // The local maps are double-buffered: `map` points at the set the solvers read; mlh_map_set_pair_overlapped stages the NEXT frame's maps into the
    // other set on a second stream while a submitted solve still reads this one, then switches `map` (launches capture a set's device pointers when they
    // are enqueued, so solves already in flight keep theirs).
    mlh::MapGrid map_sets[2][2];
    mlh::MapGrid *map = map_sets[0];
    int map_set_cur = 0;
    hipStream_t stream2 = nullptr;            // staging stream of the overlapped path (created on first use)
    hipEvent_t ev_set_built[2] = {nullptr, nullptr};   // recorded on the staging stream when set s has been built (the host waits on it)

    mlh::FeatSet feat[2];
    mlh::ScanBuf scan;
    mlh::DevBuf state;       // SolverState
    mlh::DevBuf partials;    // NE_STRIDE doubles per fit/linearise tile (surf tiles, then corner tiles)
    int n_partial_tiles = 0;
    mlh::DevBuf oob_flag;    // map staging: bit k set = the cloud of kind k has points outside its grid box
    bool oob_init = false;
    mlh::DevBuf ticket;      // arrival counter of the fused GN finish
    // The Levenberg-Marquardt side of the solver chain (match.hip: lm_consume_launch). One owner: match.hip calls the methods, no other unit names a member.
    struct LmChain {
        mlh::DevBuf pp;                       // two LmState records of the consumer-side schedule: launch g reads [(g - 1) & 1], one workgroup of it writes [g & 1]
        unsigned long long count = 0;         // consumer launches so far
        mlh::DevBuf tagged;                   // lm_loop_kernel: the iterations' records as tagged words (reduce_dev.hpp: lmc_sum_records_tagged), two sets of 64 words per tile
        unsigned launch_seq = 0;              // ... and the launch number their tags carry (24 bits). Zero is never a tag
        hipError_t ensure_states(hipStream_t st)
        {
            if (pp.p) return hipSuccess;
            const hipError_t e = pp.ensure(2 * sizeof(mlh::LmState));
            return e != hipSuccess ? e : hipMemsetAsync(pp.p, 0, 2 * sizeof(mlh::LmState), st);
        }
        unsigned next_seq() const { const unsigned n = (launch_seq + 1u) & 0xffffffu; return n ? n : 1u; }
        // the tagged sets of a loop over `tiles` tiles; a fresh allocation and a wrap of the launch number clear the words
        hipError_t ensure_tagged(size_t tiles, hipStream_t st)
        {
            const size_t bytes = sizeof(unsigned long long) * 64 * tiles * 2;
            const bool clear = bytes > tagged.cap || next_seq() <= launch_seq;
            const hipError_t e = tagged.ensure(bytes);
            if (e != hipSuccess || !clear) return e;
            return hipMemsetAsync(tagged.p, 0, tagged.cap, st);
        }
        // the transitions: a consumer launch is certain; a loop launch with tagged records is
        void consumer_launch() { ++count; }
        void tagged_launch() { launch_seq = next_seq(); }
        mlh::LmState *state_in() const { return pp.as<mlh::LmState>() + ((count - 1) & 1); }
        mlh::LmState *state_out() const { return pp.as<mlh::LmState>() + (count & 1); }
        unsigned tag_base() const { return launch_seq << 8; }       // (launch number << 8; the iteration goes into the low byte)
    } lm;
    mlh::DevBuf stats;       // IterStatDev[...]
    mlh::DevBuf knn_q, knn_idx, knn_d;
    mlh::DevBuf tmp;         // H2D staging of caller records before packing
    mlh::DevBuf tmp_stage;   // the same for mlh_map_set_pair_overlapped, whose copies and pack kernels run on the staging stream beside the main stream's
    mlh::PinnedHalves h_pts;     // landing place of a caller's PAGEABLE scan points (mlh_scan_upload, MLH_SCAN_STAGE_PINNED=1)
    struct SolveSlot {                 // what mlh_scan2map_end needs to know about the solve whose record is SolveLedger::record(seq)
        enum Kind : int { GN /* mlh_gn_solve_begin* */, SCAN2MAP /* mlh_scan2map_begin* */, SCAN2MAP_NO_MAP /* ... on maps too small to optimise against: the start pose comes back */ } kind = GN;
        bool chained = false;
        double start[7] = {0, 0, 0, 0, 0, 0, 1};
        mlh_solver_opts opts;
        unsigned long long epoch = 0;  // stage_epoch at submission
        bool tainted = false;          // chained behind a frame whose LM loop outgrew its look-ahead: began from an unfinished pose (mlh_scan2map_end status 3)
        int loop_tiles = 0;            // > 0: the frame's LM loops were submitted as one launch each over this many workgroups (lm_loop_kernel)
    };
    // The solves submitted with mlh_gn_solve_begin* / mlh_scan2map_begin* and not yet collected: at most two, numbered from 1 in submission order; solve `seq` publishes
    // into its own pinned record and is described by slot[seq & 1].
    struct SolveLedger {
        mlh::PinnedBuf records;                                   // HostPublish x 2
        unsigned long long submitted = 0, collected = 0;          // (at most two apart)
        unsigned long long set_reader[2] = {0, 0};                // the youngest submitted solve that reads map set 0 / 1
        SolveSlot slot[2];
        int lm_lookahead_auto = 10;       // mlh_scan2map_begin(lm_lookahead = 0): the previous frame's largest LM iteration count + 2 (10 until a frame has been collected)
        int in_flight() const { return int(submitted - collected); }
        bool pending() const { return submitted != collected; }
        mlh::HostPublish *record(unsigned long long seq) const { return records.as<mlh::HostPublish>() + (seq & 1); }
        // the next solve's number, record and slot -- or `refusal` (MLH_ERR_STATE) while two are in flight. Nothing is counted until commit().
        int admit(mlh_ctx *ctx, const char *refusal, unsigned long long *seq, mlh::HostPublish **rec, SolveSlot **s)
        {
            if (in_flight() >= 2) return mlh::fail(ctx, MLH_ERR_STATE, refusal);
            const hipError_t e = records.ensure(2 * sizeof(mlh::HostPublish), 0, true);      // one record per solve in flight
            if (e != hipSuccess) return mlh::fail(ctx, MLH_ERR_HIP, "pinned records of the solves in flight", e);
            *seq = submitted + 1; *rec = record(*seq); *s = &slot[*seq & 1];
            return MLH_OK;
        }
        // solve `seq` has been enqueued; reader_of_set >= 0: its launches read that map set (mlh_map_set_pair_overlapped rewrites a set only behind its readers)
        void commit(unsigned long long seq, int reader_of_set)
        {
            submitted = seq;
            if (reader_of_set >= 0) set_reader[reader_of_set] = seq;
        }
        unsigned long long oldest() const { return collected + 1; }
        void retire(unsigned long long seq) { collected = seq; }
        bool set_has_reader(int set) const { return set_reader[set] > collected; }
        // a younger solve chained behind `seq` began from whatever pose that one left on the device: if `seq` did not produce a result, neither did that one
        void taint_successor(unsigned long long seq) { if (pending() && slot[(seq + 1) & 1].chained) slot[(seq + 1) & 1].tainted = true; }
    } solves;
    // Bumped on entry by every call that restages a map or a feature set (also when it then fails: the set is disturbed). A frame in flight remembers the value it was
    // submitted under (SolveSlot::epoch); mlh_scan2map_end re-solves it only while that value stands: a re-solve is only sound on the inputs the frame was submitted with.
    unsigned long long stage_epoch = 0;
    bool map_read_unsynced = false;   // a launch that reads the current map set was enqueued and its call did not wait for it (mlh_pure_odom_add_matches)
    // mlh_scan_upload_ahead: the NEXT scan's points copied to the device on a stream of their own (the copy engine beside this frame's kernels); the mlh_scan_upload
    // that names the same host buffer packs from `buf` instead of copying
    struct ScanAhead {
        hipStream_t cs = nullptr;
        mlh::DevBuf buf;
        hipEvent_t ev_arrived = nullptr, ev_consumed = nullptr;
        const void *src = nullptr;
        int n = 0, stride = 0;
        bool valid = false, consumed_recorded = false, src_pinned = false;
        unsigned long long issued = 0, used = 0;     // (tests)
    } ahead;
    mlh::PinnedBuf h_state;  // three HostPublish records the device writes the result pose(s) into (solve_host.hip: publish_slot)
    mlh::PinnedBuf h_occ;    // mirror of the two maps' occupancy totals (grid.hip): {cells, squares} per kind, written behind every index build
    unsigned long long publish_seq = 0;
    // mlh_scan2map_cov: the two matrices of the most recently collected scan2map solve, copied out of its pinned record at collection (solve_host.hip: pose_cov_*)
    struct PoseCov {
        enum State : int { NONE /* nothing collected yet */, VALID, UNFLAGGED /* collected without MLH_FLAG_POSE_COV */, NOT_A_RESULT /* its pose_out was not a result */ } state = NONE;
        double H[36], cov[36];
    } pose_cov;
    mlh::DevBuf uct_buf;     // point-uncertainty scratch
    mlh::VoxBuf vox;
    mlh::KfStore kf;         // keyframe store + local map (keyframes.hip)
    mlh::WinStore win;       // the odometry's sliding window + its local maps (window.hip)
    mlh::OdomSet odom;
    mlh::MargPrior marg;     // the window's prior (marg.hip)
    mlh::CalibStore calib;   // the accumulated calibration features (calib.hip)
    mlh::ScStore sc;         // the Scan Context store (scancontext.hip)
    mlh::LoopStore loop;     // the loop closure's local maps and matches (loopreg.hip)
    mlh::FgrStore fgr;       // FPFH + Fast Global Registration over the loop store's surf clouds (fgr.hip)
    mlh::PgStore pg;         // the loop closure's pose graph and its optimisation (posegraph.hip)
    mlh::SessStore sess;     // the session image's staging and the last export / import (session.hip)
    mlh::InitExtStore ie;    // the initial extrinsic calibration (initext.hip)
    mlh::SegBuf seg;
    mlh::TrackSet track;
    mlh::FusedClouds fused;  // body-frame union of the LiDARs' mapping features (mlh_fuse_*)
    mlh::PinnedBuf h_dev_err;   // one int a kernel sets when it has to give up (device std::sort: a wait that was never released); see device_error_check
    mlh::PinnedHalves h_rings;  // the ring tables of mlh_scan_upload on their way to the device
    mlh::ScanHandoff handoff;              // this context as the reader, or the owner, of a cross-context read
    mlh::PinnedBuf h_sync;                 // the word stream_wait_spin's launch stores into
    unsigned long long sync_seq = 0;
    unsigned long long counts_seq = 0;      // publications of the thinned feature counts straight from a kernel (voxel.hip)
    // downsample_current_scan_pair_run(.., defer = true): the thinning was enqueued and NOT waited for -- where its two counts will be (device; pinned host + the
    // sequence number their publication carries)
    const int *thin_counts_dev = nullptr;
    const int *thin_counts_host = nullptr;
    const unsigned long long *thin_seq_host = nullptr;
    unsigned long long thin_seq = 0;
    // the form the most recent mlh_downsample_current_scan_pair / mlh_downsample_scan2map took (mlh_thin_info): host words, stored where the decision is made
    struct ThinNote {
        int path = MLH_THIN_NONE, n_in[2] = {0, 0};
        void begin(int n_surf, int n_corner) { path = MLH_THIN_NONE; n_in[0] = n_surf; n_in[1] = n_corner; }
    } thin_note;
    mlh::PinnedBuf h_scratch;  // one ScratchBlock: the landing place of the few-int read-backs (record counts) that end a staging call
    int knn_lanes_override = 0;   // MLH_KNN_LANES=8|16|32, or SSCC (816, 832, 1632: surf lanes, corner lanes), in the environment at mlh_create: pins the correspondence kernel's lanes per query (tests, tuning)
    int knn_wg_override = 0;      // MLH_KNN_WG_THREADS=256|512|1024, in the environment at mlh_create: pins the workgroup width of the correspondence launches that have wide forms (match_plan_host.hpp: knn_plan_width; tests, A/B runs)
    int knn_wg_last = 0;          // the width the last such launch took
    int gn_final_defer = 1;       // mlh_set_gn_schedule: 0: a solve submitted with mlh_gn_solve_begin* finishes its LAST iteration in its own fit launch (classic); 1: that
                                  // iteration, too, only leaves its records -- the next mlh_gn_solve_begin_chained completes it in its first launch (and publishes the pose
                                  // from there), mlh_gn_solve_end or any other solver call completes it with a one-workgroup launch if no successor did
    // An iteration's records: where a Gauss-Newton iteration that finished nothing left what the next launch's prologue sums (match.hip: prologue_reads).
    struct GnRecords {
        double *p = nullptr;      // device; null: the context's `partials` (the fit launch's tile records)
        int rows = 1;             // per 256-feature tile: 1 record (fit_linearize_kernel's) or 4 wavefront rows (a fused launch's, in GnChain::rows)
        int tiles = 0;            // 256-feature tiles
    };
    struct GnPending {            // the last iteration of the newest submitted solve is still a set of records
        bool active = false;
        GnRecords recs;
        int slot = 0, freeze = 0; // the SolverState::xi slot of the pose those records update
        double thre = 100.0;
        void *rec = nullptr;      // HostPublish of that solve
        unsigned long long seq = 0;
    };
    // The fit in the tail of the search launch (match.hip: knn_features_wide_kernel<.., FIT>; match_plan_host.hpp: knn_fit_in_search).
    int gn_fit_in_search = -1;    // -1: the rule (chip-filling wide launches fuse); MLH_GN_FIT_IN_SEARCH=0|1 in the environment at mlh_create pins it: none / every launch that can (tests, A/B runs)
    int gn_fused_launches = 0;    // fused launches the last submitted Gauss-Newton solve enqueued
    // The Gauss-Newton chain: what an iteration leaves for the launch behind it, and a submitted solve for its successor. One owner: match.hip and solve_host.hip
    // call the transitions, no other unit names a member (tests/test_abi.py); the slot arithmetic is solve_plan_host.hpp's.
    struct GnChain {
        GnPending pending;
        GnRecords last;           // the newest iteration that left records
        mlh::DevBuf rows;         // two sets of wavefront rows (4 x NE_STRIDE doubles per 256-feature tile), half the buffer each, a set beginning at a multiple of 256 bytes:
        int rows_set = 0;         // a fused launch writes the set its prologue does not read (a fast workgroup stores its row while a slow one still sums); the set last written
        int slot_base = 0;        // xi slots of the next submitted solve
        static size_t rows_bytes(int tiles256) { return 2 * sizeof(double) * mlh::NE_STRIDE * 4 * size_t(tiles256) + 512; }
        bool rows_hold(int tiles256) const { return rows_bytes(tiles256) <= rows.cap; }
        double *rows_ptr(int set) const { return reinterpret_cast<double *>(static_cast<char *>(rows.p) + size_t(set) * ((rows.cap / 2) & ~size_t(255))); }
        // a launch left its iteration: its fit launch's tile records in `partials`, or (fused) the other set of wavefront rows
        void launch_left(bool fused, int tiles)
        {
            last = GnRecords{nullptr, 1, tiles};
            if (fused) { rows_set ^= 1; last.p = rows_ptr(rows_set); last.rows = 4; }
        }
        // a submitted solve takes its pair of xi slots; the next one gets the other
        int solve_begins() { const int base = slot_base; slot_base = mlh::gn_next_slot_base(base); return base; }
        // ... and left its last iteration as the records `last` names, its pose in its last slot
        void solve_left_last(int base, int n_iters, double thre, void *rec, unsigned long long seq) { pending = GnPending{true, last, mlh::gn_last_slot(base, n_iters), 0, thre, rec, seq}; }
        // a successor's first launch consumed the pending iteration, or gn_flush_pending completes it: what it was
        GnPending take_pending() { const GnPending p = pending; pending.active = false; return p; }
    } gn;
    int gn_defer = 1;             // mlh_set_gn_schedule: 0: Gauss-Newton solves keep the classic finish (the fit kernel's last-arriving workgroup) in every iteration (A/B, tests)
    int knn_warm = 1;             // mlh_set_gn_schedule: 0: iterations >= 1 of a solve search without the previous iteration's neighbours as a bound (A/B, tests)
    // multi-GPU
    bool shard_lo = false, shard_hi = false;
    float lo_plane[4] = {0, 0, 0, 0}, hi_plane[4] = {0, 0, 0, 0};
    int own_mod = 1, own_rem = 0;   // feature-index ownership (replicated map): mlh_shard_set_features
    void *comm = nullptr;    // ncclComm_t
    // the mailbox communicator (comm.hip): every rank's mailbox mapped into this process; one kernel per all-reduce, no library in between
    struct P2p {
        bool active = false;
        void *mailbox = nullptr;                      // this rank's own (device memory, exported through hipIpc)
        void *peer[16] = {};                          // rank r's mailbox as this process sees it (peer[rank] == mailbox)
        void *counter = nullptr;                      // device word: exchanges completed (its parity picks the half of the mailboxes in use)
    } p2p;
    mlh::DevBuf allreduce_buf;   // staging of mlh_allreduce_f64
    int extract_tie_ref = 1;           // extractCloud, equal curvatures inside a sector: 1 = the order the reference's std::sort call leaves (default), 0 = (curvature, index)
    int vox_member_order = 1;          // voxel filters, members of a voxel: 1 = in the order libstdc++'s std::sort leaves them (the reference's), produced on the device
                                       // (stdsort.hip); 2 = the same through a host pass that calls the platform's own std::sort; 0 = in point-index order
    mlh::DevBuf stdsort;               // scratch of device_std_sort_by_key
    mlh::PinnedBuf vox_order_host;  // staging of that host pass (voxelgrid.hip): [slot n][members n]
    mlh::PinnedBuf select_host[2];  // staging of the good-feature selection, per feature kind (select.hip)
    std::vector<char> select_rows[2];   // the same rows in ordinary (CPU-cached) memory: what the selection loops read
    unsigned long long select_seq[2] = {0, 0};  // stream_flag_post after each kind's copies to the host
    bool select_staged[2] = {false, false};
    long select_fps_start[2] = {-1, -1};        // 'fps': the starting point drawn at staging time
    struct { int active = 0, m = 0, n_use = 0, cur0 = 0; void *host_dst = nullptr; } fps_pending[2];   // 'fps': a kind's loop staged but not yet launched (select.hip: good_feature_fps_flush)
    int n_ranks = 1, rank = 0;
    mlh::Profile prof;
};

namespace mlh {

// MLH_CHECK_LAUNCH=1 (debug runs): hipGetLastError() right behind EVERY kernel launch, so that a bad launch configuration is reported under the name of the kernel
// that caused it instead of surfacing at the next synchronisation under another call's name. The error is sticky for the calling thread: the next MLH_HIP check
// (every entry point runs several) returns MLH_ERR_HIP with "launch of <kernel>: <hip error>". Off (the default) the launches are followed by nothing.
bool launch_check_enabled();
void launch_check(const char *kernel);
hipError_t launch_check_take(const char **kernel);      // this thread's sticky launch error (hipSuccess when none); cleared by the call
int fail_launch(mlh_ctx *ctx, const char *kernel, hipError_t e);
#define MLH_LAUNCH(kern, grid, block, lds, st, ...)                                \
    do {                                                                           \
        hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);               \
        if (::mlh::launch_check_enabled()) ::mlh::launch_check(#kern);             \
    } while (0)

#define MLH_HIP(ctx, expr)                                                         \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) return ::mlh::fail((ctx), MLH_ERR_HIP, #expr, _e);   \
        if (::mlh::launch_check_enabled()) {                                       \
            const char *_k = nullptr;                                              \
            const hipError_t _le = ::mlh::launch_check_take(&_k);                  \
            if (_le != hipSuccess) return ::mlh::fail_launch((ctx), _k, _le);      \
        }                                                                          \
    } while (0)

inline int ScanHandoff::wait_readers(mlh_ctx *ctx)
{
    if (reader_pending.exchange(false, std::memory_order_acq_rel)) MLH_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev_reader, 0));
    return MLH_OK;
}
inline int ScanHandoff::borrow_begin(mlh_ctx *ctx, mlh_ctx *src)
{
    if (!ev_handover) MLH_HIP(ctx, hipEventCreateWithFlags(&ev_handover, hipEventDisableTiming));
    MLH_HIP(ctx, hipEventRecord(ev_handover, src->stream));
    MLH_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev_handover, 0));
    return MLH_OK;
}
inline int ScanHandoff::borrow_end(mlh_ctx *ctx, mlh_ctx *src)
{
    ScanHandoff &owner = src->handoff;
    if (!owner.ev_reader) MLH_HIP(ctx, hipEventCreateWithFlags(&owner.ev_reader, hipEventDisableTiming));
    MLH_HIP(ctx, hipEventRecord(owner.ev_reader, ctx->stream));
    owner.reader_pending.store(true, std::memory_order_release);
    return MLH_OK;
}

// ---- intake of a caller's records (records.hpp, capi.hip): every entry point that takes a cloud validates it with records_check (MLH_ERR_INVALID, mlh_last_error
// = "<entry>: bad <argument>") and reads it where records_stage says; the *_run functions below take records their entry point has validated
int records_check(mlh_ctx *ctx, const char *entry, const mlh::Records &r, bool allow_empty = false);
// *dev = where kernels read the records: the caller's own pointer (MLH_MEM_DEVICE), or `staging` + `at` bytes behind a copy enqueued on `st` (MLH_MEM_HOST; whoever
// stages several clouds into one buffer sizes it first). Which buffer stages is the caller's choice: it encodes which streams may still be reading which buffer.
int records_stage(mlh_ctx *ctx, const mlh::Records &r, mlh::DevBuf &staging, hipStream_t st, const unsigned char **dev, size_t at = 0);
// the one pack kernel: records -> float4 {x, y, z, w} (+ the covariance diagonal when covd != nullptr); w = the f32 at byte offset w_off >= 0, or one of
enum { PACK_W_ZERO = -1, PACK_W_INDEX = -2 /* the record's index, as int bits */, PACK_W_VALUE = -3 /* w_value */ };
void pack_points_launch(hipStream_t st, const unsigned char *dev, int stride, int n, int w_off, float w_value, int cov_off, float4 *out, float4 *covd);
int stage_points(mlh_ctx *ctx, const mlh::Records &r, int w_off, mlh::DevBuf &dst, mlh::DevBuf *covd, mlh::DevBuf &tmp, const unsigned char **dev_src = nullptr);
// "hex[,hex...]" -> CU-mask words / the first half of the device's compute units as mask words (capi.hip; the solver's and the staging stream's masks)
std::vector<uint32_t> parse_cu_mask(const char *text, int cu_count);
std::vector<uint32_t> lower_half_cu_mask(int cu_count);

// profiling brackets (HIP events on the context's stream)
void prof_begin(mlh_ctx *ctx, int id);
void prof_end(mlh_ctx *ctx, int id);
void prof_collect(mlh_ctx *ctx);
// events whose timestamps come from the dispatch itself (hipExtLaunchKernelGGL); false when kernel id is not profiled
bool prof_kernel_events(mlh_ctx *ctx, int id, hipEvent_t *start, hipEvent_t *stop);

// extract.hip, scan.hip
int extract_run(mlh_ctx *ctx);
int scan_totals(mlh_ctx *ctx, bool want_vox);
// voxel.hip
int ring_voxel_run(mlh_ctx *ctx, float leaf);
// track.hip
int track_set_prev_rings(mlh_ctx *ctx, int kind, const unsigned char *d_src, int stride, int n, int intensity_off, int *host_bad);
int track_match_launch(mlh_ctx *ctx, int kind_mask, const mlh::TrackArgs &a);
int track_linearize_launch(mlh_ctx *ctx, int kind_mask, const mlh::TrackArgs &a);
int track_lm_loop_launch(mlh_ctx *ctx, int kind_mask, const mlh::TrackArgs &a);      // one round's whole LM loop (begin at the round's pose .. termination) in one launch
// odom.hip
int pure_odom_add_matches(mlh_ctx *ctx, int kind, int frame_idx, int ext_idx);
// solve_host.hip: what mlh_pure_odom_add_matches, mlh_pure_odom_add_matches_gf and mlh_calib_accumulate begin with -- the state, rel_pose into it, one match pass
// of `kind` whose correspondences (validity + f32 coefficients) stay in HBM
int match_for_factors(mlh_ctx *ctx, int kind, const double rel_pose[7], int k_neigh, uint32_t flags, float min_match_sq_dis, float min_plane_dis);
int pure_odom_feature_rows(mlh_ctx *ctx, int kind, const double pivot[7], const double pose_i[7], const double ext[7]);      // odom.hip: validity + scored rows of the staged features -> FeatSet::flag8 / J
// the table's normal equations at the given state enqueued into OdomSet::ne_out (zeros for an empty table), the poses left in OdomSet::poses; nothing waited for
// calib.hip: the store of accumulated LidarOnlineCalib factors and its term in the window's normal equations
int calib_accumulate(mlh_ctx *ctx, int kind, int ext_idx);       // appends the valid correspondences the last match pass of `kind` left in HBM
bool calib_active(const mlh_ctx *ctx);                            // in use and not empty: the calls below have something to add
int calib_ne_prepare(mlh_ctx *ctx, int n_ext);                    // MLH_ERR_INVALID when n_ext does not cover the store; buffers and tile lists for this n_ext
// two launches behind the assembly: tile sums at the extrinsics of poses_dev ([pivot | frames | extrinsics], 7 each), then their addition into ne_dev (D*D + D + 2)
void calib_ne_enqueue(mlh_ctx *ctx, const double *poses_dev, int n_frames, int n_ext, double huber_delta, double *ne_dev);
int window_assemble(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext, double huber_delta);
// marg.hip
// MLH_OK, or MLH_ERR_STATE (text set) when the installed prior's block map -- or, with ext_bit, the extrinsic prior that bit enables -- does not fit the window
int window_prior_fits(mlh_ctx *ctx, const char *entry, int n_frames, int n_ext, uint32_t ext_bit);
bool window_prior_in_solve(const mlh_ctx *ctx);      // a prior, or extrinsic rows with bit 1, is installed: mlh_pure_odom_gn_solve adds the term
// one launch: the prior's term (and the extrinsic rows `ext_bit` enables) at the poses in `poses_dev` added into `ne_dev`; nothing when neither is installed
void window_prior_term_enqueue(mlh_ctx *ctx, const double *poses_dev, int n_frames, int n_ext, double *ne_dev, uint32_t ext_bit, double *res_out);
// voxelgrid.hip
int device_exclusive_scan(mlh_ctx *ctx, int *data, long long n, mlh::DevBuf &sums, int *grand_total);
// A kernel that cannot honour its contract (today: the device std::sort when a queue wait runs out, or a range it was never told about) sets
// the context's pinned error word instead of leaving a wrong order behind silently; every call that waits for the stream afterwards reports it.
inline int *device_error_word(mlh_ctx *ctx)
{
    (void)ctx->h_dev_err.ensure(sizeof(int), 0, true);       // (nullptr on allocation failure)
    return ctx->h_dev_err.as<int>();
}
inline int device_error_check(mlh_ctx *ctx)
{
    int *word = ctx->h_dev_err.as<int>();
    if (word && *static_cast<volatile int *>(word) != 0) {
        const int code = *word;
        *word = 0;
        if (code == 2)
            return fail(ctx, MLH_ERR_STATE, "a peer rank did not arrive at a mailbox exchange within 5 s: the normal equations were NOT summed over the job, no update was applied from them, "
                                            "and the ranks may no longer hold the same pose -- the result of this call is not valid");
        return fail(ctx, MLH_ERR_STATE, "a device kernel gave up (std::sort emulation: unreleased wait or an unannounced range); the results of this call are not valid");
    }
    return MLH_OK;
}
// One turn of a host-side wait on a pinned word (the publications of the solves, the staging hand-shakes, the few-int read-backs): those waits are microseconds
// long, so the default is to spin (`pause`) -- a sleeping thread's wake-up costs tens. A process with one thread per LiDAR + the mapper + the tracker, each in
// such a wait, burns that many cores; MLH_HOST_WAIT=yield (read once per process) spins the first 64 turns (~2 us: the common case still pays nothing) and then
// gives the core to whoever is runnable between two looks. Either way a wait falls back to the blocking hipStreamSynchronize after 200 ms (host_spin below).
inline void host_wait_relax(unsigned spins)
{
    static const bool yield_mode = [] { const char *e = std::getenv("MLH_HOST_WAIT"); return e && std::strcmp(e, "yield") == 0; }();
    if (yield_mode && spins > 64u) { sched_yield(); return; }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}
// THE host-side wait: looks (acquire loads of a pinned word, an event query) with host_wait_relax between them, the clock read every 1024 looks. True: `arrived`
// held at a look; false: it did not for 200 ms (a long LM run, a profiler, a fault) -- the caller goes on to the blocking wait on its stream.
template <typename Arrived> inline bool host_spin(Arrived arrived)
{
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (!arrived()) {
        if ((++spins & 0x3ff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return false;
        host_wait_relax(spins);
    }
    return true;
}
// ... with that blocking wait on `st`, which also surfaces errors. `late` (may be null): the failure (MLH_ERR_HIP) when `arrived` does not hold even behind it.
template <typename Arrived> inline int host_wait(mlh_ctx *ctx, Arrived arrived, hipStream_t st, const char *late)
{
    if (host_spin(arrived)) return MLH_OK;
    MLH_HIP(ctx, hipStreamSynchronize(st));
    if (late && !arrived()) return fail(ctx, MLH_ERR_HIP, late);
    return MLH_OK;
}
// the publication that ends such a wait: `word` holds exactly `seq` (a sequence number stored with system-scope release behind the data it announces)
inline int host_wait_seq(mlh_ctx *ctx, const unsigned long long *word, unsigned long long seq, hipStream_t st, const char *late)
{
    return host_wait(ctx, [=] { return __atomic_load_n(word, __ATOMIC_ACQUIRE) == seq; }, st, late);
}
// the context's pinned ScratchBlock (lazily allocated); nullptr on allocation failure
inline ScratchBlock *scratch_block(mlh_ctx *ctx)
{
    (void)ctx->h_scratch.ensure(sizeof(ScratchBlock));
    return ctx->h_scratch.as<ScratchBlock>();
}
// Everything enqueued on the context's stream so far (kernels, and copies into PINNED host memory) has completed when this returns. A one-thread launch stores a
// sequence number into pinned host memory (system-scope release) and the host spins on that word: a few microseconds, where hipStreamSynchronize's wake-up
// costs tens -- a mapper frame has three such read-backs (fused cloud sizes, thinned record counts, feature counts). Falls back to the blocking call after
// 200 ms (a profiler, a fault). solve_host.hip has the definition.
hipError_t stream_wait_spin(mlh_ctx *ctx);
// the two halves of it: post a marker behind what is enqueued now; wait for a posted marker later
hipError_t stream_flag_post(mlh_ctx *ctx, unsigned long long *seq_out);
hipError_t stream_flag_wait(mlh_ctx *ctx, unsigned long long seq);
// *out <- one device int, through the pinned block (a pageable landing place costs a staging hop); waits for the stream
inline hipError_t read_back_int(mlh_ctx *ctx, const void *dev, int *out)
{
    ScratchBlock *h = scratch_block(ctx);
    int *dst = h ? &h->read_back : out;
    hipError_t e = hipMemcpyAsync(dst, dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = h ? stream_wait_spin(ctx) : hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && h) *out = *dst;
    return e;
}
// stdsort.hip: vals_out <- the permutation of 0..n-1 that std::sort (libstdc++, comparator on the key only) leaves for keys[0..n0) and keys[n0..n)
// Voxel keys computed INSIDE the sort's init launch (the frame's thinning pipeline, voxel.hip: downsample_current_scan_pair_run): point i of cloud 0 (i < n0) or
// cloud 1 -> its voxel index in the cloud's own dense grid, the second grid numbered behind the first (the arithmetic of vox_mark_kernel / PCL's VoxelGrid).
struct VoxKeyGen {
    const unsigned char *src0, *src1;
    int stride, n0;
    float inv_leaf0, inv_leaf1;
    int min_b0[3], mul1_0, mul2_0;
    int min_b1[3], mul1_1, mul2_1, cell_off1;
};
int device_std_sort_by_key(mlh_ctx *ctx, const int *src_keys, int n0, int n, int *vals_out, const VoxKeyGen *gen = nullptr);
const int *device_std_sort_keys(mlh_ctx *ctx, int n);       // the keys of the last device_std_sort_by_key over n elements, sorted, once its launches have run
int device_std_sort_segments(mlh_ctx *ctx, const int *src_keys, const int *counts, const int *offsets, int stride, int field, int n_segments, int n, int longest,
                             int *vals_out, bool counters_cleared = false);
int *device_std_sort_counters(mlh_ctx *ctx, int n, int *n_counters);
void host_std_sort_permutation(const int *slot, int lo, int hi, int *members);   // voxelgrid.hip: the platform's own std::sort
// voxel.hip
void compound_pose_with_cov(const double p1[7], const double c1[36], const double p2[7], const double c2[36], double pc[7], double cc[36]);
int downsample_current_scan_run(mlh_ctx *ctx, const void *points, int stride, int n, int intensity_off, int mem, float leaf, const double *ext_poses,
                                const double *ext_covs, int n_lidar, const double cov_meas[9], int with_ua, double trace_thr, mlh::DevBuf &pts_out,
                                mlh::DevBuf &covd_out, float *out11_dev, int *n_out, const float *known_bounds = nullptr);
int voxel_filter_run(mlh_ctx *ctx, const void *points, int stride, int n, int intensity_off, int cov_off, int trace_off, float leaf,
                     float trace_thr, void *out_host, int *n_out, int mem, const float *known_bounds = nullptr, bool sync_total = true,
                     bool centroid_all = false);
// A filter whose result stays on the device, collected: voxel_filter_run over n > 0 device records with the bounds decoded from the cloud's six state words
// (bounds_dev.hpp) as the host read them back, then ctx->vox.out (n records' room: the filter never returns more) copied to `dst` and ctx->vox.total to the device
// word `count_word`. Nothing is waited for. voxelgrid.hip.
int voxel_filter_collect(mlh_ctx *ctx, const void *points, int stride, int n, int intensity_off, int cov_off, int trace_off, float leaf, float trace_thr,
                         const int enc_bounds[6], bool centroid_all, void *dst, int *count_word);
// cloudbuild.hip: stored clouds transformed and concatenated into map clouds, each then voxel-filtered (the odometry window's local maps, the loop closure's)
struct CloudSegment {                       // one stored cloud on its way into a map cloud; the caller lists them in destination order
    size_t src;                             // its first record in its arena
    int n;                                  // its records (0: contributes nothing)
    int xf;                                 // its transform in the call's table
    int cloud;                              // the output cloud it is appended to; odd: read from the second arena
};
struct CloudBuildBufs {                     // the calling store's own: clouds, table, their allocation counter, and a pinned landing place of >= 7 n_clouds ints
    DevBuf &pre, &flt, &tab;
    std::vector<unsigned char> &htab;
    long long &allocations;
    int *h_pin;
};
// Cloud c = its segments' records, each under its transform, back to back at record off[c] of B.pre (len[c] of them, as the caller summed them), and its
// pcl::VoxelGrid at leaf[c] at the same offset of B.flt, flt_n[c] records. ONE transform launch, one upload, two host waits. Without a record: MLH_OK at once,
// nothing touched, flt_n as the caller left it.
int stored_clouds_build(mlh_ctx *ctx, const float4 *arena_even, const float4 *arena_odd, const std::vector<FuseXf> &xfs, const std::vector<CloudSegment> &segs,
                        int n_clouds, const int *off, const int *len, const float *leaf, const CloudBuildBufs &B, int *flt_n);
// frontend.hip
void gather_points_launch(mlh_ctx *ctx, const float4 *pts, const int *list, int n, float4 *out);
int transform_cloud_launch(mlh_ctx *ctx, void *dev, int stride, int n, const double pose[7]);
int transform_to_end_launch(mlh_ctx *ctx, void *dev, int stride, int n, int intensity_off, const double pose[7], int b_distortion, float scan_period);
int fuse_append_launch(mlh_ctx *ctx, ScanBuf &sb, int ring_begin, int ring_end, int lidar_idx, const double ext_pose[7]);   // sb: this context's scan or another's (mlh_fuse_add_scan_from)
int voxel_filter_run2(mlh_ctx *ctx, const void *src0, int n0, const float bounds0[6], float leaf0, const void *src1, int n1, const float bounds1[6],
                      float leaf1, int stride, int intensity_off, int *first_voxels_word);
int downsample_current_scan_pair_run(mlh_ctx *ctx, const void *surf, int n_surf, const float bounds_surf[6], float leaf_surf, const void *corner, int n_corner,
                                     const float bounds_corner[6], float leaf_corner, int stride, int intensity_off, const double *ext_poses, const double *ext_covs,
                                     int n_lidar, const double cov_meas[9], int with_ua, double trace_thr, int *n_surf_out, int *n_corner_out, bool defer = false);
// keyframes.hip
void keyframes_release(mlh_ctx *ctx);
void global_map_release_run(mlh_ctx *ctx);
// window.hip
int window_reset_run(mlh_ctx *ctx, int n_lidar, int window_size);
// stack[lidar][slot] = the cloud of `kind`: n packed float4 records on the device (read on the context's stream), or none (n == 0). Arguments already validated.
int window_assign_device(mlh_ctx *ctx, int lidar, int slot, int kind, const float4 *dev, int n);
int window_check_slot(mlh_ctx *ctx, const char *entry, int lidar, int slot);     // MLH_ERR_STATE before mlh_window_reset, MLH_ERR_INVALID out of range
// grid.hip
int grid_build(mlh_ctx *ctx, int kind_mask, bool recompute_bounds);
int grid_build_grids(mlh_ctx *ctx, mlh::MapGrid **grids, int n_grids, bool recompute_bounds, int *pub_oob = nullptr, mlh::HostPublish *pub = nullptr,
                     unsigned long long pub_seq = 0);
void knn_lanes_for(const mlh_ctx *ctx, int kind_mask, int lanes[2]);
int map_stage_and_build(mlh_ctx *ctx, int n_maps, const int *kinds, const unsigned char *const *src, const int *n, int stride, const float *sq_dis,
                        mlh::HostPublish *pub, unsigned long long seq);
// match.hip (its launchers and their arguments: solve_host.hpp)
int gn_flush_pending(mlh_ctx *ctx);      // completes a pending last iteration with a one-workgroup launch (no-op when nothing is pending)
int lm_loop_occupancy(int blocks_per_cu[2], int blocks_per_cu_cov[2]);      // hipOccupancyMaxActiveBlocksPerMultiprocessor of lm_loop_kernel<false> / <true>; _cov: of the instantiations that publish the pose covariance
int track_loop_occupancy(int *blocks_per_cu);     // ... of track_lm_loop_kernel (track.hip)
// the arrival counters of the fused finishes and of lm_loop_kernel's barrier: four zeroed words, whoever asks first ([0]: the finish tickets of match.hip and
// track.hip; [1] arrivals, [2] departures, [3] release flag of the loop kernel). One place, so that no caller can leave the others' words unallocated or unzeroed.
// The schedule switches that select the reference forms of the solvers (the tests compare them bit for bit): "=0" in the environment takes the reference form. Read
// at every call: tests run both forms in one process.
//   LM_CONSUMER  MLH_LM_CONSUMER=0: scan2map's LM steps in the classic launches (the linearise kernel's last workgroup) instead of the consumer of the records
//   LM_LOOP      MLH_LM_LOOP=0: one launch per LM iteration instead of scan2map's whole LM loop in one launch (match.hip: lm_loop_kernel)
//   LOOP_TAGGED  MLH_LOOP_TAGGED=0: the one-launch loop exchanges plain records behind a grid barrier instead of tagged records, and keeps the fit launch of its own
//   TRACK_LOOP   MLH_TRACK_LOOP=0: track_cloud runs 2 + max_lm_iterations launches per round instead of two (track.hip: track_lm_loop_kernel)
enum class Schedule { LM_CONSUMER, LM_LOOP, LOOP_TAGGED, TRACK_LOOP };
inline bool schedule_on(Schedule s)
{
    const char *e = nullptr;
    switch (s) {
        case Schedule::LM_CONSUMER: e = std::getenv("MLH_LM_CONSUMER"); break;
        case Schedule::LM_LOOP: e = std::getenv("MLH_LM_LOOP"); break;
        case Schedule::LOOP_TAGGED: e = std::getenv("MLH_LOOP_TAGGED"); break;
        case Schedule::TRACK_LOOP: e = std::getenv("MLH_TRACK_LOOP"); break;
    }
    return !(e && std::atoi(e) == 0);
}

inline hipError_t ensure_ticket(mlh_ctx *ctx)
{
    if (ctx->ticket.p) return hipSuccess;
    hipError_t e = ctx->ticket.ensure(4 * sizeof(unsigned));
    if (e != hipSuccess) return e;
    return hipMemsetAsync(ctx->ticket.p, 0, 4 * sizeof(unsigned), ctx->stream);
}
int knn_launch(mlh_ctx *ctx, int kind, const float *q_host, int nq, int32_t *idx, float *d2);
// select.hip
}  // namespace mlh
#include <random>
namespace mlh {
int good_feature_select(mlh_ctx *ctx, int kind, int method, double ratio, std::mt19937 &rng, float min_match_sq_dis,
                        float min_plane_dis, std::vector<int32_t> &sel_out, double H[36], uint8_t *matched_out);
// its two halves: the dense pass + copies to the host, enqueued (no wait); the selection loop on the copied rows, flags sent back (no wait)
int good_feature_stage(mlh_ctx *ctx, int kind, int method, double ratio, std::mt19937 &rng, float min_match_sq_dis, float min_plane_dis, bool defer_fps = false);
int good_feature_fps_flush(mlh_ctx *ctx);          // launches what the stages called with defer_fps left pending (both kinds' 'fps' loops in one launch)
int odom_good_feature_select(mlh_ctx *ctx, int kind, float gf_ratio, std::mt19937 &rng, std::vector<int32_t> &sel_out);     // select.hip: Estimator::goodFeatureMatching's loop over those rows
int good_feature_finish(mlh_ctx *ctx, int kind, int method, double ratio, std::mt19937 &rng, std::vector<int32_t> &sel_out, double H[36],
                        uint8_t *matched_out);
// solver.hip
int reduce_only_launch(mlh_ctx *ctx, int to_ce);
int gn_update_prereduced_launch(mlh_ctx *ctx, double map_eig_thre, int stat_slot);
int gn_update_blocks_prereduced_launch(mlh_ctx *ctx, int n_blocks, const double *eig_thre, const int *freeze, int stat_slot);
// comm.hip
inline bool distributed(const mlh_ctx *ctx) { return ctx->comm != nullptr || ctx->p2p.active; }
int comm_allreduce_state(mlh_ctx *ctx, int to_ce);
int comm_allreduce_blocks(mlh_ctx *ctx, int n_blocks);
void comm_destroy(mlh_ctx *ctx);   // in-place ncclAllReduce of SolverState::ne / ::ce on the stream
int lm_begin_launch(mlh_ctx *ctx, double map_eig_thre, int max_iterations, int stat_slot, int min_blocks = 0, const double *init_pose = nullptr);
int lm_step_launch(mlh_ctx *ctx, int max_iterations, int stat_slot);
int lm_finish_launch(mlh_ctx *ctx, int stat_slot);
// loopreg.hip: what every entry of the loop process that runs kernels against the context's maps and solver state begins with (loop registration, FGR, the pose
// graph): refused while a submitted solve is uncollected (MLH_ERR_STATE) or under a communicator (MLH_ERR_UNSUPPORTED); then a pending last iteration is flushed
int loop_process_gate(mlh_ctx *ctx, const char *entry);

}  // namespace mlh
