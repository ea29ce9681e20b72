// Local-map index build for gfx950: a dense cell grid over the map cloud, points counting-sorted by cell.
// Replaces the FLANN kd-tree build the reference performs every frame
// (pcl::KdTreeFLANN::setInputCloud, estimator/src/lidarMapper/lidar_mapper_keyframe.cpp:433-434).
//
// Layout in HBM: raw[n] and sorted[n] as float4 {x, y, z, original index}; cell_start[ncell+1] (int32, exclusive prefix),
// cells ordered x fastest so the 3 x-adjacent cells of a query form ONE contiguous run of `sorted` (9 runs per query).
// One steady-state build = 4 launches for BOTH maps together (count, chunk-local scan, add, scatter); all streaming:
//   count   16 B/pt read + 1 returning atomic + 4 B rank      scan+add   16 B/cell + 4 B/cell (twin clear)
//   scatter 16 B + 4 B read, 16 B written per point, no atomics
// The count lands in cell_start[c+1] and the value the atomic returns is the point's rank inside its cell; the in-place
// INCLUSIVE scan turns slot c+1 into start[c+1], so with cell_start[0] = 0 the array is the exclusive prefix the queries read
// and the scatter writes to start[c] + rank. Two cell arrays alternate: the add pass of one build clears the other array,
// so the next build starts from zeros without a clear launch; with few chunks (<= 4096) the add pass also sums the chunk
// totals before it itself instead of a separate single-workgroup scan launch.
#include "ctx.hpp"
#include "solve_host.hpp"
#include "bounds_dev.hpp"
#include "wg_dev.hpp"
#include <cstdlib>
#include <vector>
#include <cmath>
#include <climits>

namespace mlh {

// bounding box as order-preserving integer keys (enc_f): one partial record per workgroup (no atomics: a few thousand wavefronts hammering six
// words cost 0.5 ms on a 500 k map), folded by the host, which needs the box for the grid dimensions anyway
constexpr int BOUNDS_BLOCKS = 128;
constexpr float GRID_MARGIN_XY = 2.f, GRID_MARGIN_Z = 1.f;
__global__ __launch_bounds__(256) void bounds_kernel(const float4 *__restrict__ pts, int n, int *__restrict__ partial)
{
    __shared__ int lds[4][6];
    int m[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 p = pts[i];
        int kx = enc_f(p.x), ky = enc_f(p.y), kz = enc_f(p.z);
        m[0] = min(m[0], kx); m[3] = max(m[3], kx);
        m[1] = min(m[1], ky); m[4] = max(m[4], ky);
        m[2] = min(m[2], kz); m[5] = max(m[5], kz);
    }
    int r;
    if (block_fold_bounds<1>(m, lds, r)) partial[blockIdx.x * 6 + threadIdx.x] = r;
}

// ---- one job per map; kernels take both jobs and split their grid between them
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_CHUNK = 256 * SCAN_ITEMS;
constexpr int FUSED_SUMS_MAX = 4096;   // chunk count up to which scan_add sums the chunk totals itself (no scan_sums launch)

struct GridJob {
    const float4 *raw;
    float4 *sorted;
    int *cell_start;       // ncell + 1: the array being built
    int *cell_next;        // the twin array, cleared here for the NEXT build
    int *rank;             // n: arrival rank of each point inside its cell
    int *block_sums;
    long long *occ_host;   // pinned host mirror of occ[0..1] (or null)
    int occ_parts;         // partials behind occ[2]
    long long *occ;        // occupancy statistics of this build (null: not wanted): [0] non-empty cells, [1] sum of squared cell populations,
                           // then one (cells, squares) partial per scanning workgroup
    int n;
    int ncell;
    float ox, oy, oz, inv_h;
    int nx, ny, nz;
    int nb_pts;            // workgroups streaming the points
    int nb_scan;           // workgroups scanning the cells
    int need_zero;         // the array being built was not cleared by the previous build
    int sums_scanned;      // block_sums already hold exclusive prefixes (large grids: scan_sums_kernel ran)
};
struct GridJobs {
    GridJob j[2];
    // optional: the staging pass's fit flags leave for the host in the first launch of the build (one thread), instead of a launch of their own
    int *pub_oob; HostPublish *pub; unsigned long long pub_seq;
    int pub_stage;         // 0: cell_count_kernel publishes (the clouds were packed by the launch before it); 1: scan_local_kernel does (pack_count_kernel packed them)
};

// a frame's local map arrives as a cloud of caller records: packed to float4 {x,y,z,index} and, in the same pass, checked against the grid box already set up for
// this kind (flag word, OR-ed)
struct PackJob { const unsigned char *src; float4 *out; int n, stride; float lo[3], hi[3]; int nb; };
struct PackJobs { PackJob j[2]; int *oob; };

__device__ __forceinline__ int cell_of(const GridJob &J, const float4 &p)
{
    float fx = fminf(fmaxf(floorf((p.x - J.ox) * J.inv_h), 0.f), float(J.nx - 1));
    float fy = fminf(fmaxf(floorf((p.y - J.oy) * J.inv_h), 0.f), float(J.ny - 1));
    float fz = fminf(fmaxf(floorf((p.z - J.oz) * J.inv_h), 0.f), float(J.nz - 1));
    return (int(fz) * J.ny + int(fy)) * J.nx + int(fx);
}

// cell_start lives 3 ints into its allocation, so A = cell_start + 1 (the array the scan works on) is 16-byte aligned
__device__ __forceinline__ void zero_chunk(int *cells, int ncell, int b)
{
    int4 *A4 = reinterpret_cast<int4 *>(cells + 1);
    const int base4 = b * (SCAN_CHUNK / 4) + threadIdx.x * 2;           // in int4 units
    const int n4 = (ncell + 3) / 4;                                      // allocation is padded to a multiple of 4 (+4)
    const int4 z = make_int4(0, 0, 0, 0);
    if (base4 < n4) A4[base4] = z;
    if (base4 + 1 < n4) A4[base4 + 1] = z;
    if (b == 0 && threadIdx.x == 0) cells[0] = 0;
}

__global__ __launch_bounds__(256) void zero_cells_kernel(GridJobs G)
{
    const int job = blockIdx.x >= G.j[0].nb_scan ? 1 : 0;
    const GridJob &J = G.j[job];
    if (!J.need_zero) return;
    zero_chunk(J.cell_start, J.ncell, job ? blockIdx.x - G.j[0].nb_scan : blockIdx.x);
}

// per-cell counts land in cell_start[c + 1]; the value the atomic returns is the point's rank inside its cell.
// Device-scope atomics execute at the memory side on a multi-XCD part and bound this kernel, so lanes are merged first: the
// map arrives ordered by voxel index, x fastest (it is the output of the voxel filter), i.e. neighbouring lanes usually fall
// into the same cell -- every run of equal cells inside a wavefront issues ONE atomic for the whole run (a cloud in random
// order degrades to one atomic per lane, as before).
__global__ __launch_bounds__(256) void cell_count_kernel(GridJobs G)
{
    const int job = blockIdx.x >= G.j[0].nb_pts ? 1 : 0;
    const GridJob &J = G.j[job];
    const int b = job ? blockIdx.x - G.j[0].nb_pts : blockIdx.x;
    const int lane = threadIdx.x & 63;
    if (G.pub && G.pub_stage == 0 && blockIdx.x == 0 && threadIdx.x == 0) {   // the packed clouds' fit flags: final before this launch started
        G.pub->done = *G.pub_oob;
        *G.pub_oob = 0;
        __hip_atomic_store(&G.pub->seq, G.pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    for (int base = b * 256; base < J.n; base += J.nb_pts * 256) {       // uniform over the workgroup
        const int i = base + threadIdx.x;
        const bool valid = i < J.n;
        const int c = valid ? cell_of(J, J.raw[i]) : -1 - lane;           // distinct negatives: never merged
        const int prev = __shfl_up(c, 1);
        const bool head = (lane == 0) || (c != prev);
        const unsigned long long H = __ballot(head);
        const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
        const int my_head = 63 - __clzll(H & upto);
        const unsigned long long above = (my_head == 63) ? 0ull : (H & ~((2ull << my_head) - 1ull));
        const int next = above ? (__ffsll((long long)above) - 1) : 64;
        int first = 0;
        if (head && valid) first = atomicAdd(&J.cell_start[c + 1], next - my_head);
        first = __shfl(first, my_head);
        if (valid) J.rank[i] = first + (lane - my_head);
    }
}

// pack + fit check + count in ONE pass over the caller's records (every staged kind keeps its grid geometry: the steady state of a mapper between keyframes): the
// record is read once, the packed point goes to raw[] and straight into cell_of() -- pack_check_kernel and cell_count_kernel as one launch (~6 us of a frame's
// index build and a kernel boundary). A point outside the box is counted in the clamped cell like any other; the flag it raises makes the host lay out a new box
// and build again, as before. The flags leave for the host from the NEXT launch (scan_local_kernel, pub_stage 1).
__global__ __launch_bounds__(256) void pack_count_kernel(GridJobs G, PackJobs P)
{
    const int job = blockIdx.x >= G.j[0].nb_pts ? 1 : 0;
    const GridJob &J = G.j[job];
    const PackJob &Q = P.j[job];
    const int b = job ? blockIdx.x - G.j[0].nb_pts : blockIdx.x;
    const int lane = threadIdx.x & 63;
    bool bad = false;
    for (int base = b * 256; base < J.n; base += J.nb_pts * 256) {       // uniform over the workgroup
        const int i = base + threadIdx.x;
        const bool valid = i < J.n;
        int c = -1 - lane;                                               // distinct negatives: never merged
        if (valid) {
            const float *rec = reinterpret_cast<const float *>(Q.src + size_t(i) * Q.stride);
            const float x = rec[0], y = rec[1], z = rec[2];
            const float4 p = make_float4(x, y, z, __int_as_float(i));
            Q.out[i] = p;
            bad = bad || !(x >= Q.lo[0] && x < Q.hi[0] && y >= Q.lo[1] && y < Q.hi[1] && z >= Q.lo[2] && z < Q.hi[2]);   // NaN -> bad
            c = cell_of(J, p);
        }
        const int prev = __shfl_up(c, 1);
        const bool head = (lane == 0) || (c != prev);
        const unsigned long long H = __ballot(head);
        const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
        const int my_head = 63 - __clzll(H & upto);
        const unsigned long long above = (my_head == 63) ? 0ull : (H & ~((2ull << my_head) - 1ull));
        const int next = above ? (__ffsll((long long)above) - 1) : 64;
        int first = 0;
        if (head && valid) first = atomicAdd(&J.cell_start[c + 1], next - my_head);
        first = __shfl(first, my_head);
        if (valid) J.rank[i] = first + (lane - my_head);
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(P.oob, 1 << job);
}

// in-place INCLUSIVE scan of A[i] = cell_start[i + 1], i in [0, ncell): chunk-local part (8 ints = 2 x int4 per thread).
// Inclusive, so that cell_start[c + 1] = start of cell c + 1 and (with cell_start[0] = 0) the array is the exclusive prefix.
__global__ __launch_bounds__(256) void scan_local_kernel(GridJobs G)
{
    __shared__ int lds[4];
    __shared__ long long lds_occ[8];
    const int job = blockIdx.x >= G.j[0].nb_scan ? 1 : 0;
    const GridJob &J = G.j[job];
    const int b = job ? blockIdx.x - G.j[0].nb_scan : blockIdx.x;
    if (G.pub && G.pub_stage == 1 && blockIdx.x == 0 && threadIdx.x == 0) {   // pack_count_kernel's fit flags: final before this launch started
        G.pub->done = *G.pub_oob;
        *G.pub_oob = 0;
        __hip_atomic_store(&G.pub->seq, G.pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    int4 *A4 = reinterpret_cast<int4 *>(J.cell_start + 1);
    const int base = b * SCAN_CHUNK + threadIdx.x * SCAN_ITEMS;
    const int n_pad = ((J.ncell + 3) / 4) * 4;                           // padded tail holds zeros
    int4 v0 = make_int4(0, 0, 0, 0), v1 = v0;
    if (base < n_pad) v0 = A4[base / 4];
    if (base + 4 < n_pad) v1 = A4[base / 4 + 1];
    const int s = ((v0.x + v0.y) + (v0.z + v0.w)) + ((v1.x + v1.y) + (v1.z + v1.w));
    long long occ[2] = {0, 0};                                           // occupancy statistics (non-empty cells, squared populations): one partial per workgroup, summed by occ_total()
    if (J.occ) {
        occ[0] = (v0.x > 0) + (v0.y > 0) + (v0.z > 0) + (v0.w > 0) + (v1.x > 0) + (v1.y > 0) + (v1.z > 0) + (v1.w > 0);
        occ[1] = (long long)v0.x * v0.x + (long long)v0.y * v0.y + (long long)v0.z * v0.z + (long long)v0.w * v0.w +
                 (long long)v1.x * v1.x + (long long)v1.y * v1.y + (long long)v1.z * v1.z + (long long)v1.w * v1.w;
        wave_sum(occ);
        if ((threadIdx.x & 63) == 0) { lds_occ[2 * (threadIdx.x >> 6)] = occ[0]; lds_occ[2 * (threadIdx.x >> 6) + 1] = occ[1]; }
    }
    int total;
    int ex = block_excl_scan<4>(s, lds, total);
    int4 o0, o1;
    ex += v0.x; o0.x = ex; ex += v0.y; o0.y = ex; ex += v0.z; o0.z = ex; ex += v0.w; o0.w = ex;
    ex += v1.x; o1.x = ex; ex += v1.y; o1.y = ex; ex += v1.z; o1.z = ex; ex += v1.w; o1.w = ex;
    if (base < n_pad) A4[base / 4] = o0;
    if (base + 4 < n_pad) A4[base / 4 + 1] = o1;
    if (threadIdx.x == 0) {
        J.block_sums[b] = total;
        if (J.occ) {                                                     // the block scan above synchronised after the LDS writes
            J.occ[2 + 2 * b] = lds_occ[0] + lds_occ[2] + lds_occ[4] + lds_occ[6];
            J.occ[3 + 2 * b] = lds_occ[1] + lds_occ[3] + lds_occ[5] + lds_occ[7];
        }
    }
}

// sums the per-workgroup occupancy partials of one index build into occ[0..1] (256 threads, all of them)
__device__ __forceinline__ void occ_total(long long *occ, int n_part, long long *lds)
{
    long long nz = 0, sq = 0;
    for (int i = threadIdx.x; i < n_part; i += 256) { nz += occ[2 + 2 * i]; sq += occ[3 + 2 * i]; }
    nz = wave_sum(nz); sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) { lds[2 * (threadIdx.x >> 6)] = nz; lds[2 * (threadIdx.x >> 6) + 1] = sq; }
    __syncthreads();
    if (threadIdx.x == 0) { occ[0] = lds[0] + lds[2] + lds[4] + lds[6]; occ[1] = lds[1] + lds[3] + lds[5] + lds[7]; }
    __syncthreads();
}

// large grids only: exclusive scan of the chunk totals
__global__ __launch_bounds__(256) void scan_sums_kernel(GridJobs G)
{
    __shared__ int lds[4];
    const GridJob &J = G.j[blockIdx.x];
    if (!J.sums_scanned) return;
    int carry = 0;
    for (int start = 0; start < J.nb_scan; start += 256) {
        int i = start + threadIdx.x;
        int v = (i < J.nb_scan) ? J.block_sums[i] : 0;
        int total;
        int ex = block_excl_scan<4>(v, lds, total);
        if (i < J.nb_scan) J.block_sums[i] = carry + ex;
        carry += total;
    }
}

// adds the totals of the preceding chunks (summed here when there are few chunks) and clears the twin array for the next build
__global__ __launch_bounds__(256) void scan_add_kernel(GridJobs G)
{
    __shared__ int lds[4];
    const int job = blockIdx.x >= G.j[0].nb_scan ? 1 : 0;
    const GridJob &J = G.j[job];
    const int b = job ? blockIdx.x - G.j[0].nb_scan : blockIdx.x;
    zero_chunk(J.cell_next, J.ncell, b);
    int add;
    if (J.sums_scanned) {
        add = J.block_sums[b];
    } else {
        int s = 0;
        for (int i = threadIdx.x; i < b; i += 256) s += J.block_sums[i];
        add = block_sum<4>(s, lds);
    }
    if (b == 0) {                                                        // first chunk: offset 0 -- the idle workgroup totals the occupancy statistics
        if (J.occ) {
            __shared__ long long lds_occ[8];
            occ_total(J.occ, J.occ_parts, lds_occ);
            if (threadIdx.x == 0 && J.occ_host) { J.occ_host[0] = J.occ[0]; J.occ_host[1] = J.occ[1]; }   // pinned mirror, read by the NEXT staging call
        }
        return;
    }
    int4 *A4 = reinterpret_cast<int4 *>(J.cell_start + 1);
    const int base = b * SCAN_CHUNK + threadIdx.x * SCAN_ITEMS;
    const int n_pad = ((J.ncell + 3) / 4) * 4;
    if (base < n_pad) { int4 v = A4[base / 4]; v.x += add; v.y += add; v.z += add; v.w += add; A4[base / 4] = v; }
    if (base + 4 < n_pad) { int4 v = A4[base / 4 + 1]; v.x += add; v.y += add; v.z += add; v.w += add; A4[base / 4 + 1] = v; }
}

// no atomics: position = start of the cell + the rank taken while counting
__global__ __launch_bounds__(256) void scatter_kernel(GridJobs G)
{
    const int job = blockIdx.x >= G.j[0].nb_pts ? 1 : 0;
    const GridJob &J = G.j[job];
    const int b = job ? blockIdx.x - G.j[0].nb_pts : blockIdx.x;
    for (int i = b * 256 + threadIdx.x; i < J.n; i += J.nb_pts * 256) {
        const float4 p = J.raw[i];
        const int r = J.rank[i];
        J.sorted[J.cell_start[cell_of(J, p)] + r] = p;
    }
}

// bounds of one point set: the kernel + the copy of its partial records into hp (6 * BOUNDS_BLOCKS ints), nothing waited for
static int bounds_launch(mlh_ctx *ctx, MapGrid &g, int *hp)
{
    hipStream_t st = ctx->stream;
    const int grid_pts = std::min((g.n + 255) / 256, BOUNDS_BLOCKS);
    MLH_HIP(ctx, g.bounds.ensure(6 * BOUNDS_BLOCKS * sizeof(int)));
    MLH_LAUNCH(bounds_kernel, dim3(grid_pts), dim3(256), 0, st, g.raw.as<float4>(), g.n, g.bounds.as<int>());
    MLH_HIP(ctx, hipMemcpyAsync(hp, g.bounds.p, sizeof(int) * 6 * size_t(grid_pts), hipMemcpyDeviceToHost, st));
    return MLH_OK;
}

// ... and, once the stream has been waited for, the grid geometry and buffers that follow from them
static int bounds_finish(mlh_ctx *ctx, MapGrid &g, const int *hp, float min_match_sq_dis)
{
    const int n = g.n;
    const int grid_pts = std::min((n + 255) / 256, BOUNDS_BLOCKS);
    int hb[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    for (int blk = 0; blk < grid_pts; ++blk)
        for (int d = 0; d < 3; ++d) { hb[d] = std::min(hb[d], hp[blk * 6 + d]); hb[3 + d] = std::max(hb[3 + d], hp[blk * 6 + 3 + d]); }
    float mn[3], mx[3];
    for (int d = 0; d < 3; ++d) { mn[d] = dec_f(hb[d]); mx[d] = dec_f(hb[3 + d]); }
    // a geometry becomes the kind's (and reusable by the next staging call) only once every check has passed and every buffer for it is sized: a refusal
    // leaves the kind without a box -- a "valid" box whose cell count does not fit an int, with cell arrays sized for another, would be built into by the
    // next cloud that fits it (make_job narrows ncell, the count pass adds into cell_start[c + 1] far outside the allocation)
    g.geom_valid = false;
    g.built = false;
    for (int d = 0; d < 3; ++d)
        if (!std::isfinite(mn[d]) || !std::isfinite(mx[d])) return fail(ctx, MLH_ERR_INVALID, "map cloud has non-finite coordinates");
    const float h = std::sqrt(min_match_sq_dis) * 1.001f, inv_h = 1.0f / h;
    // the box is laid GRID_MARGIN cells wider than the cloud (one cell in z): the next frames' local maps -- the same keyframe window
    // moved a little -- then fit the geometry already set up, and mlh_map_set skips this host round trip (map_stage_and_build)
    const float ox = mn[0] - GRID_MARGIN_XY * h, oy = mn[1] - GRID_MARGIN_XY * h, oz = mn[2] - GRID_MARGIN_Z * h;
    // (the counts as doubles first: a cloud with a point tens of kilometres out gives a quotient beyond int, whose conversion is undefined)
    const double fnx = std::floor((mx[0] + GRID_MARGIN_XY * h - ox) * inv_h) + 1.0, fny = std::floor((mx[1] + GRID_MARGIN_XY * h - oy) * inv_h) + 1.0,
                 fnz = std::floor((mx[2] + GRID_MARGIN_Z * h - oz) * inv_h) + 1.0;
    const double cell_limit = double((1ll << 31) - 2 * SCAN_CHUNK);
    if (!(fnx >= 1.0 && fny >= 1.0 && fnz >= 1.0) || !(fnx * fny * fnz < cell_limit)) return fail(ctx, MLH_ERR_UNSUPPORTED, "map extent needs more than 2^31 cells");
    const int nx = int(fnx), ny = int(fny), nz = int(fnz);
    const long long ncell = (long long)nx * ny * nz;
    const int nb = int((ncell + SCAN_CHUNK) / SCAN_CHUNK);   // covers ncell + 1 entries
    MLH_HIP(ctx, g.sorted.ensure(sizeof(float4) * size_t(n)));
    MLH_HIP(ctx, g.cell_start.ensure(sizeof(int) * size_t(ncell + 16)));   // 3 ints of lead-in (alignment of cell_start + 1) + padded tail
    MLH_HIP(ctx, g.cell_fill.ensure(sizeof(int) * size_t(ncell + 16)));    // the twin (cleared by one build for the next)
    MLH_HIP(ctx, g.cell_id.ensure(sizeof(int) * size_t(n)));               // per-point rank inside its cell
    MLH_HIP(ctx, g.block_sums.ensure(sizeof(int) * size_t(nb + 1)));
    g.h = h; g.inv_h = inv_h;
    g.ox = ox; g.oy = oy; g.oz = oz;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.ncell = ncell;
    g.cur = 0;
    g.twin_clean = false;
    g.geom_sq_dis = min_match_sq_dis;
    g.geom_valid = true;
    return MLH_OK;
}

// the build goes into the twin of the array the queries currently read when that twin is clean, else into array 0 after a clear
static GridJob make_job(MapGrid &g)
{
    GridJob J;
    std::memset(&J, 0, sizeof(J));
    const int dst = g.twin_clean ? 1 - g.cur : 0;
    J.need_zero = g.twin_clean ? 0 : 1;
    g.cur = dst;
    g.twin_clean = true;
    J.cell_start = g.cells(dst); J.cell_next = g.cells(1 - dst); J.rank = g.cell_id.as<int>();
    J.raw = g.raw.as<float4>(); J.sorted = g.sorted.as<float4>(); J.block_sums = g.block_sums.as<int>(); J.occ = g.want_occ ? g.occ.as<long long>() : nullptr; J.occ_parts = g.occ_parts; J.occ_host = g.want_occ ? g.occ_host : nullptr;
    J.n = g.n; J.ncell = int(g.ncell); J.ox = g.ox; J.oy = g.oy; J.oz = g.oz; J.inv_h = g.inv_h; J.nx = g.nx; J.ny = g.ny; J.nz = g.nz;
    J.nb_pts = std::min((g.n + 255) / 256, 4096);
    J.nb_scan = int((g.ncell + SCAN_CHUNK) / SCAN_CHUNK);
    J.sums_scanned = J.nb_scan > FUSED_SUMS_MAX ? 1 : 0;
    return J;
}

// (re)builds the index of up to two point sets in one set of launches
static int grid_build_grids_packed(mlh_ctx *ctx, MapGrid **grids, int n_grids, bool recompute_bounds, int *pub_oob, HostPublish *pub, unsigned long long pub_seq, const PackJobs *pack);
int grid_build_grids(mlh_ctx *ctx, MapGrid **grids, int n_grids, bool recompute_bounds, int *pub_oob, HostPublish *pub, unsigned long long pub_seq)
{
    return grid_build_grids_packed(ctx, grids, n_grids, recompute_bounds, pub_oob, pub, pub_seq, nullptr);
}

// pack: the staged clouds' records, when the pack + fit check is to ride in the build's first launch (map_stage_and_build; grids[k] <-> pack->j[k])
static int grid_build_grids_packed(mlh_ctx *ctx, MapGrid **grids, int n_grids, bool recompute_bounds, int *pub_oob, HostPublish *pub, unsigned long long pub_seq, const PackJobs *pack)
{
    hipStream_t st = ctx->stream;
    GridJobs G;
    std::memset(&G, 0, sizeof(G));
    G.pub_oob = pub_oob; G.pub = pub; G.pub_seq = pub_seq;
    int nj = 0;
    for (int k = 0; k < n_grids && k < 2; ++k)
        if (grids[k]->n <= 0 || !grids[k]->raw.p) return fail(ctx, MLH_ERR_STATE, "no points staged for this index");
    // a build without a bounds pass goes into the box the kind already has: after a refused staging call there is none
    for (int k = 0; k < n_grids && k < 2; ++k)
        if (!recompute_bounds && !grids[k]->geom_valid) return fail(ctx, MLH_ERR_STATE, "this index has no grid box (the last staging call for it failed)");
    if (recompute_bounds) {
        // the bounding boxes of all point sets in ONE host round trip (which also completes whatever the caller enqueued before)
        int hp[2][6 * BOUNDS_BLOCKS];
        for (int k = 0; k < n_grids && k < 2; ++k) { int rc = bounds_launch(ctx, *grids[k], hp[k]); if (rc) return rc; }
        MLH_HIP(ctx, hipStreamSynchronize(st));
        for (int k = 0; k < n_grids && k < 2; ++k) { int rc = bounds_finish(ctx, *grids[k], hp[k], grids[k]->min_match_sq_dis); if (rc) return rc; }
    }
    for (int k = 0; k < n_grids && k < 2; ++k) {
        MapGrid &g = *grids[k];
        if (g.want_occ) {               // occupancy partials: one per scanning workgroup
            g.occ_parts = int((g.ncell + SCAN_CHUNK) / SCAN_CHUNK);
            MLH_HIP(ctx, g.occ.ensure(sizeof(long long) * size_t(2 + 2 * g.occ_parts)));
        }
        G.j[nj++] = make_job(g);
    }
    if (nj == 0) return MLH_OK;
    const int nb_scan = G.j[0].nb_scan + G.j[1].nb_scan, nb_pts = G.j[0].nb_pts + G.j[1].nb_pts;
    prof_begin(ctx, MLH_K_GRID_BUILD);
    if (G.j[0].need_zero || G.j[1].need_zero) MLH_LAUNCH(zero_cells_kernel, dim3(nb_scan), dim3(256), 0, st, G);
    if (pack) { G.pub_stage = 1; MLH_LAUNCH(pack_count_kernel, dim3(nb_pts), dim3(256), 0, st, G, *pack); }
    else MLH_LAUNCH(cell_count_kernel, dim3(nb_pts), dim3(256), 0, st, G);
    MLH_LAUNCH(scan_local_kernel, dim3(nb_scan), dim3(256), 0, st, G);
    if (G.j[0].sums_scanned || G.j[1].sums_scanned) MLH_LAUNCH(scan_sums_kernel, dim3(nj), dim3(256), 0, st, G);
    MLH_LAUNCH(scan_add_kernel, dim3(nb_scan), dim3(256), 0, st, G);
    MLH_LAUNCH(scatter_kernel, dim3(nb_pts), dim3(256), 0, st, G);
    prof_end(ctx, MLH_K_GRID_BUILD);
    MLH_HIP(ctx, hipGetLastError());
    for (int k = 0; k < nj; ++k) grids[k]->built = true;
    return MLH_OK;
}

// ---- a frame's local map arrives as a cloud of caller records: pack to float4 {x,y,z,index} and, in the same pass, check that every
// point lies inside the grid box already set up for this kind (flag word, OR-ed). One launch for both maps.
__global__ __launch_bounds__(256) void pack_check_kernel(PackJobs G)
{
    const int job = blockIdx.x >= G.j[0].nb ? 1 : 0;
    const PackJob &J = G.j[job];
    const int i = (job ? blockIdx.x - G.j[0].nb : blockIdx.x) * 256 + threadIdx.x;
    bool bad = false;
    if (i < J.n) {
        const float *rec = reinterpret_cast<const float *>(J.src + size_t(i) * J.stride);
        const float x = rec[0], y = rec[1], z = rec[2];
        J.out[i] = make_float4(x, y, z, __int_as_float(i));
        bad = !(x >= J.lo[0] && x < J.hi[0] && y >= J.lo[1] && y < J.hi[1] && z >= J.lo[2] && z < J.hi[2]);   // NaN -> bad
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(G.oob, 1 << job);
}

// the fit flags go to the host as soon as the clouds are packed (the index build that follows does not change them)
__global__ void publish_flag_kernel(int *oob, HostPublish *h, unsigned long long seq)
{
    if (threadIdx.x == 0) {
        h->done = *oob;          // the record's `done` slot carries the flag word here
        *oob = 0;
        __hip_atomic_store(&h->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Stages 1 or 2 clouds (device pointers to strided records) and builds their indices. When a kind's grid geometry from an earlier call
// still applies (same acceptance radius), nothing waits for the host until the end: pack + fit check, index build, then ONE pinned-memory
// hand-shake that returns the fit flags; only a cloud that has outgrown its box takes the bounds round trip (and gets a new box).
int map_stage_and_build(mlh_ctx *ctx, int n_maps, const int *kinds, const unsigned char *const *src, const int *n, int stride, const float *sq_dis,
                        HostPublish *pub, unsigned long long seq)
{
    hipStream_t st = ctx->stream;
    PackJobs G;
    std::memset(&G, 0, sizeof(G));
    MLH_HIP(ctx, ctx->oob_flag.ensure(sizeof(int)));
    if (!ctx->oob_init) { MLH_HIP(ctx, hipMemsetAsync(ctx->oob_flag.p, 0, sizeof(int), st)); ctx->oob_init = true; }
    G.oob = ctx->oob_flag.as<int>();
    MapGrid *grids[2];
    int need_bounds = 0;
    for (int k = 0; k < n_maps; ++k) {
        MapGrid &g = ctx->map[kinds[k]];
        grids[k] = &g;
        g.built = false;
        MLH_HIP(ctx, g.raw.ensure(sizeof(float4) * size_t(n[k])));
        g.want_occ = true;
        const bool reuse = g.geom_valid && g.geom_sq_dis == sq_dis[k];
        if (!reuse) need_bounds |= 1 << k;
        g.n = n[k];
        g.min_match_sq_dis = sq_dis[k];
        PackJob &J = G.j[k];
        J.src = src[k]; J.out = g.raw.as<float4>(); J.n = n[k]; J.stride = stride; J.nb = (n[k] + 255) / 256;
        // a box that accepts everything when there is no geometry to check against (the bounds pass follows anyway)
        J.lo[0] = reuse ? g.ox : -INFINITY; J.lo[1] = reuse ? g.oy : -INFINITY; J.lo[2] = reuse ? g.oz : -INFINITY;
        J.hi[0] = reuse ? g.ox + float(g.nx) * g.h : INFINITY; J.hi[1] = reuse ? g.oy + float(g.ny) * g.h : INFINITY;
        J.hi[2] = reuse ? g.oz + float(g.nz) * g.h : INFINITY;
    }
    // every staged kind keeps its geometry (a mapper between keyframes): pack + fit check ride in the index build's first launch (pack_count_kernel)
    const bool pack_in_build = need_bounds == 0;
    if (!pack_in_build) MLH_LAUNCH(pack_check_kernel, dim3(G.j[0].nb + G.j[1].nb), dim3(256), 0, st, G);
    // the fit flags are final once the clouds are packed: they leave for the host NOW, and the optimistic index build of the kinds whose
    // geometry is reused is enqueued behind them -- the host learns the outcome (and can go on enqueueing the frame's solver launches)
    // while the GPU is still building the index, instead of the GPU idling through the host's reaction time after the build. When such a
    // build follows, its first launch carries the publication (one thread of its first workgroup); otherwise a launch of its own does.
    const bool build_follows = need_bounds != ((1 << n_maps) - 1);
    if (!build_follows) MLH_LAUNCH(publish_flag_kernel, dim3(1), dim3(64), 0, st, G.oob, pub, seq);
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, ctx->h_occ.ensure(sizeof(long long) * 4, 0, true));
    long long *h_occ = ctx->h_occ.as<long long>();
    for (int k = 0; k < n_maps; ++k) grids[k]->occ_host = h_occ + 2 * kinds[k];
    // occupancy statistics (they only steer the lanes-per-query choice): what the previous staging call's builds left in the pinned mirror
    for (int k = 0; k < n_maps; ++k) if (!(need_bounds & (1 << k)) && h_occ[2 * kinds[k]] > 0) {
        grids[k]->occupied = int(h_occ[2 * kinds[k]]); grids[k]->pop_sq = h_occ[2 * kinds[k] + 1];
    }
    if (build_follows) {
        MapGrid *fast[2];
        int nf = 0;
        for (int k = 0; k < n_maps; ++k) if (!(need_bounds & (1 << k))) {
            MapGrid &g = *grids[k];
            MLH_HIP(ctx, g.sorted.ensure(sizeof(float4) * size_t(g.n)));
            MLH_HIP(ctx, g.cell_id.ensure(sizeof(int) * size_t(g.n)));
            fast[nf++] = &g;
        }
        int rc = grid_build_grids_packed(ctx, fast, nf, false, G.oob, pub, seq, pack_in_build ? &G : nullptr);
        if (rc) return rc;
    }
    // spin on the pinned record (pack + fit check have completed when the sequence number arrives; the builds may still be running)
    { const int rc = host_wait_seq(ctx, &pub->seq, seq, st, "map staging did not complete"); if (rc) return rc; }
    const int oob = int(pub->done);
    for (int k = 0; k < n_maps; ++k) if (oob & (1 << k)) need_bounds |= 1 << k;
    if (need_bounds) {
        MapGrid *slow[2];
        int ns = 0;
        for (int k = 0; k < n_maps; ++k) if (need_bounds & (1 << k)) { grids[k]->built = false; grids[k]->geom_valid = false; slow[ns++] = grids[k]; }
        int rc = grid_build_grids(ctx, slow, ns, true);
        if (rc) return rc;
        long long hocc[2][2] = {{0, 0}, {0, 0}};
        for (int k = 0; k < ns; ++k) MLH_HIP(ctx, hipMemcpyAsync(hocc[k], slow[k]->occ.p, 2 * sizeof(long long), hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipStreamSynchronize(st));
        for (int k = 0; k < ns; ++k) { slow[k]->occupied = int(hocc[k][0]); slow[k]->pop_sq = hocc[k][1]; }
    }
    return MLH_OK;
}

// (re)builds the index of the maps selected by kind_mask
int grid_build(mlh_ctx *ctx, int kind_mask, bool recompute_bounds)
{
    MapGrid *g[2];
    int n = 0;
    for (int k = 0; k < 2; ++k) {
        if (!(kind_mask & (1 << k))) continue;
        if (ctx->map[k].n <= 0 || !ctx->map[k].raw.p) return fail(ctx, MLH_ERR_STATE, "map_set has not been called for this kind");
        g[n++] = &ctx->map[k];
    }
    return grid_build_grids(ctx, g, n, recompute_bounds);
}

}  // namespace mlh

using namespace mlh;

extern "C" {

// ---------------------------------------------------------------- map
// host records are copied to the staging buffer first (both clouds back to back); device records are read in place
static int map_set_impl(mlh_ctx *ctx, int n_maps, const int *kinds, const void *const *points, const int *n, int stride_bytes, float min_match_sq_dis, int mem)
{
    if (ctx) ++ctx->stage_epoch;
    if (!(min_match_sq_dis > 0.f)) return fail(ctx, MLH_ERR_INVALID, "min_match_sq_dis must be positive");
    Records r[2];
    size_t off[2] = {0, 0}, total = 0;
    for (int k = 0; k < n_maps; ++k) {
        r[k] = records_of(points[k], stride_bytes, n[k], mem);
        { const int rc = records_check(ctx, n_maps == 1 ? "mlh_map_set" : "mlh_map_set_pair", r[k]); if (rc) return rc; }
        off[k] = total; total += ((r[k].bytes() + 255) / 256) * 256;
    }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    // the overlapped path runs on the staging stream beside whatever the main stream has queued (a scan upload's pack kernel may still be reading ctx->tmp):
    // it stages through a buffer of its own
    DevBuf &tmp = (ctx->stream2 && ctx->stream == ctx->stream2) ? ctx->tmp_stage : ctx->tmp;
    if (mem == MLH_MEM_HOST) MLH_HIP(ctx, tmp.ensure(total));
    const unsigned char *src[2] = {nullptr, nullptr};
    for (int k = 0; k < n_maps; ++k) { const int rc = records_stage(ctx, r[k], tmp, ctx->stream, &src[k], off[k]); if (rc) return rc; }
    HostPublish *pub;
    unsigned long long seq;
    int rc = publish_slot(ctx, &pub, &seq);
    if (rc) return rc;
    float sq[2] = {min_match_sq_dis, min_match_sq_dis};
    rc = map_stage_and_build(ctx, n_maps, kinds, src, n, stride_bytes, sq, pub, seq);
    if (rc) return rc;
    for (int k = 0; k < n_maps; ++k) ctx->feat[kinds[k]].matched = false;
    return MLH_OK;
}

int mlh_map_set(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, float min_match_sq_dis, int mem)
{
    if (!ctx || kind < 0 || kind > 1) return MLH_ERR_INVALID;
    const void *pts[1] = {points};
    return map_set_impl(ctx, 1, &kind, pts, &n, stride_bytes, min_match_sq_dis, mem);
}

int mlh_map_set_pair(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                     float min_match_sq_dis, int mem)
{
    if (!ctx) return MLH_ERR_INVALID;
    const int kinds[2] = {MLH_SURF, MLH_CORNER};
    const void *pts[2] = {surf_points, corner_points};
    const int n[2] = {n_surf, n_corner};
    return map_set_impl(ctx, 2, kinds, pts, n, stride_bytes, min_match_sq_dis, mem);
}

// The next maps staged WHILE the main stream is busy with something that does not read a map: a submitted solve (mlh_gn_solve_begin) still running on the
// current set, or -- no solve in flight, device-resident clouds -- the frame's own front end (upload, extractCloud, fusion, thinning: the local map comes from
// earlier keyframes and does not wait for the scan). Pack + fit check + index build go to the context's second stream and into the other map set; the call
// returns when they are complete (the host waits, the main stream does not) and the context has switched to the new set, so every launch enqueued after this
// call reads it. With host-resident clouds and no solve in flight it behaves like mlh_map_set_pair (the upload staging buffer is shared with the main stream).
int mlh_map_set_pair_overlapped(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                                float min_match_sq_dis, int mem)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!ctx->solves.pending() && mem != MLH_MEM_DEVICE) return mlh_map_set_pair(ctx, surf_points, n_surf, corner_points, n_corner, stride_bytes, min_match_sq_dis, mem);
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->map_read_unsynced) {
        // mlh_pure_odom_add_matches returns with its map-reading launch still queued. Whatever set it reads, it must be done before a set is rewritten -- also
        // with a solve in flight (begin(A); add_matches(A); overlapped -> B; end; begin(B); overlapped -> A would otherwise rewrite A under that launch): the
        // main stream is drained, the solve included. Rare (the window's factor table is not built beside a pipelined mapper solve), so correctness first.
        MLH_HIP(ctx, stream_wait_spin(ctx));
        ctx->map_read_unsynced = false;
    }
    if (!ctx->stream2) {
        // The staging stream may use the first half of the compute units: its kernels are atomics- / latency-bound and lose ~5 % on half the device, while the
        // solver's launches they run beside lose less to them (step 0.1452 -> 0.1415 ms, three alternations in one gpurun call; every other CU, a quarter of the
        // CUs and 8 CUs per 32 measured no better). The mask is sized from the device's compute-unit count. MLH_STAGE_CU_MASK=<hex word>[,<hex word>...]
        // overrides (32 compute units per word; a single word is repeated over the first half of the words, a second one over the other half -- round 3's
        // "lo,hi" form; "ffffffff,ffffffff" = no mask).
        std::vector<uint32_t> words = lower_half_cu_mask(ctx->caps.cu_count);
        if (const char *m = std::getenv("MLH_STAGE_CU_MASK")) {
            const int nw = int(words.size());
            std::vector<uint32_t> given = parse_cu_mask(m, 32 * nw);
            int n_given = 1;
            for (const char *q = m; *q; ++q) n_given += *q == ',';
            if (!given.empty() && n_given <= 2 && nw > 2) {
                const uint32_t lo = given[0], hi = n_given == 2 ? given[1] : given[0];
                for (int i = 0; i < nw; ++i) given[size_t(i)] = i < nw / 2 ? lo : hi;
            }
            if (!given.empty()) {
                if (ctx->caps.cu_count % 32) given.back() &= (1u << (ctx->caps.cu_count % 32)) - 1u;
                words = given;
            }
        }
        int bits = 0;
        for (uint32_t w : words) bits += __builtin_popcount(w);
        if (bits <= 0 || bits >= ctx->caps.cu_count) MLH_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
        else {
            MLH_HIP(ctx, hipExtStreamCreateWithCUMask(&ctx->stream2, uint32_t(words.size()), words.data()));
            ctx->caps.staging_masked = true;
        }
        for (int i = 0; i < 2; ++i) MLH_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_set_built[i], hipEventDisableTiming));
    }
    // The other set's last reader is the solve submitted BEFORE the one in flight; with at most one solve in flight here it has been collected, i.e. it is done:
    // no device-side wait is needed before its buffers are overwritten. (Round 3 first ordered the two streams with events on the solver's stream -- a record
    // after every solve, a wait before the next: two barrier packets, ~10 us of idle stream per frame in the kernel trace. Both are gone: the host orders.)
    if (ctx->solves.in_flight() > 1) return fail(ctx, MLH_ERR_STATE, "collect the older solve (mlh_gn_solve_end) before staging the next frame's maps");
    const int target = 1 - ctx->map_set_cur;
    // ... unless the caller stages twice beside ONE solve (begin on A; overlapped -> B; overlapped -> A again with that solve uncollected): then the target's reader
    // is the solve in flight, and the set is rewritten only once the main stream has run dry (scripts/soak_schedule.py found this as a rare, timing-dependent
    // difference of 1e-5 m: the index of A rebuilt under a correspondence launch)
    if (ctx->solves.set_has_reader(target)) MLH_HIP(ctx, stream_wait_spin(ctx));
    hipStream_t main_stream = ctx->stream;
    ctx->stream = ctx->stream2;                    // everything map_set_impl enqueues (and its profiling brackets) goes to the staging stream ...
    ctx->map = ctx->map_sets[target];              // ... and into the other set
    const int kinds[2] = {MLH_SURF, MLH_CORNER};
    const void *pts[2] = {surf_points, corner_points};
    const int n[2] = {n_surf, n_corner};
    const int rc = map_set_impl(ctx, 2, kinds, pts, n, stride_bytes, min_match_sq_dis, mem);
    ctx->stream = main_stream;
    if (rc) { ctx->map = ctx->map_sets[ctx->map_set_cur]; return rc; }
    ctx->map_set_cur = target;
    // the index must be complete before anything that reads it is enqueued on the solver's stream: waited for HERE, on the host (the build is ~30 us of
    // small launches, the solve in flight another ~100), so that the solver's stream carries no cross-stream wait at all
    MLH_HIP(ctx, hipEventRecord(ctx->ev_set_built[target], ctx->stream2));
    hipEvent_t built = ctx->ev_set_built[target];
    return host_wait(ctx, [=] { return hipEventQuery(built) != hipErrorNotReady; }, ctx->stream2, nullptr);
}

int mlh_map_rebuild(mlh_ctx *ctx, int kind)
{
    if (!ctx || kind < MLH_ALL_KINDS || kind > 1) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return grid_build(ctx, kind == MLH_ALL_KINDS ? 3 : (1 << kind), false);
}

int mlh_map_info(mlh_ctx *ctx, int kind, int32_t *n_points, int32_t *occupied_cells, double *mean_cell_population, int32_t *knn_lanes)
{
    if (!ctx || kind < 0 || kind > 1) return MLH_ERR_INVALID;
    const MapGrid &g = ctx->map[kind];
    if (n_points) *n_points = g.built ? g.n : 0;
    if (occupied_cells) *occupied_cells = g.built ? g.occupied : 0;
    if (mean_cell_population) *mean_cell_population = (g.built && g.n > 0) ? double(g.pop_sq) / double(g.n) : 0.0;
    if (knn_lanes) { int lanes[2]; knn_lanes_for(ctx, 3, lanes); *knn_lanes = lanes[kind]; }
    return MLH_OK;
}

int mlh_knn(mlh_ctx *ctx, int kind, const float *queries_xyz, int nq, int k, int32_t *idx, float *sqdist)
{
    if (!ctx || kind < 0 || kind > 1 || !queries_xyz || !idx || !sqdist) return MLH_ERR_INVALID;
    if (k != 5) return fail(ctx, MLH_ERR_UNSUPPORTED, "only k = 5 is implemented");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return knn_launch(ctx, kind, queries_xyz, nq, idx, sqdist);
}

}  // extern "C"
