// FPFH + Fast Global Registration for the loop closure on the device (gfx950): LoopRegistration::performGlobalRegistration (mloam_loop/src/loop_registration.cpp:
// 18-101) over the loop store's two filtered surf clouds. include/mloam_hip.h, section (f13), has the contract and every CHOSEN / DEPARTURE; fgr_host.hpp the
// arithmetic shared with the host tail and the tests' restatement (pair features, bins, eigen33, the L2 functor) and the tail itself.
//   the self-index   grid.hip's build over a MapGrid of the store's own, then fgr_order_kernel: the points inside a cell in ascending original index (the grid
//                build's rank inside a cell comes from an atomic and differs from run to run). The 27-cell neighbourhood is 9 x-runs of the ordered array; every
//                kernel visits the runs in the same order, so every sum below has one order.
//   fgr_normal_kernel   16 lanes per point (as loop_match_kernel): lane l takes candidates l, l + 16, .. of every run, nine f32 sums + the count, a butterfly over the
//                16 lanes (both partners add the same two values: every lane ends with the same bits), fgr_normal_from_sums by every lane, lane 0 stores.
//   fgr_spfh_kernel     16 lanes per point: computePairFeatures per neighbour, three integer LDS atomics per pair; counts and the neighbour count stored.
//   fgr_spfh_value_kernel   count -> PCL's f32 bin value, one thread per bin.
//   fgr_fpfh_kernel     one wavefront per point, lane b = bin b: the neighbours one after the other (the sum per bin is sequential in walk order), the block sums in
//                PCL's interleaved order through 11 lane broadcasts per neighbour.
//   fgr_norm_stats_kernel / fgr_norm_apply_kernel   NormalizePoints: one workgroup per cloud, 256 strided chains + a tree; then the shift and the divide.
//   fgr_nn_kernel       exact 33-dimensional nearest row: 128 queries per workgroup in registers, tiles of 32 rows in LDS (every lane reads the same word: a
//                broadcast), the dataset split over blockIdx.y; results merge through atomicMin on (distance bits, row) keys -- a minimum is order-independent.
//   fgr_mutual_kernel   one workgroup: the cross check, an ordered compaction in ascending i, the un-swap and the gather of the normalised points.
//   the device tail (mlh_fgr_register_device), behind fgr_mutual_kernel with no host wait in between:
//   fgr_tuple_count_kernel / fgr_tuple_scan_kernel / fgr_tuple_emit_kernel   the tuple test over independent trials: a count per segment of consecutive trials, the
//                exclusive prefix, the accepted trials of rank < tuple_max_cnt written in trial order. Integer decisions only; no atomics.
//   fgr_optimize_kernel   OptimizePairwise in ONE workgroup: 28 f64 sums per iteration in a fixed order, the 6 x 6 solve by every thread.
#include "ctx.hpp"
#include <algorithm>
#include <cmath>
#include "knn_dev.hpp"
#include "fgr_host.hpp"
#include "wg_dev.hpp"

namespace mlh {

namespace {

constexpr int FGR_G = 16, FGR_PPB = TPB / FGR_G;          // lanes per point, points per workgroup (normals, SPFH)
constexpr int FGR_WPB = TPB / 64;                         // points per workgroup of the FPFH kernel (one wavefront each)
constexpr int NN_Q = 128, NN_TILE = 32;                   // queries per workgroup, dataset rows per LDS tile
constexpr unsigned long long NN_NONE = ~0ull;

struct Runs { int b[9], e[9]; };

// the 9 x-runs of p's 27-cell neighbourhood, in (dz, dy) order; an absent run is empty
__device__ __forceinline__ void runs_of(const GridDev &g, float x, float y, float z, Runs &R)
{
    const int cx = int(clamp_cell_f(x, g.ox, g.inv_h, g.nx)), cy = int(clamp_cell_f(y, g.oy, g.inv_h, g.ny)), cz = int(clamp_cell_f(z, g.oz, g.inv_h, g.nz));
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int yy = cy + (r % 3) - 1, zz = cz + (r / 3) - 1;
        int b = 0, e = 0;
        if (x0 <= x1 && yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
            const int row = (zz * g.ny + yy) * g.nx;
            b = g.cell_start[row + x0];
            e = g.cell_start[row + x1 + 1];
        }
        R.b[r] = b; R.e[r] = e;
    }
}

// sorted[] position p -> out[cell begin + the number of points of the cell with a smaller original index]
__global__ __launch_bounds__(TPB) void fgr_order_kernel(GridDev g, float4 *__restrict__ out)
{
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= g.n) return;
    const float4 pt = g.sorted[p];
    // grid.hip: cell_of
    const float fx = fminf(fmaxf(floorf((pt.x - g.ox) * g.inv_h), 0.f), float(g.nx - 1));
    const float fy = fminf(fmaxf(floorf((pt.y - g.oy) * g.inv_h), 0.f), float(g.ny - 1));
    const float fz = fminf(fmaxf(floorf((pt.z - g.oz) * g.inv_h), 0.f), float(g.nz - 1));
    const int c = (int(fz) * g.ny + int(fy)) * g.nx + int(fx);
    const int b = g.cell_start[c], e = g.cell_start[c + 1];
    const int me = __float_as_int(pt.w);
    int rank = 0;
    for (int q = b; q < e; ++q) rank += __float_as_int(g.sorted[q].w) < me ? 1 : 0;
    const int dst = b + rank;
    if (p >= b && p < e && dst < e) out[dst] = pt;
}

__device__ __forceinline__ float group_sum16(float v)
{
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, FGR_G);
    return v;
}
__device__ __forceinline__ int group_sum16(int v)
{
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, FGR_G);
    return v;
}

__global__ __launch_bounds__(TPB) void fgr_normal_kernel(GridDev g, const float4 *__restrict__ ordered, int n, float r2, float4 *__restrict__ normals)
{
    const int grp = threadIdx.x / FGR_G, gl = threadIdx.x % FGR_G;
    const int i = blockIdx.x * FGR_PPB + grp;
    if (i >= n) return;                                  // (uniform over the group; no workgroup barrier below)
    const float4 p = g.raw[i];
    Runs R;
    runs_of(g, p.x, p.y, p.z, R);
    float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
#pragma unroll 1
    for (int r = 0; r < 9; ++r)
        for (int pos = R.b[r] + gl; pos < R.e[r]; pos += FGR_G) {
            const float4 q = ordered[pos];
            if (fgr_sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2) {
                a[0] += q.x * q.x; a[1] += q.x * q.y; a[2] += q.x * q.z; a[3] += q.y * q.y; a[4] += q.y * q.z; a[5] += q.z * q.z;
                a[6] += q.x; a[7] += q.y; a[8] += q.z;
                ++cnt;
            }
        }
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = group_sum16(a[k]);
    cnt = group_sum16(cnt);
    const float pp[3] = {p.x, p.y, p.z};
    float out[4];
    fgr_normal_from_sums<float>(a, cnt, pp, out, nullptr, nullptr);
    if (gl == 0) normals[i] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(TPB) void fgr_spfh_kernel(GridDev g, const float4 *__restrict__ ordered, const float4 *__restrict__ normals, int n, float r2,
                                                       int *__restrict__ spfh, int *__restrict__ nbr_k)
{
    __shared__ int s_h[FGR_PPB][FGR_DIM];
    const int grp = threadIdx.x / FGR_G, gl = threadIdx.x % FGR_G;
    const int i = blockIdx.x * FGR_PPB + grp;
    for (int b = gl; b < FGR_DIM; b += FGR_G) s_h[grp][b] = 0;
    __syncthreads();
    int cnt = 0;
    if (i < n) {
        const float4 p = g.raw[i], n1 = normals[i];
        const float pp[3] = {p.x, p.y, p.z}, nn1[3] = {n1.x, n1.y, n1.z};
        Runs R;
        runs_of(g, p.x, p.y, p.z, R);
#pragma unroll 1
        for (int r = 0; r < 9; ++r)
            for (int pos = R.b[r] + gl; pos < R.e[r]; pos += FGR_G) {
                const float4 q = ordered[pos];
                if (!(fgr_sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2)) continue;
                ++cnt;
                const int j = __float_as_int(q.w);
                if (j == i || j < 0 || j >= n) continue;                      // computePointSPFHSignature skips the point itself by index
                const float4 n2 = normals[j];
                const float qq[3] = {q.x, q.y, q.z}, nn2[3] = {n2.x, n2.y, n2.z};
                float f1, f2, f3;
                if (!fgr_pair_features<float>(pp, nn1, qq, nn2, f1, f2, f3)) continue;
                atomicAdd(&s_h[grp][fgr_bin(fgr_unit_f1(f1))], 1);
                atomicAdd(&s_h[grp][FGR_BINS + fgr_bin(fgr_unit_f23(f2))], 1);
                atomicAdd(&s_h[grp][2 * FGR_BINS + fgr_bin(fgr_unit_f23(f3))], 1);
            }
    }
    cnt = group_sum16(cnt);
    __syncthreads();
    if (i < n) {
        for (int b = gl; b < FGR_DIM; b += FGR_G) spfh[size_t(i) * FGR_DIM + b] = s_h[grp][b];
        if (gl == 0) nbr_k[i] = cnt;
    }
}

__global__ __launch_bounds__(TPB) void fgr_spfh_value_kernel(const int *__restrict__ spfh, const int *__restrict__ nbr_k, int n, float *__restrict__ val)
{
    const size_t t = size_t(blockIdx.x) * TPB + threadIdx.x;
    if (t >= size_t(n) * FGR_DIM) return;
    val[t] = fgr_spfh_value(spfh[t], nbr_k[t / FGR_DIM]);
}

__global__ __launch_bounds__(TPB) void fgr_fpfh_kernel(GridDev g, const float4 *__restrict__ ordered, const float *__restrict__ val, int n, float r2, float *__restrict__ feat)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * FGR_WPB + (threadIdx.x >> 6);
    if (i >= n) return;                                  // (uniform over the wavefront; no workgroup barrier below)
    const float4 p = g.raw[i];
    Runs R;
    runs_of(g, p.x, p.y, p.z, R);
    const bool bin = lane < FGR_DIM;
    const int base = bin ? FGR_BINS * (lane / FGR_BINS) : 0;
    float h = 0.f, S = 0.f;
#pragma unroll 1
    for (int r = 0; r < 9; ++r)
        for (int pos = R.b[r]; pos < R.e[r]; ++pos) {        // (uniform over the wavefront)
            const float4 q = ordered[pos];
            const float d2 = fgr_sqdist3(p.x, p.y, p.z, q.x, q.y, q.z);
            if (!(d2 < r2) || d2 == 0.f) continue;
            const int j = __float_as_int(q.w);
            if (j < 0 || j >= n) continue;
            const float w = 1.0f / d2;
            const float v = bin ? val[size_t(j) * FGR_DIM + lane] * w : 0.f;
            h += v;
#pragma unroll
            for (int t = 0; t < FGR_BINS; ++t) S += __shfl(v, base + t);
        }
    if (bin) feat[size_t(i) * FGR_DIM + lane] = h * fgr_block_scale(S);
}

// scal[4 c ..]: cloud c's mean and the largest norm of its shifted points
__global__ __launch_bounds__(TPB) void fgr_norm_stats_kernel(const float4 *__restrict__ raw0, int n0, const float4 *__restrict__ raw1, int n1, float *__restrict__ scal)
{
    __shared__ float s[3][TPB];
    __shared__ float s_mean[3];
    const int c = blockIdx.x, t = threadIdx.x;
    const float4 *raw = c ? raw1 : raw0;
    const int n = c ? n1 : n0;
    float x = 0.f, y = 0.f, z = 0.f;
    for (int i = t; i < n; i += TPB) { const float4 p = raw[i]; x += p.x; y += p.y; z += p.z; }
    s[0][t] = x; s[1][t] = y; s[2][t] = z;
    __syncthreads();
    for (int w = TPB / 2; w >= 1; w >>= 1) {
        if (t < w) { s[0][t] += s[0][t + w]; s[1][t] += s[1][t + w]; s[2][t] += s[2][t + w]; }
        __syncthreads();
    }
    if (t < 3) s_mean[t] = n > 0 ? s[t][0] / float(n) : 0.f;          // mean = mean / npti
    __syncthreads();
    const float mx = s_mean[0], my = s_mean[1], mz = s_mean[2];
    float m = 0.f;
    for (int i = t; i < n; i += TPB) {
        const float4 p = raw[i];
        const float a = p.x - mx, b = p.y - my, d = p.z - mz;
        const float nrm = sqrtf((a * a + b * b) + d * d);
        if (nrm > m) m = nrm;
    }
    __syncthreads();
    s[0][t] = m;
    __syncthreads();
    for (int w = TPB / 2; w >= 1; w >>= 1) {
        if (t < w) s[0][t] = fmaxf(s[0][t], s[0][t + w]);
        __syncthreads();
    }
    if (t == 0) { scal[4 * c] = mx; scal[4 * c + 1] = my; scal[4 * c + 2] = mz; scal[4 * c + 3] = s[0][0]; }
}

__device__ __forceinline__ float global_scale_of(const float *scal, int use_absolute_scale)
{
    float scale = 0.f;
    if (scal[3] > scale) scale = scal[3];
    if (scal[7] > scale) scale = scal[7];
    return use_absolute_scale ? 1.0f : scale;
}

__global__ __launch_bounds__(TPB) void fgr_norm_apply_kernel(const float4 *__restrict__ raw0, int n0, const float4 *__restrict__ raw1, int n1, const float *__restrict__ scal,
                                                             int use_absolute_scale, float4 *__restrict__ out0, float4 *__restrict__ out1)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    const float G = global_scale_of(scal, use_absolute_scale);
    if (i < n0) { const float4 p = raw0[i]; out0[i] = make_float4((p.x - scal[0]) / G, (p.y - scal[1]) / G, (p.z - scal[2]) / G, p.w); }
    if (i < n1) { const float4 p = raw1[i]; out1[i] = make_float4((p.x - scal[4]) / G, (p.y - scal[5]) / G, (p.z - scal[6]) / G, p.w); }
}

// best[q] <- min over this slice's finite rows d of (bits of |Q[q] - D[d]|^2, d); a non-finite query row keeps NN_NONE
__global__ __launch_bounds__(NN_Q) void fgr_nn_kernel(const float *__restrict__ Q, int nq, const float *__restrict__ D, int nd, int rows_per_slice, unsigned long long *__restrict__ best)
{
    __shared__ float s_tile[NN_TILE * FGR_DIM];
    __shared__ int s_ok[NN_TILE];
    const int qi = blockIdx.x * NN_Q + threadIdx.x;
    float q[FGR_DIM];
#pragma unroll
    for (int k = 0; k < FGR_DIM; ++k) q[k] = qi < nq ? Q[size_t(qi) * FGR_DIM + k] : 0.f;
    const bool q_ok = qi < nq && fgr_row_finite(q);
    const int d_begin = blockIdx.y * rows_per_slice, d_end = min(nd, d_begin + rows_per_slice);
    unsigned long long mine = NN_NONE;
    for (int t0 = d_begin; t0 < d_end; t0 += NN_TILE) {                 // (uniform over the workgroup)
        const int rows = min(NN_TILE, d_end - t0);
        __syncthreads();
        for (int w = threadIdx.x; w < rows * FGR_DIM; w += NN_Q) s_tile[w] = D[size_t(t0) * FGR_DIM + w];
        __syncthreads();
        if (threadIdx.x < rows) s_ok[threadIdx.x] = fgr_row_finite(&s_tile[threadIdx.x * FGR_DIM]) ? 1 : 0;
        __syncthreads();
        if (q_ok)
            for (int r = 0; r < rows; ++r) {
                if (!s_ok[r]) continue;
                const float d = fgr_l2_33(q, &s_tile[r * FGR_DIM]);
                const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(t0 + r);
                if (key < mine) mine = key;
            }
    }
    if (q_ok && mine != NN_NONE) atomicMin(&best[qi], mine);
}

// i runs over the larger cloud (cloud 1 when swapped); nn_i[i] / nn_j[j]: the keys of fgr_nn_kernel. out: the mutual pairs in ascending i, un-swapped, with their
// normalised points (np0 / np1 may be null: zeros). counts[0] <- the number of pairs. ONE workgroup.
__global__ __launch_bounds__(TPB) void fgr_mutual_kernel(const unsigned long long *__restrict__ nn_i, int ni, const unsigned long long *__restrict__ nn_j, int nj, int swapped,
                                                         const float4 *__restrict__ np0, const float4 *__restrict__ np1, FgrPair *__restrict__ out, int *__restrict__ counts)
{
    __shared__ int s_wave[TPB / 64];
    __shared__ int s_base;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int at = 0; at < ni; at += TPB) {                              // (uniform over the workgroup)
        const int i = at + threadIdx.x;
        int j = -1;
        if (i < ni) {
            const unsigned long long k = nn_i[i];
            if (k != NN_NONE) {
                const int jj = int(unsigned(k));
                if (jj >= 0 && jj < nj) { const unsigned long long kj = nn_j[jj]; if (kj != NN_NONE && int(unsigned(kj)) == i) j = jj; }
            }
        }
        const unsigned long long m = __ballot(j >= 0);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (j >= 0) {
            FgrPair rec;
            rec.i = swapped ? j : i; rec.j = swapped ? i : j;
            const float4 a = np0 ? np0[rec.i] : make_float4(0.f, 0.f, 0.f, 0.f), b = np1 ? np1[rec.j] : make_float4(0.f, 0.f, 0.f, 0.f);
            rec.p[0] = a.x; rec.p[1] = a.y; rec.p[2] = a.z; rec.q[0] = b.x; rec.q[1] = b.y; rec.q[2] = b.z;
            out[off + before] = rec;
        }
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int w = 0; w < TPB / 64; ++w) tot += s_wave[w]; s_base += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { counts[0] = s_base; counts[1] = 0; }
}

// ---------------------------------------------------------------- the device tail (mlh_fgr_register_device): the tuple test as count -> scan -> emit over
// independent trials (fgr_host.hpp has the plan's arithmetic and the trial), then OptimizePairwise in one workgroup. Four launches behind fgr_mutual_kernel; the
// pair count is read where that kernel left it.
// the record the one device-to-pinned copy brings to the host, and the words the tuple test's kernels hand to the optimiser (device only)
struct FgrTailRecord {
    float scal[8];                       // per cloud: mean xyz, max norm (fgr_norm_stats_kernel); zeros from the test entries
    int32_t n_mutual, pad;
    float trans[16];
    double final_cost, final_cost_normalize;
    int32_t n_tuples, n_corres, n_trials, optimised;
};
static_assert(sizeof(FgrTailRecord) == 136, "the tail's record");
struct FgrTailHead { int32_t n_tuples, n_corres, n_trials, total, cap_segment, pad[3]; };
constexpr size_t TAIL_HEAD_AT = 192, TAIL_BYTES = TAIL_HEAD_AT + sizeof(FgrTailHead);

// seg_counts[segment] <- the accepted trials of the segment (0 for a segment behind the last trial). One workgroup per segment of the LARGEST pair count possible.
__global__ __launch_bounds__(FGR_TT_TPB) void fgr_tuple_count_kernel(const uint64_t *__restrict__ table, const FgrPair *__restrict__ pairs, const int *__restrict__ n_pairs, int pair_cap,
                                                                     int swapped, float scale, uint64_t seed, int *__restrict__ seg_counts)
{
    __shared__ int s_wave[FGR_TT_TPB / 64];
    const int ncorr = max(0, min(*n_pairs, pair_cap));
    long long b, e;
    fgr_tt_run(fgr_tt_total_trials(ncorr), blockIdx.x, threadIdx.x, &b, &e);
    int c = __popc(fgr_tt_run_mask(table, pairs, ncorr, swapped != 0, scale, seed, b, e));
    c = block_sum<FGR_TT_TPB / 64>(c, s_wave);
    if (threadIdx.x == 0) seg_counts[blockIdx.x] = c;
}

// seg_base[s] <- the accepted trials in front of segment s (saturated at the cap: such a segment emits nothing); head <- the tuples kept, n_trials when the cap is
// never reached, the segment that holds rank cap - 1 (-1: none). ONE workgroup.
__global__ __launch_bounds__(TPB) void fgr_tuple_scan_kernel(const int *__restrict__ seg_counts, int nseg, const int *__restrict__ n_pairs, int pair_cap, int tuple_max_cnt,
                                                             int *__restrict__ seg_base, FgrTailHead *__restrict__ head)
{
    __shared__ int s_wave[TPB / 64];
    __shared__ long long s_carry;
    if (threadIdx.x == 0) { s_carry = 0; head->cap_segment = -1; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int at = 0; at < nseg; at += TPB) {                            // (uniform over the workgroup)
        const int i = at + threadIdx.x;
        const int c = i < nseg ? seg_counts[i] : 0;
        const int incl = wave_incl_scan(c);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        long long before = s_carry + (incl - c);
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (i < nseg) {
            seg_base[i] = int(before < (long long)tuple_max_cnt ? before : (long long)tuple_max_cnt);
            if (before < (long long)tuple_max_cnt && before + c >= (long long)tuple_max_cnt) head->cap_segment = i;
        }
        __syncthreads();
        if (threadIdx.x == 0) { long long tot = 0; for (int w = 0; w < TPB / 64; ++w) tot += s_wave[w]; s_carry += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long total = s_carry;
        const int ncorr = max(0, min(*n_pairs, pair_cap));
        const int tuples = fgr_tt_tuples(total, tuple_max_cnt);
        head->n_tuples = tuples; head->n_corres = 3 * tuples;
        head->total = int(total < 0x7fffffffll ? total : 0x7fffffffll);
        if (!fgr_tt_cap_reached(total, tuple_max_cnt)) head->n_trials = int(fgr_tt_total_trials(ncorr));      // (otherwise the emit kernel's thread of rank cap - 1 writes it)
    }
}

// the accepted trials of rank < tuple_max_cnt -> corres[3 rank ..], ranks in trial order: the segment's base + the accepted trials of the threads in front (a scan
// over each wavefront, the wavefronts' totals added in wavefront order -- the pattern of fgr_mutual_kernel with a count per lane in place of a ballot's bit) + those
// of the thread's own run in front. Only the segments that keep something recompute their trials. No atomics.
__global__ __launch_bounds__(FGR_TT_TPB) void fgr_tuple_emit_kernel(const uint64_t *__restrict__ table, const FgrPair *__restrict__ pairs, const int *__restrict__ n_pairs, int pair_cap,
                                                                    int swapped, float scale, uint64_t seed, int tuple_max_cnt, const int *__restrict__ seg_counts,
                                                                    const int *__restrict__ seg_base, int *__restrict__ corres, int corres_cap_tuples, FgrTailHead *__restrict__ head)
{
    __shared__ int s_wave[FGR_TT_TPB / 64];
    const int ncorr = max(0, min(*n_pairs, pair_cap));
    const int base = seg_base[blockIdx.x];
    if (!fgr_tt_segment_emits(base, seg_counts[blockIdx.x], tuple_max_cnt)) return;          // (uniform over the workgroup)
    long long b, e;
    fgr_tt_run(fgr_tt_total_trials(ncorr), blockIdx.x, threadIdx.x, &b, &e);
    const uint32_t mask = fgr_tt_run_mask(table, pairs, ncorr, swapped != 0, scale, seed, b, e);
    const int c = __popc(mask);
    const int incl = wave_incl_scan(c);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int rank = base + (incl - c);
    for (int w = 0; w < wave; ++w) rank += s_wave[w];
    if (mask == 0u) return;
    FgrRng rng = fgr_rng_at(table, seed, uint64_t(b) * 3ull);
    for (long long t = b; t < e; ++t) {
        int r[3];
        fgr_trial_draw(ncorr, rng, r);
        if (!((mask >> int(t - b)) & 1u)) continue;
        if (fgr_tt_rank_kept(rank, tuple_max_cnt) && rank < corres_cap_tuples) { corres[3 * size_t(rank)] = r[0]; corres[3 * size_t(rank) + 1] = r[1]; corres[3 * size_t(rank) + 2] = r[2]; }
        if (fgr_tt_rank_is_last(rank, tuple_max_cnt)) head->n_trials = int(t);
        ++rank;
    }
}

// OptimizePairwise (fgr_host.hpp: fgr_optimize_pairwise) on the head's n_corres correspondences. ONE workgroup; thread t owns the correspondences t, t + TPB, ..
// and adds them to its 28 sums in that order; a __shfl_xor butterfly per wavefront (both partners add the same two values: every lane ends with the same bits), the
// four wavefronts' sums added in wavefront order by every thread -- the fixed order of calib_ne_kernel -- so that every thread solves the same 6 x 6 system,
// forms the same delta and moves its own copies of q with it; no broadcast. REG: p and the working q live in registers (n <= FGR_OPT_REG_MAX); otherwise in `work`.
template <bool REG>
__device__ __forceinline__ void fgr_optimize_body(const FgrPair *__restrict__ pairs, int pair_cap, const int *__restrict__ corres, int n, double par, double div_factor, double max_corr_dist,
                                                  int iteration_number, float *__restrict__ work, double *s_red, float trans[16], double cost[2])
{
    float p[REG ? FGR_OPT_QREG : 1][3], q[REG ? FGR_OPT_QREG : 1][3];
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < FGR_OPT_QREG; ++k) {
            const int c = int(threadIdx.x) + k * FGR_OPT_TPB;
#pragma unroll
            for (int d = 0; d < 3; ++d) { p[k][d] = 0.f; q[k][d] = 0.f; }
            if (c < n) {
                const FgrPair rec = pairs[max(0, min(corres[c], pair_cap - 1))];
#pragma unroll
                for (int d = 0; d < 3; ++d) { p[k][d] = rec.p[d]; q[k][d] = rec.q[d]; }
            }
        }
    } else {
        for (int c = threadIdx.x; c < n; c += FGR_OPT_TPB) {
            const FgrPair rec = pairs[max(0, min(corres[c], pair_cap - 1))];
            for (int d = 0; d < 3; ++d) { work[6 * size_t(c) + d] = rec.p[d]; work[6 * size_t(c) + 3 + d] = rec.q[d]; }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int itr = 0; itr < iteration_number; ++itr) {                  // (uniform over the workgroup)
        par = fgr_par_step(par, itr, max_corr_dist, div_factor);
        double acc[FGR_OPT_SUMS];
#pragma unroll
        for (int i = 0; i < FGR_OPT_SUMS; ++i) acc[i] = 0.0;
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < FGR_OPT_QREG; ++k)
                if (int(threadIdx.x) + k * FGR_OPT_TPB < n) fgr_pairwise_accumulate(p[k], q[k], par, acc);
        } else {
            for (int c = threadIdx.x; c < n; c += FGR_OPT_TPB) {
                const float *w = work + 6 * size_t(c);
                const float pp[3] = {w[0], w[1], w[2]}, qq[3] = {w[3], w[4], w[5]};
                fgr_pairwise_accumulate(pp, qq, par, acc);
            }
        }
#pragma unroll
        for (int i = 0; i < FGR_OPT_SUMS; ++i) acc[i] = wave_sum(acc[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < FGR_OPT_SUMS; ++i) s_red[wave * FGR_OPT_SUMS + i] = acc[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < FGR_OPT_SUMS; ++i)
            acc[i] = ((s_red[i] + s_red[FGR_OPT_SUMS + i]) + s_red[2 * FGR_OPT_SUMS + i]) + s_red[3 * FGR_OPT_SUMS + i];
        __syncthreads();
        float delta[16];
        fgr_pairwise_delta(acc, delta);
        fgr_mat4_mul(delta, trans, trans);
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < FGR_OPT_QREG; ++k) fgr_transform_point(delta, q[k]);
        } else {
            for (int c = threadIdx.x; c < n; c += FGR_OPT_TPB) {
                float *w = work + 6 * size_t(c) + 3;
                float qq[3] = {w[0], w[1], w[2]};
                fgr_transform_point(delta, qq);
                w[0] = qq[0]; w[1] = qq[1]; w[2] = qq[2];
            }
        }
        cost[0] = acc[FGR_OPT_R2];
        cost[1] = acc[FGR_OPT_R2] / double(n);
    }
}

// scal (may be null: start_scale_given is StartScale): the normalisation's scalars, copied into the record with the pair count. ONE workgroup of FGR_OPT_TPB.
__global__ __launch_bounds__(FGR_OPT_TPB) void fgr_optimize_kernel(const FgrPair *__restrict__ pairs, int pair_cap, const int *__restrict__ corres, const FgrTailHead *__restrict__ head, int corres_cap,
                                                                   const float *__restrict__ scal, const int *__restrict__ n_pairs, int use_absolute_scale, double start_scale_given,
                                                                   double div_factor, double max_corr_dist, int iteration_number, float *__restrict__ work,
                                                                   FgrTailRecord *__restrict__ out)
{
    static_assert(FGR_OPT_TPB == 256, "four wavefronts: the sums are added ((w0 + w1) + w2) + w3");
    __shared__ double s_red[(FGR_OPT_TPB / 64) * FGR_OPT_SUMS];
    const int n = max(0, min(head->n_corres, corres_cap));
    float trans[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) trans[i] = (i % 5 == 0) ? 1.f : 0.f;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double cost[2] = {nan, nan};
    const bool run = n >= FGR_MIN_CORRES && pair_cap > 0;               // app.cpp:412
    if (run) {
        double start_scale = start_scale_given;
        if (scal) {                                                     // app.cpp:371-377
            float scale = 0.f;
            if (scal[3] > scale) scale = scal[3];
            if (scal[7] > scale) scale = scal[7];
            start_scale = double(use_absolute_scale ? scale : 1.0f);
        }
        if (n <= FGR_OPT_REG_MAX) fgr_optimize_body<true>(pairs, pair_cap, corres, n, start_scale, div_factor, max_corr_dist, iteration_number, work, s_red, trans, cost);
        else fgr_optimize_body<false>(pairs, pair_cap, corres, n, start_scale, div_factor, max_corr_dist, iteration_number, work, s_red, trans, cost);
    }
    if (threadIdx.x == 0) {
        for (int i = 0; i < 8; ++i) out->scal[i] = scal ? scal[i] : 0.f;
        out->n_mutual = *n_pairs; out->pad = 0;
        for (int i = 0; i < 16; ++i) out->trans[i] = trans[i];
        out->final_cost = cost[0]; out->final_cost_normalize = cost[1];
        out->n_tuples = head->n_tuples; out->n_corres = n; out->n_trials = head->n_trials; out->optimised = run ? 1 : 0;
    }
}

// ---------------------------------------------------------------- host side
struct FgrPinned { float scal[8]; int counts[2]; int pad[6]; };        // the pair records follow
static_assert(sizeof(FgrPinned) == 64, "the pinned header");

size_t grid_bytes(const MapGrid &g) { return g.raw.cap + g.sorted.cap + g.cell_id.cap + g.cell_start.cap + g.cell_fill.cap + g.block_sums.cap + g.bounds.cap + g.occ.cap; }

int fgr_opts_take(mlh_ctx *ctx, const char *entry, const mlh_fgr_opts *opts, mlh_fgr_opts &o)
{
    if (opts) o = *opts; else fgr_opts_defaults(o);
    if (const char *fault = fgr_opts_fault(o)) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": bad " + fault).c_str());
    return MLH_OK;
}

int fgr_gate(mlh_ctx *ctx, const char *entry)
{
    { const int rc = loop_process_gate(ctx, entry); if (rc) return rc; }
    ctx->fgr.launches = 0; ctx->fgr.host_waits = 0;          // (a refused call leaves the previous call's counts)
    return MLH_OK;
}

int side_of(mlh_ctx *ctx, const char *entry, int which, int *s)
{
    if (which != MLH_LOOP_MODEL_SURF && which != MLH_LOOP_DATA_SURF) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": which is MLH_LOOP_MODEL_SURF or MLH_LOOP_DATA_SURF").c_str());
    *s = which == MLH_LOOP_DATA_SURF ? 1 : 0;
    return MLH_OK;
}
int cloud_n(const mlh_ctx *ctx, int s) { return ctx->loop.flt_n[s ? MLH_LOOP_DATA_SURF : MLH_LOOP_MODEL_SURF]; }
const float4 *cloud_pts(const mlh_ctx *ctx, int s) { return ctx->loop.flt.as<float4>() + ctx->loop.off[s ? MLH_LOOP_DATA_SURF : MLH_LOOP_MODEL_SURF]; }

int fgr_buffers_ensure(mlh_ctx *ctx, int s, int n)
{
    FgrStore &F = ctx->fgr;
    const size_t rows = size_t(n) + 1;
    MLH_HIP(ctx, ensure_counted(F.normals[s], sizeof(float4) * rows, F.allocations));
    MLH_HIP(ctx, ensure_counted(F.spfh[s], sizeof(int) * FGR_DIM * rows, F.allocations));
    MLH_HIP(ctx, ensure_counted(F.nbr_k[s], sizeof(int) * rows, F.allocations));
    MLH_HIP(ctx, ensure_counted(F.spfh_val[s], sizeof(float) * FGR_DIM * rows, F.allocations));
    MLH_HIP(ctx, ensure_counted(F.feat[s], sizeof(float) * FGR_DIM * rows, F.allocations));
    return MLH_OK;
}

// the self-index of cloud s at cell edge `edge`, unless it stands for the staged cloud already. One host wait (the bounds) when it is built.
int fgr_index_ensure(mlh_ctx *ctx, int s, float edge)
{
    FgrStore &F = ctx->fgr;
    const int n = cloud_n(ctx, s);
    if (n == 0 || (F.index_gen[s] == ctx->loop.cloud_gen && F.index_edge[s] == edge)) return MLH_OK;
    F.index_gen[s] = FgrStore::NO_GEN;
    MapGrid &g = F.grid[s];
    const size_t before = grid_bytes(g);
    MLH_HIP(ctx, g.raw.ensure(sizeof(float4) * (size_t(n) + 1)));
    pack_points_launch(ctx->stream, reinterpret_cast<const unsigned char *>(cloud_pts(ctx, s)), int(sizeof(float4)), n, PACK_W_INDEX, 0.f, -1, g.raw.as<float4>(), nullptr);
    g.n = n; g.min_match_sq_dis = edge * edge; g.want_occ = false; g.built = false; g.geom_valid = false;
    MapGrid *gp = &g;
    { const int rc = grid_build_grids(ctx, &gp, 1, true); if (rc) return rc; }
    ++F.host_waits;
    if (grid_bytes(g) > before) ++F.allocations;
    MLH_HIP(ctx, ensure_counted(F.ordered[s], sizeof(float4) * (size_t(n) + 1), F.allocations));
    MLH_LAUNCH(fgr_order_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, ctx->stream, g.dev(), F.ordered[s].as<float4>());
    F.launches += 2;
    MLH_HIP(ctx, hipGetLastError());
    F.index_gen[s] = ctx->loop.cloud_gen; F.index_edge[s] = edge;
    return MLH_OK;
}

enum { STAGE_NORMALS = 0, STAGE_SPFH = 1, STAGE_FPFH = 2 };

// the stages from `first` on for cloud s; nothing is waited for behind the index build
int fgr_stages_run(mlh_ctx *ctx, int s, const mlh_fgr_opts &o, int first)
{
    FgrStore &F = ctx->fgr;
    const LoopStore &L = ctx->loop;
    const int n = cloud_n(ctx, s);
    hipStream_t st = ctx->stream;
    { const int rc = fgr_buffers_ensure(ctx, s, n); if (rc) return rc; }
    if (n > 0) {
        { const int rc = fgr_index_ensure(ctx, s, std::max(o.normal_radius, o.fpfh_radius)); if (rc) return rc; }
        const GridDev g = F.grid[s].dev();
        const float4 *ordered = F.ordered[s].as<float4>();
        if (first <= STAGE_NORMALS) {
            MLH_LAUNCH(fgr_normal_kernel, dim3((n + FGR_PPB - 1) / FGR_PPB), dim3(TPB), 0, st, g, ordered, n, o.normal_radius * o.normal_radius, F.normals[s].as<float4>());
            ++F.launches;
        }
        const float r2 = o.fpfh_radius * o.fpfh_radius;
        if (first <= STAGE_SPFH) {
            MLH_LAUNCH(fgr_spfh_kernel, dim3((n + FGR_PPB - 1) / FGR_PPB), dim3(TPB), 0, st, g, ordered, (const float4 *)F.normals[s].as<float4>(), n, r2, F.spfh[s].as<int>(),
                       F.nbr_k[s].as<int>());
            MLH_LAUNCH(fgr_spfh_value_kernel, dim3(unsigned((size_t(n) * FGR_DIM + TPB - 1) / TPB)), dim3(TPB), 0, st, (const int *)F.spfh[s].as<int>(),
                       (const int *)F.nbr_k[s].as<int>(), n, F.spfh_val[s].as<float>());
            F.launches += 2;
        }
        MLH_LAUNCH(fgr_fpfh_kernel, dim3((n + FGR_WPB - 1) / FGR_WPB), dim3(TPB), 0, st, g, ordered, (const float *)F.spfh_val[s].as<float>(), n, r2, F.feat[s].as<float>());
        ++F.launches;
        MLH_HIP(ctx, hipGetLastError());
    }
    if (first <= STAGE_NORMALS) { F.normals_gen[s] = L.cloud_gen; F.normals_radius[s] = o.normal_radius; }
    if (first <= STAGE_SPFH) F.spfh_gen[s] = L.cloud_gen;
    F.feat_gen[s] = L.cloud_gen; F.fpfh_radius[s] = o.fpfh_radius; F.fn[s] = n;
    F.feat_user[s] = first != STAGE_NORMALS;
    return MLH_OK;
}

bool features_valid(const mlh_ctx *ctx, int s, const mlh_fgr_opts &o)
{
    const FgrStore &F = ctx->fgr;
    if (F.feat_gen[s] != ctx->loop.cloud_gen || F.fn[s] != cloud_n(ctx, s)) return false;
    return F.feat_user[s] || (F.normals_gen[s] == ctx->loop.cloud_gen && F.normals_radius[s] == o.normal_radius && F.fpfh_radius[s] == o.fpfh_radius);
}

int fgr_pin(mlh_ctx *ctx, size_t records)
{
    MLH_HIP(ctx, ctx->fgr.h_pin.ensure(sizeof(FgrPinned) + sizeof(FgrPair) * (records + 1), 4096, true));      // (nothing is in flight into the block between calls)
    return MLH_OK;
}

// both directions of the nearest-row search and the cross check; the pairs' records and their count stay on the device
int fgr_match_enqueue(mlh_ctx *ctx, bool with_points, bool *swapped_out)
{
    FgrStore &F = ctx->fgr;
    hipStream_t st = ctx->stream;
    const int n0 = F.fn[0], n1 = F.fn[1];
    const bool swapped = n1 > n0;                                          // app.cpp:121-127
    *swapped_out = swapped;
    MLH_HIP(ctx, ensure_counted(F.nn[0], sizeof(unsigned long long) * (size_t(n0) + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.nn[1], sizeof(unsigned long long) * (size_t(n1) + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.pairs, sizeof(FgrPair) * (size_t(std::min(n0, n1)) + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.scal, 64, F.allocations));
    MLH_HIP(ctx, hipMemsetAsync(F.nn[0].p, 0xFF, sizeof(unsigned long long) * (size_t(n0) + 1), st));
    MLH_HIP(ctx, hipMemsetAsync(F.nn[1].p, 0xFF, sizeof(unsigned long long) * (size_t(n1) + 1), st));
    if (n0 > 0 && n1 > 0) {
        for (int s = 0; s < 2; ++s) {                                      // rows of cloud s against the rows of the other cloud
            const int nq = s ? n1 : n0, nd = s ? n0 : n1;
            const int qblocks = (nq + NN_Q - 1) / NN_Q;
            int slices = std::max(1, std::min((nd + 4 * NN_TILE - 1) / (4 * NN_TILE), 2048 / qblocks));
            int rows_per_slice = (nd + slices - 1) / slices;
            rows_per_slice = ((rows_per_slice + NN_TILE - 1) / NN_TILE) * NN_TILE;
            slices = (nd + rows_per_slice - 1) / rows_per_slice;
            MLH_LAUNCH(fgr_nn_kernel, dim3(qblocks, slices), dim3(NN_Q), 0, st, (const float *)F.feat[s].as<float>(), nq, (const float *)F.feat[1 - s].as<float>(), nd,
                       rows_per_slice, F.nn[s].as<unsigned long long>());
            ++F.launches;
        }
    }
    const int si = swapped ? 1 : 0;
    MLH_LAUNCH(fgr_mutual_kernel, dim3(1), dim3(TPB), 0, st, (const unsigned long long *)F.nn[si].as<unsigned long long>(), F.fn[si],
               (const unsigned long long *)F.nn[1 - si].as<unsigned long long>(), F.fn[1 - si], swapped ? 1 : 0,
               with_points ? (const float4 *)F.npts[0].as<float4>() : nullptr, with_points ? (const float4 *)F.npts[1].as<float4>() : nullptr, F.pairs.as<FgrPair>(),
               reinterpret_cast<int *>(F.scal.as<float>() + 8));
    ++F.launches;
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// the scalars, the count and the records into the pinned block; ONE wait
int fgr_fetch_pairs(mlh_ctx *ctx, std::vector<FgrPair> &pairs, FgrPinned *head)
{
    FgrStore &F = ctx->fgr;
    const size_t cap = size_t(std::min(F.fn[0], F.fn[1]));
    { const int rc = fgr_pin(ctx, cap); if (rc) return rc; }
    unsigned char *pin = F.h_pin.as<unsigned char>();
    MLH_HIP(ctx, hipMemcpyAsync(pin, F.scal.p, 40, hipMemcpyDeviceToHost, ctx->stream));
    if (cap) MLH_HIP(ctx, hipMemcpyAsync(pin + sizeof(FgrPinned), F.pairs.p, sizeof(FgrPair) * cap, hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    ++F.host_waits;
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    std::memcpy(head, pin, sizeof(FgrPinned));
    const size_t cnt = size_t(std::max(0, std::min(head->counts[0], int(cap))));
    const FgrPair *rec = reinterpret_cast<const FgrPair *>(pin + sizeof(FgrPinned));
    pairs.assign(rec, rec + cnt);
    return MLH_OK;
}

int features_run(mlh_ctx *ctx, int s, const mlh_fgr_opts &o, int first, const char *entry)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, entry); if (rc) return rc; }
    const unsigned long long gen = ctx->loop.cloud_gen;
    if (first >= STAGE_SPFH && (F.normals_gen[s] != gen)) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": no normals for the staged cloud").c_str());
    if (first >= STAGE_FPFH && (F.spfh_gen[s] != gen)) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": no SPFH for the staged cloud").c_str());
    return fgr_stages_run(ctx, s, o, first);
}

int match_run(mlh_ctx *ctx, int32_t *pairs_out, int32_t capacity, int32_t *n_pairs)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, "mlh_fgr_match"); if (rc) return rc; }
    for (int s = 0; s < 2; ++s)
        if (F.feat_gen[s] != ctx->loop.cloud_gen) return fail(ctx, MLH_ERR_STATE, "mlh_fgr_match: no features for the staged clouds (mlh_fgr_features or mlh_fgr_set_features, both clouds)");
    bool swapped = false;
    { const int rc = fgr_match_enqueue(ctx, false, &swapped); if (rc) return rc; }
    std::vector<FgrPair> pairs;
    FgrPinned head;
    { const int rc = fgr_fetch_pairs(ctx, pairs, &head); if (rc) return rc; }
    const size_t w = std::min(pairs.size(), size_t(std::max(capacity, 0)));
    for (size_t e = 0; e < w && pairs_out; ++e) { pairs_out[2 * e] = pairs[e].i; pairs_out[2 * e + 1] = pairs[e].j; }
    if (n_pairs) *n_pairs = int32_t(pairs_out ? w : pairs.size());
    return MLH_OK;
}

// ---- the device tail's host side
// the most tuples a call can keep, and so the correspondences the buffers hold
int tail_tuples_cap(int pair_cap, int tuple_max_cnt) { return int(std::min<long long>(tuple_max_cnt, fgr_tt_total_trials(pair_cap))); }
int *pair_count_dev(FgrStore &F) { return reinterpret_cast<int *>(F.scal.as<float>() + 8); }
FgrTailHead *tail_head_dev(FgrStore &F) { return reinterpret_cast<FgrTailHead *>(F.tail.as<unsigned char>() + TAIL_HEAD_AT); }

// the tail's buffers for up to pair_cap pairs and n_corres_cap correspondences; the generator's table goes to the device the first time
int fgr_tail_ensure(mlh_ctx *ctx, int pair_cap, int n_corres_cap)
{
    FgrStore &F = ctx->fgr;
    const size_t nseg = size_t(fgr_tt_segments(pair_cap));
    MLH_HIP(ctx, ensure_counted(F.rng_table, sizeof(uint64_t) * FGR_RNG_TABLE_WORDS, F.allocations));
    MLH_HIP(ctx, ensure_counted(F.tt_counts, sizeof(int) * 2 * (nseg + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.corres, sizeof(int) * (size_t(n_corres_cap) + 3), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.tail, TAIL_BYTES, F.allocations));
    if (n_corres_cap > FGR_OPT_REG_MAX) MLH_HIP(ctx, ensure_counted(F.work, sizeof(float) * 6 * size_t(n_corres_cap), F.allocations));
    if (!F.rng_table_ready) {
        MLH_HIP(ctx, hipMemcpyAsync(F.rng_table.p, fgr_rng_table(), sizeof(uint64_t) * FGR_RNG_TABLE_WORDS, hipMemcpyHostToDevice, ctx->stream));
        F.rng_table_ready = true;
    }
    return MLH_OK;
}

// count -> scan -> emit on the pairs and the pair count where they stand on the device (at most pair_cap pairs); the buffers hold tail_tuples_cap tuples
int fgr_tuple_enqueue(mlh_ctx *ctx, const mlh_fgr_opts &o, bool swapped, int pair_cap)
{
    FgrStore &F = ctx->fgr;
    hipStream_t st = ctx->stream;
    const int nseg = fgr_tt_segments(pair_cap);
    const uint64_t *table = F.rng_table.as<uint64_t>();
    const FgrPair *pairs = F.pairs.as<FgrPair>();
    int *counts = F.tt_counts.as<int>(), *base = counts + nseg + 1;
    if (nseg > 0) {
        MLH_LAUNCH(fgr_tuple_count_kernel, dim3(nseg), dim3(FGR_TT_TPB), 0, st, table, pairs, (const int *)pair_count_dev(F), pair_cap, swapped ? 1 : 0, o.tuple_scale, o.seed, counts);
        ++F.launches;
    }
    MLH_LAUNCH(fgr_tuple_scan_kernel, dim3(1), dim3(TPB), 0, st, (const int *)counts, nseg, (const int *)pair_count_dev(F), pair_cap, o.tuple_max_cnt, base, tail_head_dev(F));
    ++F.launches;
    if (nseg > 0) {
        MLH_LAUNCH(fgr_tuple_emit_kernel, dim3(nseg), dim3(FGR_TT_TPB), 0, st, table, pairs, (const int *)pair_count_dev(F), pair_cap, swapped ? 1 : 0, o.tuple_scale, o.seed,
                   o.tuple_max_cnt, (const int *)counts, (const int *)base, F.corres.as<int>(), tail_tuples_cap(pair_cap, o.tuple_max_cnt), tail_head_dev(F));
        ++F.launches;
    }
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// OptimizePairwise on the head's correspondences; scal: the normalisation's scalars on the device, or null with StartScale given
int fgr_optimize_enqueue(mlh_ctx *ctx, const mlh_fgr_opts &o, int pair_cap, int n_corres_cap, const float *scal, double start_scale)
{
    FgrStore &F = ctx->fgr;
    MLH_LAUNCH(fgr_optimize_kernel, dim3(1), dim3(FGR_OPT_TPB), 0, ctx->stream, (const FgrPair *)F.pairs.as<FgrPair>(), pair_cap, (const int *)F.corres.as<int>(),
               (const FgrTailHead *)tail_head_dev(F), n_corres_cap, scal, (const int *)pair_count_dev(F), o.use_absolute_scale, start_scale, o.div_factor, o.max_corr_dist,
               o.iteration_number, n_corres_cap > FGR_OPT_REG_MAX ? F.work.as<float>() : nullptr, F.tail.as<FgrTailRecord>());
    ++F.launches;
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// the record into the pinned block; ONE wait
int fgr_tail_fetch(mlh_ctx *ctx, FgrTailRecord *rec)
{
    FgrStore &F = ctx->fgr;
    MLH_HIP(ctx, F.h_pin.ensure(256, 4096, true));
    MLH_HIP(ctx, hipMemcpyAsync(F.h_pin.p, F.tail.p, sizeof(FgrTailRecord), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    ++F.host_waits;
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    std::memcpy(rec, F.h_pin.p, sizeof(FgrTailRecord));
    return MLH_OK;
}

// host records (n x {p, q}) -> the pair buffer and the pair count, through the pinned block; nothing is waited for: the block is not written again before
// the call's one wait
int fgr_stage_pairs(mlh_ctx *ctx, const float *pq, int n, size_t pin_bytes)
{
    FgrStore &F = ctx->fgr;
    MLH_HIP(ctx, ensure_counted(F.pairs, sizeof(FgrPair) * (size_t(n) + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.scal, 64, F.allocations));
    MLH_HIP(ctx, F.h_pin.ensure(pin_bytes, 4096, true));
    unsigned char *pin = F.h_pin.as<unsigned char>();
    int *cnt = reinterpret_cast<int *>(pin + 256);
    cnt[0] = n; cnt[1] = 0;
    FgrPair *rec = reinterpret_cast<FgrPair *>(pin + 320);
    for (int e = 0; e < n; ++e) {
        rec[e].i = rec[e].j = e;
        for (int d = 0; d < 3; ++d) { rec[e].p[d] = pq[6 * size_t(e) + d]; rec[e].q[d] = pq[6 * size_t(e) + 3 + d]; }
    }
    MLH_HIP(ctx, hipMemcpyAsync(pair_count_dev(F), cnt, 8, hipMemcpyHostToDevice, ctx->stream));
    if (n) MLH_HIP(ctx, hipMemcpyAsync(F.pairs.p, rec, sizeof(FgrPair) * size_t(n), hipMemcpyHostToDevice, ctx->stream));
    return MLH_OK;
}

int tail_tuple_test_run(mlh_ctx *ctx, const mlh_fgr_opts &o, const float *pq, int n, bool swapped, int32_t *corres_out, int32_t *n_tuples, int32_t *n_trials)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, "mlh_fgr_tail_tuple_test"); if (rc) return rc; }
    const int tuples_cap = tail_tuples_cap(n, o.tuple_max_cnt);
    { const int rc = fgr_tail_ensure(ctx, n, 3 * tuples_cap); if (rc) return rc; }
    { const int rc = fgr_stage_pairs(ctx, pq, n, 320 + sizeof(FgrPair) * (size_t(n) + 1) + sizeof(int) * (3 * size_t(tuples_cap) + 3)); if (rc) return rc; }
    { const int rc = fgr_tuple_enqueue(ctx, o, swapped, n); if (rc) return rc; }
    // the head and the correspondences, behind the staged records in the pinned block; ONE wait
    unsigned char *pin = F.h_pin.as<unsigned char>();
    FgrTailHead *head = reinterpret_cast<FgrTailHead *>(pin);
    int *got = reinterpret_cast<int *>(pin + 320 + sizeof(FgrPair) * (size_t(n) + 1));
    MLH_HIP(ctx, hipMemcpyAsync(head, tail_head_dev(F), sizeof(FgrTailHead), hipMemcpyDeviceToHost, ctx->stream));
    if (tuples_cap) MLH_HIP(ctx, hipMemcpyAsync(got, F.corres.p, sizeof(int) * 3 * size_t(tuples_cap), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    ++F.host_waits;
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    const int k = std::max(0, std::min(head->n_tuples, tuples_cap));
    if (k) std::memcpy(corres_out, got, sizeof(int) * 3 * size_t(k));
    *n_tuples = k; *n_trials = head->n_trials;
    return MLH_OK;
}

int tail_optimize_run(mlh_ctx *ctx, const mlh_fgr_opts &o, const float *pq, int n, double start_scale, float *trans, double *cost, int32_t *optimised)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, "mlh_fgr_tail_optimize"); if (rc) return rc; }
    { const int rc = fgr_tail_ensure(ctx, n, n); if (rc) return rc; }
    const size_t ids_at = 320 + sizeof(FgrPair) * (size_t(n) + 1);
    { const int rc = fgr_stage_pairs(ctx, pq, n, ids_at + sizeof(int) * (size_t(n) + 1)); if (rc) return rc; }
    // every record is a correspondence, in its order
    unsigned char *pin = F.h_pin.as<unsigned char>();
    FgrTailHead *head = reinterpret_cast<FgrTailHead *>(pin + 288);
    *head = FgrTailHead();
    head->n_tuples = n / 3; head->n_corres = n; head->total = n / 3; head->cap_segment = -1;
    int *ids = reinterpret_cast<int *>(pin + ids_at);
    for (int e = 0; e < n; ++e) ids[e] = e;
    MLH_HIP(ctx, hipMemcpyAsync(tail_head_dev(F), head, sizeof(FgrTailHead), hipMemcpyHostToDevice, ctx->stream));
    if (n) MLH_HIP(ctx, hipMemcpyAsync(F.corres.p, ids, sizeof(int) * size_t(n), hipMemcpyHostToDevice, ctx->stream));
    { const int rc = fgr_optimize_enqueue(ctx, o, n, n, nullptr, start_scale); if (rc) return rc; }
    FgrTailRecord rec;
    { const int rc = fgr_tail_fetch(ctx, &rec); if (rc) return rc; }
    std::memcpy(trans, rec.trans, sizeof(rec.trans));
    cost[0] = rec.final_cost; cost[1] = rec.final_cost_normalize;
    *optimised = rec.optimised;
    return MLH_OK;
}

// features (unless valid), NormalizePoints, the match: what both register entries enqueue in front of their tails
int register_front(mlh_ctx *ctx, const mlh_fgr_opts &o, const char *entry, mlh_fgr_result *res, bool *swapped)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, entry); if (rc) return rc; }
    std::memset(res, 0, sizeof(*res));
    for (int s = 0; s < 2; ++s)
        if (!features_valid(ctx, s, o)) { const int rc = fgr_stages_run(ctx, s, o, STAGE_NORMALS); if (rc) return rc; }
    const int n0 = cloud_n(ctx, 0), n1 = cloud_n(ctx, 1);
    hipStream_t st = ctx->stream;
    MLH_HIP(ctx, ensure_counted(F.npts[0], sizeof(float4) * (size_t(n0) + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.npts[1], sizeof(float4) * (size_t(n1) + 1), F.allocations));
    MLH_HIP(ctx, ensure_counted(F.scal, 64, F.allocations));
    MLH_LAUNCH(fgr_norm_stats_kernel, dim3(2), dim3(TPB), 0, st, cloud_pts(ctx, 0), n0, cloud_pts(ctx, 1), n1, F.scal.as<float>());
    ++F.launches;
    if (std::max(n0, n1) > 0) {
        MLH_LAUNCH(fgr_norm_apply_kernel, dim3((std::max(n0, n1) + TPB - 1) / TPB), dim3(TPB), 0, st, cloud_pts(ctx, 0), n0, cloud_pts(ctx, 1), n1, (const float *)F.scal.as<float>(),
                   o.use_absolute_scale, F.npts[0].as<float4>(), F.npts[1].as<float4>());
        ++F.launches;
    }
    return fgr_match_enqueue(ctx, true, swapped);
}

int register_run(mlh_ctx *ctx, const mlh_fgr_opts &o, mlh_fgr_result *res)
{
    FgrStore &F = ctx->fgr;
    bool swapped = false;
    { const int rc = register_front(ctx, o, "mlh_fgr_register", res, &swapped); if (rc) return rc; }
    std::vector<FgrPair> pairs;
    FgrPinned head;
    { const int rc = fgr_fetch_pairs(ctx, pairs, &head); if (rc) return rc; }
    // app.cpp:371-377
    float scale = 0.f;
    if (head.scal[3] > scale) scale = head.scal[3];
    if (head.scal[7] > scale) scale = head.scal[7];
    const float global_scale = o.use_absolute_scale ? 1.0f : scale, start_scale = o.use_absolute_scale ? scale : 1.0f;
    fgr_host_tail(pairs, swapped, head.scal, head.scal + 4, global_scale, start_scale, o, *res);
    res->host_waits = F.host_waits;
    if (ctx->prof.mask) prof_collect(ctx);
    return MLH_OK;
}

// the same call with the tail on the device: four launches behind the match, one 136-byte record to the host, GetOutputTrans and `accepted` on it
int register_device_run(mlh_ctx *ctx, const mlh_fgr_opts &o, mlh_fgr_result *res)
{
    FgrStore &F = ctx->fgr;
    bool swapped = false;
    { const int rc = register_front(ctx, o, "mlh_fgr_register_device", res, &swapped); if (rc) return rc; }
    const int pair_cap = std::min(F.fn[0], F.fn[1]);
    const int n_corres_cap = 3 * tail_tuples_cap(pair_cap, o.tuple_max_cnt);
    { const int rc = fgr_tail_ensure(ctx, pair_cap, n_corres_cap); if (rc) return rc; }
    { const int rc = fgr_tuple_enqueue(ctx, o, swapped, pair_cap); if (rc) return rc; }
    { const int rc = fgr_optimize_enqueue(ctx, o, pair_cap, n_corres_cap, F.scal.as<float>(), 1.0); if (rc) return rc; }
    FgrTailRecord rec;
    { const int rc = fgr_tail_fetch(ctx, &rec); if (rc) return rc; }
    float scale = 0.f;                                                   // app.cpp:371-377
    if (rec.scal[3] > scale) scale = rec.scal[3];
    if (rec.scal[7] > scale) scale = rec.scal[7];
    const float global_scale = o.use_absolute_scale ? 1.0f : scale, start_scale = o.use_absolute_scale ? scale : 1.0f;
    fgr_output_trans(rec.trans, rec.scal, rec.scal + 4, global_scale, res->T_relative);
    res->final_cost = rec.final_cost; res->final_cost_normalize = rec.final_cost_normalize;
    res->accepted = (rec.optimised && rec.final_cost_normalize <= o.global_registration_threshold) ? 1 : 0;
    res->swapped = swapped ? 1 : 0;
    res->n_mutual = rec.n_mutual; res->n_tuples = rec.n_tuples; res->n_corres = rec.n_corres; res->n_trials = rec.n_trials;
    res->global_scale = double(global_scale); res->start_scale = double(start_scale);
    for (int d = 0; d < 3; ++d) { res->means[d] = double(rec.scal[d]); res->means[3 + d] = double(rec.scal[4 + d]); }
    res->host_waits = F.host_waits;
    if (ctx->prof.mask) prof_collect(ctx);
    return MLH_OK;
}

int fetch_run(mlh_ctx *ctx, int s, int what, void *out, int32_t *k_out)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, "mlh_fgr_fetch"); if (rc) return rc; }
    const unsigned long long gen = ctx->loop.cloud_gen;
    const unsigned long long have = what == MLH_FGR_NORMALS ? F.normals_gen[s] : what == MLH_FGR_SPFH ? F.spfh_gen[s] : F.feat_gen[s];
    if (have != gen) return fail(ctx, MLH_ERR_STATE, "mlh_fgr_fetch: that stage has not been computed for the staged cloud");
    const size_t n = size_t(what == MLH_FGR_FPFH ? F.fn[s] : cloud_n(ctx, s));
    if (n > 0) {
        if (what == MLH_FGR_NORMALS) MLH_HIP(ctx, hipMemcpyAsync(out, F.normals[s].p, sizeof(float4) * n, hipMemcpyDeviceToHost, ctx->stream));
        else if (what == MLH_FGR_SPFH) {
            MLH_HIP(ctx, hipMemcpyAsync(out, F.spfh[s].p, sizeof(int) * FGR_DIM * n, hipMemcpyDeviceToHost, ctx->stream));
            if (k_out) MLH_HIP(ctx, hipMemcpyAsync(k_out, F.nbr_k[s].p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
        } else MLH_HIP(ctx, hipMemcpyAsync(out, F.feat[s].p, sizeof(float) * FGR_DIM * n, hipMemcpyDeviceToHost, ctx->stream));
    }
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ++F.host_waits;
    return device_error_check(ctx);
}

// a stage's output from the host. n must be the staged cloud's size -- or, for the features alone, the cloud may be empty
int set_run(mlh_ctx *ctx, int s, int what, int32_t n, const void *a, const int32_t *k)
{
    FgrStore &F = ctx->fgr;
    { const int rc = fgr_gate(ctx, "mlh_fgr_set_*"); if (rc) return rc; }
    const int cn = cloud_n(ctx, s);
    if (n < 0 || (n > 0 && !a) || (what == MLH_FGR_SPFH && n > 0 && !k) || !(n == cn || (what == MLH_FGR_FPFH && cn == 0)))
        return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_set_*: n must be the staged cloud's size (features alone: or the cloud empty), with its array");
    { const int rc = fgr_buffers_ensure(ctx, s, n); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    const unsigned long long gen = ctx->loop.cloud_gen;
    if (what == MLH_FGR_NORMALS) {
        if (n) MLH_HIP(ctx, hipMemcpyAsync(F.normals[s].p, a, sizeof(float4) * size_t(n), hipMemcpyHostToDevice, st));
        F.normals_gen[s] = gen; F.normals_radius[s] = 0.f; F.spfh_gen[s] = FgrStore::NO_GEN; F.feat_gen[s] = FgrStore::NO_GEN;
    } else if (what == MLH_FGR_SPFH) {
        if (n) {
            MLH_HIP(ctx, hipMemcpyAsync(F.spfh[s].p, a, sizeof(int) * FGR_DIM * size_t(n), hipMemcpyHostToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(F.nbr_k[s].p, k, sizeof(int) * size_t(n), hipMemcpyHostToDevice, st));
            MLH_LAUNCH(fgr_spfh_value_kernel, dim3(unsigned((size_t(n) * FGR_DIM + TPB - 1) / TPB)), dim3(TPB), 0, st, (const int *)F.spfh[s].as<int>(),
                       (const int *)F.nbr_k[s].as<int>(), n, F.spfh_val[s].as<float>());
            ++F.launches;
            MLH_HIP(ctx, hipGetLastError());
        }
        F.spfh_gen[s] = gen; F.feat_gen[s] = FgrStore::NO_GEN;
    } else {
        if (n) MLH_HIP(ctx, hipMemcpyAsync(F.feat[s].p, a, sizeof(float) * FGR_DIM * size_t(n), hipMemcpyHostToDevice, st));
        F.feat_gen[s] = gen; F.fn[s] = n; F.feat_user[s] = true;
    }
    MLH_HIP(ctx, hipStreamSynchronize(st));               // the caller's array has been read when the call returns
    ++F.host_waits;
    return MLH_OK;
}

}  // namespace

}  // namespace mlh

using namespace mlh;

extern "C" {

void mlh_fgr_opts_default(mlh_fgr_opts *o)
{
    if (o) fgr_opts_defaults(*o);
}

static int fgr_stage_entry(mlh_ctx *ctx, const char *entry, int which, const mlh_fgr_opts *opts, int first)
{
    if (!ctx) return MLH_ERR_INVALID;
    int s = 0;
    { const int rc = side_of(ctx, entry, which, &s); if (rc) return rc; }
    mlh_fgr_opts o;
    { const int rc = fgr_opts_take(ctx, entry, opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return features_run(ctx, s, o, first, entry);
}

int mlh_fgr_features(mlh_ctx *ctx, int which, const mlh_fgr_opts *opts) { return fgr_stage_entry(ctx, "mlh_fgr_features", which, opts, STAGE_NORMALS); }
int mlh_fgr_spfh(mlh_ctx *ctx, int which, const mlh_fgr_opts *opts) { return fgr_stage_entry(ctx, "mlh_fgr_spfh", which, opts, STAGE_SPFH); }
int mlh_fgr_fpfh(mlh_ctx *ctx, int which, const mlh_fgr_opts *opts) { return fgr_stage_entry(ctx, "mlh_fgr_fpfh", which, opts, STAGE_FPFH); }

int mlh_fgr_fetch(mlh_ctx *ctx, int which, int what, void *out, int32_t *k_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    int s = 0;
    { const int rc = side_of(ctx, "mlh_fgr_fetch", which, &s); if (rc) return rc; }
    if (what < MLH_FGR_NORMALS || what > MLH_FGR_FPFH || !out) return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_fetch: bad `what` or null output");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return fetch_run(ctx, s, what, out, k_out);
}

static int fgr_set_entry(mlh_ctx *ctx, int which, int what, int32_t n, const void *a, const int32_t *k)
{
    if (!ctx) return MLH_ERR_INVALID;
    int s = 0;
    { const int rc = side_of(ctx, "mlh_fgr_set_*", which, &s); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return set_run(ctx, s, what, n, a, k);
}

int mlh_fgr_set_normals(mlh_ctx *ctx, int which, int32_t n, const float *normals4) { return fgr_set_entry(ctx, which, MLH_FGR_NORMALS, n, normals4, nullptr); }
int mlh_fgr_set_spfh(mlh_ctx *ctx, int which, int32_t n, const int32_t *counts, const int32_t *k) { return fgr_set_entry(ctx, which, MLH_FGR_SPFH, n, counts, k); }
int mlh_fgr_set_features(mlh_ctx *ctx, int which, int32_t n, const float *features) { return fgr_set_entry(ctx, which, MLH_FGR_FPFH, n, features, nullptr); }

int mlh_fgr_match(mlh_ctx *ctx, const mlh_fgr_opts *opts, int32_t *pairs_out, int32_t capacity, int32_t *n_pairs)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_fgr_opts o;
    { const int rc = fgr_opts_take(ctx, "mlh_fgr_match", opts, o); if (rc) return rc; }
    if (capacity < 0 || (capacity > 0 && !pairs_out)) return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_match: bad capacity");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return match_run(ctx, pairs_out, capacity, n_pairs);
}

int mlh_fgr_register(mlh_ctx *ctx, const mlh_fgr_opts *opts, mlh_fgr_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!result) return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_register: null result");
    mlh_fgr_opts o;
    { const int rc = fgr_opts_take(ctx, "mlh_fgr_register", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return register_run(ctx, o, result);
}

int mlh_fgr_register_device(mlh_ctx *ctx, const mlh_fgr_opts *opts, mlh_fgr_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!result) return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_register_device: null result");
    mlh_fgr_opts o;
    { const int rc = fgr_opts_take(ctx, "mlh_fgr_register_device", opts, o); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return register_device_run(ctx, o, result);
}

int mlh_fgr_tail_tuple_test(mlh_ctx *ctx, const float *pq, int32_t n, int32_t swapped, const mlh_fgr_opts *opts, int32_t *corres_out, int32_t capacity_tuples, int32_t *n_tuples,
                            int32_t *n_trials)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_fgr_opts o;
    { const int rc = fgr_opts_take(ctx, "mlh_fgr_tail_tuple_test", opts, o); if (rc) return rc; }
    if (n < 0 || n > 20000000 || (n > 0 && !pq) || (swapped != 0 && swapped != 1) || !n_tuples || !n_trials)
        return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_tail_tuple_test: 0 <= n <= 20000000 records with their array, swapped 0 or 1, non-null n_tuples and n_trials");
    if (capacity_tuples < tail_tuples_cap(n, o.tuple_max_cnt) || (capacity_tuples > 0 && !corres_out))
        return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_tail_tuple_test: capacity_tuples must hold min(tuple_max_cnt, 100 n) tuples, with their array");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return tail_tuple_test_run(ctx, o, pq, n, swapped != 0, corres_out, n_tuples, n_trials);
}

int mlh_fgr_tail_optimize(mlh_ctx *ctx, const float *pq, int32_t n, double start_scale, const mlh_fgr_opts *opts, float *trans, double *cost, int32_t *optimised)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_fgr_opts o;
    { const int rc = fgr_opts_take(ctx, "mlh_fgr_tail_optimize", opts, o); if (rc) return rc; }
    if (n < 0 || n > 3000000 || (n > 0 && !pq) || !std::isfinite(start_scale) || !(start_scale > 0.0) || !trans || !cost || !optimised)
        return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_tail_optimize: 0 <= n <= 3000000 records with their array, a finite start_scale > 0, non-null trans, cost and optimised");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return tail_optimize_run(ctx, o, pq, n, start_scale, trans, cost, optimised);
}

int mlh_fgr_info(mlh_ctx *ctx, mlh_fgr_info_t *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_fgr_info: null output");
    const FgrStore &F = ctx->fgr;
    const unsigned long long gen = ctx->loop.cloud_gen;
    std::memset(out, 0, sizeof(*out));
    size_t bytes = F.scal.cap + F.pairs.cap + F.rng_table.cap + F.tt_counts.cap + F.corres.cap + F.tail.cap + F.work.cap;
    for (int s = 0; s < 2; ++s) {
        out->n[s] = F.fn[s];
        out->have_normals[s] = F.normals_gen[s] == gen; out->have_spfh[s] = F.spfh_gen[s] == gen; out->have_features[s] = F.feat_gen[s] == gen;
        bytes += grid_bytes(F.grid[s]) + F.ordered[s].cap + F.normals[s].cap + F.spfh[s].cap + F.nbr_k[s].cap + F.spfh_val[s].cap + F.feat[s].cap + F.npts[s].cap + F.nn[s].cap;
    }
    out->launches = F.launches; out->host_waits = F.host_waits;
    out->allocations = F.allocations;
    out->bytes_hbm = int64_t(bytes);
    return MLH_OK;
}

}  // extern "C"
