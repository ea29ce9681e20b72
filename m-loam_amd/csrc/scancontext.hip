// Scan Context place recognition on gfx950: SCManager (mloam_loop/src/scan_context.cpp:155-323) as PoseGraph::detectLoop drives it (mloam_loop/src/pose_graph.cpp:
// 281-328). include/mloam_hip.h (f11) states what is reproduced and what is chosen; sc_host.hpp holds the arithmetic of one point, shared by the kernel and the host.
//   sc_desc_kernel     makeScancontext (cpp:155-186). Grid-stride over the records of all clouds. Every workgroup keeps an image of the polar grid in LDS as
//                      order-preserving integer encodings of f32 (<= 32 KB), one LDS atomic max per point, then ONE global integer atomic max per non-empty cell
//                      per workgroup. Points within SC_EDGE_MARGIN_SECTORS of a sector edge go to the undecided list (one global counter: ~0.08 % of a cloud).
//   sc_finish_kernel   one workgroup: the host's verdicts on the undecided points, decode, empty cells -> 0, the descriptor as f32 in place of the integers, the
//                      ring key, sector key and column norms of cpp:188-218 into the entry's slot
//   sc_desc_batch_kernel / sc_finish_batch_kernel   the same two steps for a batch of keyframes of the mapper's store (mlh_sc_add_keyframes): a workgroup per chunk
//                      of one entry's points, then a workgroup per entry; the bodies are those of the two kernels above (sc_point, sc_finish_body)
//   sc_keydist_kernel  nanoflann's L2_Adaptor (nanoflann.hpp:432-461) in f32 against every searched entry: (distance bits << 32 | index), one thread per entry
//   sc_select_kernel   one workgroup: the num_candidates smallest of those words by an 8-pass byte-wise radix selection, then ranked -> the candidates in the order
//                      cpp:286 visits them (equal distances: the lower index first)
//   sc_score_kernel    distanceBtnScanContext (cpp:123-153), one workgroup per candidate: fastAlignUsingVkey over all S shifts (a thread per shift), then one
//                      wavefront per shift of the search space, a lane per column, the (2 radius + 1) x S column cosines of distDirectSC (cpp:80-101)
//   sc_argmin_kernel   cpp:286-298 in candidate order, strict <
// mlh_sc_detect: those four + the marker launch of the wait, one copy, ONE host wait -- whatever the size of the store and num_candidates.
// No float atomics: every cross-workgroup combination is an integer max or an ordered reduction.
#include "ctx.hpp"
#include "wg_dev.hpp"
#include <algorithm>
#include <cmath>

namespace mlh {

constexpr int SC_DESC_THREADS = 256;      // points a workgroup takes per pass
constexpr int SC_DESC_MAX_BLOCKS = 128;   // ... and the workgroups of a launch: 32 768 points per pass of the grid-stride loop
constexpr int SC_UNC_FIRST = 2048;        // undecided points fetched with the counters (a 120 k-point cloud has ~100); more than that: one more copy
constexpr int SC_PIN_HEAD = 64;           // pinned block: [0, 64) counters / results, the lists behind
constexpr int SC_KEY_LDS = 1024;          // sector keys of up to this many sectors are staged in LDS by the score kernel

struct ScCloudDev { const unsigned char *p; int n; };
struct ScDescArgs {
    ScCloudDev c[3];
    int stride, n_total, R, S;
    double lidar_height, max_radius;
    int *grid;            // R * S cells of the entry's slot, preset to sc_encode(SC_NO_POINT)
    float4 *unc;          // n_total
    int *counters;
};

// one point of makeScancontext (cpp:163-175) as far as the device takes it: the sc_* arithmetic of sc_host.hpp, for sc_desc_kernel and sc_desc_batch_kernel alike
enum { SC_PT_DROPPED = 0, SC_PT_SKIPPED, SC_PT_UNDECIDED, SC_PT_BINNED };
struct ScPoint { int what, ring, cell, e; float zf; };
__device__ __forceinline__ ScPoint sc_point(float x, float y, float z, int R, int S, double lidar_height, double max_radius)
{
    ScPoint p = {SC_PT_DROPPED, 0, 0, 0, 0.f};
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) { p.what = SC_PT_SKIPPED; return p; }
    const float range = sc_range(x, y);
    if (double(range) > max_radius) return p;
    p.zf = sc_height(z, lidar_height);
    p.ring = sc_ring(range, max_radius, R);
    const double sv = sc_sector_value(sc_xy2theta(x, y), S);
    if (sc_in_band(sv)) { p.what = SC_PT_UNDECIDED; return p; }      // this libm does not speak for the host's so close to an edge (a NaN is not in the band)
    p.e = sc_encode(p.zf);
    if (p.e > sc_encode(SC_NO_POINT)) { p.what = SC_PT_BINNED; p.cell = sc_bin(p.ring, sc_sector(sv, S), R); }
    return p;
}

__global__ __launch_bounds__(SC_DESC_THREADS) void sc_desc_kernel(ScDescArgs A)
{
    extern __shared__ int s_grid[];
    const int bins = A.R * A.S, empty = sc_encode(SC_NO_POINT);
    for (int b = threadIdx.x; b < bins; b += SC_DESC_THREADS) s_grid[b] = empty;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * SC_DESC_THREADS + threadIdx.x; i < A.n_total; i += (long long)gridDim.x * SC_DESC_THREADS) {
        int j = int(i), k = 0;
        if (j >= A.c[0].n) { j -= A.c[0].n; k = 1; if (j >= A.c[1].n) { j -= A.c[1].n; k = 2; } }
        const float *rec = reinterpret_cast<const float *>(A.c[k].p + size_t(j) * size_t(A.stride));
        const float x = rec[0], y = rec[1];
        const ScPoint p = sc_point(x, y, rec[2], A.R, A.S, A.lidar_height, A.max_radius);
        if (p.what == SC_PT_SKIPPED) atomicAdd(&A.counters[1], 1);
        else if (p.what == SC_PT_UNDECIDED) {
            const int u = atomicAdd(&A.counters[0], 1);
            if (u < A.n_total) A.unc[u] = make_float4(x, y, p.zf, __int_as_float(p.ring));
        }
        else if (p.what == SC_PT_BINNED) atomicMax(&s_grid[p.cell], p.e);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += SC_DESC_THREADS) {
        const int e = s_grid[b];
        if (e > empty) atomicMax(&A.grid[b], e);
    }
}

// The batched build (mlh_sc_add_keyframes): one workgroup per chunk of sc_host.hpp's plan -- a run of ONE entry's points, its keyframe's three clouds back to back in
// the order sc_desc_kernel reads them. The same LDS image of the polar grid, flushed into the entry's own slot; the undecided points of the whole batch go to one
// list through one counter, each with its entry in the parallel array unc_entry (the fourth word keeps the ring, as in the single add).
struct ScBatchEntry { unsigned long long off[3]; int n[3]; int pad; };      // a keyframe's clouds: first records in KfStore::pts, lengths
struct ScDescBatchArgs {
    const float4 *pts;
    const ScBatchEntry *entries;
    const ScChunk *chunks;
    int R, S, unc_cap;
    double lidar_height, max_radius;
    int *grid0;           // the slot of the batch's first entry; entry e's is R * S * e cells further
    float4 *unc;          // unc_cap = the batch's point count
    int *unc_entry;
    int *counters;
};

__global__ __launch_bounds__(SC_DESC_THREADS) void sc_desc_batch_kernel(ScDescBatchArgs A)
{
    extern __shared__ int s_grid[];
    const int bins = A.R * A.S, empty = sc_encode(SC_NO_POINT);
    const ScChunk ch = A.chunks[blockIdx.x];
    const ScBatchEntry en = A.entries[ch.entry];
    for (int b = threadIdx.x; b < bins; b += SC_DESC_THREADS) s_grid[b] = empty;
    __syncthreads();
    for (long long o = threadIdx.x; o < ch.count; o += SC_DESC_THREADS) {
        int j = ch.first + int(o), k = 0;
        if (j >= en.n[0]) { j -= en.n[0]; k = 1; if (j >= en.n[1]) { j -= en.n[1]; k = 2; } }
        const float4 v = A.pts[en.off[k] + (unsigned long long)j];
        const ScPoint p = sc_point(v.x, v.y, v.z, A.R, A.S, A.lidar_height, A.max_radius);
        if (p.what == SC_PT_SKIPPED) atomicAdd(&A.counters[1], 1);
        else if (p.what == SC_PT_UNDECIDED) {
            const int u = atomicAdd(&A.counters[0], 1);
            if (u < A.unc_cap) { A.unc[u] = make_float4(v.x, v.y, p.zf, __int_as_float(p.ring)); A.unc_entry[u] = ch.entry; }
        }
        else if (p.what == SC_PT_BINNED) atomicMax(&s_grid[p.cell], p.e);
    }
    __syncthreads();
    int *grid = A.grid0 + size_t(ch.entry) * size_t(bins);
    for (int b = threadIdx.x; b < bins; b += SC_DESC_THREADS) {
        const int e = s_grid[b];
        if (e > empty) atomicMax(&grid[b], e);
    }
}

struct ScFinishArgs {
    int *grid;            // in: the cells as integers; out: the descriptor as f32, column-major
    const int2 *fix;      // {cell, encoded z'} per undecided point the host kept
    int n_fix, R, S;
    float *ring_key;
    double *sector_key, *col_norm;
};

// the body of both finish kernels: one workgroup of 1024 threads, s_cell = R * S ints of LDS
__device__ __forceinline__ void sc_finish_body(const ScFinishArgs &F, int *s_cell)
{
    const int bins = F.R * F.S;
    for (int b = threadIdx.x; b < bins; b += 1024) s_cell[b] = F.grid[b];
    __syncthreads();
    for (int k = threadIdx.x; k < F.n_fix; k += 1024) {
        const int2 f = F.fix[k];
        if (f.x >= 0 && f.x < bins) atomicMax(&s_cell[f.x], f.y);
    }
    __syncthreads();
    float *desc = reinterpret_cast<float *>(F.grid);
    for (int b = threadIdx.x; b < bins; b += 1024) {
        float v = sc_decode(s_cell[b]);
        if (v == SC_NO_POINT) v = 0.f;                                   // cpp:181-184
        desc[b] = v;
        s_cell[b] = __float_as_int(v);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < F.R; r += 1024) {                      // makeRingkeyFromScancontext: the row's mean, left to right; eig2stdvec makes it float
        double acc = 0.0;
        for (int c = 0; c < F.S; ++c) acc += double(__int_as_float(s_cell[c * F.R + r]));
        F.ring_key[r] = float(acc / double(F.S));
    }
    for (int c = threadIdx.x; c < F.S; c += 1024) {                      // makeSectorkeyFromScancontext: the column's mean; and the column's norm
        double acc = 0.0, sq = 0.0;
        for (int r = 0; r < F.R; ++r) { const double v = double(__int_as_float(s_cell[c * F.R + r])); acc += v; sq += v * v; }
        F.sector_key[c] = acc / double(F.R);
        F.col_norm[c] = sqrt(sq);
    }
}

__global__ __launch_bounds__(1024) void sc_finish_kernel(ScFinishArgs F)
{
    extern __shared__ int s_cell[];
    sc_finish_body(F, s_cell);
}

// the batch's: one workgroup per entry, with that entry's range of the verdicts (grouped by entry on the host: fix_start[e] .. fix_start[e + 1])
struct ScFinishBatchArgs {
    int *grid0;
    const int2 *fix;
    const int *fix_start;
    int R, S;
    float *ring_key0;
    double *sector_key0, *col_norm0;
};

__global__ __launch_bounds__(1024) void sc_finish_batch_kernel(ScFinishBatchArgs B)
{
    extern __shared__ int s_cell[];
    const size_t e = blockIdx.x;
    ScFinishArgs F;
    F.grid = B.grid0 + e * size_t(B.R) * size_t(B.S);
    F.fix = B.fix + B.fix_start[e]; F.n_fix = B.fix_start[e + 1] - B.fix_start[e]; F.R = B.R; F.S = B.S;
    F.ring_key = B.ring_key0 + e * size_t(B.R);
    F.sector_key = B.sector_key0 + e * size_t(B.S);
    F.col_norm = B.col_norm0 + e * size_t(B.S);
    sc_finish_body(F, s_cell);
}

// a query's small arrays, one block of device memory
struct ScWork {
    double score; int nn_idx, shift, n_scored, pad;      // sc_argmin_kernel's result (24 bytes + pad: 32)
    double pad2;
    int cand[SC_MAX_CANDIDATES];
    int cand_shift[SC_MAX_CANDIDATES];
    double cand_dist[SC_MAX_CANDIDATES];
    float cand_d2[SC_MAX_CANDIDATES];
};

__global__ __launch_bounds__(256) void sc_keydist_kernel(const float *ring_key, int R, int P, int que, unsigned long long *keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float *a = ring_key + size_t(que) * R, *b = ring_key + size_t(i) * R;
    float result = 0.f;
    int d = 0;
    for (; d + 3 < R; d += 4) {
        const float d0 = a[d] - b[d], d1 = a[d + 1] - b[d + 1], d2 = a[d + 2] - b[d + 2], d3 = a[d + 3] - b[d + 3];
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; d < R; ++d) { const float d0 = a[d] - b[d]; result += d0 * d0; }
    keys[i] = ((unsigned long long)__float_as_uint(result) << 32) | (unsigned long long)(unsigned)i;      // result >= 0: its bits order as it does
}

__global__ __launch_bounds__(1024) void sc_select_kernel(const unsigned long long *keys, int P, int k, ScWork *W)
{
    __shared__ unsigned long long s_sel[SC_MAX_CANDIDATES];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_prefix, s_mask;
    __shared__ int s_remaining, s_count;
    const int t = threadIdx.x, n_out = min(P, k);
    unsigned long long bound = ~0ull;                    // every word <= bound is a candidate
    if (P > k) {
        // the k-th smallest word (they are all different: the index is part of them), a byte per pass from the top
        if (t == 0) { s_prefix = 0ull; s_mask = 0ull; s_remaining = k; }
        for (int pass = 7; pass >= 0; --pass) {
            const int sh = pass * 8;
            if (t < 256) s_hist[t] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix, mask = s_mask;
            for (int i = t; i < P; i += 1024) {
                const unsigned long long w = keys[i];
                if ((w & mask) == prefix) atomicAdd(&s_hist[int((w >> sh) & 255ull)], 1);
            }
            __syncthreads();
            if (t == 0) {
                int left = s_remaining, b = 0;
                while (b < 255 && s_hist[b] < left) { left -= s_hist[b]; ++b; }
                s_remaining = left;
                s_prefix = prefix | ((unsigned long long)b << sh);
                s_mask = mask | (255ull << sh);
            }
            __syncthreads();
        }
        bound = s_prefix;
    }
    if (t == 0) s_count = 0;
    __syncthreads();
    for (int i = t; i < P; i += 1024) {
        const unsigned long long w = keys[i];
        if (w <= bound) { const int at = atomicAdd(&s_count, 1); if (at < SC_MAX_CANDIDATES) s_sel[at] = w; }
    }
    __syncthreads();
    if (t < n_out) {
        const unsigned long long w = s_sel[t];
        int rank = 0;
        for (int j = 0; j < n_out; ++j) rank += s_sel[j] < w ? 1 : 0;
        W->cand[rank] = int(unsigned(w & 0xffffffffull));
        W->cand_d2[rank] = __uint_as_float(unsigned(w >> 32));
    }
}

struct ScScoreArgs {
    const float *desc;
    const double *sector_key, *col_norm;
    ScWork *W;
    int single;           // >= 0: score this entry as candidate 0 (mlh_sc_distance) instead of W->cand[blockIdx.x]
    int que, R, S, radius;
};

__device__ __forceinline__ bool sc_better(double d, int s, double best_d, int best_s) { return d < best_d || (d == best_d && s < best_s); }

__global__ __launch_bounds__(256) void sc_score_kernel(ScScoreArgs A)
{
    __shared__ double s_key[2 * SC_KEY_LDS];
    __shared__ double s_val[256];
    __shared__ int s_idx[256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, R = A.R, S = A.S;
    const int cand = A.single >= 0 ? A.single : A.W->cand[blockIdx.x];
    const double *qk = A.sector_key + size_t(A.que) * S, *ck = A.sector_key + size_t(cand) * S;
    if (S <= SC_KEY_LDS) {
        for (int c = t; c < S; c += 256) { s_key[c] = qk[c]; s_key[SC_KEY_LDS + c] = ck[c]; }
        qk = s_key; ck = s_key + SC_KEY_LDS;
    }
    __syncthreads();
    // fastAlignUsingVkey (cpp:104-120): shifted.col((i + s) % S) = key2.col(i); the first lowest Frobenius norm, starting from 1e7 at shift 0
    double best = 10000000.0;
    int best_s = 0;
    for (int s = t; s < S; s += 256) {
        double sq = 0.0;
        int cc = S - s;                                   // (0 - s) mod S
        if (cc == S) cc = 0;
        for (int c = 0; c < S; ++c) {
            const double d = qk[c] - ck[cc];
            sq += d * d;
            if (++cc == S) cc = 0;
        }
        const double nrm = sqrt(sq);
        if (nrm < best) { best = nrm; best_s = s; }       // this thread's shifts ascend
    }
    s_val[t] = best; s_idx[t] = best_s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o && sc_better(s_val[t + o], s_idx[t + o], s_val[t], s_idx[t])) { s_val[t] = s_val[t + o]; s_idx[t] = s_idx[t + o]; }
        __syncthreads();
    }
    const int align = s_idx[0];
    __syncthreads();
    // the search space (cpp:130-137) and distDirectSC at each of its shifts (cpp:142-151): ascending shifts and strict < = the least (distance, shift)
    const int n_sh = 2 * A.radius + 1 >= S ? S : 2 * A.radius + 1;
    const float *qd = A.desc + size_t(A.que) * size_t(R) * S, *cd = A.desc + size_t(cand) * size_t(R) * S;
    const double *qn = A.col_norm + size_t(A.que) * S, *cn = A.col_norm + size_t(cand) * S;
    best = 10000000.0; best_s = 0;
    for (int j = wave; j < n_sh; j += 4) {
        int sh = n_sh == S ? j : (align - A.radius + j) % S;
        if (sh < 0) sh += S;
        double sum = 0.0, cnt = 0.0;
        for (int c = lane; c < S; c += 64) {
            int cc = c - sh;
            if (cc < 0) cc += S;
            const double n1 = qn[c], n2 = cn[cc];
            if ((n1 == 0) | (n2 == 0)) continue;          // cpp:89
            const float *u = qd + size_t(c) * R, *v = cd + size_t(cc) * R;
            double dot = 0.0;
            for (int r = 0; r < R; ++r) dot += double(u[r]) * double(v[r]);
            sum += dot / (n1 * n2);
            cnt += 1.0;
        }
        sum = wave_sum(sum); cnt = wave_sum(cnt);
        const double dist = 1.0 - sum / cnt;              // no effective column: 0 / 0, a NaN that never wins
        if (sc_better(dist, sh, best, best_s)) { best = dist; best_s = sh; }
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = best_s; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) if (sc_better(s_val[w], s_idx[w], best, best_s)) { best = s_val[w]; best_s = s_idx[w]; }
        A.W->cand_dist[blockIdx.x] = best;
        A.W->cand_shift[blockIdx.x] = best_s;
    }
}

__global__ void sc_argmin_kernel(ScWork *W, int n)
{
    if (threadIdx.x != 0) return;
    double min_dist = 10000000.0;
    int nn_align = 0, nn_idx = -1;
    for (int i = 0; i < n; ++i) {
        const double d = W->cand_dist[i];
        if (d < min_dist) { min_dist = d; nn_align = W->cand_shift[i]; nn_idx = W->cand[i]; }
    }
    W->score = min_dist; W->nn_idx = nn_idx; W->shift = nn_align; W->n_scored = n;
}

// ---- host side
namespace {

size_t sc_desc_bytes(const ScStore &S) { return sizeof(float) * size_t(S.opts.num_ring) * size_t(S.opts.num_sector); }

int sc_require(mlh_ctx *ctx, const char *entry)
{
    if (!ctx->sc.configured) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": mlh_sc_reset has not been called").c_str());
    return MLH_OK;
}

int sc_check_index(mlh_ctx *ctx, const char *entry, int index)
{
    if (index < 0 || index >= ctx->sc.n) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": no such entry").c_str());
    return MLH_OK;
}

// the pinned block with room for `bytes`; a block that has to grow is only replaced once nothing enqueued can still be copying out of it
int sc_pin(mlh_ctx *ctx, size_t bytes)
{
    ScStore &S = ctx->sc;
    if (bytes <= S.h_pin.cap) return MLH_OK;
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MLH_HIP(ctx, S.h_pin.ensure(bytes, 4096));
    return MLH_OK;
}

// room for `more` entries behind the stored ones: the buffers grow once, to the capacity that many single adds would have doubled their way to
int sc_room(mlh_ctx *ctx, int more)
{
    ScStore &S = ctx->sc;
    if ((long long)S.n + more <= (long long)S.cap) return MLH_OK;
    const size_t have = size_t(S.n), want = size_t(sc_grown_cap(S.n, S.cap, more));
    if (want > size_t(INT32_MAX)) return fail(ctx, MLH_ERR_INVALID, "Scan Context store: more than 2^31 entries");
    const size_t R = size_t(S.opts.num_ring), C = size_t(S.opts.num_sector);
    hipStream_t st = ctx->stream;
    hipError_t e;
    if ((e = S.desc.grow(sizeof(float) * R * C * want, sizeof(float) * R * C * have, st)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc Scan Context store", e);
    if ((e = S.ring_key.grow(sizeof(float) * R * want, sizeof(float) * R * have, st)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc Scan Context store", e);
    if ((e = S.sector_key.grow(sizeof(double) * C * want, sizeof(double) * C * have, st)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc Scan Context store", e);
    if ((e = S.col_norm.grow(sizeof(double) * C * want, sizeof(double) * C * have, st)) != hipSuccess) return fail(ctx, MLH_ERR_HIP, "alloc Scan Context store", e);
    S.cap = int(want);
    return MLH_OK;
}

// one entry from up to three clouds the kernels can read (device records of `stride`)
int sc_add_run(mlh_ctx *ctx, const ScCloudDev dev[3], int stride, const double *position, int32_t *index_out)
{
    ScStore &S = ctx->sc;
    hipStream_t st = ctx->stream;
    const int R = S.opts.num_ring, C = S.opts.num_sector, bins = R * C;
    const long long total = (long long)dev[0].n + dev[1].n + dev[2].n;
    if (total > (long long)INT32_MAX) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add: more than 2^31 points");
    const int n_total = int(total);
    { const int rc = sc_room(ctx, 1); if (rc) return rc; }
    { const int rc = sc_pin(ctx, SC_PIN_HEAD + sizeof(float4) * SC_UNC_FIRST); if (rc) return rc; }
    MLH_HIP(ctx, S.counters.ensure(2 * sizeof(int)));
    MLH_HIP(ctx, S.unc.ensure(sizeof(float4) * size_t(std::max(n_total, 1))));
    int *slot = reinterpret_cast<int *>(S.desc.as<float>() + size_t(S.n) * bins);
    MLH_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(slot), sc_encode(SC_NO_POINT), size_t(bins), st));
    MLH_HIP(ctx, hipMemsetAsync(S.counters.p, 0, 2 * sizeof(int), st));
    int n_unc = 0, n_skipped = 0;
    std::vector<int2> fix;
    if (n_total > 0) {
        ScDescArgs A;
        for (int k = 0; k < 3; ++k) A.c[k] = dev[k];
        A.stride = stride; A.n_total = n_total; A.R = R; A.S = C;
        A.lidar_height = S.opts.lidar_height; A.max_radius = S.opts.max_radius;
        A.grid = slot; A.unc = S.unc.as<float4>(); A.counters = S.counters.as<int>();
        const int blocks = std::min((n_total + SC_DESC_THREADS - 1) / SC_DESC_THREADS, SC_DESC_MAX_BLOCKS);
        MLH_LAUNCH(sc_desc_kernel, dim3(blocks), dim3(SC_DESC_THREADS), sizeof(int) * size_t(bins), st, A);
        MLH_HIP(ctx, hipGetLastError());
        // the counters and the first undecided points in one wait; the host's libm decides them
        unsigned char *pin = S.h_pin.as<unsigned char>();
        int *hc = reinterpret_cast<int *>(pin);
        float4 *hu = reinterpret_cast<float4 *>(pin + SC_PIN_HEAD);
        MLH_HIP(ctx, hipMemcpyAsync(hc, S.counters.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipMemcpyAsync(hu, S.unc.p, sizeof(float4) * size_t(std::min(n_total, SC_UNC_FIRST)), hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, stream_wait_spin(ctx));
        n_unc = std::min(hc[0], n_total); n_skipped = hc[1];
        std::vector<float4> pts(hu, hu + std::min(n_unc, SC_UNC_FIRST));
        if (n_unc > SC_UNC_FIRST) {
            { const int rc = sc_pin(ctx, SC_PIN_HEAD + sizeof(float4) * size_t(n_unc)); if (rc) return rc; }
            hu = reinterpret_cast<float4 *>(S.h_pin.as<unsigned char>() + SC_PIN_HEAD);
            MLH_HIP(ctx, hipMemcpyAsync(hu, S.unc.as<float4>() + SC_UNC_FIRST, sizeof(float4) * size_t(n_unc - SC_UNC_FIRST), hipMemcpyDeviceToHost, st));
            MLH_HIP(ctx, stream_wait_spin(ctx));
            pts.insert(pts.end(), hu, hu + (n_unc - SC_UNC_FIRST));
        }
        const int empty = sc_encode(SC_NO_POINT);
        fix.reserve(pts.size());
        for (const float4 &p : pts) {
            int ring;
            std::memcpy(&ring, &p.w, 4);
            const int e = sc_encode(p.z);
            if (e > empty && ring >= 1 && ring <= R) fix.push_back(make_int2(sc_bin(ring, sc_decide_sector(p.x, p.y, C), R), e));
        }
    }
    ScFinishArgs F;
    F.grid = slot; F.fix = nullptr; F.n_fix = int(fix.size()); F.R = R; F.S = C;
    F.ring_key = S.ring_key.as<float>() + size_t(S.n) * R;
    F.sector_key = S.sector_key.as<double>() + size_t(S.n) * C;
    F.col_norm = S.col_norm.as<double>() + size_t(S.n) * C;
    if (!fix.empty()) {
        // the verdicts travel through the pinned block (the stream is idle: nothing reads it) into the undecided list's own memory (8 <= 16 bytes per point)
        { const int rc = sc_pin(ctx, SC_PIN_HEAD + sizeof(int2) * fix.size()); if (rc) return rc; }
        int2 *hf = reinterpret_cast<int2 *>(S.h_pin.as<unsigned char>() + SC_PIN_HEAD);
        std::memcpy(hf, fix.data(), sizeof(int2) * fix.size());
        MLH_HIP(ctx, hipMemcpyAsync(S.unc.p, hf, sizeof(int2) * fix.size(), hipMemcpyHostToDevice, st));
        F.fix = S.unc.as<int2>();
    }
    MLH_LAUNCH(sc_finish_kernel, dim3(1), dim3(1024), sizeof(int) * size_t(bins), st, F);
    MLH_HIP(ctx, hipGetLastError());
    for (int d = 0; d < 3; ++d) S.pos.push_back(position ? position[d] : 0.0);
    S.has_pos.push_back(position ? 1 : 0);
    S.last_host_decided = n_unc; S.last_skipped = n_skipped;
    S.points_host_decided += n_unc; S.points_skipped += n_skipped;
    if (index_out) *index_out = S.n;
    S.n += 1;
    return MLH_OK;
}

// n > 0 entries from keyframes [first_key, first_key + n) of the mapper's store: what n sc_add_run calls leave, in a fixed number of launches and at most two waits
int sc_add_batch_run(mlh_ctx *ctx, int first_key, int n, int32_t *first_index_out)
{
    ScStore &S = ctx->sc;
    const KfStore &K = ctx->kf;
    hipStream_t st = ctx->stream;
    const int R = S.opts.num_ring, C = S.opts.num_sector, bins = R * C;
    std::vector<ScBatchEntry> ent(static_cast<size_t>(n));
    std::vector<int> n_points(size_t(n), 0);
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        const KfStore::Key &k = K.keys[size_t(first_key) + size_t(i)];
        long long of_entry = 0;
        for (int c = 0; c < 3; ++c) { ent[size_t(i)].off[c] = k.off[c]; ent[size_t(i)].n[c] = k.n[c]; of_entry += k.n[c]; }
        ent[size_t(i)].pad = 0;
        total += of_entry;
        if (total > (long long)INT32_MAX) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add_keyframes: more than 2^31 points in one batch");
        n_points[size_t(i)] = int(of_entry);
    }
    const int n_total = int(total), target = 2 * std::max(ctx->caps.cu_count, 1);
    std::vector<ScChunk> chunks(sc_batch_chunk_bound(n, target));
    const size_t n_chunks = sc_batch_plan(n_points.data(), n, target, chunks.data());
    { const int rc = sc_room(ctx, n); if (rc) return rc; }
    const size_t pin_first = SC_PIN_HEAD + (sizeof(float4) + sizeof(int)) * SC_UNC_FIRST;
    { const int rc = sc_pin(ctx, std::max(pin_first, SC_PIN_HEAD + sizeof(int) * (size_t(n) + 1))); if (rc) return rc; }
    MLH_HIP(ctx, S.counters.ensure(2 * sizeof(int)));
    MLH_HIP(ctx, S.unc.ensure(sizeof(float4) * size_t(std::max(n_total, 1))));
    MLH_HIP(ctx, S.unc_entry.ensure(sizeof(int) * size_t(std::max(n_total, 1))));
    // every table of the call in one upload; the verdicts' ranges follow into their place once the host has made them
    std::vector<unsigned char> &h = S.htab;
    h.clear();
    const size_t o_ent = put(h, ent.data(), ent.size());
    const size_t o_chk = put(h, chunks.data(), n_chunks);
    const size_t o_rng = put<int>(h, nullptr, size_t(n) + 1);
    MLH_HIP(ctx, S.batch_tab.ensure(h.size() + 16));
    unsigned char *dt = S.batch_tab.as<unsigned char>();
    MLH_HIP(ctx, hipMemcpyAsync(dt, h.data(), o_rng, hipMemcpyHostToDevice, st));
    MLH_HIP(ctx, hipMemsetAsync(dt + o_rng, 0, sizeof(int) * (size_t(n) + 1), st));      // no verdicts: every entry's range is empty
    int *slot0 = reinterpret_cast<int *>(S.desc.as<float>() + size_t(S.n) * bins);
    MLH_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(slot0), sc_encode(SC_NO_POINT), size_t(bins) * size_t(n), st));
    MLH_HIP(ctx, hipMemsetAsync(S.counters.p, 0, 2 * sizeof(int), st));
    ScBatchStats B;
    B.n_entries = n; B.n_chunks = int(n_chunks); B.first_index = S.n; B.n_points = n_total;
    int n_unc = 0, n_skipped = 0;
    std::vector<int> start(size_t(n) + 1, 0);
    std::vector<int2> fix;
    if (n_chunks > 0) {
        ScDescBatchArgs A;
        A.pts = K.pts.as<float4>(); A.entries = reinterpret_cast<const ScBatchEntry *>(dt + o_ent); A.chunks = reinterpret_cast<const ScChunk *>(dt + o_chk);
        A.R = R; A.S = C; A.unc_cap = n_total; A.lidar_height = S.opts.lidar_height; A.max_radius = S.opts.max_radius;
        A.grid0 = slot0; A.unc = S.unc.as<float4>(); A.unc_entry = S.unc_entry.as<int>(); A.counters = S.counters.as<int>();
        MLH_LAUNCH(sc_desc_batch_kernel, dim3(unsigned(n_chunks)), dim3(SC_DESC_THREADS), sizeof(int) * size_t(bins), st, A);
        MLH_HIP(ctx, hipGetLastError());
        B.launches += 1;
        // the counters and the first undecided points with their entries in one wait
        unsigned char *pin = S.h_pin.as<unsigned char>();
        int *hc = reinterpret_cast<int *>(pin);
        float4 *hu = reinterpret_cast<float4 *>(pin + SC_PIN_HEAD);
        int *he = reinterpret_cast<int *>(pin + SC_PIN_HEAD + sizeof(float4) * SC_UNC_FIRST);
        const size_t first = size_t(std::min(n_total, SC_UNC_FIRST));
        MLH_HIP(ctx, hipMemcpyAsync(hc, S.counters.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipMemcpyAsync(hu, S.unc.p, sizeof(float4) * first, hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, hipMemcpyAsync(he, S.unc_entry.p, sizeof(int) * first, hipMemcpyDeviceToHost, st));
        MLH_HIP(ctx, stream_wait_spin(ctx));
        B.launches += 1; B.host_waits += 1;
        n_unc = std::min(hc[0], n_total); n_skipped = hc[1];
        std::vector<float4> pts(hu, hu + std::min(n_unc, SC_UNC_FIRST));
        std::vector<int> of(he, he + std::min(n_unc, SC_UNC_FIRST));
        if (n_unc > SC_UNC_FIRST) {
            const size_t rest = size_t(n_unc - SC_UNC_FIRST);
            { const int rc = sc_pin(ctx, SC_PIN_HEAD + (sizeof(float4) + sizeof(int)) * rest); if (rc) return rc; }
            hu = reinterpret_cast<float4 *>(S.h_pin.as<unsigned char>() + SC_PIN_HEAD);
            he = reinterpret_cast<int *>(S.h_pin.as<unsigned char>() + SC_PIN_HEAD + sizeof(float4) * rest);
            MLH_HIP(ctx, hipMemcpyAsync(hu, S.unc.as<float4>() + SC_UNC_FIRST, sizeof(float4) * rest, hipMemcpyDeviceToHost, st));
            MLH_HIP(ctx, hipMemcpyAsync(he, S.unc_entry.as<int>() + SC_UNC_FIRST, sizeof(int) * rest, hipMemcpyDeviceToHost, st));
            MLH_HIP(ctx, stream_wait_spin(ctx));
            B.launches += 1; B.host_waits += 1;
            pts.insert(pts.end(), hu, hu + rest);
            of.insert(of.end(), he, he + rest);
        }
        // the host's verdicts (sc_decide_sector), grouped by entry: a counting sort; within an entry their order does not matter to a maximum
        const int empty = sc_encode(SC_NO_POINT);
        std::vector<int2> verdict(pts.size(), make_int2(-1, 0));
        for (size_t u = 0; u < pts.size(); ++u) {
            const float4 &p = pts[u];
            int ring;
            std::memcpy(&ring, &p.w, 4);
            const int e = sc_encode(p.z);
            if (e > empty && ring >= 1 && ring <= R && of[u] >= 0 && of[u] < n) {
                verdict[u] = make_int2(sc_bin(ring, sc_decide_sector(p.x, p.y, C), R), e);
                start[size_t(of[u]) + 1] += 1;
            }
        }
        for (int i = 0; i < n; ++i) start[size_t(i) + 1] += start[size_t(i)];
        fix.resize(size_t(start[size_t(n)]));
        std::vector<int> at(start.begin(), start.end() - 1);
        for (size_t u = 0; u < pts.size(); ++u) if (verdict[u].x >= 0) fix[size_t(at[size_t(of[u])]++)] = verdict[u];
    }
    if (!fix.empty()) {
        // the verdicts and their ranges travel through the pinned block (the stream is idle behind the wait: nothing reads it)
        const size_t at_fix = (SC_PIN_HEAD + sizeof(int) * start.size() + 15) & ~size_t(15);
        { const int rc = sc_pin(ctx, at_fix + sizeof(int2) * fix.size()); if (rc) return rc; }
        unsigned char *pin = S.h_pin.as<unsigned char>();
        std::memcpy(pin + SC_PIN_HEAD, start.data(), sizeof(int) * start.size());
        MLH_HIP(ctx, hipMemcpyAsync(dt + o_rng, pin + SC_PIN_HEAD, sizeof(int) * start.size(), hipMemcpyHostToDevice, st));
        std::memcpy(pin + at_fix, fix.data(), sizeof(int2) * fix.size());
        MLH_HIP(ctx, hipMemcpyAsync(S.unc.p, pin + at_fix, sizeof(int2) * fix.size(), hipMemcpyHostToDevice, st));      // (8 <= 16 bytes per point: it fits)
    }
    ScFinishBatchArgs F;
    F.grid0 = slot0; F.fix = S.unc.as<int2>(); F.fix_start = reinterpret_cast<const int *>(dt + o_rng); F.R = R; F.S = C;
    F.ring_key0 = S.ring_key.as<float>() + size_t(S.n) * R;
    F.sector_key0 = S.sector_key.as<double>() + size_t(S.n) * C;
    F.col_norm0 = S.col_norm.as<double>() + size_t(S.n) * C;
    MLH_LAUNCH(sc_finish_batch_kernel, dim3(unsigned(n)), dim3(1024), sizeof(int) * size_t(bins), st, F);
    MLH_HIP(ctx, hipGetLastError());
    B.launches += 1;
    for (int i = 0; i < n; ++i) {
        const KfStore::Key &k = K.keys[size_t(first_key) + size_t(i)];
        for (int d = 0; d < 3; ++d) S.pos.push_back(k.pose[d]);
        S.has_pos.push_back(1);
    }
    S.last_host_decided = n_unc; S.last_skipped = n_skipped;
    S.points_host_decided += n_unc; S.points_skipped += n_skipped;
    B.host_decided = n_unc; B.skipped = n_skipped;
    S.batch = B;
    if (first_index_out) *first_index_out = S.n;
    S.n += n;
    return MLH_OK;
}

int sc_work(mlh_ctx *ctx, ScWork **W)
{
    MLH_HIP(ctx, ctx->sc.work.ensure(sizeof(ScWork)));
    *W = ctx->sc.work.as<ScWork>();
    return MLH_OK;
}

// the candidates of entry `que` among entries [0, prefix) into ScWork::cand, nearest first; two launches
int sc_search_enqueue(mlh_ctx *ctx, int que, int prefix, ScWork *W)
{
    ScStore &S = ctx->sc;
    MLH_HIP(ctx, S.keys.ensure(sizeof(unsigned long long) * size_t(std::max(S.cap, 1))));
    MLH_LAUNCH(sc_keydist_kernel, dim3((prefix + 255) / 256), dim3(256), 0, ctx->stream, (const float *)S.ring_key.as<float>(), S.opts.num_ring, prefix, que,
               S.keys.as<unsigned long long>());
    MLH_LAUNCH(sc_select_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)S.keys.as<unsigned long long>(), prefix, S.opts.num_candidates, W);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

void sc_score_enqueue(mlh_ctx *ctx, int que, int single, int n_cand, ScWork *W)
{
    ScStore &S = ctx->sc;
    ScScoreArgs A;
    A.desc = S.desc.as<float>(); A.sector_key = S.sector_key.as<double>(); A.col_norm = S.col_norm.as<double>(); A.W = W;
    A.single = single; A.que = que; A.R = S.opts.num_ring; A.S = S.opts.num_sector; A.radius = sc_search_radius(S.opts.search_ratio, S.opts.num_sector);
    MLH_LAUNCH(sc_score_kernel, dim3(n_cand), dim3(256), 0, ctx->stream, A);
}

}  // namespace

}  // namespace mlh

using namespace mlh;

extern "C" {

void mlh_sc_opts_default(mlh_sc_opts *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->lidar_height = 2.0; o->num_ring = 20; o->num_sector = 60; o->max_radius = 80.0;       // config_loop_realvehicle.yaml
    o->num_exclude_recent = 50; o->num_candidates = 50; o->search_ratio = 0.1; o->dist_thres = 0.5; o->tree_making_period = 10;
    o->loop_distance_threshold = 50.0;
}

int mlh_sc_reset(mlh_ctx *ctx, const mlh_sc_opts *opts)
{
    if (!ctx) return MLH_ERR_INVALID;
    mlh_sc_opts o;
    if (opts) o = *opts; else mlh_sc_opts_default(&o);
    if (const char *fault = sc_opts_fault(o)) return fail(ctx, MLH_ERR_INVALID, (std::string("mlh_sc_reset: bad ") + fault).c_str());
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ScStore &S = ctx->sc;
    S.desc.release(); S.ring_key.release(); S.sector_key.release(); S.col_norm.release();
    S.unc.release(); S.counters.release(); S.keys.release(); S.work.release(); S.unc_entry.release(); S.batch_tab.release();
    S.batch = ScBatchStats();
    S.opts = o; S.configured = true;
    S.n = 0; S.cap = 0; S.pos.clear(); S.has_pos.clear(); S.book = ScBook();
    S.last_host_decided = S.last_skipped = 0; S.points_host_decided = S.points_skipped = 0;
    return MLH_OK;
}

int mlh_sc_add(mlh_ctx *ctx, const void *const *clouds, const int32_t *n, int n_clouds, int stride_bytes, int mem, const double *position, int32_t *index_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_add"); if (rc) return rc; }
    if (n_clouds < 0 || n_clouds > 3 || (n_clouds > 0 && (!clouds || !n))) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add: 0..3 clouds");
    if (position && !(std::isfinite(position[0]) && std::isfinite(position[1]) && std::isfinite(position[2]))) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add: bad position");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    Records rec[3];
    size_t host_bytes = 0;
    for (int k = 0; k < n_clouds; ++k) {
        rec[k] = records_of(clouds[k], stride_bytes, n[k], mem);
        const int rc = records_check(ctx, "mlh_sc_add", rec[k], true);
        if (rc) return rc;
        if (mem == MLH_MEM_HOST) host_bytes += rec[k].bytes();
    }
    if (host_bytes) MLH_HIP(ctx, ctx->tmp.ensure(host_bytes));        // the clouds are staged side by side: sized before the first one lands
    ScCloudDev dev[3] = {{nullptr, 0}, {nullptr, 0}, {nullptr, 0}};
    size_t at = 0;
    for (int k = 0; k < n_clouds; ++k) {
        const unsigned char *d = nullptr;
        const int rc = records_stage(ctx, rec[k], ctx->tmp, ctx->stream, &d, at);
        if (rc) return rc;
        if (mem == MLH_MEM_HOST) at += rec[k].bytes();
        dev[k].p = d; dev[k].n = rec[k].n;
    }
    const int rc = sc_add_run(ctx, dev, stride_bytes, position, index_out);
    if (rc) return rc;
    if (host_bytes) MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));     // the caller's clouds have been read when the call returns
    return MLH_OK;
}

int mlh_sc_add_keyframe(mlh_ctx *ctx, int32_t key, int32_t *index_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_add_keyframe"); if (rc) return rc; }
    KfStore &K = ctx->kf;
    if (key < 0 || size_t(key) >= K.keys.size()) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add_keyframe: no such keyframe");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const KfStore::Key &k = K.keys[size_t(key)];
    ScCloudDev dev[3];
    for (int c = 0; c < 3; ++c) {
        dev[c].n = k.n[c];
        dev[c].p = k.n[c] > 0 ? reinterpret_cast<const unsigned char *>(K.pts.as<float4>() + k.off[c]) : nullptr;
    }
    return sc_add_run(ctx, dev, int(sizeof(float4)), k.pose, index_out);
}

int mlh_sc_add_keyframes(mlh_ctx *ctx, int32_t first_key, int32_t n, int32_t *first_index_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_add_keyframes"); if (rc) return rc; }
    ScStore &S = ctx->sc;
    if (first_key < 0 || n < 0 || (long long)first_key + n > (long long)ctx->kf.keys.size()) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add_keyframes: no such keyframes");
    if ((long long)S.n + n > (long long)INT32_MAX) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_add_keyframes: more than 2^31 entries");
    if (n == 0) { if (first_index_out) *first_index_out = S.n; return MLH_OK; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return sc_add_batch_run(ctx, first_key, n, first_index_out);
}

int mlh_sc_last_batch(mlh_ctx *ctx, mlh_sc_batch_info *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_last_batch: null output");
    const ScBatchStats &B = ctx->sc.batch;
    std::memset(out, 0, sizeof(*out));
    out->n_entries = B.n_entries; out->n_chunks = B.n_chunks; out->launches = B.launches; out->host_waits = B.host_waits;
    out->first_index = B.first_index; out->chunk_points = SC_BATCH_CHUNK_POINTS; out->max_chunks_per_entry = SC_BATCH_MAX_CHUNKS;
    out->target_workgroups = 2 * std::max(ctx->caps.cu_count, 1);
    out->n_points = B.n_points; out->points_host_decided = B.host_decided; out->points_skipped = B.skipped;
    return MLH_OK;
}

int mlh_sc_detect(mlh_ctx *ctx, int32_t que_index, mlh_sc_result *result)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_detect"); if (rc) return rc; }
    if (!result) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_detect: null result");
    { const int rc = sc_check_index(ctx, "mlh_sc_detect", que_index); if (rc) return rc; }
    ScStore &S = ctx->sc;
    std::memset(result, 0, sizeof(*result));
    result->match_index = -1; result->nearest_index = -1;
    if (sc_early_return(que_index, S.opts)) { result->score = -1.0; return MLH_OK; }      // QueryResult(-1, -1, 0.0), cpp:246-250
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const int prefix = sc_book_query(S.book, que_index, S.opts);
    const int n_cand = std::min(prefix, S.opts.num_candidates);
    ScWork *W;
    { const int rc = sc_work(ctx, &W); if (rc) return rc; }
    { const int rc = sc_pin(ctx, SC_PIN_HEAD); if (rc) return rc; }
    { const int rc = sc_search_enqueue(ctx, que_index, prefix, W); if (rc) return rc; }
    sc_score_enqueue(ctx, que_index, -1, n_cand, W);
    MLH_LAUNCH(sc_argmin_kernel, dim3(1), dim3(64), 0, ctx->stream, W, n_cand);
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipMemcpyAsync(S.h_pin.p, W, 32, hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    const ScWork *h = S.h_pin.as<ScWork>();
    result->score = h->score; result->nearest_index = h->nn_idx; result->shift = h->shift; result->n_candidates_scored = h->n_scored;
    result->yaw_diff_rad = sc_yaw(h->shift, S.opts.num_sector);
    if (h->score < S.opts.dist_thres) {                                                    // cpp:304-307
        result->match_index = h->nn_idx;
        if (h->nn_idx >= 0 && S.has_pos[size_t(que_index)] && S.has_pos[size_t(h->nn_idx)] &&
            sc_too_far(&S.pos[3 * size_t(que_index)], &S.pos[3 * size_t(h->nn_idx)], S.opts.loop_distance_threshold)) {
            result->match_index = -1; result->rejected_by_distance = 1;                   // pose_graph.cpp:309-313
        }
    }
    return MLH_OK;
}

int mlh_sc_candidates(mlh_ctx *ctx, int32_t que_index, int32_t prefix, int32_t *idx_out, float *d2_out, int32_t *n_out)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_candidates"); if (rc) return rc; }
    { const int rc = sc_check_index(ctx, "mlh_sc_candidates", que_index); if (rc) return rc; }
    ScStore &S = ctx->sc;
    if (prefix < 1 || prefix > S.n || !idx_out || !n_out) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_candidates: 1 <= prefix <= entries, outputs not null");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const int n_cand = std::min(prefix, S.opts.num_candidates);
    ScWork *W;
    { const int rc = sc_work(ctx, &W); if (rc) return rc; }
    { const int rc = sc_pin(ctx, SC_PIN_HEAD + 8 * SC_MAX_CANDIDATES); if (rc) return rc; }
    { const int rc = sc_search_enqueue(ctx, que_index, prefix, W); if (rc) return rc; }
    unsigned char *pin = S.h_pin.as<unsigned char>() + SC_PIN_HEAD;
    MLH_HIP(ctx, hipMemcpyAsync(pin, W->cand, sizeof(int) * size_t(n_cand), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipMemcpyAsync(pin + 4 * SC_MAX_CANDIDATES, W->cand_d2, sizeof(float) * size_t(n_cand), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    std::memcpy(idx_out, pin, sizeof(int) * size_t(n_cand));
    if (d2_out) std::memcpy(d2_out, pin + 4 * SC_MAX_CANDIDATES, sizeof(float) * size_t(n_cand));
    *n_out = n_cand;
    return MLH_OK;
}

int mlh_sc_distance(mlh_ctx *ctx, int32_t i, int32_t j, double *dist, int32_t *shift)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_distance"); if (rc) return rc; }
    { const int rc = sc_check_index(ctx, "mlh_sc_distance", i); if (rc) return rc; }
    { const int rc = sc_check_index(ctx, "mlh_sc_distance", j); if (rc) return rc; }
    if (!dist || !shift) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_distance: null output");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    ScStore &S = ctx->sc;
    ScWork *W;
    { const int rc = sc_work(ctx, &W); if (rc) return rc; }
    { const int rc = sc_pin(ctx, SC_PIN_HEAD); if (rc) return rc; }
    sc_score_enqueue(ctx, i, j, 1, W);
    MLH_HIP(ctx, hipGetLastError());
    unsigned char *pin = S.h_pin.as<unsigned char>();
    MLH_HIP(ctx, hipMemcpyAsync(pin, W->cand_dist, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipMemcpyAsync(pin + 8, W->cand_shift, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    std::memcpy(dist, pin, sizeof(double));
    std::memcpy(shift, pin + 8, sizeof(int));
    return MLH_OK;
}

int mlh_sc_fetch(mlh_ctx *ctx, int32_t index, double *desc, float *ring_key, double *sector_key)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = sc_require(ctx, "mlh_sc_fetch"); if (rc) return rc; }
    { const int rc = sc_check_index(ctx, "mlh_sc_fetch", index); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    ScStore &S = ctx->sc;
    const size_t R = size_t(S.opts.num_ring), C = size_t(S.opts.num_sector), at_desc = SC_PIN_HEAD + sizeof(double) * C, at_ring = at_desc + sizeof(float) * R * C;
    { const int rc = sc_pin(ctx, at_ring + sizeof(float) * R); if (rc) return rc; }
    unsigned char *pin = S.h_pin.as<unsigned char>();
    hipStream_t st = ctx->stream;
    MLH_HIP(ctx, hipMemcpyAsync(pin + SC_PIN_HEAD, S.sector_key.as<double>() + size_t(index) * C, sizeof(double) * C, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipMemcpyAsync(pin + at_desc, S.desc.as<float>() + size_t(index) * R * C, sizeof(float) * R * C, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipMemcpyAsync(pin + at_ring, S.ring_key.as<float>() + size_t(index) * R, sizeof(float) * R, hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    if (sector_key) std::memcpy(sector_key, pin + SC_PIN_HEAD, sizeof(double) * C);
    if (ring_key) std::memcpy(ring_key, pin + at_ring, sizeof(float) * R);
    if (desc) {
        const float *d = reinterpret_cast<const float *>(pin + at_desc);
        for (size_t b = 0; b < R * C; ++b) desc[b] = double(d[b]);
    }
    return MLH_OK;
}

int mlh_sc_info(mlh_ctx *ctx, mlh_sc_store_info *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_sc_info: null output");
    const ScStore &S = ctx->sc;
    std::memset(out, 0, sizeof(*out));
    out->n_entries = S.n; out->searched_prefix = S.book.prefix; out->period_counter = S.book.counter;
    out->desc_tile_points = SC_DESC_THREADS; out->desc_wrap_points = SC_DESC_THREADS * SC_DESC_MAX_BLOCKS;
    out->last_host_decided = S.last_host_decided; out->last_skipped = S.last_skipped;
    out->points_host_decided = S.points_host_decided; out->points_skipped = S.points_skipped;
    out->bytes_hbm = int64_t(S.desc.cap + S.ring_key.cap + S.sector_key.cap + S.col_norm.cap + S.unc.cap + S.counters.cap + S.keys.cap + S.work.cap + S.unc_entry.cap + S.batch_tab.cap);
    return MLH_OK;
}

}  // extern "C"
