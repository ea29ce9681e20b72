// The odometry's sliding window and the local maps built from it, on the device (gfx950).
//
// The estimator keeps per LiDAR and kind a CircularBuffer<PointICloud> of WINDOW_SIZE + 1 slots (surf_points_stack_[n], corner_points_stack_[n]). Before every
// optimizeMap it thins the new scan's features into a slot (estimator/src/estimator/estimator.cpp:485-496), slides the window (slideWindow, cpp:1521-1536) and
// rebuilds one local map per LiDAR (buildLocalMap, cpp:1159-1204; buildCalibMap, cpp:1067-1110). Here:
//   the store   float4 {x, y, z, intensity} records, the layout of FeatSet::pts and of the keyframe store, in one arena per kind cut into equal slabs. A slot names
//               a slab (or the empty cloud), a slab counts the slots that name it: slideWindow's push (CircularBuffer.h:186-197) moves names and counts on the host
//               and copies no point. A cloud larger than the slabs re-cuts the arena (one allocation); in steady state nothing is allocated or freed.
//   the maps    host: the n_lidar x window_size x 2 stored clouds as SEGMENTS in destination order (per LiDAR, per kind, per slot) and one FuseXf per (LiDAR, slot)
//               from pose_local (xf_from_pose: the rotation in double, rounded once); stored_clouds_build (cloudbuild.hip: the builder shared with the loop closure's
//               local maps) does the rest: pcl::transformPointCloud of every segment into its pre-filter cloud (cpp:1185-1191 / 1095-1101; `+=` in slot order) in ONE
//               launch, then pcl::VoxelGrid<PointI> per pre-filter cloud at its leaf (cpp:1103-1109, 1195-1203). Two host waits per build.
#include "ctx.hpp"
#include <algorithm>
#include <climits>
#include <cmath>

namespace mlh {

namespace {

constexpr int WIN_MAX = 16;                 // LiDARs, window size

int slot_index(const WinStore &W, int lidar, int slot) { return lidar * (W.window + 1) + (W.start + slot) % (W.window + 1); }

void slab_unref(WinStore &W, int kind, int s)
{
    if (s >= 0 && --W.slab_refs[kind][size_t(s)] == 0) W.slab_n[kind][size_t(s)] = 0;
}

// The arena of `kind` re-cut into slabs of at least n records, the live slabs copied over. The old arena is let go of only behind those copies.
int arena_recut(mlh_ctx *ctx, int kind, int n)
{
    WinStore &W = ctx->win;
    hipStream_t st = ctx->stream;
    const size_t n_slabs = W.slab_refs[kind].size(), slab = size_t(n) + size_t(n) / 4 + 64;
    DevBuf fresh;
    ++W.allocations;
    MLH_HIP(ctx, fresh.ensure(sizeof(float4) * slab * n_slabs));
    bool copied = false;
    for (size_t s = 0; s < n_slabs; ++s) {
        if (W.slab_refs[kind][s] == 0 || W.slab_n[kind][s] == 0) continue;
        MLH_HIP(ctx, hipMemcpyAsync(fresh.as<float4>() + s * slab, W.arena[kind].as<float4>() + s * W.slab[kind], sizeof(float4) * size_t(W.slab_n[kind][s]),
                                    hipMemcpyDeviceToDevice, st));
        copied = true;
    }
    if (copied || W.arena[kind].p) MLH_HIP(ctx, hipStreamSynchronize(st));      // (an earlier launch may still be reading the old arena)
    std::swap(W.arena[kind].p, fresh.p);
    std::swap(W.arena[kind].cap, fresh.cap);
    W.slab[kind] = slab;
    return MLH_OK;
}

bool bad_pose(const double *p) { for (int i = 0; i < 7; ++i) if (!std::isfinite(p[i])) return true; return false; }

}  // namespace

int window_check_slot(mlh_ctx *ctx, const char *entry, int lidar, int slot)
{
    const WinStore &W = ctx->win;
    if (!W.ready) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": mlh_window_reset comes first").c_str());
    if (lidar < 0 || lidar >= W.n_lidar) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": no such LiDAR").c_str());
    if (slot < 0 || slot > W.window) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": the slot is outside 0 .. window_size").c_str());
    return MLH_OK;
}

int window_reset_run(mlh_ctx *ctx, int n_lidar, int window_size)
{
    if (n_lidar < 1 || n_lidar > WIN_MAX || window_size < 1 || window_size > WIN_MAX)
        return fail(ctx, MLH_ERR_INVALID, "mlh_window_reset: n_lidar and window_size are 1..16");
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    WinStore &W = ctx->win;
    const size_t n_slots = size_t(n_lidar) * size_t(window_size + 1);
    for (int k = 0; k < 2; ++k) {
        W.arena[k].release();
        W.slab[k] = 0;
        W.slab_refs[k].assign(n_slots, 0);
        W.slab_n[k].assign(n_slots, 0);
        W.slot_slab[k].assign(n_slots, -1);
    }
    W.pre.release(); W.flt.release(); W.tab.release();
    W.map_off.assign(size_t(2 * n_lidar), 0); W.map_pre_n.assign(size_t(2 * n_lidar), 0); W.map_flt_n.assign(size_t(2 * n_lidar), 0);
    W.n_lidar = n_lidar; W.window = window_size;
    W.size = 0; W.start = 0; W.pushes = 0; W.allocations = 0;
    W.ready = true;
    return MLH_OK;
}

int window_assign_device(mlh_ctx *ctx, int lidar, int slot, int kind, const float4 *dev, int n)
{
    WinStore &W = ctx->win;
    const size_t at = size_t(slot_index(W, lidar, slot));
    if (n > 0 && size_t(n) > W.slab[kind]) { const int rc = arena_recut(ctx, kind, n); if (rc) return rc; }
    slab_unref(W, kind, W.slot_slab[kind][at]);
    W.slot_slab[kind][at] = -1;
    if (n <= 0) return MLH_OK;
    // as many slabs as slots, and this slot names none: one is free
    int s = 0;
    while (W.slab_refs[kind][size_t(s)] != 0) ++s;
    MLH_HIP(ctx, hipMemcpyAsync(W.arena[kind].as<float4>() + size_t(s) * W.slab[kind], dev, sizeof(float4) * size_t(n), hipMemcpyDeviceToDevice, ctx->stream));
    W.slab_refs[kind][size_t(s)] = 1;
    W.slab_n[kind][size_t(s)] = n;
    W.slot_slab[kind][at] = s;
    return MLH_OK;
}

static int window_set_run(mlh_ctx *ctx, int lidar, int slot, const void *surf, int n_surf, const void *corner, int n_corner, int stride, int ioff, int mem)
{
    { const int rc = window_check_slot(ctx, "mlh_window_set", lidar, slot); if (rc) return rc; }
    if (ioff < 0) return fail(ctx, MLH_ERR_INVALID, "mlh_window_set: bad intensity_offset_bytes (the stored clouds keep the intensity)");
    const void *src[2] = {surf, corner};
    const int n[2] = {n_surf, n_corner};
    Records r[2];
    size_t off[2] = {0, 0}, total = 0;
    for (int k = 0; k < 2; ++k) {
        r[k] = records_of(src[k], stride, n[k], mem, ioff);
        { const int rc = records_check(ctx, "mlh_window_set", r[k], true); if (rc) return rc; }
        off[k] = total; total += ((r[k].bytes() + 255) / 256) * 256;
    }
    hipStream_t st = ctx->stream;
    // records that are not the store's own float4 {x, y, z, intensity} are packed into a scratch block first (not ctx->tmp: the host clouds are staged there)
    const bool as_stored = stride == int(sizeof(float4)) && ioff == 12;
    if (mem == MLH_MEM_HOST && total > 0) MLH_HIP(ctx, ctx->tmp.ensure(total));
    if (!as_stored) MLH_HIP(ctx, ctx->knn_q.ensure(sizeof(float4) * (size_t(n[0]) + size_t(n[1]) + 1)));
    const float4 *packed[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        if (n[k] == 0) continue;
        const unsigned char *s;
        { const int rc = records_stage(ctx, r[k], ctx->tmp, st, &s, off[k]); if (rc) return rc; }
        if (as_stored) { packed[k] = reinterpret_cast<const float4 *>(s); continue; }
        float4 *dst = ctx->knn_q.as<float4>() + (k == 0 ? 0 : n[0]);
        pack_points_launch(st, s, stride, n[k], ioff, 0.f, -1, dst, nullptr);
        packed[k] = dst;
    }
    MLH_HIP(ctx, hipGetLastError());
    for (int k = 0; k < 2; ++k) { const int rc = window_assign_device(ctx, lidar, slot, k, packed[k], n[k]); if (rc) return rc; }
    if (mem == MLH_MEM_HOST) MLH_HIP(ctx, hipStreamSynchronize(st));      // the caller's clouds have been read when the call returns
    return MLH_OK;
}

static int window_slide_run(mlh_ctx *ctx, int src_slot)
{
    { const int rc = window_check_slot(ctx, "mlh_window_slide", 0, src_slot); if (rc) return rc; }
    WinStore &W = ctx->win;
    const int cap = W.window + 1;
    const int from = (W.start + src_slot) % cap;            // operator[] (CircularBuffer.h:134-137)
    const int to = W.size < cap ? W.size : W.start;         // push (CircularBuffer.h:186-197)
    for (int k = 0; k < 2; ++k)
        for (int l = 0; l < W.n_lidar; ++l) {
            const int s = W.slot_slab[k][size_t(l * cap + from)];
            if (s >= 0) ++W.slab_refs[k][size_t(s)];        // (first: `to` may be `from`)
            slab_unref(W, k, W.slot_slab[k][size_t(l * cap + to)]);
            W.slot_slab[k][size_t(l * cap + to)] = s;
        }
    if (W.size < cap) ++W.size;
    else W.start = (W.start + 1) % cap;
    ++W.pushes;
    return MLH_OK;
}

static int window_cloud_run(mlh_ctx *ctx, int lidar, int slot, int kind, const void **device_points, int32_t *n)
{
    { const int rc = window_check_slot(ctx, "mlh_window_cloud", lidar, slot); if (rc) return rc; }
    if (kind < 0 || kind > 1 || !device_points || !n) return fail(ctx, MLH_ERR_INVALID, "mlh_window_cloud: bad arguments");
    const WinStore &W = ctx->win;
    const int s = W.slot_slab[kind][size_t(slot_index(W, lidar, slot))];
    *n = s < 0 ? 0 : W.slab_n[kind][size_t(s)];
    *device_points = s < 0 ? nullptr : W.arena[kind].as<float4>() + size_t(s) * W.slab[kind];
    return MLH_OK;
}

static int window_info_run(mlh_ctx *ctx, int32_t *n_lidar, int32_t *window_size, int64_t *pushes, int64_t *bytes_used, int64_t *bytes_reserved, int64_t *allocations)
{
    const WinStore &W = ctx->win;
    if (!W.ready) return fail(ctx, MLH_ERR_STATE, "mlh_window_info: mlh_window_reset comes first");
    if (n_lidar) *n_lidar = W.n_lidar;
    if (window_size) *window_size = W.window;
    if (pushes) *pushes = W.pushes;
    if (bytes_used) {
        int64_t used = 0;
        for (int k = 0; k < 2; ++k) for (size_t s = 0; s < W.slab_refs[k].size(); ++s) if (W.slab_refs[k][s] > 0) used += int64_t(sizeof(float4)) * W.slab_n[k][s];
        *bytes_used = used;
    }
    if (bytes_reserved) *bytes_reserved = int64_t(W.arena[0].cap + W.arena[1].cap + W.pre.cap + W.flt.cap + W.tab.cap);
    if (allocations) *allocations = W.allocations;
    return MLH_OK;
}

static int window_build_local_map_run(mlh_ctx *ctx, const double *pose_local, const mlh_window_map_opts *o, int32_t *n_pre, int32_t *n_ds)
{
    WinStore &W = ctx->win;
    if (!W.ready) return fail(ctx, MLH_ERR_STATE, "mlh_window_build_local_map: mlh_window_reset comes first");
    if (!pose_local || !o || !n_pre || !n_ds) return fail(ctx, MLH_ERR_INVALID, "mlh_window_build_local_map: bad arguments (pose_local, opts, n_pre and n_ds are needed)");
    if (o->source_lidar >= W.n_lidar) return fail(ctx, MLH_ERR_INVALID, "mlh_window_build_local_map: no such source_lidar");
    const auto pos_finite = [](float v) { return std::isfinite(v) && v > 0.f; };
    for (int l = 0; l < W.n_lidar; ++l)
        if (!pos_finite(o->leaf_surf[l]) || !pos_finite(o->leaf_corner[l])) return fail(ctx, MLH_ERR_INVALID, "mlh_window_build_local_map: every LiDAR's leaves must be finite and > 0");
    const int cap = W.window + 1, n_clouds = 2 * W.n_lidar;
    for (int i = 0; i < W.n_lidar * cap; ++i) if (bad_pose(pose_local + 7 * i)) return fail(ctx, MLH_ERR_INVALID, "mlh_window_build_local_map: non-finite pose_local");
    // the transforms and the segments, in destination order
    std::vector<FuseXf> xfs(size_t(W.n_lidar * cap));
    for (int i = 0; i < W.n_lidar * cap; ++i) xfs[size_t(i)] = xf_from_pose(pose_local + 7 * i, 0.f);
    std::vector<CloudSegment> segs;
    std::vector<int> off(size_t(n_clouds), 0), len(size_t(n_clouds), 0);
    std::vector<float> leaf(size_t(n_clouds), 0.f);
    size_t N = 0;
    for (int l = 0; l < W.n_lidar; ++l) {
        const int from = o->source_lidar < 0 ? l : o->source_lidar;
        for (int k = 0; k < 2; ++k) {
            const int c = 2 * l + k;
            off[size_t(c)] = int(N);
            leaf[size_t(c)] = k ? o->leaf_corner[l] : o->leaf_surf[l];      // pcl::VoxelGrid<PointI> per cloud (cpp:1103-1109, 1195-1203)
            for (int i = 0; i < W.window; ++i) {            // slot window_size is skipped (cpp:1182)
                const int s = W.slot_slab[k][size_t(slot_index(W, from, i))];
                const int n = s < 0 ? 0 : W.slab_n[k][size_t(s)];
                segs.push_back(CloudSegment{s < 0 ? 0 : size_t(s) * W.slab[k], n, from * cap + i, c});
                N += size_t(n);
                if (N > size_t(INT_MAX) / 2) return fail(ctx, MLH_ERR_NOMEM, "window map: too many points");
            }
            len[size_t(c)] = int(N) - off[size_t(c)];
        }
    }
    W.map_off = off; W.map_pre_n = len; W.map_flt_n.assign(size_t(n_clouds), 0);
    for (int c = 0; c < n_clouds; ++c) { n_pre[c] = len[size_t(c)]; n_ds[c] = 0; }
    MLH_HIP(ctx, W.h_pin.ensure(sizeof(int) * 7 * 2 * WIN_MAX));
    const int rc = stored_clouds_build(ctx, W.arena[0].as<float4>(), W.arena[1].as<float4>(), xfs, segs, n_clouds, off.data(), len.data(), leaf.data(),
                                       CloudBuildBufs{W.pre, W.flt, W.tab, W.htab, W.allocations, W.h_pin.as<int>()}, W.map_flt_n.data());
    for (int c = 0; c < n_clouds; ++c) n_ds[c] = W.map_flt_n[size_t(c)];
    return rc;
}

static int window_map_cloud_run(mlh_ctx *ctx, int lidar, int kind, int filtered, const void **device_points, int32_t *n)
{
    { const int rc = window_check_slot(ctx, "mlh_window_map_cloud", lidar, 0); if (rc) return rc; }
    if (kind < 0 || kind > 1 || (filtered != 0 && filtered != 1) || !device_points || !n) return fail(ctx, MLH_ERR_INVALID, "mlh_window_map_cloud: bad arguments");
    const WinStore &W = ctx->win;
    const size_t c = size_t(2 * lidar + kind);
    *n = filtered ? W.map_flt_n[c] : W.map_pre_n[c];
    *device_points = *n == 0 ? nullptr : (filtered ? W.flt : W.pre).as<float4>() + W.map_off[c];
    return MLH_OK;
}

}  // namespace mlh

using namespace mlh;

extern "C" {

void mlh_window_map_opts_default(mlh_window_map_opts *o, int n_scans, int n_lidar, int window_size)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->source_lidar = -1;
    const float ratio = 0.4 * std::min(2.0, std::max(0.75, 1.0 / 192 * float(n_scans * n_lidar * window_size)));      // cpp:1196
    for (int l = 0; l < WIN_MAX; ++l) o->leaf_surf[l] = o->leaf_corner[l] = ratio;
}

int mlh_window_reset(mlh_ctx *ctx, int n_lidar, int window_size)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return window_reset_run(ctx, n_lidar, window_size);
}

int mlh_window_set(mlh_ctx *ctx, int lidar, int slot, const void *surf, int n_surf, const void *corner, int n_corner, int stride_bytes, int intensity_offset_bytes,
                   int mem)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return window_set_run(ctx, lidar, slot, surf, n_surf, corner, n_corner, stride_bytes, intensity_offset_bytes, mem);
}

int mlh_window_slide(mlh_ctx *ctx, int src_slot)
{
    if (!ctx) return MLH_ERR_INVALID;
    return window_slide_run(ctx, src_slot);
}

int mlh_window_cloud(mlh_ctx *ctx, int lidar, int slot, int kind, const void **device_points, int32_t *n)
{
    if (!ctx) return MLH_ERR_INVALID;
    return window_cloud_run(ctx, lidar, slot, kind, device_points, n);
}

int mlh_window_info(mlh_ctx *ctx, int32_t *n_lidar, int32_t *window_size, int64_t *pushes, int64_t *bytes_used, int64_t *bytes_reserved, int64_t *allocations)
{
    if (!ctx) return MLH_ERR_INVALID;
    return window_info_run(ctx, n_lidar, window_size, pushes, bytes_used, bytes_reserved, allocations);
}

int mlh_window_build_local_map(mlh_ctx *ctx, const double *pose_local, const mlh_window_map_opts *opts, int32_t *n_pre, int32_t *n_ds)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    return window_build_local_map_run(ctx, pose_local, opts, n_pre, n_ds);
}

int mlh_window_map_cloud(mlh_ctx *ctx, int lidar, int kind, int filtered, const void **device_points, int32_t *n)
{
    if (!ctx) return MLH_ERR_INVALID;
    return window_map_cloud_run(ctx, lidar, kind, filtered, device_points, n);
}


// cpp:487-495 for the scan `src` holds: its less-sharp points through pcl::VoxelGrid at leaf_corner, its voxel-thinned less-flat cloud through pcl::VoxelGrid at
// leaf_surf (voxel_filter_run, centroid_all: the arithmetic of mlh_voxel_grid), the results named by stack[lidar][slot] (window.hip)
int mlh_window_set_from_scan(mlh_ctx *ctx, mlh_ctx *src, int lidar, int slot, float leaf_surf, float leaf_corner)
{
    if (!ctx || !src) return MLH_ERR_INVALID;
    { const int rc = window_check_slot(ctx, "mlh_window_set_from_scan", lidar, slot); if (rc) return rc; }
    if (!std::isfinite(leaf_surf) || !(leaf_surf > 0.f) || !std::isfinite(leaf_corner) || !(leaf_corner > 0.f))
        return fail(ctx, MLH_ERR_INVALID, "mlh_window_set_from_scan: the leaves must be finite and > 0");
    if (ctx->device != src->device) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_window_set_from_scan: both contexts must be on the same device");
    ScanBuf &sb = src->scan;
    if (!sb.extracted || !sb.voxelised) return fail(ctx, MLH_ERR_STATE, "mlh_window_set_from_scan: mlh_extract_run and mlh_extract_voxel_run on the source context come first");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int rc = scan_totals(src, true);       // the list sizes: fetched once per scan, on the source's own stream (this context's, or an idle one's)
    if (rc) return src == ctx ? rc : fail(ctx, MLH_ERR_HIP, mlh_last_error(src));
    const int n_in[2] = {sb.h_totals[4], sb.h_totals[1]};      // the thinned less-flat cloud -> SURF, the less-sharp points -> CORNER
    const float leaf[2] = {leaf_surf, leaf_corner};
    if (n_in[MLH_CORNER] > 0) MLH_HIP(ctx, ctx->knn_q.ensure(sizeof(float4) * size_t(n_in[MLH_CORNER])));     // gather scratch (not ctx->tmp: the staging calls may use that)
    if (src != ctx && (rc = ctx->handoff.borrow_begin(ctx, src))) return rc;
    for (int k = 0; k < 2 && !rc; ++k) {
        int n_out = 0;
        if (n_in[k] > 0) {
            const void *in = sb.vox_out.p;
            if (k == MLH_CORNER) {
                gather_points_launch(ctx, sb.pts.as<float4>(), sb.lists[1].as<int>(), n_in[k], ctx->knn_q.as<float4>());
                in = ctx->knn_q.p;
            }
            rc = voxel_filter_run(ctx, in, 16, n_in[k], 12, -1, -1, leaf[k], 0.f, nullptr, &n_out, MLH_MEM_DEVICE, nullptr, true, true);
        }
        if (!rc) rc = window_assign_device(ctx, lidar, slot, k, ctx->vox.out.as<float4>(), n_out);      // copied out of the filter's buffer, behind the filter
    }
    if (src != ctx) { const int erc = ctx->handoff.borrow_end(ctx, src); if (!rc) rc = erc; }
    return rc;
}

}  // extern "C"
