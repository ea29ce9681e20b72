// The scan a context holds, from the caller's records to the extractor's lists (the kernels: extract.hip, voxel.hip): upload, upload ahead, the extraction's entry
// points and read-backs, the undistortion in place. Host logic only.
#include "ctx.hpp"
#include <algorithm>
#include <cstdlib>

namespace mlh {

// the list sizes of the scan the context holds (and the thinned less-flat count once it exists): one host round trip per scan
int scan_totals(mlh_ctx *ctx, bool want_vox)
{
    ScanBuf &sb = ctx->scan;
    const bool need_lists = !sb.h_lists_valid, need_vox = want_vox && !sb.h_vox_valid;
    if (!need_lists && !need_vox) return MLH_OK;
    if (need_lists) MLH_HIP(ctx, hipMemcpyAsync(sb.h_totals, sb.totals.p, sizeof(int) * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (need_vox || (sb.voxelised && !sb.h_vox_valid))
        MLH_HIP(ctx, hipMemcpyAsync(sb.h_totals + 4, sb.ring_vox.as<int>() + 2 * sb.n_rings, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sb.h_lists_valid = true;
    if (sb.voxelised) sb.h_vox_valid = true;
    return MLH_OK;
}

}  // namespace mlh

using namespace mlh;

extern "C" {

// The points of the scan a LATER mlh_scan_upload will stage, sent to the device now, on a copy stream of the context's own: the copy engine moves them beside whatever
// kernels the context's stream is running (the previous scan's extraction, thinning, ...), and the upload leaves the frame's chain (framebench, the estimator / mapper
// pair: period 0.48-0.50 -> 0.42-0.43 ms with the caller's own prefetch; this is the same inside the library). One scan ahead; a second call replaces the first.
int mlh_scan_upload_ahead(mlh_ctx *ctx, const void *points, int stride_bytes, int n)
{
    if (!ctx) return MLH_ERR_INVALID;
    { const int rc = records_check(ctx, "mlh_scan_upload_ahead", records_of(points, stride_bytes, n, MLH_MEM_HOST)); if (rc) return rc; }
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    mlh_ctx::ScanAhead &A = ctx->ahead;
    if (!A.cs) {
        MLH_HIP(ctx, hipStreamCreateWithFlags(&A.cs, hipStreamNonBlocking));
        MLH_HIP(ctx, hipEventCreateWithFlags(&A.ev_arrived, hipEventDisableTiming));
        MLH_HIP(ctx, hipEventCreateWithFlags(&A.ev_consumed, hipEventDisableTiming));
    }
    A.valid = false;
    const size_t bytes = size_t(n) * size_t(stride_bytes);
    if (A.buf.cap < bytes) {
        // a pack kernel of the main stream may still be reading the old block
        if (A.consumed_recorded) MLH_HIP(ctx, hipEventSynchronize(A.ev_consumed));
        MLH_HIP(ctx, hipStreamSynchronize(A.cs));
        MLH_HIP(ctx, A.buf.ensure(bytes));
    }
    // the block is overwritten only behind the pack kernel that read the previous scan out of it
    if (A.consumed_recorded) MLH_HIP(ctx, hipStreamWaitEvent(A.cs, A.ev_consumed, 0));
    MLH_HIP(ctx, hipMemcpyAsync(A.buf.p, points, bytes, hipMemcpyHostToDevice, A.cs));
    MLH_HIP(ctx, hipEventRecord(A.ev_arrived, A.cs));
    // a page-locked source is read by the copy engine in place, later: the consuming mlh_scan_upload gives it back to the caller (it waits for the arrival there);
    // a pageable one has been taken into the runtime's staging memory when hipMemcpyAsync returns
    {
        hipPointerAttribute_t at;
        A.src_pinned = hipPointerGetAttributes(&at, points) == hipSuccess && at.type == hipMemoryTypeHost;
        (void)hipGetLastError();
    }
    A.src = points; A.n = n; A.stride = stride_bytes; A.valid = true;
    ++A.issued;
    return MLH_OK;
}

int mlh_scan_upload(mlh_ctx *ctx, const void *points, int stride_bytes, int intensity_offset_bytes, int n, const int *scan_start,
                    const int *scan_end, int n_rings, int mem)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!scan_start || !scan_end || n_rings <= 0) return fail(ctx, MLH_ERR_INVALID, "bad ring table");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    { const int wrc = ctx->handoff.wait_readers(ctx); if (wrc) return wrc; }
    ScanBuf &sb = ctx->scan;
    sb.extracted = false;
    sb.voxelised = false;
    sb.h_lists_valid = sb.h_vox_valid = false;
    Records rec = records_of(points, stride_bytes, n, mem, intensity_offset_bytes);
    { const int rc = records_check(ctx, "mlh_scan_upload", rec); if (rc) return rc; }
    // A caller's PAGEABLE buffer (a ROS message) goes through hipMemcpyAsync as it is: like cudaMemcpyAsync, the call returns once the pageable source has been
    // copied into the runtime's own staging memory (the DMA to the device may still be in flight), so the buffer is the caller's again when this call returns,
    // and nothing here waits for the stream. MLH_SCAN_STAGE_PINNED=1 makes that independent of the runtime: the points are first copied into a pinned block the
    // context owns (two halves, an event per half) and go to the device from there -- measured +0.08 ms per two-LiDAR frame (the runtime writes small pageable
    // copies faster than an explicit memcpy + DMA pair: scripts/framebench.py, C++ leg, 0.859 against 0.940 ms, two alternations), hence not the default.
    // (A buffer the caller pinned is copied from in place; that case waits below.)
    bool caller_pinned = false;
    int pts_half = -1;
    if (mem == MLH_MEM_HOST) {
        hipPointerAttribute_t at;
        caller_pinned = hipPointerGetAttributes(&at, points) == hipSuccess && at.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        static const bool stage_pinned = std::getenv("MLH_SCAN_STAGE_PINNED") && std::atoi(std::getenv("MLH_SCAN_STAGE_PINNED")) != 0;
        if (!caller_pinned && stage_pinned) {
            const size_t bytes = rec.bytes();
            void *dst = nullptr;
            MLH_HIP(ctx, ctx->h_pts.take(bytes, ((bytes + bytes / 4 + 4095) / 4096) * 4096, ctx->stream, &pts_half, &dst));
            std::memcpy(dst, points, bytes);
            rec.p = static_cast<const unsigned char *>(dst);
        }
    }
    // sent ahead (mlh_scan_upload_ahead with this very buffer)? then the points are on the device already, or on their way: the main stream waits for their arrival and
    // packs from there. Any other host upload drops what was sent ahead (it was another scan's).
    mlh_ctx::ScanAhead &AH = ctx->ahead;
    bool from_ahead = false;
    if (mem == MLH_MEM_HOST && AH.valid) {
        if (AH.src == points && AH.n == n && AH.stride == stride_bytes && pts_half < 0) {
            MLH_HIP(ctx, hipStreamWaitEvent(ctx->stream, AH.ev_arrived, 0));
            if (AH.src_pinned) MLH_HIP(ctx, hipEventSynchronize(AH.ev_arrived));      // issued a frame ago: long done
            rec.p = AH.buf.as<unsigned char>(); rec.mem = MLH_MEM_DEVICE; from_ahead = true; caller_pinned = false;
            ++AH.used;
        }
        AH.valid = false;
    }
    int rc = stage_points(ctx, rec, intensity_offset_bytes >= 0 ? intensity_offset_bytes : PACK_W_ZERO, sb.pts, nullptr, ctx->tmp);
    if (rc) return rc;
    if (from_ahead) { MLH_HIP(ctx, hipEventRecord(AH.ev_consumed, ctx->stream)); AH.consumed_recorded = true; }
    if (pts_half >= 0) MLH_HIP(ctx, ctx->h_pts.record(pts_half, ctx->stream));
    // The ring tables go to the device from a pinned block the context owns (two halves, used alternately; an event says when a half's copy has been read):
    // nothing has to be waited for before this call returns, so the host enqueues the extraction while the points are still being uploaded -- a blocking
    // wait here was ~40 us of idle GPU per frame (profiles/r03_frame_timeline.txt: the gap in front of the curvature kernel).
    const size_t ring_bytes = sizeof(int) * 2 * size_t(n_rings);
    int half = 0;
    void *ring_dst = nullptr;
    MLH_HIP(ctx, ctx->h_rings.take(ring_bytes, ring_bytes + ring_bytes / 2, ctx->stream, &half, &ring_dst));
    int *hs = static_cast<int *>(ring_dst), *he = hs + n_rings;
    if (mem == MLH_MEM_HOST) {
        std::memcpy(hs, scan_start, sizeof(int) * n_rings);
        std::memcpy(he, scan_end, sizeof(int) * n_rings);
    } else {
        MLH_HIP(ctx, hipMemcpyAsync(hs, scan_start, sizeof(int) * n_rings, hipMemcpyDeviceToHost, ctx->stream));
        MLH_HIP(ctx, hipMemcpyAsync(he, scan_end, sizeof(int) * n_rings, hipMemcpyDeviceToHost, ctx->stream));
        MLH_HIP(ctx, stream_wait_spin(ctx));
    }
    // rings are labelled by independent workgroups: that is exact only when the neighbour-suppression reach (+-5) of one
    // ring cannot touch another ring's labelled span, which the ImageSegmenter insets (+5 / -6) guarantee.
    int max_len = 0, prev_end = -1000000;
    for (int r = 0; r < n_rings; ++r) {
        if (he[r] - hs[r] < 6) continue;   // skipped by the extractor (cpp:155)
        if (hs[r] < 5 || he[r] + 5 > n) return fail(ctx, MLH_ERR_INVALID, "scan_start/scan_end must be inset by 5 from the cloud ends");
        if (hs[r] <= prev_end + 4) return fail(ctx, MLH_ERR_UNSUPPORTED, "rings must be ascending and separated by the +5/-6 insets of ScanInfo");
        prev_end = he[r];
        max_len = std::max(max_len, he[r] - hs[r]);
    }
    MLH_HIP(ctx, sb.start.ensure(sizeof(int) * 2 * size_t(n_rings)));                  // [start | end], as they sit in the pinned block: one copy
    MLH_HIP(ctx, hipMemcpyAsync(sb.start.p, hs, sizeof(int) * 2 * n_rings, hipMemcpyHostToDevice, ctx->stream));
    sb.end_alias = sb.start.as<int>() + n_rings;
    MLH_HIP(ctx, ctx->h_rings.record(half, ctx->stream));
    // a buffer the CALLER pinned is read by the copy engine in place, asynchronously, and is the caller's to reuse after this call: that (rare) case waits here
    if (caller_pinned) MLH_HIP(ctx, stream_wait_spin(ctx));
    sb.n = n; sb.n_rings = n_rings; sb.max_ring_len = max_len;
    return MLH_OK;
}

int mlh_extract_run(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    { const int wrc = ctx->handoff.wait_readers(ctx); if (wrc) return wrc; }
    return extract_run(ctx);
}

int mlh_extract_fetch(mlh_ctx *ctx, int32_t *label, float *curvature, int32_t *picked, int32_t *idx_out[4], int32_t n_out[4])
{
    if (!ctx) return MLH_ERR_INVALID;
    ScanBuf &sb = ctx->scan;
    if (!sb.extracted) return fail(ctx, MLH_ERR_STATE, "extract_run has not been called");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int totals[4] = {0, 0, 0, 0};
    MLH_HIP(ctx, hipMemcpyAsync(totals, sb.totals.p, sizeof(totals), hipMemcpyDeviceToHost, st));
    if (label) MLH_HIP(ctx, hipMemcpyAsync(label, sb.label.p, sizeof(int) * size_t(sb.n), hipMemcpyDeviceToHost, st));
    if (curvature) MLH_HIP(ctx, hipMemcpyAsync(curvature, sb.curvature.p, sizeof(float) * size_t(sb.n), hipMemcpyDeviceToHost, st));
    if (picked) MLH_HIP(ctx, hipMemcpyAsync(picked, sb.picked.p, sizeof(int) * size_t(sb.n), hipMemcpyDeviceToHost, st));
    MLH_HIP(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) {
        if (n_out) n_out[i] = totals[i];
        if (idx_out && idx_out[i] && totals[i] > 0)
            MLH_HIP(ctx, hipMemcpyAsync(idx_out[i], sb.lists[i].p, sizeof(int) * size_t(totals[i]), hipMemcpyDeviceToHost, st));
    }
    MLH_HIP(ctx, hipStreamSynchronize(st));
    prof_collect(ctx);
    return MLH_OK;
}

int mlh_extract_voxel_run(mlh_ctx *ctx, float leaf)
{
    if (!ctx || !(leaf > 0.f)) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    { const int wrc = ctx->handoff.wait_readers(ctx); if (wrc) return wrc; }
    return ring_voxel_run(ctx, leaf);
}

int mlh_extract_fetch_voxel(mlh_ctx *ctx, float *xyzi_out, int32_t *n_out)
{
    if (!ctx || !n_out) return MLH_ERR_INVALID;
    ScanBuf &sb = ctx->scan;
    if (!sb.voxelised) return fail(ctx, MLH_ERR_STATE, "extract_voxel_run has not been called");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    int total = 0;
    MLH_HIP(ctx, hipMemcpyAsync(&total, sb.ring_vox.as<int>() + 2 * sb.n_rings, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = total;
    if (xyzi_out && total > 0) {
        MLH_HIP(ctx, hipMemcpyAsync(xyzi_out, sb.vox_out.p, sizeof(float4) * size_t(total), hipMemcpyDeviceToHost, ctx->stream));
        MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    prof_collect(ctx);
    return device_error_check(ctx);
}

// Estimator::undistortMeasurements (estimator.cpp:376-410) for the scan the context holds: its points (laser_cloud, and with them the
// less-sharp corners the lists index) and its thinned less-flat cloud move to the end of the sweep, in place, on the device
int mlh_scan_undistort(mlh_ctx *ctx, const double pose_undist[7], float scan_period)
{
    if (!ctx || !pose_undist || !(scan_period > 0.f)) return MLH_ERR_INVALID;
    ScanBuf &sb = ctx->scan;
    if (!sb.extracted) return fail(ctx, MLH_ERR_STATE, "extract_run has not been called");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    { const int wrc = ctx->handoff.wait_readers(ctx); if (wrc) return wrc; }
    int rc = transform_to_end_launch(ctx, sb.pts.p, 16, sb.n, 12, pose_undist, 1, scan_period);
    if (rc || !sb.voxelised) return rc;
    if ((rc = scan_totals(ctx, true))) return rc;      // the thinned cloud's count (fetched once per scan, shared with the hand-overs)
    return transform_to_end_launch(ctx, sb.vox_out.p, 16, sb.h_totals[4], 12, pose_undist, 1, scan_period);
}

}  // extern "C"
