// Front-end kernels around the extractor (gfx950): per-point rigid transforms and gathers that keep the clouds on the device between
// extractCloud, the tracker and the mapper.
//   fuse_append_kernel        transformCloudFeature (estimator/src/utility/visualization.cpp:39-51) + concatenation
//   transform_cloud_kernel    pcl::transformPointCloud with a float 4x4 (estimator.cpp:1185-1192)
//   transform_to_end_kernel   TransformToEnd / TransformToStart (estimator/src/utility/utility.h:55-100; estimator.cpp:376-410)
//   gather_points_kernel      a feature list of the extractor as a dense cloud (estimator.cpp:426-427, 532-543)
//   pack_points_kernel        a caller's records as float4 points (every staging path)
//   fused_publish_kernel      the fused clouds' counts and bounding boxes into pinned host memory
// and the entry points that own nothing but these launches: mlh_transform_*, mlh_fuse_*, mlh_fused_cloud (mlh_ctx::fused is this unit's), mlh_debug_bad_launch.
#include "ctx.hpp"
#include "dev_math.hpp"
#include "wg_dev.hpp"
#include <cfloat>

namespace mlh {

__global__ __launch_bounds__(256) void gather_points_kernel(const float4 *__restrict__ pts, const int *__restrict__ list, int n, float4 *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = pts[list[i]];
}

void gather_points_launch(mlh_ctx *ctx, const float4 *pts, const int *list, int n, float4 *out)
{
    MLH_LAUNCH(gather_points_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, pts, list, n, out);
}

// pcl::transformPointCloud(cloud, cloud, pose.T_.cast<float>()) in place: p' = R p + t in single precision (R rounded once from the
// double rotation matrix of the unit quaternion), every other field kept -- the window clouds on their way into the pivot frame
// (estimator.cpp:1185-1192)
__global__ __launch_bounds__(256) void transform_cloud_kernel(unsigned char *p, int stride, int n, FuseXf xf)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float *r = reinterpret_cast<float *>(p + size_t(i) * stride);
    const float x = r[0], y = r[1], z = r[2];
    r[0] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[0], x), __fmul_rn(xf.r[1], y)), __fmul_rn(xf.r[2], z)), xf.t[0]);
    r[1] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[3], x), __fmul_rn(xf.r[4], y)), __fmul_rn(xf.r[5], z)), xf.t[1]);
    r[2] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[6], x), __fmul_rn(xf.r[7], y)), __fmul_rn(xf.r[8], z)), xf.t[2]);
}

int transform_cloud_launch(mlh_ctx *ctx, void *dev, int stride, int n, const double pose[7])
{
    if (n <= 0) return MLH_OK;
    MLH_LAUNCH(transform_cloud_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, static_cast<unsigned char *>(dev), stride, n, xf_from_pose(pose, 0.f));
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// TransformToEnd (utility.h:79-100) in place over strided records: p^b = T^-1 T(s) p^c with s = frac(intensity) / scan_period when
// b_distortion, else 1; T(s) = (slerp(s, q), s t) (Eigen 3.3 slerp from the identity), f64 math, the intermediate and the result
// rounded to f32 exactly where the reference stores them into float points
struct UndistArgs { unsigned char *p; int stride, n, intensity_off, b_distortion; float scan_period; double pose[7]; };
__global__ __launch_bounds__(256) void transform_to_end_kernel(UndistArgs A)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    float *rec = reinterpret_cast<float *>(A.p + size_t(i) * A.stride);
    const float inten = *reinterpret_cast<const float *>(A.p + size_t(i) * A.stride + A.intensity_off);
    double sI = 1.0;
    if (A.b_distortion) sI = double((inten - float(int(inten))) / A.scan_period);
    const q4 q{A.pose[3], A.pose[4], A.pose[5], A.pose[6]};
    const d3 t{A.pose[0], A.pose[1], A.pose[2]};
    // Identity.slerp(s, q)
    const double one = 1.0 - 2.220446049250313e-16;
    const double d = q.w, absD = fabs(d);
    double scale0, scale1;
    if (absD >= one) { scale0 = 1.0 - sI; scale1 = sI; }
    else {
        const double theta = acos(absD), sinTheta = sin(theta);
        scale0 = sin((1.0 - sI) * theta) / sinTheta;
        scale1 = sin(sI * theta) / sinTheta;
    }
    if (d < 0.0) scale1 = -scale1;
    const q4 qs{scale0 * 0.0 + scale1 * q.x, scale0 * 0.0 + scale1 * q.y, scale0 * 0.0 + scale1 * q.z, scale0 * 1.0 + scale1 * q.w};
    const d3 r = qrot(qs, d3{double(rec[0]), double(rec[1]), double(rec[2])});
    const float ux = float(r.x + sI * t.x), uy = float(r.y + sI * t.y), uz = float(r.z + sI * t.z);     // un_point_tmp (a float point)
    const double n2 = (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w);
    const q4 qi{-q.x / n2, -q.y / n2, -q.z / n2, q.w / n2};
    const d3 e = qrot(qi, d3{double(ux) - t.x, double(uy) - t.y, double(uz) - t.z});
    rec[0] = float(e.x); rec[1] = float(e.y); rec[2] = float(e.z);
}

int transform_to_end_launch(mlh_ctx *ctx, void *dev, int stride, int n, int intensity_off, const double pose[7], int b_distortion, float scan_period)
{
    if (n <= 0) return MLH_OK;
    UndistArgs A;
    A.p = static_cast<unsigned char *>(dev); A.stride = stride; A.n = n; A.intensity_off = intensity_off; A.b_distortion = b_distortion;
    A.scan_period = scan_period;
    for (int i = 0; i < 7; ++i) A.pose[i] = pose[i];
    MLH_LAUNCH(transform_to_end_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, A);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// transformCloudFeature (visualization.cpp:39-51): p' = R p + t in single precision, intensity <- LiDAR index
struct FuseArgs {
    const float4 *pts, *vox_out;
    const int *list1, *ring_offsets, *vox_off;
    int rb, re;                // rings [rb, re) of the scan
    FuseXf xf;
    float4 *out[2];            // fused surf / corner clouds
    const int *cnt;            // record counts before this append (not read by the first append after a reset: `first`) ...
    int first;
    int *cnt_next;             // ... and after it (the next append's base): a prefix table, one pair per append
    float *part;               // this append's partial bounds: [kind][FUSE_BLOCKS][6]
};
__global__ __launch_bounds__(256) void fuse_append_kernel(FuseArgs A)
{
    __shared__ float lds[4][6];
    const int kind = blockIdx.y;                       // 0: surf <- voxel-thinned less-flat, 1: corner <- less-sharp
    const int b = kind == 0 ? A.vox_off[A.rb] : A.ring_offsets[A.rb * 4 + 1];
    const int e = kind == 0 ? A.vox_off[A.re] : A.ring_offsets[A.re * 4 + 1];
    const int base = A.first ? 0 : A.cnt[kind];
    if (blockIdx.x == 0 && threadIdx.x == 0) A.cnt_next[kind] = base + (e - b);      // depends on nothing the other workgroups do: no bump launch
    const FuseXf &xf = A.xf;
    float m[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e - b; i += FUSE_BLOCKS * 256) {
        const float4 p = kind == 0 ? A.vox_out[b + i] : A.pts[A.list1[b + i]];
        float4 o;
        // products and sums kept separate (no contraction) so that the result is one well-defined float32 expression
        o.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[0], p.x), __fmul_rn(xf.r[1], p.y)), __fmul_rn(xf.r[2], p.z)), xf.t[0]);
        o.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[3], p.x), __fmul_rn(xf.r[4], p.y)), __fmul_rn(xf.r[5], p.z)), xf.t[1]);
        o.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf.r[6], p.x), __fmul_rn(xf.r[7], p.y)), __fmul_rn(xf.r[8], p.z)), xf.t[2]);
        o.w = xf.id;
        A.out[kind][base + i] = o;
        m[0] = fminf(m[0], o.x); m[1] = fminf(m[1], o.y); m[2] = fminf(m[2], o.z);
        m[3] = fmaxf(m[3], o.x); m[4] = fmaxf(m[4], o.y); m[5] = fmaxf(m[5], o.z);
    }
    float r;
    if (block_fold_bounds<1>(m, lds, r)) A.part[(kind * FUSE_BLOCKS + blockIdx.x) * 6 + threadIdx.x] = r;
}
// the scan's thinned less-flat cloud -> fused SURF, its less-sharp corners -> fused CORNER (rings [ring_begin, ring_end)); counts on the device
int fuse_append_launch(mlh_ctx *ctx, ScanBuf &sb, int ring_begin, int ring_end, int lidar_idx, const double ext_pose[7])
{
    hipStream_t st = ctx->stream;
    FuseArgs A;
    A.xf = xf_from_pose(ext_pose, float(lidar_idx));
    // the counts live on the device (no host round trip per scan); capacity follows a host-side upper bound: the scan's point count
    for (int k = 0; k < 2; ++k) {
        MLH_HIP(ctx, ctx->fused.pts[k].grow(sizeof(float4) * (ctx->fused.bound[k] + size_t(sb.n)), sizeof(float4) * ctx->fused.bound[k], st));
        ctx->fused.bound[k] += size_t(sb.n);
        A.out[k] = ctx->fused.pts[k].as<float4>();
    }
    A.pts = sb.pts.as<float4>(); A.vox_out = sb.vox_out.as<float4>(); A.list1 = sb.lists[1].as<int>();
    A.ring_offsets = sb.ring_offsets.as<int>(); A.vox_off = sb.ring_vox.as<int>() + sb.n_rings;
    // counts: prefix table [append][kind]; this append reads row `parts` and writes row `parts + 1`
    MLH_HIP(ctx, ctx->fused.cnt.grow(sizeof(int) * 2 * size_t(ctx->fused.parts + 2), sizeof(int) * 2 * size_t(ctx->fused.parts + 1), st));
    A.first = ctx->fused.parts == 0 ? 1 : 0;
    A.rb = ring_begin; A.re = ring_end; A.cnt = ctx->fused.cnt.as<int>() + 2 * ctx->fused.parts; A.cnt_next = ctx->fused.cnt.as<int>() + 2 * (ctx->fused.parts + 1);
    const size_t part_floats = size_t(2) * FUSE_BLOCKS * 6;
    MLH_HIP(ctx, ctx->fused.part.grow(sizeof(float) * part_floats * size_t(ctx->fused.parts + 1), sizeof(float) * part_floats * size_t(ctx->fused.parts), st));
    A.part = ctx->fused.part.as<float>() + part_floats * size_t(ctx->fused.parts);
    ++ctx->fused.parts;
    MLH_LAUNCH(fuse_append_kernel, dim3(FUSE_BLOCKS, 2), dim3(256), 0, st, A);
    MLH_HIP(ctx, hipGetLastError());
    return MLH_OK;
}

// AoS records (stride bytes) -> float4 {x,y,z,w}; w = f32 at w_off, or what PACK_W_* says (ctx.hpp)
__global__ __launch_bounds__(256) void pack_points_kernel(const unsigned char *__restrict__ src, int stride, int n, int w_off, float w_value,
                                                          int cov_off, float4 *__restrict__ out, float4 *__restrict__ covd)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *rec = reinterpret_cast<const float *>(src + size_t(i) * stride);
    float4 p;
    p.x = rec[0]; p.y = rec[1]; p.z = rec[2];
    if (w_off == PACK_W_INDEX) p.w = __int_as_float(i);
    else if (w_off == PACK_W_VALUE) p.w = w_value;
    else if (w_off >= 0) p.w = *reinterpret_cast<const float *>(src + size_t(i) * stride + w_off);
    else p.w = 0.f;
    out[i] = p;
    if (covd) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cov_off >= 0) {
            const float *cv = reinterpret_cast<const float *>(src + size_t(i) * stride + cov_off);
            c.x = cv[0]; c.y = cv[3]; c.z = cv[5];
        }
        covd[i] = c;
    }
}

void pack_points_launch(hipStream_t st, const unsigned char *dev, int stride, int n, int w_off, float w_value, int cov_off, float4 *out, float4 *covd)
{
    MLH_LAUNCH(pack_points_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dev, stride, n, w_off, w_value, cov_off, out, covd);
}

}  // namespace mlh

using namespace mlh;

extern "C" {

// the way out of the two in-place transforms: a host cloud goes home from `dev` and is waited for; a failed launch drains the stream first
static int transform_finish(mlh_ctx *ctx, int rc, const Records &r, void *points, const unsigned char *dev)
{
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    if (r.mem == MLH_MEM_HOST) {
        MLH_HIP(ctx, hipMemcpyAsync(points, dev, r.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        MLH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MLH_OK;
}

int mlh_transform_point_cloud(mlh_ctx *ctx, void *points, int stride_bytes, int n, const double pose[7], int mem)
{
    if (!ctx || !points || !pose) return MLH_ERR_INVALID;
    const Records r = records_of(points, stride_bytes, n, mem);
    { const int rc = records_check(ctx, "mlh_transform_point_cloud", r, true); if (rc) return rc; }
    if (n == 0) return MLH_OK;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned char *dev;
    { const int rc = records_stage(ctx, r, ctx->tmp, ctx->stream, &dev); if (rc) return rc; }
    return transform_finish(ctx, transform_cloud_launch(ctx, const_cast<unsigned char *>(dev), stride_bytes, n, pose), r, points, dev);
}

int mlh_transform_to_end(mlh_ctx *ctx, void *points, int stride_bytes, int n, int intensity_offset_bytes, const double pose[7], int b_distortion,
                         float scan_period, int mem)
{
    if (!ctx || !points || !pose || intensity_offset_bytes < 12 || !(scan_period > 0.f)) return MLH_ERR_INVALID;
    const Records r = records_of(points, stride_bytes, n, mem, intensity_offset_bytes);
    { const int rc = records_check(ctx, "mlh_transform_to_end", r, true); if (rc) return rc; }
    if (n == 0) return MLH_OK;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned char *dev;
    { const int rc = records_stage(ctx, r, ctx->tmp, ctx->stream, &dev); if (rc) return rc; }
    const int rc = transform_to_end_launch(ctx, const_cast<unsigned char *>(dev), stride_bytes, n, intensity_offset_bytes, pose, b_distortion, scan_period);
    return mem == MLH_MEM_DEVICE ? rc : transform_finish(ctx, rc, r, points, dev);      // (a device cloud: nothing to wait for either way)
}

int mlh_fuse_reset(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    FusedClouds &F = ctx->fused;
    MLH_HIP(ctx, F.cnt.ensure(sizeof(int) * 2 * 8));                               // prefix table of the record counts, one pair per append (grows);
                                                                                   // its first row is never read: the first append starts from zero by argument
    F.bound[0] = F.bound[1] = 0;
    F.parts = 0;
    F.publish_empty();
    return MLH_OK;
}

int mlh_fuse_add_rings(mlh_ctx *ctx, int ring_begin, int ring_end, int lidar_idx, const double ext_pose[7])
{
    if (!ctx || !ext_pose || lidar_idx < 0) return MLH_ERR_INVALID;
    ScanBuf &sb = ctx->scan;
    if (!sb.extracted || !sb.voxelised) return fail(ctx, MLH_ERR_STATE, "mlh_extract_run and mlh_extract_voxel_run come first");
    if (ring_begin < 0 || ring_end > sb.n_rings || ring_begin >= ring_end) return fail(ctx, MLH_ERR_INVALID, "bad ring range");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->fused.cnt.p) { int rc = mlh_fuse_reset(ctx); if (rc) return rc; }
    { int rc = fuse_append_launch(ctx, sb, ring_begin, ring_end, lidar_idx, ext_pose); if (rc) return rc; }
    ctx->fused.mark_dirty();
    return MLH_OK;
}

int mlh_fuse_add_scan(mlh_ctx *ctx, int lidar_idx, const double ext_pose[7])
{
    if (!ctx) return MLH_ERR_INVALID;
    return mlh_fuse_add_rings(ctx, 0, ctx->scan.n_rings, lidar_idx, ext_pose);
}

// mlh_fuse_add_scan with the scan ANOTHER context of the same device holds: every LiDAR's segmentCloud -> extractCloud on a context (a thread) of its own -- the
// host-side cluster searches side by side -- and one context gathers their features for the mapper without a host hop. Ordered on the device: ctx's stream waits for
// src's work so far (an event of ctx's on src's stream), and whatever rewrites src's scan next waits for this append (an event of src's on ctx's stream).
int mlh_fuse_add_scan_from(mlh_ctx *ctx, mlh_ctx *src, int lidar_idx, const double ext_pose[7])
{
    if (!ctx || !src || !ext_pose || lidar_idx < 0) return MLH_ERR_INVALID;
    if (src == ctx) return mlh_fuse_add_scan(ctx, lidar_idx, ext_pose);
    if (ctx->device != src->device) return fail(ctx, MLH_ERR_UNSUPPORTED, "mlh_fuse_add_scan_from: both contexts must be on the same device");
    ScanBuf &sb = src->scan;
    if (!sb.extracted || !sb.voxelised) return fail(ctx, MLH_ERR_STATE, "mlh_fuse_add_scan_from: mlh_extract_run and mlh_extract_voxel_run on the source context come first");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->fused.cnt.p) { int rc = mlh_fuse_reset(ctx); if (rc) return rc; }
    { int rc = ctx->handoff.borrow_begin(ctx, src); if (rc) return rc; }
    { int rc = fuse_append_launch(ctx, sb, 0, sb.n_rings, lidar_idx, ext_pose); if (rc) return rc; }
    ctx->fused.mark_dirty();
    return ctx->handoff.borrow_end(ctx, src);
}

// The two record counts and the two bounding boxes of the fused clouds, reduced over the appends' per-workgroup partial boxes and written straight into pinned
// host memory by one launch (sequence word last, system-scope release): what used to be two copies and a marker launch behind them.
__global__ __launch_bounds__(256) void fused_publish_kernel(const int *__restrict__ cnt2, const float *__restrict__ part, int n_boxes_per_kind_and_part, int parts,
                                                            int *h_cnt, float *h_box, unsigned long long *h_seq, unsigned long long seq)
{
    __shared__ float s_red[4][12];
    const int t = threadIdx.x;
    float v[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) v[c] = (c % 6) < 3 ? FLT_MAX : -FLT_MAX;
    for (int i = t; i < parts * n_boxes_per_kind_and_part; i += 256) {          // one partial box of each kind per step: [append][kind][workgroup][6]
        const int a = i / n_boxes_per_kind_and_part, b = i - a * n_boxes_per_kind_and_part;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float *q = part + (size_t(a) * 2 * n_boxes_per_kind_and_part + size_t(k) * n_boxes_per_kind_and_part + b) * 6;
#pragma unroll
            for (int d = 0; d < 6; ++d) v[k * 6 + d] = d < 3 ? fminf(v[k * 6 + d], q[d]) : fmaxf(v[k * 6 + d], q[d]);
        }
    }
    float r;
    if (block_fold_bounds<2>(v, s_red, r)) h_box[t] = r;
    if (t == 0) { h_cnt[0] = cnt2[0]; h_cnt[1] = cnt2[1]; }
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int mlh_fused_cloud(mlh_ctx *ctx, int kind, const void **device_points, int32_t *n)
{
    if (!ctx || kind < 0 || kind > 1 || !device_points || !n) return MLH_ERR_INVALID;
    FusedClouds &F = ctx->fused;
    if (F.dirty) {
        MLH_HIP(ctx, hipSetDevice(ctx->device));
        if (F.parts == 0) F.publish_empty();                        // nothing appended since the reset
        else {
            MLH_HIP(ctx, F.host.ensure(sizeof(FusedPublish), 0, true));
            FusedPublish *pub = F.host.as<FusedPublish>();
            int *h_cnt = pub->count;
            float *h_box = pub->box;
            unsigned long long *h_seq = &pub->seq;
            const unsigned long long seq = ++F.seq;
            MLH_LAUNCH(fused_publish_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int *)(F.cnt.as<int>() + 2 * F.parts),
                               (const float *)F.part.as<float>(), FUSE_BLOCKS, F.parts, h_cnt, h_box, h_seq, seq);
            MLH_HIP(ctx, hipGetLastError());
            { const int rc = host_wait_seq(ctx, h_seq, seq, ctx->stream, "the fused clouds' sizes did not arrive"); if (rc) return rc; }
            F.take_published();
        }
    }
    *device_points = F.pts[kind].p;
    *n = F.n[kind];
    return MLH_OK;
}

__global__ void debug_noop_kernel(int *p) { if (p && threadIdx.x == 4096) *p = 0; }
// Debug: a launch with an impossible configuration (4096 threads per workgroup). Under MLH_CHECK_LAUNCH=1 the call returns MLH_ERR_HIP and mlh_last_error names
// debug_noop_kernel; without it the call returns MLH_OK and the runtime's sticky error is left for whoever asks next (what every launch of the library used to do).
int mlh_debug_bad_launch(mlh_ctx *ctx)
{
    if (!ctx) return MLH_ERR_INVALID;
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    MLH_LAUNCH(debug_noop_kernel, dim3(1), dim3(4096), 0, ctx->stream, (int *)nullptr);
    MLH_HIP(ctx, hipSuccess);                 // (the check every entry point runs behind its launches)
    if (!launch_check_enabled()) (void)hipGetLastError();      // do not leave the provoked error behind in a run that does not check launches
    return MLH_OK;
}

}  // extern "C"
