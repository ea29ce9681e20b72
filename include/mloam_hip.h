/*
 * mloam_hip.h -- C-ABI of the MI355X-native (gfx950) scan-to-map hot path of M-LOAM.
 *
 * One shared library (libmloam_hip.so, hand-written HIP kernels) behind plain C entry points: opaque context,
 * plain pointers and sizes, int status (0 = ok, negative = error; text via mlh_last_error). No exceptions cross
 * the boundary. A context owns one HIP stream and all device buffers; distinct contexts may be used from
 * different threads concurrently (FeatureExtract::extractCloud is called from NUM_OF_LASER OpenMP threads,
 * estimator/src/estimator/estimator.cpp:249-263 -> one context per thread), a single context is not re-entrant.
 *
 * Every entry point names the reference interface it replaces (paths relative to the M-LOAM source tree).
 * Pose / parameter blocks are double[7] = [tx ty tz qx qy qz qw] exactly as the reference's Ceres parameter
 * blocks (estimator/src/factor/lidar_map_factor.hpp:46-47).
 *
 * Pointer arguments marked HOST are host memory, DEV are device memory on the context's device. Points are read
 * through (base, stride_bytes): x,y,z are 3 consecutive floats at the start of each record, so pcl::PointXYZI
 * (32 B), pcl::PointXYZIWithCov (48 B, mloam_pcl/include/mloam_pcl/point_with_cov.hpp:45-53) and packed float4
 * clouds can all be passed without repacking on the caller side.
 */
#ifndef MLOAM_HIP_H
#define MLOAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mlh_ctx mlh_ctx;

enum { MLH_SURF = 0, MLH_CORNER = 1 };              /* feature / map kind ('s' / 'c' in PointPlaneFeature::type_) */
#define MLH_ALL_KINDS (-1)                          /* mlh_map_rebuild: both maps in one set of launches */
enum { MLH_MEM_HOST = 0, MLH_MEM_DEVICE = 1 };

/* status codes */
enum {
    MLH_OK = 0,
    MLH_ERR_INVALID = -1,     /* bad argument */
    MLH_ERR_HIP = -2,         /* a HIP runtime call failed */
    MLH_ERR_STATE = -3,       /* call order violated (e.g. match before map_set) */
    MLH_ERR_NOMEM = -4,
    MLH_ERR_UNSUPPORTED = -5,
    MLH_ERR_INCOMPLETE = -6   /* mlh_scan2map_end with status_out == NULL on a frame whose pose_out is NOT a result (status 1 / 3 below) */
};

/* flags for mlh_match_linearize / solver options */
enum {
    MLH_FLAG_CHECK_FOV = 1u << 0,   /* CHECK_FOV argument of match*FromMap (feature_extract.hpp:696-715) */
    MLH_FLAG_WITH_UA = 1u << 1,     /* with_ua_flag: weight from the feature's own covariance (lidar_mapper_keyframe.cpp:541-544) */
    MLH_FLAG_NO_LOSS = 1u << 2,     /* reduce un-corrected rows (ActiveFeatureSelection's H, lidar_mapper.h:162-164) */
    MLH_FLAG_POSE_COV = 1u << 3     /* mlh_scan2map, mlh_scan2map_begin*, mlh_downsample_scan2map: the solve also delivers evalHessian at the pose it returns and its
                                     * inverse (lidar_mapper_keyframe.cpp:600-606), read with mlh_scan2map_cov. Ignored by mlh_gn_solve*, mlh_match_linearize and
                                     * every other call that takes solver options: they run no Levenberg-Marquardt loop whose state holds that matrix */
};

/* ---------------------------------------------------------------- context */
int mlh_create(mlh_ctx **out, int device_id);
void mlh_destroy(mlh_ctx *ctx);
const char *mlh_last_error(const mlh_ctx *ctx);
const char *mlh_version(void);
/* the context's HIP stream (hipStream_t), for callers that interleave their own device work */
void *mlh_stream(mlh_ctx *ctx);
int mlh_synchronize(mlh_ctx *ctx);
/* What mlh_create found on the device, and what the in-kernel Levenberg-Marquardt loops (the one-launch forms of scan2MapOptimization's ceres::Solve,
 * lidar_mapper_keyframe.cpp:586-596, and of trackCloud's, lidar_tracker.cpp:106-113) did with it. Those launches synchronise their workgroups among themselves and
 * therefore need all of them resident at once: loop_max_tiles is the number of 256-feature tiles the context will put behind one such barrier --
 * min(hipOccupancyMaxActiveBlocksPerMultiprocessor, 6) x the compute units the solver's stream may use, less a margin of an eighth of those compute units (at
 * least 8; kernels of other streams and contexts are transient and only delay an arrival), never more than the 160 tiles beyond which every workgroup re-summing every record stops
 * paying (the fused thinning + solve call: 512). A frame with more tiles, a partitioned or smaller device, a CU-masked solver
 * stream (environment at mlh_create: MLH_SOLVER_CU_MASK=<hex word>[,<hex word>...], 32 compute units per word) take the launch-per-iteration forms: the same
 * arithmetic, the same pose bits, no residency requirement. Should a barrier nevertheless not complete within MLH_LOOP_TIMEOUT_US (default 20 000), the frame is
 * solved again through those forms (loop_fallbacks; the caller gets the same pose, later) and loop_max_tiles is halved for the context. MLH_LOOP_MAX_TILES=<n>
 * lowers the limits by hand (0: never use the one-launch loops). */
typedef struct mlh_device_info {
    int32_t cu_count;                /* compute units of the device */
    int32_t cu_solver;               /* ... the solver's stream may use */
    int32_t loop_blocks_per_cu[3];   /* occupancy query: scan2map's loop kernel, its device-counted variant (mlh_downsample_scan2map), the tracker's */
    int32_t loop_max_tiles[3];       /* the gates in force now, same order */
    int32_t scan_uploads_from_ahead; /* mlh_scan_upload calls that packed from what mlh_scan_upload_ahead had sent (wraps) */
    uint64_t loop_launches;          /* frames / tracker calls that went through the one-launch loops */
    uint64_t loop_timeouts;          /* ... whose barrier was given up on */
    uint64_t loop_fallbacks;         /* ... and that were solved again by the launch-per-iteration form inside the same call */
} mlh_device_info;
int mlh_get_info(mlh_ctx *ctx, mlh_device_info *out);

/* ---------------------------------------------------------------- per-kernel timing (HIP events on the context's stream)
 * Single-kernel ids (KNN, FIT, LINEARIZE) are timed with the dispatch's own start/stop timestamps (hipExtLaunchKernelGGL with
 * start/stop events: the same clock rocprofv3 reports); multi-kernel ids (SOLVE, GRID_BUILD, EXTRACT) are bracketed with
 * hipEventRecord on the context's stream. Durations / launch counts are read back with mlh_profile_get. Kernel ids: */
enum {
    MLH_K_KNN = 0,           /* correspondence kernel (exact 5-NN, surf + corner features in one launch) -- the roofline kernel */
    MLH_K_FIT = 1,           /* fit + gates + residual/Jacobian + J^T J reduction (+ fused GN solve in its last workgroup)     */
    MLH_K_LINEARIZE = 2,     /* re-linearisation on stored correspondences (LM iterations)                                     */
    MLH_K_SOLVE = 3,         /* stand-alone partial-sum reduction + degeneracy + 6x6 solve / LM step kernels                   */
    MLH_K_GRID_BUILD = 4,    /* local-map index build (all kernels of one build)                                               */
    MLH_K_EXTRACT = 5,       /* extractCloud (all kernels of one extraction)                                                   */
    MLH_K_ALLREDUCE = 6,     /* the RCCL all-reduce of the packed normal equations (N > 1)                                     */
    MLH_K_KNN_PRE = 7,       /* the correspondence kernel of iterations >= 1 of a deferred-finish Gauss-Newton solve: the same search (bounded by the previous
                                iteration's neighbours) behind the prologue that completes the previous iteration (sum of the tiles' records, 6x6 solve, Plus)          */
    MLH_K_KNN_FIRST = 8,     /* the correspondence kernel of iteration 0 of a CHAINED solve that completes its predecessor first (final_in_successor): the predecessor's last
                                iteration summed, solved and published, this frame's start pose chained from it, then the cold search                                        */
    MLH_K_COUNT = 9
};
/* kernel_mask: bit k enables the brackets of kernel id k (0 = profiling off, -1 = all) */
int mlh_profile_enable(mlh_ctx *ctx, int kernel_mask);
/* bracket only every n-th launch of a single-kernel id (an event pair costs host + queue time of its own); default 1 */
int mlh_profile_sample(mlh_ctx *ctx, int every_n);
int mlh_profile_reset(mlh_ctx *ctx);
int mlh_profile_get(mlh_ctx *ctx, int kernel_id, double *total_ms, long long *launches);

/* ---------------------------------------------------------------- (f3) ImageSegmenter::segmentCloud
 * replaces ImageSegmenter::segmentCloud(laser_cloud_in, laser_cloud_out, laser_cloud_outlier, scan_info)
 *   estimator/src/imageSegmenter/image_segmenter.hpp:139-393 (projectCloud :88-136, setParameter image_segmenter.cpp:18-63), called by
 *   Estimator::inputCloud (estimator.cpp:228, 258, 298, 317).
 * In: the raw, UNORDERED cloud of one LiDAR (HOST or DEVICE records: x y z at offset 0, f32 intensity at intensity_offset_bytes or -1).
 * Out: the ring-major cloud [x y z intensity + row] and ScanInfo::scan_start_ind_ / scan_end_ind_ (+5 / -6 insets), staged as the context's
 * scan exactly as mlh_scan_upload leaves it -- mlh_extract_run follows directly, the cloud never has to be assembled on the host -- and,
 * when the pointers are given, copied back: cloud_out (up to n x 4 floats), scan_start / scan_end (vertical_scans each), outlier_out
 * (laser_cloud_outlier: rows of 4 floats; the caller states the rows it has room for in outlier_capacity, writes are clamped to it and
 * *n_outlier always reports the rows the cloud HAS, so a short buffer is detected, not overrun. An upper bound that never truncates:
 * min(n, vertical_scans * ((horizon_scans + 4) / 5)) + 1 -- one row per infeasible-cluster pixel in a column that is a multiple of 5,
 * image_segmenter.hpp:366-378, plus the first output point, hpp:391). Projection, ground pairs and the final gather run on the GPU; the cluster search and
 * the outlier erasure are defined by their sequential order and run on the host inside this call (m-loam_amd/csrc/segment.hip says why).
 * The reference's undefined spots -- alpha used before it is set, erase with shifted positions, the 64-ring ground loop's row 64 -- behave as
 * INTEGRATION.md documents. vertical_scans 16, 32 or 64. */
typedef struct mlh_segment_params {
    int32_t vertical_scans;            /* N_SCANS */
    int32_t horizon_scans;             /* HORIZON_SCAN (horizon_scan) */
    int32_t min_cluster_size;          /* MIN_CLUSTER_SIZE */
    int32_t segment_valid_point_num;   /* SEGMENT_VALID_POINT_NUM */
    int32_t segment_valid_line_num;    /* SEGMENT_VALID_LINE_NUM */
    float segment_theta;               /* SEGMENT_THETA */
    double roi_range;                  /* ROI_RANGE */
    int32_t segment_flag;              /* ScanInfo::segment_flag_ (segment_cloud): 0 = project and reorder only, nothing is erased */
} mlh_segment_params;
void mlh_segment_params_default(mlh_segment_params *p);     /* config_realvehicle_hercules.yaml:7-13, 102 */
int mlh_segment_cloud(mlh_ctx *ctx, const void *points, int stride_bytes, int intensity_offset_bytes, int n, int mem, const mlh_segment_params *prm,
                      float *cloud_out, int32_t *n_out, int32_t *scan_start, int32_t *scan_end, float *outlier_out, int32_t outlier_capacity, int32_t *n_outlier);

/* ---------------------------------------------------------------- (a1-a3) FeatureExtract::extractCloud
 * replaces FeatureExtract::extractCloud(const PointICloud&, const ScanInfo&, cloudFeature&)
 *   estimator/src/featureExtract/feature_extract.cpp:118-297, declared feature_extract.hpp:74.
 * The cloud is ring-major; scan_start[r]/scan_end[r] are ScanInfo::scan_start_ind_/scan_end_ind_
 * (already inset by +5/-6, image_segmenter.hpp:385-387).
 *
 * mlh_scan_upload   stages one cloud (+ring table) in HBM             [HOST or DEV source]; intensity_offset_bytes (-1: none) is the
 *                   byte offset of the f32 intensity field the per-ring VoxelGrid averages with the coordinates (the tracker reads
 *                   the ring id from it, image_segmenter.hpp:128)
 * mlh_extract_run   curvature (cpp:133-142), per-sector sort + greedy labelling (cpp:152-265), index lists
 * mlh_extract_fetch copies results back: label[n] in {2,1,0,-1} (cloud_label), curvature[n], and the four index
 *                   lists in the reference's emission order: 0 corner_points_sharp, 1 corner_points_less_sharp,
 *                   2 surf_points_flat, 3 surf_points_less_flat BEFORE the per-ring VoxelGrid (positions with
 *                   label<=0, cpp:258-264). Any output pointer may be NULL.
 */
int mlh_scan_upload(mlh_ctx *ctx, const void *points, int stride_bytes, int intensity_offset_bytes, int n, const int *scan_start,
                    const int *scan_end, int n_rings, int mem);
/* mlh_scan_upload_ahead: the points of the scan a LATER mlh_scan_upload(.., MLH_MEM_HOST) will stage, sent to the device NOW on a copy stream of the context's own,
 * while the context's stream still works on the current scan (extraction, thinning, a solve): the copy engine beside the kernels, the upload off the frame's chain
 * (a replayed bag, a driver with the next sweep already in memory; with a live sensor there is nothing to send ahead). The mlh_scan_upload that names the SAME
 * points / stride_bytes / n packs from what arrived instead of copying; any other host upload in between drops it; a second call replaces the first (one scan
 * ahead). `points` must stay valid and unchanged until that mlh_scan_upload has returned. No reference counterpart: the reference's clouds never leave the host
 * (estimator.cpp:248-263 hands pcl clouds to extractCloud). */
int mlh_scan_upload_ahead(mlh_ctx *ctx, const void *points, int stride_bytes, int n);
int mlh_extract_run(mlh_ctx *ctx);
/* The order of EQUAL curvatures inside a sector. The reference sorts a sector's point indices with std::sort and compObject, which compares
 * cloudCurvature only (feature_extract.cpp:152-162), so among equal values the greedy walks meet the points in whatever order libstdc++'s
 * introsort leaves them.
 *   1 (default)  that order: a sector whose sorted curvatures show two equal values (or a NaN) is re-ordered ON THE DEVICE by the library's
 *                algorithm on the same initial arrangement (m-loam_amd/csrc/stdsort_dev.hpp: the same comparison sequence, hence the same
 *                permutation); sectors with distinct curvatures -- every sector of ordinary float data -- have one sorted order and pay nothing;
 *   0            (curvature, index) ascending, NaN curvatures last by index: a total order that does not depend on a standard library. */
int mlh_set_extract_tie_order(mlh_ctx *ctx, int mode);
int mlh_extract_fetch(mlh_ctx *ctx, int32_t *label, float *curvature, int32_t *picked, int32_t *idx_out[4], int32_t n_out[4]);
/* (a3) the per-ring pcl::VoxelGrid(leaf = 0.2 m) extractCloud applies to the less-flat points of every ring
 * (feature_extract.cpp:266-271): run after mlh_extract_run; fetch returns "surf_points_less_flat" as the reference emits it
 * (ring asc, voxel index asc; x y z intensity centroids). PCL sums a voxel's members in the order an unstable std::sort (comparator on
 * the voxel index only) left them; with the context's default member order (mlh_set_voxel_member_order, below) the sums run along that same
 * permutation -- one device std::sort per ring -- and the centroids are the reference's bit for bit; with mode 0 the members are summed in
 * scan order (equal up to f32 rounding of the sum, ~0.1 ms per scan pair cheaper). */
int mlh_extract_voxel_run(mlh_ctx *ctx, float leaf);
int mlh_extract_fetch_voxel(mlh_ctx *ctx, float *xyzi_out, int32_t *n_out);

/* (a18) per-point uncertainty of downsampleCurrentScan (lidar_mapper_keyframe.cpp:375-418): for every point (intensity =
 * LiDAR index n) Sigma_p = evalPointUncertainty(pose_ext[n]^-1 * p, pose_ext[n])  (associate_uct.hpp:196-215) with
 * cov_input = diag(ext_covs[n] (6x6), cov_measurement (3x3)). Outputs the f32 cov_vec[6] of PointXYZIWithCov per point and
 * keep[i] = 0 where trace > trace_threshold (TRACE_THRESHOLD_MAPPING; <= 0 keeps everything); the caller appends the kept
 * points in order, as the reference's loop does. */
int mlh_point_uncertainty(mlh_ctx *ctx, const void *points, int stride_bytes, int n, int intensity_offset_bytes, int mem,
                          const double *ext_poses, const double *ext_covs, int n_lidar, const double cov_measurement[9],
                          double trace_threshold, float *cov_vec_out, int32_t *keep_out);

/* The staged feature set of `kind` (mlh_features_set / mlh_downsample_current_scan) copied from context `src` to context `dst` on the same GPU, device to
 * device. The reference runs extraction / odometry and mapping as separate nodes joined by ROS messages (estimator.cpp publishes the feature clouds, lidar_mapper_
 * keyframe.cpp:162-190 queues them); two contexts driven by two host threads are the same arrangement on one GPU -- the estimator-side context extracts and thins
 * frame k + 1 while the mapper-side context solves frame k -- and this call is the message. Meant to be called from the thread that drives dst; of src it only needs the feature set to stay as it is until the call returns
 * (then src may restage at once). */
int mlh_features_copy(mlh_ctx *dst, mlh_ctx *src, int kind);
/* (f2) downsampleCurrentScan for one feature kind (lidar_mapper_keyframe.cpp:356-421), device-resident: VoxelGridCovarianceMLOAM<PointI>
 * at `leaf` (plain branch), then per thinned point (intensity = LiDAR index n) Sigma = evalPointUncertainty(pose_ext[n]^-1 * p,
 * pose_ext[n]) and the trace gate (with_ua only; Sigma = 0 and no gate otherwise). The kept points BECOME the kind's feature set
 * (as if handed to mlh_features_set with their covariance), so extraction output can flow into the solver without touching the
 * host; features_out (HOST, n x 11 floats [x y z i cov6 trace], may be NULL) additionally returns them. */
int mlh_downsample_current_scan(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, int intensity_offset_bytes, int mem,
                                float leaf, const double *ext_poses, const double *ext_covs, int n_lidar, const double cov_measurement[9],
                                int with_ua, double trace_threshold, float *features_out, int32_t *n_features);
/* The same for both feature kinds in one call (the mapper thins the surf and the corner cloud back to back, cpp:359-368). When both
 * clouds are the context's fused clouds (mlh_fused_cloud) they run through ONE thinning pipeline -- half the dependent launches, one
 * host round trip; other inputs take the two single calls. Records of both clouds share stride / intensity offset / memory kind;
 * afterwards both feature sets are staged exactly as two single calls leave them. A gate that keeps nothing of a kind (every trace above
 * trace_threshold) is no error of the thinning, in any form: the kind's count comes back 0 and its feature set is staged empty; the solver
 * calls then answer as they do for a kind that was never staged (MLH_ERR_STATE). */
int mlh_downsample_current_scan_pair(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                                     int intensity_offset_bytes, int mem, float leaf_surf, float leaf_corner, const double *ext_poses,
                                     const double *ext_covs, int n_lidar, const double cov_measurement[9], int with_ua, double trace_threshold,
                                     int32_t *n_surf_features, int32_t *n_corner_features);
/* The staged feature set of `kind` as the solver will read it (whatever staged it: mlh_features_set, mlh_features_copy, the thinning calls, mlh_downsample_
 * scan2map), read only: *n records of 7 floats [x y z intensity cxx cyy czz] -- the point, the LiDAR index the thinning left with it (0 from mlh_features_set,
 * which stages none), and the diagonal of its cov_vec that the factors' weight is made from (zeros for a set staged without covariance) -- copied to out (HOST,
 * room for `capacity` records; may be NULL when capacity is 0). *n is always set.
 * MLH_ERR_INVALID when capacity < *n (nothing is copied; call again with room for *n), MLH_ERR_UNSUPPORTED for a set staged in several pose blocks
 * (mlh_features_set_block: their padding slots are not this call's business). Waits for the context's stream, as the other fetches do. */
int mlh_features_fetch(mlh_ctx *ctx, int kind, float *out, int capacity, int32_t *n);
/* Which form the most recent mlh_downsample_current_scan_pair or mlh_downsample_scan2map took to thin its two clouds (every form stages the same bits; the
 * forms differ in launches and host round trips). Noted on the host where the decision is made: the calls themselves launch, copy and wait as before. */
enum {
    MLH_THIN_NONE = 0,           /* no such call yet, or the most recent one was refused before it chose */
    MLH_THIN_SORT_FIRST = 1,     /* both fused clouds through one pipeline, voxel keys made inside the std::sort launch (up to 4 LiDARs, the default member order) */
    MLH_THIN_SHARED_GRID = 2,    /* both fused clouds through one pipeline over a shared occupancy grid */
    MLH_THIN_SINGLE_CALLS = 3    /* mlh_downsample_current_scan once per kind (inputs that are not the context's fused clouds, grids too large to share) */
};
typedef struct mlh_thin_info_t {
    int32_t path;                /* MLH_THIN_* */
    int32_t n_in[2];             /* the call's input records: surf, corner */
    int32_t reserved;
} mlh_thin_info_t;
int mlh_thin_info(mlh_ctx *ctx, mlh_thin_info_t *out);

/* ---------------------------------------------------------------- (f1) covariance-aware voxel thinning
 * replaces pcl::VoxelGridCovarianceMLOAM<PointT>::filter (mloam_pcl/include/mloam_pcl/voxel_grid_covariance_mloam_impl.hpp:68-457),
 * the filter that produces the voxel-thinned local map (lidar_mapper_keyframe.cpp:343-347) and thins the scan features
 * (cpp:359-368). cov_offset_bytes >= 0 selects the covariance branch (PointXYZIWithCov, :296-333): members with |trace| >=
 * trace_threshold are dropped, w = trace_threshold - trace, mu = sum w p / sum w, cov = sum w^2 cov_i / (sum w)^2, intensity of the
 * heaviest member, trace recomputed; otherwise the plain branch (PointXYZI, :392-420): xyz mean, intensity of the last member.
 * Output (HOST, capacity n records) uses the input's record layout and is ordered by voxel index like the reference's.
 * MEMBER ORDER. The reference groups a voxel's members with std::sort and a comparator that sees the voxel index only (impl.hpp:227), i.e.
 * inside a voxel they come in whatever order libstdc++'s introsort leaves. That order decides "the last member" of the plain branch --
 * for a fused multi-LiDAR cloud the LiDAR id downsampleCurrentScan propagates the uncertainty through (lidar_mapper_keyframe.cpp:377) --,
 * the first-heaviest member of the covariance branch on equal weights, and the association of every f32 sum. Every voxel filter of the
 * context (mlh_voxel_filter, mlh_voxel_grid, mlh_downsample_current_scan, ..._pair; and extractCloud's per-ring grid, mlh_extract_voxel_run, where
 * modes 1 and 2 both mean the device path) follows mlh_set_voxel_member_order(ctx, mode):
 *   1 (default)  the reference's order, produced ON THE DEVICE: libstdc++'s std::sort (introsort: median-of-three pivot at the same
 *                positions, the same unguarded Hoare partition, the same depth budget and heap-sort fallback, the same final insertion
 *                pass) restated data-parallel -- one launch per recursion depth, a range's partition from rank tables -- so the
 *                permutation equals std::sort's element for element and the filters' results equal the reference's bit for bit;
 *   2            the same order through a host pass: the points' slots come back (pinned), the platform's OWN std::sort runs on the
 *                same sequence, the member lists go back (+1.2 ms for a frame's clouds). For a build against a standard library
 *                whose std::sort is not the algorithm mode 1 restates (GCC's libstdc++, unchanged in this respect since 4.x);
 *                mlh_std_sort_permutation lets an integrator compare the two on any key sequence;
 *   0            members in ascending point index (what a stable sort would give), device only and a few launches cheaper. Voxel set,
 *                output order and counts stay identical to the reference's and sums agree to f32 rounding, but the surviving id of a
 *                voxel that MIXES ids can differ (on a two-LiDAR frame: ~31 % of the 0.4 m surf voxels, ~5 % of the 0.2 m corner
 *                voxels; with uncertainty weighting that moved the frame's pose by 5 mm in scripts/framebench.py). A single-LiDAR
 *                cloud has no mixed voxels. */
int mlh_set_voxel_member_order(mlh_ctx *ctx, int mode);
/* Debug aid, no reference counterpart. With MLH_CHECK_LAUNCH=1 in the environment every kernel launch of the library is followed by hipGetLastError(): a bad
 * launch configuration is reported by the entry point that made it, as MLH_ERR_HIP with "launch of <kernel>: <error>" in mlh_last_error, instead of surfacing at
 * a later synchronisation under another call's name. mlh_debug_bad_launch makes one launch with an impossible configuration (4096 threads per workgroup) so that
 * the mechanism itself can be tested: MLH_ERR_HIP naming debug_noop_kernel under MLH_CHECK_LAUNCH=1, MLH_OK otherwise. */
int mlh_debug_bad_launch(mlh_ctx *ctx);
/* perm_out[0..n) (HOST) <- the permutation of 0..n-1 that two std::sort calls -- over [0, n0) and [n0, n), comparator on keys[] (HOST,
 * non-negative) only -- leave: mode 1 = the device restatement the voxel filters use, mode 2 = the platform's std::sort on the host. */
int mlh_std_sort_permutation(mlh_ctx *ctx, const int32_t *keys, int n0, int n, int32_t *perm_out, int mode);
/* mlh_voxel_filter: `mem` describes BOTH buffers: MLH_MEM_DEVICE takes device records and leaves the result in device memory (`out`), so a map
 * assembled with mlh_cloud_uct_associate_to_map can be thinned and handed to mlh_map_set without leaving HBM. */
int mlh_voxel_filter(mlh_ctx *ctx, const void *points, int stride_bytes, int n, int intensity_offset_bytes, int cov_offset_bytes,
                     int trace_offset_bytes, float leaf, float trace_threshold, void *out, int32_t *n_out, int mem);

/* ---------------------------------------------------------------- (a19) odometry-side three-block factors
 * replaces the per-feature LidarPureOdomPlaneNormFactor / LidarPureOdomEdgeFactor objects Estimator::optimizeMap hands to Ceres
 * (estimator.cpp:700-780) and their Evaluate (lidar_pure_odom_factor.hpp:38-102, 209-282): one residual + three 1x7 Jacobians
 * (pivot pose, window pose i, extrinsic n), point moved with T_pivot^-1 T_i T_ext.
 * mlh_pure_odom_set stages the factor table once per optimisation: type[i] 0 = plane ('s'), 1 = edge ('c'); points n x 3;
 * coeffs n x 6 (plane: [n, d, -, -], edge: the two line points); sqrt_info may be NULL (= 1.0, as the reference constructs them);
 * frame_idx / ext_idx select rows of the pose arrays given to mlh_pure_odom_evaluate.
 * Types and block indices are checked before the context or the device is touched: a type that is neither 0 nor 1, a negative index or one beyond 19 (a window
 * has at most 22 parameter blocks: the pivot, at most 20 frames, at most 20 extrinsics) is MLH_ERR_INVALID, and a rejected call leaves the staged table as it was.
 * mlh_pure_odom_evaluate: residuals n; jacobians n x 21 row-major [pivot 1x7 | frame 1x7 | extrinsic 1x7] or NULL. The columns
 * are the reference's expressions term by term (two of them are not exact derivatives; see m-loam_amd/csrc/odom.hip). */
int mlh_pure_odom_set(mlh_ctx *ctx, int n, const int32_t *type, const double *points, const double *coeffs, const double *sqrt_info,
                      const int32_t *frame_idx, const int32_t *ext_idx);
int mlh_pure_odom_evaluate(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext,
                           double *residuals, double *jacobians);
/* The same factor table built WITHOUT the host: mlh_pure_odom_begin starts an empty table; every mlh_pure_odom_add_matches matches the
 * staged feature set of `kind` (mlh_features_set / mlh_downsample_current_scan, one LiDAR's features in that LiDAR's frame) against the
 * resident map -- the window's local map in the pivot frame, estimator.cpp:1160-1268 -- at rel_pose = T_pivot^-1 T_frame T_ext
 * (FeatureExtract::matchCornerFromMap / matchSurfFromMap as Estimator::optimizeMap calls them, estimator.cpp:700-780; k_neigh 5 or 10,
 * MLH_FLAG_CHECK_FOV honoured) and appends one factor per valid correspondence: type = kind, point = the feature, coefficients = the
 * fitted plane / line, s = 1.0, blocks (frame_idx, ext_idx). Nothing is copied back; the number of factors is returned by
 * mlh_pure_odom_normal_eq (n_residuals). Such a table serves mlh_pure_odom_normal_eq only (its regions are padded to whole tiles);
 * mlh_pure_odom_evaluate needs a host-staged one. */
int mlh_pure_odom_begin(mlh_ctx *ctx);
int mlh_pure_odom_add_matches(mlh_ctx *ctx, int kind, const double rel_pose[7], int k_neigh, uint32_t flags, float min_match_sq_dis,
                              float min_plane_dis, int frame_idx, int ext_idx);
/* The same with the ODOMETRY's good-feature selection in front of the append -- Estimator::goodFeatureMatching with Estimator::evaluateFeatJacobian
 * (estimator.cpp:1273-1517), which buildLocalMap runs on every (frame, LiDAR) group with gf_ratio = ODOM_GF_RATIO (estimator.cpp:1241-1263; 0.8 in every shipped
 * configuration): all features of the group are matched on the GPU at rel_pose (= the Pose of T_pivot^-1 T_i T_ext, as the caller builds it), the row the
 * selection scores -- a surf feature's LidarPureOdomPlaneNormFactor(point, coeffs, 1.0) frame block at (pivot, pose_i, ext); (1 0 0 0 0 0) for a corner feature,
 * cpp:1339-1342 -- is evaluated for every matched feature in one launch, and the sequential draw loop runs on the host with the reference's draw sequence
 * (std::mt19937(seed) + uniform_int_distribution; MAX_RANDOM_QUEUE_TIME = 10, estimator.h:63; ten failed draws restart the round instead of ending the selection,
 * as the reference's loop does; its 7 ms wall-clock cut-off is not applied -- the loop ends when nothing is left to draw). gf_ratio == 1.0: every matched
 * feature, no loop. gf_ratio is a float, as ODOM_GF_RATIO is: the number of features asked for is size_t(n * (double)gf_ratio).
 * Only the selected correspondences are appended as factors. sel_out (nullable, capacity = the staged feature count) / n_sel (nullable): the selected feature
 * indices in selection order. One GPU (the loop needs the whole group's features). */
int mlh_pure_odom_add_matches_gf(mlh_ctx *ctx, int kind, const double rel_pose[7], const double pivot[7], const double pose_i[7], const double ext[7], int k_neigh,
                                 uint32_t flags, float min_match_sq_dis, float min_plane_dis, int frame_idx, int ext_idx, float gf_ratio, uint64_t seed,
                                 int32_t *sel_out, int32_t *n_sel);
/* The normal equations of the COUPLED window problem those factors form (BASELINE config 4; Estimator::optimizeMap, estimator.cpp:687-848):
 * local parameters in para_ids order [pivot | frames 0..n_frames) | extrinsics 0..n_ext)], 6 each (PoseLocalParameterization::ComputeJacobian
 * = [I6; 0]), D = 6 (1 + n_frames + n_ext). What Estimator::evalResidual gets from problem.Evaluate (estimator.cpp:1577-1595) -- rows
 * loss-corrected with HuberLoss(huber_delta) (1.0 at estimator.cpp:602; <= 0: no loss), every listed block variable -- reduced on the device:
 * JtJ D x D row-major (symmetric, both triangles filled), Jtr D, cost = sum rho(r^2)/2, n_residuals. evalDegenracy (estimator.cpp:1598-1680)
 * reads its diagonal 6x6 blocks (mlh_eval_degeneracy on each); with several GPUs (factors split over the ranks) the record is summed with
 * mlh_allreduce_f64 -- D (D + 1) / 2 + D + 2 = 326 doubles for the 24-dimensional hercules window. Deterministic (no atomics).
 * At most 22 parameter blocks (D = 132: the assembly is LDS-resident); more is MLH_ERR_UNSUPPORTED here and in mlh_pure_odom_gn_solve.
 * An installed window prior (mlh_window_prior_set / mlh_window_marginalize) or extrinsic prior is NOT added here: evalResidual evaluates res_ids_proj only
 * (estimator.cpp:1588-1593), and evalDegenracy must keep seeing the feature factors alone.
 * With a calibration store in use (f10 below: mlh_calib_use) its LidarOnlineCalib factors ARE added -- the reference pushes them to res_ids_proj (cpp:733, 778), so
 * evalResidual / evalDegenracy see them: JtJ / Jtr get the diagonal block and gradient rows of their extrinsic, cost and n_residuals count them. An empty factor
 * table with a non-empty store in use is legal and returns the store's system. n_ext must cover the store's largest extrinsic index (MLH_ERR_INVALID). Under a
 * communicator the record stays additive: every rank holds its OWN store and adds its own factors, so a store must not be replicated over the ranks. */
int mlh_pure_odom_normal_eq(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext,
                            double huber_delta, double *JtJ, double *Jtr, double *cost, int32_t *n_residuals);
/* The coupled window problem solved on the device: n_iters Gauss-Newton iterations on the staged (or device-built) factor table -- per iteration the
 * normal equations above, then ONE workgroup gathers the rows / columns of the blocks that are not held constant, factorises them (Cholesky in LDS; + 1e-6 I
 * and a second attempt when not positive definite) and applies PoseLocalParameterization::Plus block by block; three launches per iteration, the poses stay in
 * HBM until the call returns. replaces the ceres::Solve of Estimator::optimizeMap on the LidarPureOdom / LidarOnlineCalib factors (estimator.cpp:593-680,
 * 852-861) for the part of that problem built here (Gauss-Newton steps, not Ceres' trust region). With a window prior installed in the context (below) every
 * iteration adds its MarginalizationFactor term (estimator.cpp:658-665) -- and, with bit 1 of mlh_window_ext_prior_set, the extrinsics' PriorFactor rows (cpp:675-685)
 * -- to the assembled system on the device, one more one-workgroup launch between the assembly and the factorisation; `cost` then includes them, n_residuals
 * still counts the feature factors. Without either, the launches and every output bit are what they are without this feature. A prior whose block map does not
 * fit (n_frames, n_ext) is MLH_ERR_STATE. With a calibration store in use (f10 below) every iteration's system includes its factors (cpp:729-733, 776-778 inside
 * ceres::Solve): two more launches per iteration, n_residuals counts them; not in use or empty: the launches and every output bit are unchanged. Unlike
 * mlh_pure_odom_normal_eq and mlh_window_marginalize the solve still needs a non-empty factor table: on an empty one it is MLH_ERR_STATE, store or no store (the
 * reference's calibration problem always holds the reference LiDAR's window factors).
 *   const_block_mask  bit b set = block b of [pivot | frames 0.. | extrinsics 0..] is held constant (estimator.cpp:636 para_pose_[0], :642 the reference LiDAR's
 *                     extrinsic; 1u | 1u << (1 + n_frames) for the reference's choice)
 *   V_update          NULL (identity) or 36 doubles per block, row-major: what Estimator::evalDegenracy (estimator.cpp:1598-1680; facade evalDegenracy) left in
 *                     every block's PoseLocalParameterization -- a projector for a degenerate pose block, zero for an extrinsic that is not to be updated
 *   frames / exts     in: the linearisation point, out: the result.  cost / n_residuals: of the LAST linearisation (before the final update).
 *   status            0 solved, 1 some iteration needed the + 1e-6 I, 2 some iteration's system was not positive definite even then (that update was skipped)
 * Under a communicator (mlh_comm_init / mlh_p2p_comm_init) the call returns MLH_ERR_UNSUPPORTED: it factorises this rank's sums, and ranks holding different
 * parts of the factor table would apply different updates. Sharded callers all-reduce mlh_pure_odom_normal_eq's H / g (mlh_allreduce_f64) and solve on the host. */
int mlh_pure_odom_gn_solve(mlh_ctx *ctx, const double pivot[7], double *frames, int n_frames, double *exts, int n_ext, double huber_delta, int n_iters,
                           uint32_t const_block_mask, const double *V_update, double *cost, int32_t *n_residuals, int32_t *status);

/* ---------------------------------------------------------------- (f9) the window's marginalisation prior, on the device
 * A context holds at most one window prior -- what the reference keeps in last_marginalization_info_ / last_marginalization_parameter_blocks_: n_keep kept
 * blocks (6 local parameters each), a block map kept block k -> block id of the window layout [pivot | frames 0.. | extrinsics 0..], the linearisation points x0
 * (7 doubles per kept block, [t, q(xyzw)]), linearized_jacobians J0 (n x n row-major, n = 6 n_keep) and linearized_residuals r0 (n). It stays in HBM between the
 * call that makes it and the solves that read it (mlh_pure_odom_gn_solve above).
 * mlh_window_prior_set: installs a caller's prior (restoring saved state; at most 21 kept blocks, distinct ids in 0..21).
 * mlh_window_prior_get: reads it back; every buffer may be NULL. info: see the struct. MLH_ERR_STATE when a buffer is asked for and no prior is installed.
 * mlh_window_prior_clear: drops it (Estimator::clearState, estimator.cpp:1729-1731).
 * mlh_window_prior_evaluate: MarginalizationFactor::Evaluate (marginalization_factor.cpp:358-410) at the given state -- the n residuals r0 + J0 dx, with dx per
 *   kept block x - x0 for the translation and 2 positify(q0^-1 q).vec() for the rotation, the sign flip of cpp:383-386 as written; H (D x D, D = 6 (1 + n_frames
 *   + n_ext)) = J0^T J0 scattered through the block map; g (D) = J0^T (r0 + J0 dx); cost = 0.5 |r0 + J0 dx|^2. Outputs may be NULL. The extrinsic prior is not part
 *   of it. MLH_ERR_STATE without a prior or when its block map does not fit (n_frames, n_ext).
 * mlh_window_ext_prior_set: the PriorFactor of every extrinsic (prior_factor.hpp:27-72; estimator.cpp:675-685, 891-900). rows = n_ext x 9: t[3], q[4] (x y z w),
 *   pos_scale, rot_scale (tbl_[n], qbl_[n], PRIOR_FACTOR_POS, PRIOR_FACTOR_ROT): 6 residuals sqrt_info [P - t, 2 (q^-1 Q).vec()] and the 6 x 6 Jacobian
 *   sqrt_info [I, 0; 0, LeftQuatMatrix(Q^-1 q).topLeftCorner<3, 3>()] (common/algos/math.hpp:77-87) -- the Jacobian the reference's own comment calls wrong,
 *   reproduced. flags bit 0: the rows enter mlh_window_marginalize (cpp:891-900, whatever ESTIMATE_EXTRINSIC is); bit 1: they also enter mlh_pure_odom_gn_solve
 *   (cpp:675-685, online calibration only). n_ext = 0 removes them.
 * mlh_window_marginalize: replaces estimator.cpp:871-1063 (MarginalizationInfo::preMarginalize / marginalize / getParameterBlocks, marginalization_factor.cpp:
 *   126-144, 189-341) for the factors the device table holds, at the given state (the solve's result): the table's normal equations over ALL blocks
 *   (marginalisation ignores constness) with the loss correction of ResidualBlockInfo::Evaluate (marginalization_factor.cpp:50-81; for HuberLoss on a scalar
 *   residual rho[2] <= 0, the sqrt(rho[1]) branch: what mlh_pure_odom_normal_eq applies), plus the installed prior's term with its pivot block in the drop set
 *   (cpp:877-889), plus the extrinsic prior rows when their bit 0 is set. The pivot block is marginalised (m = 6): Amm = 0.5 (Amm + Amm^T), pseudo-inverse
 *   through a symmetric eigen-decomposition with eps = 1e-8, Schur complement, second decomposition, J0 = sqrt(S) V^T, r0 = sqrt(S^-1) V^T b -- all f64, on the
 *   device (cyclic Jacobi in one workgroup). The result REPLACES the installed prior: kept blocks [frames | extrinsics] in window order, x0 = this call's poses,
 *   block map already slid as addr_shift does (cpp:1042-1050): frame i -> block i (frame 0 is the next window's pivot), extrinsic e -> 1 + n_frames + e. When
 *   nothing touches the pivot (empty table, no prior on block 0) the prior is cleared and info.valid = 0 (the reference's m == 0). At most 22 blocks
 *   (MLH_ERR_UNSUPPORTED before anything is enqueued); under a communicator MLH_ERR_UNSUPPORTED. The LidarOnlineCalib factors on the accumulated features
 *   (cpp:921-938, 960-977) enter the assembled system when a calibration store is in use (f10 below): they carry no drop set and never touch the pivot, so they land
 *   in Arr only. The store is NOT cleared by the call; the caller clears it, as the reference does after the marginalisation on calibration frames (cpp:936-937,
 *   975-976). The only host wait is the one that fills info_out -- and, with a store in use, the first call after an append to the store (or with another
 *   n_ext) waits twice more while the store's tile lists for this extrinsic count go to the device. */
typedef struct mlh_window_prior_info {
    int32_t valid, n_keep, n;             /* n = 6 n_keep */
    int32_t kept_mm, kept_rr;             /* eigenvalues > 1e-8 kept: of Amm (6) and of the Schur complement (n); -1: the prior was installed by mlh_window_prior_set */
    int32_t sweeps_mm, sweeps_rr;         /* Jacobi sweeps the two decompositions used */
    int32_t reserved;
    double min_kept_mm, max_dropped_mm;   /* smallest kept / largest dropped eigenvalue (0 when there is none) */
    double min_kept_rr, max_dropped_rr;
} mlh_window_prior_info;
int mlh_window_prior_set(mlh_ctx *ctx, int n_keep, const int32_t *block_ids, const double *x0, const double *J0, const double *r0);
int mlh_window_prior_get(mlh_ctx *ctx, mlh_window_prior_info *info, int32_t *block_ids, double *x0, double *J0, double *r0);
int mlh_window_prior_clear(mlh_ctx *ctx);
int mlh_window_prior_evaluate(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext,
                              double *residuals, double *H, double *g, double *cost);
int mlh_window_ext_prior_set(mlh_ctx *ctx, int n_ext, const double *rows, uint32_t flags);
int mlh_window_marginalize(mlh_ctx *ctx, const double pivot[7], const double *frames, int n_frames, const double *exts, int n_ext, double huber_delta,
                           mlh_window_prior_info *info_out);

/* ---------------------------------------------------------------- (f10) the accumulated calibration features, on the device
 * The online extrinsic calibration (ESTIMATE_EXTRINSIC == 1): Estimator::optimizeMap gives window factors to the reference LiDAR only (estimator.cpp:687-712,
 * 744-760); the extrinsic of every other LiDAR n is constrained by the one-block LidarOnlineCalibPlaneNormFactor / LidarOnlineCalibEdgeFactor
 * (lidar_online_calib_factor.hpp:35-62, 135-165) built from cumu_surf_map_features_[n] / cumu_corner_map_features_[n]: LiDAR n's pivot-frame correspondences,
 * accumulated over N_CUMU_FEATURE frames and added to the problem on every N_CUMU_FEATURE-th frame (cpp:714-735, 762-780) and to the marginalisation (cpp:921-938,
 * 960-977). A context keeps those lists as a store of factor records in HBM (point[3], coeff[6], sqrt_info as f64, type 0 plane / 1 edge) in 256-factor tiles, every
 * tile belonging to one extrinsic. The store persists across windows: mlh_pure_odom_begin and mlh_pure_odom_set do not touch it.
 * mlh_calib_accumulate: twin of mlh_pure_odom_add_matches. Matches the staged feature set of `kind` -- LiDAR ext_idx's pivot-frame features -- against the resident
 *   map -- buildCalibMap's map of that LiDAR (mlh_window_build_local_map with source_lidar >= 0) -- at rel_pose = pose_local_[n][pivot_idx] with k_neigh 10 and
 *   MLH_FLAG_CHECK_FOV (cpp:1131-1149) and appends the valid correspondences to the store in feature order, s = 1.0: cpp:714-719, 762-767 without the host lists.
 *   Nothing comes back to the host. MLH_ERR_STATE without staged features or a map, MLH_ERR_INVALID for a negative ext_idx.
 * mlh_calib_add: the same append from host lists (callers that keep them; tests). ext_idx is per factor; the factors are grouped by extrinsic into tiles, stable
 *   within a group. sqrt_info may be NULL (= 1.0).
 * mlh_calib_use: whether the store's factors enter mlh_pure_odom_normal_eq, mlh_pure_odom_gn_solve and mlh_window_marginalize -- the
 *   frame_cnt_ % N_CUMU_FEATURE == 0 gate of cpp:721, 769, 921, 960, whose arithmetic stays the caller's. Off by default.
 * mlh_calib_clear: empties the store and turns `use` off (cpp:736-740, 781-785, 936-937, 975-976; Estimator::clearState cpp:175-176).
 * mlh_calib_info: see the struct; n_valid reads one device word back when mlh_calib_accumulate has appended.
 * mlh_calib_evaluate: per-factor residual (n_valid) and 1 x 7 Jacobian row (n_valid x 7, 7th column zero, may be NULL), without the loss correction, in the order
 *   the factors were given -- for a store made by mlh_calib_add alone; MLH_ERR_STATE otherwise, as mlh_pure_odom_evaluate refuses device-built tables. exts: n_ext x 7,
 *   covering the store's largest extrinsic index (MLH_ERR_INVALID). An edge factor whose point lies exactly on its line has nu = 0: residual 0 and a zero row, as
 *   Eigen's normalized() leaves the zero vector. */
typedef struct mlh_calib_store_info {
    int32_t n_appends;                    /* mlh_calib_accumulate / mlh_calib_add calls since the last clear */
    int32_t n_tiles, n_slots;             /* n_slots = 256 n_tiles, padding included */
    int32_t n_valid;                      /* factors */
    int32_t max_ext;                      /* largest extrinsic index (-1: empty) */
    int32_t in_use;
} mlh_calib_store_info;
int mlh_calib_accumulate(mlh_ctx *ctx, int kind, const double rel_pose[7], int k_neigh, uint32_t flags, float min_match_sq_dis, float min_plane_dis, int ext_idx);
int mlh_calib_add(mlh_ctx *ctx, int n, const int32_t *type, const double *points, const double *coeffs, const double *sqrt_info, const int32_t *ext_idx);
int mlh_calib_use(mlh_ctx *ctx, int on);
int mlh_calib_clear(mlh_ctx *ctx);
int mlh_calib_info(mlh_ctx *ctx, mlh_calib_store_info *out);
int mlh_calib_evaluate(mlh_ctx *ctx, const double *exts, int n_ext, double *residuals, double *jacobians);

/* ---------------------------------------------------------------- (f11) Scan Context place recognition, on the device
 * The front of the loop-closure process: SCManager (mloam_loop/src/scan_context.cpp:155-323) as PoseGraph::detectLoop drives it (mloam_loop/src/pose_graph.cpp:
 * 281-328). A context keeps one store in HBM: per entry the descriptor (f32, num_ring x num_sector, column-major as Eigen stores it), the ring key (f32), the sector
 * key and the column norms (f64), and on the host the optional position. The geometric verification is sections (f12) and (f13); the pose graph is section
 * (f14).
 * Reproduced, with the lines restated:
 *   descriptor (cpp:155-186): z' = float(double(z) + lidar_height); range = sqrt(x x + y y) in f32; dropped only if range > max_radius (a point at exactly
 *     max_radius stays); ring = max(min(R, int(ceil(double(range) / max_radius * R))), 1); angle = xy2theta (cpp:38-51) as written, signed zeros and infinities
 *     included; sector = max(min(S, int(ceil(double(angle) / 360.0 * S))), 1); a cell is the maximum of z', starting at -1000; cells still equal to -1000 become 0,
 *     so a z' of exactly -1000 or below reads as empty. The maximum is order-independent: the descriptor is bit-exact whatever the schedule. Every value is a
 *     widened float, so it is stored as f32.
 *   CHOSEN: xy2theta calls unqualified atan on floats; which overload a translation unit gets depends on its includes. The float overloads are restated (atanf,
 *     then (180 / M_PI) * ... in double, returned as float). The choice matters only within a few f32 ulps of a sector edge: a point whose sector value lies within
 *     4e-4 sectors of an integer is not binned by the kernel; the host decides it with its own libm and its verdict is applied before the keys are made
 *     (mlh_sc_store_info::points_host_decided counts them: ~0.08 % of a cloud, and every point on an axis).
 *   CHOSEN: x = y = 0 makes the reference convert a NaN to int; what x86 does is restated (ring 1, sector 1).
 *   DEPARTURE: a point with a non-finite coordinate is skipped and counted (points_skipped); the reference's behaviour there is undefined.
 *   keys (cpp:188-218, 225): ring key = row means in f64, cast to f32; sector key = column means in f64; the f64 column norms distDirectSC recomputes for every
 *     shift are kept beside them. Sums run left to right (Eigen's reduction order is not restated).
 *   candidates (cpp:246-278): early return when que_index < num_exclude_recent + 1 (the period counter does not advance); the searched set is the prefix
 *     [0, que_index - num_exclude_recent) AS OF THE LAST REBUILD, rebuilt when counter % tree_making_period == 0 -- stale in between, reproduced. Exact k-NN with
 *     nanoflann's L2_Adaptor arithmetic in f32 (nanoflann.hpp:432-461: groups of four, result += d0 d0 + d1 d1 + d2 d2 + d3 d3, then the tail), bit-exact.
 *     CHOSEN: a brute-force kernel replaces the tree, and equal distances go to the lower index (in the reference: the tree's visiting order). With fewer searched
 *     entries than num_candidates the reference's zero-filled index array re-scores entry 0, which changes nothing: every searched entry is scored once
 *     (n_candidates_scored).
 *   score (cpp:80-153, 286-322): fast alignment = first-lowest Frobenius norm over all S shifts of the candidate's sector key; search radius
 *     round(0.5 search_ratio S), the shifts within it visited in ascending order; distDirectSC in f64 skips columns where either norm is 0 -- with no effective
 *     column the distance is NaN, NaN never wins: nearest_index stays -1 and score 1e7; strict < over shifts and over candidates, in candidate order;
 *     yaw_diff_rad = deg2rad(float(shift * (360.0 / S))) with the reference's float deg2rad; then score < dist_thres; then detectLoop's rejection
 *     |t_que - t_match| > loop_distance_threshold (pose_graph.cpp:296-315) on the stored positions -- none when either entry has no position.
 * mlh_sc_reset = setParameter: validates (MLH_ERR_INVALID outside num_ring >= 1, num_sector >= 1, num_ring * num_sector <= 8192, 1 <= num_candidates <= 256,
 *   a finite positive max_radius, tree_making_period >= 1, num_exclude_recent >= 0, a finite lidar_height and search_ratio >= 0), empties the store, frees its
 *   memory and zeroes the period counter. opts == NULL: the defaults. The other calls return MLH_ERR_STATE before the first reset.
 * mlh_sc_add = makeAndSaveScancontextAndKeys of the concatenation of n_clouds <= 3 clouds (full_cloud_ + outlier_cloud_, pose_graph.cpp:283-286): records of
 *   stride_bytes in `mem`, only xyz read; empty clouds are allowed (n[k] == 0, clouds[k] may be NULL). position (3 doubles, may be NULL) is the keyframe's
 *   pose_w_.t_. *index_out (may be NULL) <- the entry's index. One host wait (the undecided points), one more when there are more than 2048 of them.
 * mlh_sc_add_keyframe: the same from keyframe `key` of the store of (f5) / (f7): its surf, corner and outlier clouds device to device, its stored translation.
 *   DEPARTURE: the mapper's store has no full cloud, so these descriptors are built from thinned features: comparable with each other, not with descriptors of
 *   full clouds.
 * mlh_sc_add_keyframes (row f17: the per-keyframe addKeyFrameIntoDB loop of loadPoseGraph / loadKeyFrame, pose_graph.cpp:696-781, 225-279, 77-90, in one call):
 *   DEFINED AS n calls of mlh_sc_add_keyframe(first_key + i), i = 0..n-1. Reproduced bit for bit: every entry's descriptor, ring key, sector key and column norms,
 *   its position, points_host_decided, points_skipped and the store's capacity (the buffers grow ONCE, to the capacity the single adds would have doubled their
 *   way to). DEPARTURE: last_host_decided / last_skipped are those of the whole batch. *first_index_out (may be NULL) <- the index of the first new entry; n == 0
 *   changes nothing; first_key < 0, n < 0 or first_key + n beyond the stored keyframes: MLH_ERR_INVALID, nothing changed. A batch holds fewer than 2^31 points.
 *   Three launches and ONE host wait whatever n (descriptor kernel, the marker of the wait, finish kernel); one more of each only when the batch leaves more
 *   than 2048 points undecided, as the single add does; a batch without a point launches the finish kernel alone. CHOSEN: the host cuts each keyframe's points
 *   (surf, corner, outlier back to back) into chunks of a multiple of 256 points, as many per keyframe as bring the grid to two workgroups per compute unit
 *   when n alone does not, at most 64; a workgroup builds its chunk's cells in LDS and merges them into the entry's slot with integer max, so the result does not
 *   depend on the cutting. CHOSEN: the undecided points of the whole batch share one list (capacity: the batch's points) and one counter; a point's entry
 *   travels in a parallel int array, its ring in the record's fourth word as in the single add. The host decides them with its libm and groups the verdicts by
 *   entry; the finish kernel runs one workgroup per entry. mlh_sc_last_batch reports the last batch of the context (zero before the first, and after
 *   mlh_sc_reset).
 * mlh_sc_detect = detectLoopClosureID(que_index) + detectLoop's rejection. Five launches and one copy whatever the size of the store and num_candidates (key
 *   distances, selection, one workgroup per candidate, the ordered argmin, the marker of the wait) and ONE host wait. A result that the distance test rejects keeps
 *   score, shift, yaw and nearest_index, has match_index -1 and rejected_by_distance 1. The early return gives {-1, score -1, yaw 0, nearest -1}.
 * mlh_sc_candidates: the candidate search alone, stateless: the min(prefix, num_candidates) nearest ring keys of entry que_index among entries [0, prefix), in
 *   the order they are scored, with their squared distances (d2_out may be NULL). idx_out: capacity >= num_candidates.
 * mlh_sc_distance = distanceBtnScanContext(descriptor i, descriptor j): (min distance, its shift); the distance is 1e7 and the shift 0 when every shift is NaN.
 * mlh_sc_fetch: entry `index` as f64 num_ring x num_sector column-major (desc), f32 num_ring (ring_key), f64 num_sector (sector_key); each may be NULL. The
 *   host makes getScanContextImage of it.
 * mlh_keyframes_reset does not touch this store; mlh_destroy frees it. */
typedef struct mlh_sc_opts {
    double lidar_height;             /* LIDAR_HEIGHT */
    int32_t num_ring, num_sector;    /* PC_NUM_RING, PC_NUM_SECTOR */
    double max_radius;               /* PC_MAX_RADIUS */
    int32_t num_exclude_recent;      /* NUM_EXCLUDE_RECENT */
    int32_t num_candidates;          /* NUM_CANDIDATES_FROM_TREE */
    double search_ratio;             /* SEARCH_RATIO */
    double dist_thres;               /* SC_DIST_THRES */
    int32_t tree_making_period;      /* TREE_MAKING_PERIOD */
    int32_t reserved;
    double loop_distance_threshold;  /* LOOP_DISTANCE_THRESHOLD; < 0: no rejection */
} mlh_sc_opts;
typedef struct mlh_sc_result {
    int32_t match_index;             /* -1: no loop */
    int32_t nearest_index;           /* the argmin before the threshold (-1: nothing scored below 1e7) */
    int32_t shift;                   /* nn_align, in sectors */
    int32_t n_candidates_scored;
    int32_t rejected_by_distance;
    float yaw_diff_rad;
    double score;                    /* min_dist */
} mlh_sc_result;
typedef struct mlh_sc_store_info {
    int32_t n_entries;
    int32_t searched_prefix;         /* entries [0, searched_prefix) as of the last rebuild */
    int32_t period_counter;          /* tree_making_period_conter_ */
    int32_t desc_tile_points;        /* points a workgroup of the descriptor kernel takes per pass */
    int32_t desc_wrap_points;        /* points all its workgroups take per pass: a larger cloud goes round the grid-stride loop again */
    int32_t last_host_decided, last_skipped;     /* of the most recent add */
    int32_t reserved;
    int64_t points_host_decided;     /* since the last reset: points the host binned with its libm */
    int64_t points_skipped;          /* ... points with a non-finite coordinate */
    int64_t bytes_hbm;               /* device memory the store holds */
} mlh_sc_store_info;
void mlh_sc_opts_default(mlh_sc_opts *o);    /* mloam_loop/config/config_loop_realvehicle.yaml: 2.0, 20, 60, 80.0, 50, 50, 0.1, 0.5, 10, 50.0 */
int mlh_sc_reset(mlh_ctx *ctx, const mlh_sc_opts *opts);
int mlh_sc_add(mlh_ctx *ctx, const void *const *clouds, const int32_t *n, int n_clouds, int stride_bytes, int mem, const double *position, int32_t *index_out);
int mlh_sc_add_keyframe(mlh_ctx *ctx, int32_t key, int32_t *index_out);
typedef struct mlh_sc_batch_info {
    int32_t n_entries, n_chunks;     /* of the last mlh_sc_add_keyframes: entries added, workgroups of its descriptor kernel */
    int32_t launches, host_waits;    /* kernel launches (the waits' markers included) and host waits it took */
    int32_t first_index;             /* index of its first entry */
    int32_t chunk_points;            /* the plan's constants: a chunk holds a multiple of this many points (but an entry's last) ... */
    int32_t max_chunks_per_entry;    /* ... an entry is cut into at most this many ... */
    int32_t target_workgroups;       /* ... and only while the grid is below this: two per compute unit */
    int64_t n_points;
    int64_t points_host_decided, points_skipped;
} mlh_sc_batch_info;
int mlh_sc_add_keyframes(mlh_ctx *ctx, int32_t first_key, int32_t n, int32_t *first_index_out);
int mlh_sc_last_batch(mlh_ctx *ctx, mlh_sc_batch_info *out);
int mlh_sc_detect(mlh_ctx *ctx, int32_t que_index, mlh_sc_result *result);
int mlh_sc_candidates(mlh_ctx *ctx, int32_t que_index, int32_t prefix, int32_t *idx_out, float *d2_out, int32_t *n_out);
int mlh_sc_distance(mlh_ctx *ctx, int32_t i, int32_t j, double *dist, int32_t *shift);
int mlh_sc_fetch(mlh_ctx *ctx, int32_t index, double *desc, float *ring_key, double *sector_key);
int mlh_sc_info(mlh_ctx *ctx, mlh_sc_store_info *out);

/* ---------------------------------------------------------------- (f12) loop-closure local registration, on the device
 * The geometric verification that turns a Scan Context candidate into a loop edge: PoseGraph::constructLocalMap (mloam_loop/src/pose_graph.cpp:364-419) and
 * LoopRegistration::performLocalRegistration (mloam_loop/src/loop_registration.cpp:104-211) with the loop package's own match functions (mloam_loop/include/
 * mloam_loop/utility/feature_extract.hpp:28-43, 77-247) and factor (mloam_loop/include/mloam_loop/factor/lidar_map_plane_norm_factor.hpp:47-87). FGR / FPFH
 * (performGlobalRegistration) is section (f13), the pose graph and its optimisation section (f14); checkTemporalConsistency stays with the caller. T_ini comes from
 * mlh_fgr_register on the same clouds, or from the Scan Context yaw. A loop process uses a context of its own: mlh_loop_match, mlh_loop_evaluate
 * and mlh_loop_register OVERWRITE the context's two map indexes (mlh_map_set) and its solver state; they return MLH_ERR_STATE while a solve submitted with
 * mlh_*_begin is uncollected and MLH_ERR_UNSUPPORTED under a communicator. DEPARTURE from the plan of staging the data clouds as the context's feature sets: the
 * kernels read them where mlh_loop_build_clouds / mlh_loop_set_clouds left them, so the feature sets are NOT touched.
 * The four clouds: `which` = MLH_LOOP_MODEL_SURF / MODEL_CORNER (laser_cloud_*_from_map: the match side) / DATA_SURF / DATA_CORNER (laser_cloud_*: the query side),
 * 16-byte {x, y, z, intensity} records in HBM.
 * mlh_loop_build_clouds = constructLocalMap. Two lists of (keyframe key of the store of (f5), 4 x 4 f32 row-major matrix): the data list carries
 *   T_ini_map_kf.cast<float>() per keyframe (cpp:381-385), the model list T_relative.cast<float>() (cpp:405-408). WHICH keys go in -- the index windows, the
 *   `que_index + j < 0` and `match_index + j >= que_index` skips, missing keyframes -- and the f64 matrix chains are host arithmetic of the caller (the C++ facade's
 *   LoopLocalMap restates them). On the device: ONE launch transforms every segment of all four clouds (pcl::transformPointCloud in f32: ((r0 x + r1 y) + r2 z) + t,
 *   no contraction, intensity carried; the launch the window's local maps use), concatenated in list order; then four pcl::VoxelGrid<PointXYZI> filters through the
 *   context's voxel-grid path at opts->leaf_surf / leaf_corner (mlh_set_voxel_member_order applies). n_pre[4] / n_ds[4] <- the pre-filter and filtered counts.
 *   Launches do not depend on the number of keyframes; two host waits (the clouds' bounds; the filtered counts); no device allocation once the buffers have grown
 *   (mlh_loop_info::allocations). A key that is not in the store, a non-finite matrix entry or more than 4096 keys in a list: MLH_ERR_INVALID, nothing launched.
 * mlh_loop_set_clouds: the four (already filtered) clouds given directly, for callers with their own keyframe containers: records of stride_bytes with xyz at 0
 *   and the intensity at intensity_offset_bytes (< 0: stored as 0), all host or all device; empty clouds are allowed (n[k] == 0, clouds[k] may be NULL). They become
 *   the filtered clouds; the pre-filter clouds are emptied.
 * mlh_loop_cloud: the pre-filter (filtered = 0) or filtered (1) cloud `which`; *device_points is NULL for an empty one. Valid until the next build / set.
 * mlh_loop_match = matchSurfFromMap (kind MLH_SURF) / matchCornerFromMap (MLH_CORNER) of the filtered data cloud against the filtered model cloud at T (16 doubles,
 *   row-major, cast to f32 as cpp:145, 152 do) -- a test and diagnosis entry in the spirit of mlh_match_coeffs. Per data point i: valid[i]; coeffs[4 i ..] (surf) or
 *   coeffs[8 i ..] = feature1, feature2 (corner), zeros where invalid; *n_features <- features.size() (corner: two per matched point). Outputs may be NULL.
 *   Per point, in f32 with no contraction: point_sel = ((r0 x + r1 y) + r2 z) + t; the exact 5 nearest model points through the context's map index, built with
 *   min_match_sq_dis = match_sq_dis_surf / _corner so that the 27-cell search is exact for the acceptance test sq_dis[4] < 2.0 / 5.0 (strict);
 *   surf (hpp:203-243): colPivHouseholderQr().solve(-1) as the mapper path restates it, negative_OA_dot_norm = 1 / norm.norm(), normalize, a neighbour with
 *     double(fabs(n . q + d)) > plane_dis rejects, coeffs (n, d) widened to f64;
 *   corner (hpp:105-167): centroid and 3 x 3 covariance in f32 (center /= (1.0 * 5): Eigen converts the double to the vector's scalar, a division by 5.0f),
 *     SelfAdjointEigenSolver<Matrix3f> as the mapper path restates it, eig[2] > line_eig_ratio * eig[1]; X1 = 0.1f * dir + center, X2 = -0.1f * dir + center (Eigen
 *     promotes a double literal that multiplies a float expression to float); n = (X1 - X0) x (X2 - X0); w2 = n.normalized(); w1 = (w2 x (X2 - X1)).normalized();
 *     ld_1 = n.norm() / (X1 - X2).norm(); ld_p1 = -(w1 . X0 - ld_1); ld_p2 = -(w2 . X0 - 0); TWO features per point, (w1, ld_p1) * 0.5 and (w2, ld_p2) * 0.5 in f64,
 *     in that order.
 *   CHOSEN: sums of three f32 terms (dot products, squared norms, the matrix-vector product) run left to right, as in every row of this library; Eigen's own
 *     reduction order is not restated. CHOSEN: equal distances go to the lower index (the reference: FLANN's visiting order). CHOSEN: a model cloud with fewer than
 *     five points matches nothing (the reference reads past the end of the search result there).
 * mlh_loop_evaluate (test entry): matches both kinds at T_match, then evaluates every feature at `pose` [t, q(xyzw)] once: H (6 x 6 row-major J^T J), g (J^T r),
 *   *cost = sum of rho / 2, counts[2] = residual blocks of surf / corner, as Ceres would hand them to the linear solver. Per block: a = w . (q p + t) + d, r = a w
 *   (3 rows, sqrt_info_ = I), J = [W, -W R [p]x] with W = w w^T; Huber(huber_delta) on s = |r|^2 as Ceres corrects a block (rho'' <= 0: scaled by sqrt(rho')). The
 *   kernel uses the block's scalar form (residual |w| a, row |w| j: the same J^T J, J^T r and s up to rounding). Tile partials summed in a fixed order: two runs give
 *   the same bits.
 * mlh_loop_register = performLocalRegistration(the four filtered clouds, T_ini) -> *result. Per outer iteration (cpp:117-198): para_pose from
 *   Quaterniond(T.block<3,3>) (Eigen's matrix-to-quaternion conversion, not normalised) and T's translation; both matches at T.cast<float>(); the 0.2 rule (cpp:158:
 *   1.0 * surf_num / surf_size <= min_match_ratio && 1.0 * corner_num / corner_size <= min_match_ratio breaks; corner_num counts features, two per matched point,
 *   against points, so its ratio reaches 2; an empty data cloud of a kind gives NaN, which does not break); ceres::Solve as the project's Ceres-shaped
 *   Levenberg-Marquardt (max_lm_iterations, no degeneracy handling, identity V_update) in the launch-per-iteration form: one evaluate launch and one one-workgroup
 *   step launch per iteration, kernel boundaries the only synchronisation between workgroups; opti_cost = min(final_cost, opti_cost) from 1e7; T rebuilt from
 *   q.toRotationMatrix() in f64. A break in outer iteration 0 returns T_ini bit for bit with cost 1e7; a break later keeps the earlier T and cost. With both data
 *   clouds empty no break happens, the solve has no residual block, terminates at once with cost 0 and is accepted (what the restated solver does; Ceres reports
 *   the same cost). accepted = opti_cost <= local_registration_threshold (cpp:202).
 *   DEPARTURE: max_solver_time_in_seconds = 0.03 (cpp:188) is a wall-clock cut-off and is not applied.
 *   Host waits: ONE per outer iteration entered (its two counts, its LM summary and pose arrive together: the solve is enqueued behind the matches without waiting
 *   for the counts, and discarded when the 0.2 rule breaks), plus what staging the two model clouds costs when they changed since the last call (mlh_map_set x 2).
 * mlh_loop_opts_default: 0.4 / 0.4, 20, 2, 5, 2000, 1.0, 2.0 / 5.0, 0.2, 3, 0.2. Options are validated by every call that takes them (NULL: the defaults):
 *   MLH_ERR_INVALID outside finite leaves, thresholds and huber_delta > 0, 0 <= history_search_num <= 4096, 1 <= max_outer <= 8, 0 <= max_lm_iterations <= 200,
 *   plane_dis >= 0, line_eig_ratio >= 0, and a NaN anywhere. */
enum { MLH_LOOP_MODEL_SURF = 0, MLH_LOOP_MODEL_CORNER = 1, MLH_LOOP_DATA_SURF = 2, MLH_LOOP_DATA_CORNER = 3 };
typedef struct mlh_loop_opts {
    float leaf_surf, leaf_corner;            /* down_size_filter_{surf,corner}_map_ (pose_graph.cpp:33-34) */
    int32_t history_search_num;              /* LOOP_HISTORY_SEARCH_NUM (the facade's window; the library itself does not read it) */
    int32_t max_outer;                       /* cpp:117 */
    int32_t max_lm_iterations;               /* options.max_num_iterations */
    int32_t reserved;
    double local_registration_threshold;     /* LOOP_LOCAL_REGISTRATION_THRESHOLD */
    double huber_delta;                      /* ceres::HuberLoss(1) */
    float match_sq_dis_surf, match_sq_dis_corner;
    double plane_dis;
    float line_eig_ratio;
    int32_t reserved2;
    double min_match_ratio;
} mlh_loop_opts;
typedef struct mlh_loop_outer_stat {
    int32_t entered;                         /* the outer iteration matched */
    int32_t ran;                             /* ... and solved (0: the 0.2 rule broke the loop here) */
    int32_t surf_num, corner_num;            /* features.size() of the two matches */
    int32_t lm_iterations, successful_steps;
    int32_t termination;                     /* as mlh_iter_stat::termination */
    int32_t reserved;
    double initial_cost, final_cost;
} mlh_loop_outer_stat;
typedef struct mlh_loop_result {
    double T_relative[16];                   /* row-major */
    double para_pose[7];                     /* the last para_pose [t, q(xyzw)] (a break in outer iteration 0: that of T_ini) */
    double opti_cost;
    int32_t accepted;
    int32_t n_outer;                         /* outer iterations entered */
    mlh_loop_outer_stat outer[8];
} mlh_loop_result;
typedef struct mlh_loop_info {
    int32_t n_pre[4], n_ds[4];
    int64_t allocations;                     /* device allocations of the loop store since the context was made */
    int64_t bytes_hbm;
} mlh_loop_info;
void mlh_loop_opts_default(mlh_loop_opts *o);
int mlh_loop_build_clouds(mlh_ctx *ctx, const int32_t *data_keys, const float *data_T, int n_data, const int32_t *model_keys, const float *model_T, int n_model,
                          const mlh_loop_opts *opts, int32_t *n_pre, int32_t *n_ds);
int mlh_loop_set_clouds(mlh_ctx *ctx, const void *const *clouds, const int32_t *n, int stride_bytes, int intensity_offset_bytes, int mem);
int mlh_loop_cloud(mlh_ctx *ctx, int which, int filtered, const void **device_points, int32_t *n);
int mlh_loop_info_get(mlh_ctx *ctx, mlh_loop_info *out);
int mlh_loop_match(mlh_ctx *ctx, int kind, const double *T, const mlh_loop_opts *opts, uint8_t *valid, double *coeffs, int32_t *n_features);
int mlh_loop_evaluate(mlh_ctx *ctx, const double *T_match, const double *pose, const mlh_loop_opts *opts, double *H, double *g, double *cost, int32_t *counts);
int mlh_loop_register(mlh_ctx *ctx, const double *T_ini, const mlh_loop_opts *opts, mlh_loop_result *result);

/* ---------------------------------------------------------------- (f13) FPFH + Fast Global Registration for the loop closure, on the device
 * The step between (f11) and (f12): LoopRegistration::performGlobalRegistration (mloam_loop/src/loop_registration.cpp:18-101) -- pcl::NormalEstimation and
 * pcl::FPFHEstimationOMP over the two filtered surf clouds (cpp:46-66), then fgr::CApp (mloam_loop/ThirdParty/FastGlobalRegistration/app.cpp): NormalizePoints
 * (app.cpp:324-390), AdvancedMatching (113-320), OptimizePairwise (392-505), GetOutputTrans (519-534). Cloud 0 is the MODEL surf cloud (laser_map, pointcloud_[0]),
 * cloud 1 the DATA surf cloud (laser_cloud); T maps data into the model frame. The clouds are read where mlh_loop_build_clouds / mlh_loop_set_clouds left them
 * (`which` = MLH_LOOP_MODEL_SURF or MLH_LOOP_DATA_SURF everywhere below); no cloud crosses the bus: what leaves HBM is the mutual pairs' records (two indices and
 * two normalised points each) and a few scalars -- from mlh_fgr_register_device one 136-byte record. On the device: normals, SPFH, FPFH, NormalizePoints, the
 * 33-dimensional matching and the gather; on the host (mlh_fgr_register), in csrc/fgr_host.hpp: the tuple test and OptimizePairwise (bounded by 3 tuple_max_cnt
 * correspondences; mlh_fgr_register_device runs both on the device, from the same header's functions) and GetOutputTrans. The per-pair, per-bin, eigen33 and distance
 * arithmetic lives once, in fgr_host.hpp, for the kernels, the host tail and the tests' restatement. PCL and FLANN are not available to this project: what
 * fgr_host.hpp restates of PCL 1.8.0 (computeMeanAndCovarianceMatrix, eigen33 / computeRoots, solvePlaneParameters, flipNormalTowardsViewpoint, computePairFeatures,
 * computePointSPFHSignature, weightPointSPFHSignature) and of FLANN (the L2 functor, RadiusResultSet's strict comparison) is restated from memory of those
 * sources and could not be checked against them; the header's comment lists each.
 * Every entry: MLH_ERR_STATE while a solve submitted with mlh_*_begin is uncollected, MLH_ERR_UNSUPPORTED under a communicator; options validated by every call
 * (NULL: the defaults), MLH_ERR_INVALID on NaN or outside: finite radii > 0 and <= 1e3, div_factor finite and > 1, use_absolute_scale 0 / 1, max_corr_dist finite
 * and > 0, 0 <= iteration_number <= 10000, 0 < tuple_scale <= 1, 1 <= tuple_max_cnt <= 1000000, a threshold that is not NaN. No device allocation once the buffers
 * have grown (mlh_fgr_info_t::allocations).
 * The self-index: per cloud the grid build of the map indexes (grid.hip) over a MapGrid of the store's own -- the context's two map indexes are NOT touched -- at cell
 *   edge max(normal_radius, fpfh_radius) (x 1.001), so that the 27-cell walk is an exact radius search for both radii; one host wait (the cloud's bounds).
 *   DEPARTURE: the order of the points inside a cell is then fixed (ascending original index, one more launch) because the grid build's is not, and every sum below
 *   runs in that order: two runs give the same bits. CHOSEN: a neighbour counts when its f32 squared distance (dx dx + dy dy) + dz dz is strictly < r * r (the f32
 *   product), FLANN's RadiusResultSet; the query point itself is a neighbour, as in PCL. A cloud with a non-finite coordinate: MLH_ERR_INVALID (PCL skips such points).
 * mlh_fgr_features(which) = NormalEstimation::compute (radius search, viewpoint (0, 0, 0)) + FPFHEstimationOMP::compute for cloud `which`. An empty cloud gives zero
 *   features and success.
 *   normals: the nine sums of computeMeanAndCovarianceMatrix in f32, un-centred (PCL 1.8.0), 16 lanes per point, each lane its candidates in walk order, then a
 *     fixed butterfly (DEPARTURE: PCL sums in ascending distance order); fewer than 3 neighbours: NaN normal and curvature; eigen33 (scaled by the largest absolute
 *     coefficient, closed-form roots, eigenvector = the largest of the three row cross products) -> the smallest eigenvalue and its vector; curvature =
 *     |lambda / trace| (0 when the trace is 0); flipNormalTowardsViewpoint.
 *   SPFH: per point over its fpfh_radius neighbours but itself (by index), computePairFeatures in f32 (swap decided on acos(fabs(angle)); f3 the cosine of the
 *     source side; v = dp x n1 normalised, w = n1 x v, f2 = v . n2, f1 = atan2f(w . n2, n1 . n2); zero distance or zero |v| skips the pair); bins
 *     floor(11 ((f1 + pi) d_pi)) and floor(11 ((f + 1) 0.5)) in f64 on the f32 feature as PCL writes them, clamped to [0, 10]. Every pair adds the same hist_incr =
 *     100.f / (k - 1), so the device keeps INTEGER counts and the f32 bin value is the result of `count` sequential f32 additions of hist_incr.
 *     CHOSEN (NaN): a pair with a NaN normal on either side gives NaN features; x86 converts floor(NaN) to INT_MIN, which the clamp sends to bin 0 -- restated: a NaN
 *     feature counts in bin 0 of its block. So a non-finite normal anywhere in the support leaves every histogram FINITE, with bin 0 of the three blocks over-counted;
 *     FPFH has no non-finite output for finite clouds (a point whose only neighbour is itself has all 33 bins zero).
 *   FPFH: weightPointSPFHSignature: neighbours with squared distance 0 skipped, weight 1.f / d2, the 33 sums in neighbour (walk) order, the three block sums in PCL's
 *     interleaved order, each block scaled by float(100.0 / sum) when its sum is non-zero. One wavefront per point, one lane per bin.
 * mlh_fgr_fetch(which, what, out, k_out): a test and diagnosis entry. MLH_FGR_NORMALS: 4 f32 per point (nx, ny, nz, curvature); MLH_FGR_SPFH: int32 [n x 33] counts,
 *   and k_out (may be NULL) <- the per-point neighbour counts (the point itself included); MLH_FGR_FPFH: 33 f32 per point. MLH_ERR_STATE when that stage has not been
 *   computed (or set) for the staged cloud.
 * mlh_fgr_set_normals / mlh_fgr_set_spfh / mlh_fgr_set_features (test entries; host arrays of the cloud's size): override one stage's output so that the next can be
 *   run on exactly known inputs: mlh_fgr_spfh(which) runs SPFH + FPFH from the normals in place, mlh_fgr_fpfh(which) FPFH from the counts in place.
 *   mlh_fgr_set_features(which, n, feat) also lets a caller bring its own descriptors: n must be the cloud's size, or the cloud may be empty / unset, in which case
 *   the features alone are staged for mlh_fgr_match (n rows; mlh_fgr_register needs the points).
 * mlh_fgr_match(pairs_out, capacity, n_pairs) = AdvancedMatching up to and including the cross check (app.cpp:113-235) on the two feature sets. The i_to_j cache
 *   and the Mi / Mj walk reduce to the set of mutual nearest neighbours; the larger cloud is i (app.cpp:121-127: cloud 1 only when strictly larger); pairs come in
 *   ascending i and are un-swapped (app.cpp:309-316): pairs_out[2 e] = the model index, [2 e + 1] = the data index; at most `capacity` pairs are written, *n_pairs <-
 *   their number (min(n0, n1) always suffices). Feature distance in f32 as FLANN's L2 functor: four squared differences summed left to right, then added to the
 *   running sum; the 33rd term alone; no contraction; the exact arg-min (a tiled brute-force kernel; the fixed order rules out MFMA). CHOSEN: equal distances go to
 *   the lower index. CHOSEN: a row with a non-finite entry is never a nearest neighbour and matches nothing (the reference hands NaN to FLANN). One empty side:
 *   no pairs.
 * mlh_fgr_register = performGlobalRegistration end to end: features for both clouds unless still valid for the staged clouds and radii; NormalizePoints (DEPARTURE:
 *   mean in a fixed tree order -- 256 strided sequential chains, then a tree -- where the reference sums sequentially; the shift and the divide in f32 as written);
 *   match; the matched pairs' normalised points gathered into a pinned record; then the host tail: the tuple test (app.cpp:242-307; DEPARTURE: srand(time(NULL))
 *   is not reproducible: opts->seed feeds the generator of fgr_host.hpp, rand() % ncorr becomes next() % ncorr), OptimizePairwise(true) (f64 JTJ / JTr in
 *   correspondence order, f32 points and delta; CHOSEN: a plain Cholesky for llt(), the Z Y X product through quaternions as Eigen forms it) and GetOutputTrans.
 *   Fewer than 10 correspondences: OptimizePairwise returns at once (app.cpp:412), T = GetOutputTrans of the identity (rotation I, translation Means[0] - Means[1]);
 *   the reference then compares final_cost_normalize_, a member no constructor initialises, against the threshold: indeterminate. CHOSEN: the cost is NaN and
 *   accepted = 0. Otherwise accepted = cost <= global_registration_threshold (cpp:92). CHOSEN: an empty cloud has mean 0 (the reference divides 0 by 0, then reads
 *   data[0] of an empty feature set): no pairs, T = GetOutputTrans of the identity. Host waits: per cloud whose features are computed 1 (the bounds); 1 for the
 *   normalisation scalars, the pair count and the records.
 * mlh_fgr_register_device = mlh_fgr_register with the tail ON THE DEVICE: same contract, options, validation, gates and result struct. Behind the match, on the
 *   context's stream and with no host wait in between, four launches read the pair count where the cross check left it: the tuple test as independent trials
 *   (the generator of fgr_host.hpp is xorshift64*, a linear map over GF(2): the state in front of draw k is A^k s0, reached through a table of A^(2^b); trial t
 *   uses draws 3 t .. 3 t + 2 whatever earlier trials decided) -- a count per segment of FGR_TT_RUN x FGR_TT_TPB trials, one exclusive prefix, then an ordered
 *   emit of the accepted trials of rank < tuple_max_cnt: exactly the tuples of the sequential loop, in its order, and its n_trials -- and OptimizePairwise in one
 *   workgroup (the working q in registers up to FGR_OPT_REG_MAX correspondences, in HBM beyond). No pair record leaves HBM: one 136-byte record (the scalars, the
 *   counts, trans, the two costs) comes back, then one wait; GetOutputTrans and `accepted` are host code on that record. host_waits = 1 with the features reused.
 *   EQUAL to mlh_fgr_register: swapped, n_mutual, n_tuples, n_corres, n_trials, the tuples themselves, global_scale, start_scale, means. NOT bit-equal: the 28 f64
 *   sums of an OptimizePairwise iteration run in another order (each of 256 threads its correspondences t, t + 256, .. in index order, a butterfly per wavefront,
 *   the four wavefronts in order; the host sums sequentially) and sin / cos / sqrt are the device's; every iteration rounds delta to f32, which absorbs nearly all of
 *   it: T_relative within 1e-6, the costs within 1e-9 relative. Two runs, and two contexts, give the same bits.
 * mlh_fgr_tail_tuple_test / mlh_fgr_tail_optimize (test and diagnosis entries): host records pq [n x 6] = (p, q) of normalised points are staged as the pairs
 *   0 .. n - 1 and exactly the kernels of mlh_fgr_register_device run on them. tuple_test: corres_out [3 x n_tuples] <- indices into the records, *n_trials as
 *   mlh_fgr_result::n_trials; capacity_tuples must be at least min(tuple_max_cnt, 100 n), the most tuples the call can return (MLH_ERR_INVALID otherwise: nothing
 *   is truncated). optimize: every record is one correspondence, in its order; start_scale = StartScale (finite, > 0); trans [16] f32 row-major (TransOutput_),
 *   cost = {final_cost, final_cost_normalize}, *optimised = 0 with fewer than 10 records (identity, NaN costs). MLH_ERR_INVALID for bad options, n < 0 or a NULL
 *   output; they overwrite the pairs of the last match. A refused call changes nothing.
 * mlh_fgr_info: sizes, validity, allocations, launches of the last f13 call, bytes held. */
enum { MLH_FGR_NORMALS = 0, MLH_FGR_SPFH = 1, MLH_FGR_FPFH = 2 };
typedef struct mlh_fgr_opts {
    float normal_radius, fpfh_radius;        /* NORMAL_RADIUS, FPFH_RADIUS */
    double div_factor;                       /* DIV_FACTOR */
    int32_t use_absolute_scale;              /* USE_ABSOLUTE_SCALE */
    int32_t iteration_number;                /* ITERATION_NUMBER */
    double max_corr_dist;                    /* MAX_CORR_DIST */
    float tuple_scale;                       /* TUPLE_SCALE */
    int32_t tuple_max_cnt;                   /* TUPLE_MAX_CNT */
    double global_registration_threshold;    /* LOOP_GLOBAL_REGISTRATION_THRESHOLD */
    uint64_t seed;                           /* the tuple test's generator (default 1) */
} mlh_fgr_opts;
typedef struct mlh_fgr_result {
    double T_relative[16];                   /* row-major: GetOutputTrans().cast<double>() */
    double final_cost_normalize;             /* NaN with fewer than 10 correspondences */
    double final_cost;
    double global_scale, start_scale;        /* GlobalScale, StartScale */
    double means[6];                         /* Means[0], Means[1] */
    int32_t accepted;
    int32_t swapped;                         /* the data cloud was i */
    int32_t n_mutual, n_tuples, n_corres;    /* after the cross check; tuples accepted; correspondences = 3 n_tuples */
    int32_t n_trials;                        /* tuple-test trials run */
    int32_t host_waits;
    int32_t reserved;
} mlh_fgr_result;
typedef struct mlh_fgr_info_t {
    int32_t n[2];                            /* cloud sizes the feature buffers were last sized for (model, data) */
    int32_t have_normals[2], have_spfh[2], have_features[2];
    int32_t launches;                        /* kernel launches of the last f13 call (the grid build's own five to seven are not counted) */
    int32_t host_waits;                      /* ... and its host waits */
    int64_t allocations;                     /* device allocations of the FGR store since the context was made */
    int64_t bytes_hbm;
} mlh_fgr_info_t;
void mlh_fgr_opts_default(mlh_fgr_opts *o);  /* config_loop_realvehicle.yaml: 1.0, 1.5, 1.4, 1, 0.025, 64, 0.95, 1000, 2.0; seed 1 */
int mlh_fgr_features(mlh_ctx *ctx, int which, const mlh_fgr_opts *opts);
int mlh_fgr_spfh(mlh_ctx *ctx, int which, const mlh_fgr_opts *opts);
int mlh_fgr_fpfh(mlh_ctx *ctx, int which, const mlh_fgr_opts *opts);
int mlh_fgr_fetch(mlh_ctx *ctx, int which, int what, void *out, int32_t *k_out);
int mlh_fgr_set_normals(mlh_ctx *ctx, int which, int32_t n, const float *normals4);
int mlh_fgr_set_spfh(mlh_ctx *ctx, int which, int32_t n, const int32_t *counts, const int32_t *k);
int mlh_fgr_set_features(mlh_ctx *ctx, int which, int32_t n, const float *features);
int mlh_fgr_match(mlh_ctx *ctx, const mlh_fgr_opts *opts, int32_t *pairs_out, int32_t capacity, int32_t *n_pairs);
int mlh_fgr_register(mlh_ctx *ctx, const mlh_fgr_opts *opts, mlh_fgr_result *result);
int mlh_fgr_register_device(mlh_ctx *ctx, const mlh_fgr_opts *opts, mlh_fgr_result *result);
int mlh_fgr_tail_tuple_test(mlh_ctx *ctx, const float *pq, int32_t n, int32_t swapped, const mlh_fgr_opts *opts, int32_t *corres_out, int32_t capacity_tuples,
                            int32_t *n_tuples, int32_t *n_trials);
int mlh_fgr_tail_optimize(mlh_ctx *ctx, const float *pq, int32_t n, double start_scale, const mlh_fgr_opts *opts, float *trans, double *cost, int32_t *optimised);
int mlh_fgr_info(mlh_ctx *ctx, mlh_fgr_info_t *out);

/* ---------------------------------------------------------------- (f14) pose-graph optimisation for the loop closure, on the device
 * What consumes the verified transform of (f12) / (f13): KeyFrame::updateLoopInfo and one pass of PoseGraph::optimizePoseGraph (mloam_loop/src/pose_graph.cpp:
 * 136-147, 491-653) with the factor RelativeRTError (mloam_loop/include/mloam_loop/pose_graph.h:290-352) under ceres::QuaternionParameterization. A context keeps, per
 * keyframe and in HBM, one 176-byte record: pose_w_, last_pose_w_ (KeyFrame::updatePose, keyframe.cpp:89-93), loop_info_ (each [t, q(xyzw)], f64) and loop_index_
 * (-1: has_loop_ false); the host keeps global_index_, earliest_loop_index_ and a mirror of the loop indices. The optimisation thread with its 2 s sleep, the
 * mutexes, updatePath / publish* and the visualisation stay with the caller; savePoseGraph / loadPoseGraph are section (f17): the session image. The file
 * itself (fopen / fwrite of the image's bytes) is the caller's or the facade's. Ceres is not available to this project: its trust-region policy is the
 * project's Ceres-shaped Levenberg-Marquardt of the other solves, and what csrc/pg_host.hpp restates of Ceres 1.12 (QuaternionProduct, QuaternionRotatePoint,
 * QuaternionParameterization's Plus and Jacobian, HuberLoss, Corrector) is from memory of that source; the header's comment lists each.
 * Every entry but the bookkeeping ones: MLH_ERR_STATE while a solve submitted with mlh_*_begin is uncollected, MLH_ERR_UNSUPPORTED under a communicator.
 * mlh_pg_opts_default: max_num_iterations 5 (cpp:522), 4 sequential edges (cpp:555), t_var 0.1, q_var 0.01 (cpp:566, 581), HuberLoss(1.0) (cpp:525). Options are
 *   validated by every call that takes them (NULL: the defaults): MLH_ERR_INVALID outside 0 <= max_num_iterations <= 200, n_sequential == 4 (the band's shape is
 *   fixed), finite variances and huber_delta > 0.
 * mlh_pg_reset: forgets every keyframe (the buffers and the reserved capacity stay).  mlh_pg_info: the counts, earliest_loop_index_, the context's capacity of
 *   loop edges of one problem (max_loops: 128 until mlh_pg_reserve raises it), allocations and bytes held.
 * mlh_pg_reserve(max_loops): the largest number of loop edges one problem of this context may hold, 128 <= max_loops <= MLH_PG_LOOPS_LIMIT (1024), otherwise
 *   MLH_ERR_INVALID. Bookkeeping only: nothing is allocated (the buffers grow with the problems that come), mlh_pg_reset keeps it. The capacity is the caller's
 *   decision because of the memory behind it: Y is 6 (M - 1) x (6 L + 1) doubles, the dense stage's Gram image and factor about 2 x (6 L)^2 doubles -- at the
 *   limit, L = 1024, 0.6 GB for the dense stage and 0.3 GB of Y per 1000 keyframes. The earliest looped index never moves forward (cpp:140-142), so a run's L only
 *   grows: with loop_skip_interval 3 the 129th edge arrives after about 390 keyframes of revisit.
 *   mlh_pg_marginals (f18) holds O(M) more -- 252 doubles per keyframe and, up to 128 loops, the packed dense factor -- and reuses Y: its section has the figures.
 * mlh_pg_add_keyframe = the bookkeeping of PoseGraph::addKeyFrame (cpp:94-96): the keyframe gets index global_index_++; *index_out (may be NULL) <- it. CHOSEN:
 *   last_pose_w_ and loop_info_ start as the identity (the reference's KeyFrame leaves them default-constructed). A non-finite pose: MLH_ERR_INVALID.
 * mlh_pg_set_loop = KeyFrame::updateLoopInfo(loop_index, loop_info) plus the earliest-index rule (cpp:140-142); loadKeyFrame's loop case (cpp:187-206) is this call
 *   after an add. Requires 0 <= loop_index < index < the number of keyframes, otherwise MLH_ERR_INVALID; a second call for a keyframe overwrites the first (the
 *   earliest index never moves forward again, as in the reference).
 * mlh_pg_optimize(cur_index) = the body of cpp:505-642 with first_looped_index = earliest_loop_index_, over the M keyframes first..cur:
 *   - block `first` is constant; every keyframe gets its sequential edges to i - 1 .. i - 4 with the measurement taken from the CURRENT poses (cpp:559-563:
 *     Eigen's q.inverse() * v and q.inverse() * q, not normalised), no loss; a keyframe with a loop gets one edge (loop keyframe, keyframe) under HuberLoss;
 *   - ceres::Solve as the project's Ceres-shaped Levenberg-Marquardt: Jacobi scaling fixed at iteration 0, the clamped diagonal over the radius, the model cost
 *     change, step validity, the function / parameter / gradient tolerances, the radius update and the diagonal's reuse. Every decision is taken on the device in a
 *     state record; the launches of an iteration return at once when the solve has terminated; the number of launches (3 + 10 max_num_iterations + 1; for L > 128
 *     3 + (9 + 3 ceil(6 L / 64)) max_num_iterations + 1) does not depend on M, nor on L up to 128 (the one exception: cur == first has no free block and only the loop's head is launched per iteration, 3 + max_num_iterations + 1); ONE host wait (the summary). No floating-point atomics: two runs give the same bits;
 *   - the linear system (S H S + D / radius) y = S g is solved exactly as B + W^T W: B the block band of the sequential edges plus the diagonal (banded block
 *     Cholesky, one workgroup, a 5 x 5-block window in LDS), W the 6 L rows of the loop edges' corrected Jacobians; [Y | y_b] = L^-1 [W^T | S g] with one lane per
 *     column; C = I + Y^T Y and Y^T y_b by v_mfma_f64_16x16x4_f64 with K split over workgroups and a fixed-order second stage; C z = Y^T y_b by a dense Cholesky: for
 *     L <= 128 in one workgroup (LDS up to 84 rows, HBM beyond), exactly as before mlh_pg_reserve existed; for L > 128 (chosen by the problem's L, never by the
 *     capacity) by a blocked left-looking Cholesky over the whole device on 64-wide panels -- the partials summed by one workgroup per tile, each panel's update
 *     in v_mfma_f64_16x16x4_f64, the right-hand side carried as one more row (the forward substitution), a blocked backward substitution -- in
 *     3 ceil(6 L / 64) launches that replace the one, synchronised by kernel boundaries only; L^T x = y_b - Y z in one sweep. A non-positive pivot in B or in C, or a model cost change <= 0, makes the
 *     step invalid: the radius is halved as the policy prescribes (five in a row: termination 4);
 *   - write-back (cpp:615-641): updatePose(Pose(q, t)) on first..cur (Pose's constructor normalises q; the constant block too: its last pose becomes its pose),
 *     pose_drift = cur * last^-1 left-multiplied onto every later keyframe through updatePose. Keyframes before `first` keep their bits.
 *   *result: num_iterations, num_successful_steps, initial / final cost, termination (0 iteration limit, 1 gradient, 2 parameter, 3 function tolerance, 4 failure),
 *   M, L, first, the final radius, pose_drift, launches and host waits.
 *   MLH_ERR_STATE when no loop has been set or cur_index < earliest_loop_index_; MLH_ERR_INVALID for a cur_index that names no keyframe; MLH_ERR_UNSUPPORTED, with
 *   nothing changed, when first..cur holds more loop edges than the context's capacity (128, or what mlh_pg_reserve set; the message names it).
 *   DEPARTURE: the model cost change's quadratic term is summed per edge (|J S step|^2) rather than through the assembled matrix: the same number up to rounding.
 *   CHOSEN: cur == first (M = 1) has no free block: termination 1 at iteration 0, then the write-back.
 * mlh_pg_poses: n poses from `first` (7 doubles each) and, when last_poses is not NULL, the last poses.  mlh_pg_device_poses: the records in HBM for device
 *   consumers: *records (NULL while empty), their stride (176; the pose at offset 0, the last pose at 56, loop_info_ at 112, loop_index_ at 168) and their number.
 *   Valid until the next mlh_pg_add_keyframe.
 * Stage entries (tests and diagnosis; they leave the stored poses untouched):
 * mlh_pg_linearize(cur_index): the problem's edges at the stored poses in the reference's order (per keyframe: to i - 1 .. i - 4, then the loop edge): *n_edges;
 *   edge_ij[2 e ..] = the two local indices (0 = first); residuals[6 e ..]; Ji / Jj[36 e ..] = the 6 x 6 row-major local Jacobians over [rotation 3, translation 3] of
 *   the two endpoints, all as Ceres hands them to the linear solver (a loop edge scaled by sqrt(rho')); *cost = sum of rho / 2; for M <= 128 (beyond, with H or g
 *   not NULL: MLH_ERR_UNSUPPORTED) H (n x n row-major, n = 6 (M - 1): the band the device assembled plus W^T W formed on the host from the device's rows) and g (the
 *   device's). Arrays are sized by the caller for 5 M edges; any may be NULL.
 * mlh_pg_solve_step(cur_index, radius): one linear solve at the stored poses with the given radius: step[n] = the Jacobi-scaled LM step (-y), delta[n] = S step,
 *   *ok = 0 when a pivot failed.
 * mlh_pg_optimize_forced(cur_index, fail_mask): mlh_pg_optimize, write-back included, with the linear solve of iteration k + 1 declared FAILED when bit k of
 *   fail_mask is set, as a non-positive pivot would make it: the policy's invalid-step branch (radius /= decrease_factor, decrease_factor doubled, the diagonal
 *   reused, termination 4 after five in a row) on demand, for the tests -- well-posed graphs never take it on their own.
 * mlh_pg_time_stages(cur_index): a measurement entry (scripts/pgbench.py): the launches of mlh_pg_optimize WITHOUT the write-back, with an event recorded behind
 *   every stage; *result as mlh_pg_optimize fills it (drift: the identity), stage_ms[8] <- the milliseconds between the events, summed over the iterations:
 *   [0] linearise (begin, the initial and the candidates' linearisations), [1] assemble, [2] band factor (with the loop's head), [3] multi-column substitution,
 *   [4] Gram, [5] dense solve, [6] y_b - Y z and the back-substitution, [7] the LM bookkeeping (candidate and decisions). The events themselves cost a few
 *   microseconds of queue time each, which the figures include. */
enum { MLH_PG_STAGES = 8 };
enum { MLH_PG_LOOPS_LIMIT = 1024 };          /* the ceiling of mlh_pg_reserve */
typedef struct mlh_pg_opts {
    int32_t max_num_iterations;              /* options.max_num_iterations (cpp:522) */
    int32_t n_sequential;                    /* cpp:555: 4 */
    double t_var, q_var;                     /* cpp:566, 581 */
    double huber_delta;                      /* cpp:525 */
} mlh_pg_opts;
typedef struct mlh_pg_result {
    int32_t num_iterations, num_successful_steps;
    int32_t termination;                     /* as mlh_iter_stat::termination */
    int32_t n_keyframes, n_loops;            /* M, L of the problem */
    int32_t first_index;
    int32_t launches, host_waits;
    double initial_cost, final_cost, final_radius;
    double drift[7];                         /* pose_drift [t, q(xyzw)] */
    double solve_radius;                     /* the radius the last linear solve ran with (1e4 when none ran) */
} mlh_pg_result;
typedef struct mlh_pg_info_t {
    int32_t n_keyframes, n_loops;
    int32_t earliest_loop_index;             /* -1: none yet */
    int32_t max_loops;
    int64_t allocations;                     /* device allocations of the pose graph since the context was made */
    int64_t bytes_hbm;
} mlh_pg_info_t;
void mlh_pg_opts_default(mlh_pg_opts *o);
int mlh_pg_reset(mlh_ctx *ctx);
int mlh_pg_info(mlh_ctx *ctx, mlh_pg_info_t *out);
int mlh_pg_reserve(mlh_ctx *ctx, int32_t max_loops);
int mlh_pg_add_keyframe(mlh_ctx *ctx, const double *pose, int32_t *index_out);
int mlh_pg_set_loop(mlh_ctx *ctx, int32_t index, int32_t loop_index, const double *rel_pose);
int mlh_pg_optimize(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, mlh_pg_result *result);
int mlh_pg_poses(mlh_ctx *ctx, int32_t first, int32_t n, double *poses, double *last_poses);
int mlh_pg_device_poses(mlh_ctx *ctx, const void **records, int32_t *stride_bytes, int32_t *count);
int mlh_pg_linearize(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, int32_t *n_edges, int32_t *edge_ij, double *residuals, double *Ji, double *Jj,
                     double *cost, double *H, double *g);
int mlh_pg_solve_step(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, double radius, double *step, double *delta, int32_t *ok);
int mlh_pg_optimize_forced(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, uint32_t fail_mask, mlh_pg_result *result);
int mlh_pg_time_stages(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, mlh_pg_result *result, double *stage_ms);

/* (f1) cloudUCTAssociateToMap (lidar_mapper_keyframe.cpp:1116-1158): moves one keyframe's feature cloud into the map frame while
 * building the local map (extractSurroundingKeyFrames, cpp:254-354). Per point (intensity = LiDAR index n):
 *   with_ua: point_sel = pose_ext[n]^-1 * p; Sigma = evalPointUncertainty(point_sel, pose_global (+) pose_ext[n]) where the
 *            compound pose and its 6x6 covariance come from compoundPoseWithCov method 2 (associate_uct.hpp:90-147);
 *            points with trace(Sigma) > trace_threshold are dropped;
 *   always:  the record is copied, xyz <- pose_global * p (f64 math, f32 store), cov_vec <- Sigma (zeros without with_ua),
 *            cov_trace <- trace.
 * Output keeps the input order and record layout; `mem` describes both buffers (see mlh_voxel_filter).
 * Covariance layout: 6x6 row-major over [translation, rotation], as Pose::cov_. */
int mlh_cloud_uct_associate_to_map(mlh_ctx *ctx, const void *points, int stride_bytes, int n, int intensity_offset_bytes, int cov_offset_bytes,
                                   int trace_offset_bytes, const double pose_global[7], const double cov_global[36], const double *ext_poses,
                                   const double *ext_covs, int n_lidar, const double cov_measurement[9], int with_ua, double trace_threshold,
                                   void *out, int32_t *n_out, int mem);
/* compoundPoseWithCov(pose_1, pose_2, pose_cp, method = 2) (associate_uct.hpp:90-147), host arithmetic, f64 */
int mlh_compound_pose_with_cov(const double pose_1[7], const double cov_1[36], const double pose_2[7], const double cov_2[36],
                               double pose_cp[7], double cov_cp[36]);

/* ---------------------------------------------------------------- (f5) keyframe store + local map on the device
 * saveKeyframe (lidar_mapper_keyframe.cpp:641-683) and extractSurroundingKeyFrames (cpp:254-354) with clearCloud (cpp:921-927): the context keeps
 * the mapper's keyframes (pose with its cov_, the f32 position, the surf / corner clouds) and builds the local map from them in HBM.
 * The save / no-save decision stays with the caller (saveKeyframe's distance / orientation test; the C++ facade's KeyframePolicy restates it).
 * mlh_keyframe_save: one keyframe; pose [t, q(xyzw)] and its 6x6 covariance (cov_mapping), the two clouds as records of `stride_bytes` with xyz at
 *   offset 0 and the LiDAR id (intensity) at `intensity_offset_bytes`, in `mem`. Only xyz and the LiDAR id are kept (cloudUCTAssociateToMap recomputes
 *   the covariance, cpp:1143-1155). *key_out (may be NULL) <- the keyframe's index.
 * mlh_keyframe_save_staged: the same with the context's current feature sets (what mlh_downsample_current_scan(_pair) / mlh_features_set left),
 *   copied device to device.
 * mlh_local_map_assemble: extractSurroundingKeyFrames around pose_cur. In the reference's order:
 *   - no keyframes, or both filtered map clouds non-empty (cpp:256-261): nothing happens, *rebuilt = 0;
 *   - radiusSearch(pose_cur.t_ as f32, surrounding_kf_radius): nearest first, equal distances by index;
 *   - the cache (surrounding_existing_keyframes_id + the transformed clouds): entries that left the radius are erased (order kept), entering ones
 *     appended in search order and transformed ONCE, with the ext_poses / ext_covs of this call (cloudUCTAssociateToMap, the arithmetic of
 *     mlh_cloud_uct_associate_to_map bit for bit); a later call with other extrinsics does not re-transform cached entries;
 *   - VoxelGridCovarianceMLOAM<PointI>(map_sur_kf_res) over the cached keyframes' positions, intensity = position in the cache: the clouds of the
 *     entry each output point names are appended, in output order. REPRODUCED: keyframes that share a position voxel contribute only the voxel's
 *     last member (std::sort order) -- with the shipped configs (map_sur_kf_res 1.0, distance_keyframes 1.0) this happens often;
 *   - `+=` onto the pre-filter clouds, which only mlh_local_map_clear empties. REPRODUCED: while one kind filters to empty, every call rebuilds and
 *     appends the same keyframes again;
 *   - the two covariance filters (leaf_surf / leaf_corner, trace_threshold) through the context's voxel filter (mlh_set_voxel_member_order applies).
 *   *n_surf_ds / *n_corner_ds <- the filtered counts; kf_ids_out (may be NULL; capacity >= the number of keyframes) <- the ids appended this call, in
 *   order, *n_ids (may be NULL) their number. Two host waits per call (one more when a buffer grows); launches do not depend on the number of keyframes.
 *   Beside a solve submitted with mlh_*_begin the call is correct (it reads no map index and writes nothing a solve reads) but it is enqueued behind
 *   the solve on the context's stream and its waits include the solve.
 * mlh_local_map_cloud: the pre-filter (filtered = 0) or filtered (1) map cloud of `kind`: 48-byte PointIWithCov records in HBM
 *   {x, y, z, intensity, cov_vec[6], cov_trace, pad}, stride 48, intensity offset 12, cov offset 16, trace offset 40 -- for mlh_map_set_pair(_overlapped)
 *   (..., MLH_MEM_DEVICE). Valid until the next assemble / clear / reset.
 * mlh_keyframes_reset empties store, cache and map clouds and frees their memory (as does mlh_destroy). Outputs of mlh_local_map_info may be NULL. */
typedef struct mlh_local_map_opts {
    float surrounding_kf_radius;  /* SURROUNDING_KF_RADIUS, >= 0 */
    float map_sur_kf_res;         /* MAP_SUR_KF_RES, > 0 */
    float leaf_surf, leaf_corner; /* MAP_SURF_RES, MAP_CORNER_RES, > 0 */
    double trace_threshold;       /* TRACE_THRESHOLD_MAPPING */
    int with_ua;                  /* with_ua_flag */
    double cov_measurement[9];    /* COV_MEASUREMENT, 3x3 */
} mlh_local_map_opts;
int mlh_keyframes_reset(mlh_ctx *ctx);
int mlh_keyframe_save(mlh_ctx *ctx, const double pose[7], const double cov[36], const void *surf, int n_surf, const void *corner, int n_corner,
                      int stride_bytes, int intensity_offset_bytes, int mem, int32_t *key_out);
int mlh_keyframe_save_staged(mlh_ctx *ctx, const double pose[7], const double cov[36], int32_t *key_out);
int mlh_local_map_assemble(mlh_ctx *ctx, const double pose_cur[7], const double *ext_poses, const double *ext_covs, int n_lidar, const mlh_local_map_opts *opts,
                           int32_t *rebuilt, int32_t *n_surf_ds, int32_t *n_corner_ds, int32_t *kf_ids_out, int32_t *n_ids);
int mlh_local_map_clear(mlh_ctx *ctx);
int mlh_local_map_cloud(mlh_ctx *ctx, int kind, int filtered, const void **device_points, int32_t *n);
int mlh_local_map_info(mlh_ctx *ctx, int32_t *n_keyframes, int32_t *n_cached, int64_t *store_bytes, int64_t *cache_bytes);

/* ---------------------------------------------------------------- (f7) the global map on the device
 * pubGlobalMap (lidar_mapper_keyframe.cpp:780-851, the map part: cpp:796-849) and saveGlobalMap (cpp:853-919, without the PCD writing): THE map, built in HBM
 * from the keyframe store in one call instead of three calls and a host wait per keyframe.
 * mlh_keyframe_attach_outlier: saveKeyframe's third cloud (laser_cloud_outlier_cov, cpp:673, 677, 681), attached to an already saved keyframe. `points` is what
 *   downsampleCurrentScan left of the outlier cloud (cpp:366-368, 405-418: thinned at MAP_OUTLIER_RES, trace-gated); only xyz and the LiDAR id are kept.
 *   MLH_ERR_INVALID for a key that does not exist or bad records (as mlh_keyframe_save), MLH_ERR_STATE when the keyframe already has an outlier cloud; n == 0
 *   attaches nothing. A keyframe without one has an empty outlier cloud. The local map never reads it.
 * mlh_global_map_assemble, in the reference's order:
 *   - no keyframes (cpp:796): MLH_OK, all counts 0, *n_ids = 0;
 *   - selection (cpp:804-810): radiusSearch(pose_cur.t_ as f32, kf_radius), nearest first, equal distances by index (d2 <= r * r in f32); kf_radius < 0: no
 *     search, every keyframe in index order (saveGlobalMap, cpp:865-866). The hits, in that order, go through VoxelGridCovarianceMLOAM<PointI>(kf_res), plain
 *     branch, with intensity = the KEYFRAME'S OWN INDEX (cpp:666, 808; not a cache position as in the local map). REPRODUCED: with the shipped values (kf_res
 *     10, keyframes 1 m apart) many keyframes share a position voxel, and only each voxel's last member in std::sort order reaches the map.
 *     NOT reproduced: saveGlobalMap pushes onto global_map_keyframes without clearing what a concurrent pubGlobalMap left there (cpp:865-866), which depends
 *     on another thread's timing; kf_radius < 0 means a clean list. mlh_global_map_select is this step alone (host arithmetic, no context);
 *   - association: every selected keyframe is transformed on every call (no cache; the reference has none here) with its own stored pose and cov_ and the
 *     ext_poses / ext_covs of this call: cloudUCTAssociateToMap, the arithmetic of mlh_cloud_uct_associate_to_map bit for bit; points whose trace exceeds
 *     trace_threshold are dropped with with_ua (cpp:1147-1148), order preserved. split 0: one cloud, per keyframe surf, corner, outlier (cpp:818-827);
 *     split 1: cloud 0 = per keyframe surf, outlier, cloud 1 = per keyframe corner (cpp:872-882);
 *   - one covariance filter per output cloud at `leaf` (cpp:839-842 / 896-901) through the context's voxel filter (mlh_set_voxel_member_order applies; a grid of
 *     more than 2^31 cells returns the pre-filter cloud unchanged, as the reference does). The append order above decides the member order inside a voxel.
 *   n_pre[2] / n_ds[2] <- the pre-filter and filtered lengths of the two clouds; kf_ids_out (may be NULL; capacity >= the number of keyframes) <- the selected
 *   keyframes in append order, *n_ids (may be NULL) their number. MLH_ERR_INVALID on bad options (the finiteness rules of mlh_local_map_assemble; kf_radius may
 *   be negative), with_ua without ext_covs, n_lidar outside 1..16, a radius search without pose_cur; MLH_ERR_NOMEM beyond the point limit of the keyframe cache.
 *   Two host waits per call (one more when a buffer grows), one upload of all tables; the launches do not depend on the number of keyframes. It writes none of
 *   the local map's state. Beside a solve submitted with mlh_*_begin the call is correct but enqueued behind the solve on the context's stream, and its waits
 *   include the solve (as mlh_local_map_assemble). The context is not re-entrant: pubGlobalMap's own thread needs the caller's lock or a context of its own.
 * mlh_global_map_cloud: cloud `which` (0 / 1), pre-filter (filtered = 0) or filtered (1): 48-byte PointIWithCov records in HBM as mlh_local_map_cloud; valid
 *   until the next mlh_global_map_assemble / release / mlh_keyframes_reset.
 * mlh_global_map_release frees the global clouds (mlh_keyframes_reset and mlh_destroy do too). */
typedef struct mlh_global_map_opts {
    float kf_radius;            /* GLOBALMAP_KF_RADIUS; < 0: no search, every keyframe in index order (saveGlobalMap, cpp:865-866) */
    float kf_res;               /* leaf of down_size_filter_global_map_keyframes (10, cpp:1293), > 0 */
    float leaf;                 /* MAP_SURF_RES (cpp:839) or 2 * MAP_SURF_RES (cpp:896), > 0 */
    int32_t split;              /* 0: one cloud, per keyframe surf, corner, outlier (cpp:818-827); 1: cloud 0 = per keyframe surf, outlier; cloud 1 = corner (cpp:872-882) */
    double trace_threshold;     /* TRACE_THRESHOLD_MAPPING */
    int with_ua;
    double cov_measurement[9];
} mlh_global_map_opts;
void mlh_global_map_opts_default(mlh_global_map_opts *o, int for_save);   /* 0: pubGlobalMap's values, 1: saveGlobalMap's */
int mlh_keyframe_attach_outlier(mlh_ctx *ctx, int32_t key, const void *points, int n, int stride_bytes, int intensity_offset_bytes, int mem);
int mlh_global_map_assemble(mlh_ctx *ctx, const double pose_cur[7] /* may be NULL when kf_radius < 0 */, const double *ext_poses, const double *ext_covs, int n_lidar,
                            const mlh_global_map_opts *opts, int32_t n_pre[2], int32_t n_ds[2], int32_t *kf_ids_out, int32_t *n_ids);
int mlh_global_map_cloud(mlh_ctx *ctx, int which, int filtered, const void **device_points, int32_t *n);
int mlh_global_map_release(mlh_ctx *ctx);
/* host arithmetic, no context: which keyframes the global map is made of, in the order their clouds are appended (ids_out: capacity >= n; center may be NULL
 * when kf_radius < 0) */
int mlh_global_map_select(const float *positions_xyz, int n, const float center[3], float kf_radius, float kf_res, int32_t *ids_out, int32_t *n_ids);

/* ---------------------------------------------------------------- (f15) loop-corrected poses into the keyframe store
 * What consumes the poses of (f14): the mapper receives every keyframe's corrected pose on /loop_info (published by mloam_loop/src/pose_graph.cpp:873-910, taken
 * in at lidar_mapper_keyframe.cpp:197-201, 1082-1095) and calls updateKeyframe() (cpp:685-688) -- which in the reference is a stub that prints "received loop info,
 * need to update all keyframes" under "TODO: using loop info to update keyframes". There is nothing to reproduce; every rule here is CHOSEN:
 *   CHOSEN replacement: keys first_key .. first_key + n - 1 of the store of (f5) take poses[7 i ..] = [t, q(xyzw)] as given (not normalised); with covs != NULL
 *     also covs[36 i ..] (6 x 6 row-major, as mlh_keyframe_save), with covs == NULL the stored covariance stays -- the loop side carries no new one
 *     (publishLoopInfo sends the mapper's own cov_ back; section (f18) computes one on the device and has an entry that carries it here);
 *   CHOSEN position: the f32 position the radius searches read is recomputed as float(t), as mlh_keyframe_save computes it;
 *   CHOSEN "changed": a keyframe counts as changed when any of its 7 pose doubles -- or, with covs, any of its 36 covariance doubles -- differs BITWISE from what
 *     was stored (mlh_pg_optimize leaves the keyframes before its first looped index bit-identical, so they stay cached);
 *   CHOSEN drift tail: with drift_tail != 0 and a changed LAST key of the range, drift = new(last) * old(last)^-1 and every key beyond the range gets
 *     pose <- drift * pose (Pose::operator* and Pose::inverse as csrc/pg_host.hpp restates them, on the host): what optimizePoseGraph does to the keyframes behind
 *     cur_index (pose_graph.cpp:630-641), here for keyframes the mapper saved after the loop side's snapshot. Those keys count as changed. drift_out (may be NULL)
 *     <- the drift, or the identity when none was applied. The caller left-multiplies it onto its own pose_wmap_wodom / pose_wmap_curr;
 *   CHOSEN invalidation: with *n_changed > 0 every cached entry of a changed keyframe is erased (its slot recycled, the order of the remaining entries kept: the
 *     erase of extractSurroundingKeyFrames, cpp:274-293, with "changed" in the place of "left the radius") and both pre-filter and both filtered local-map clouds are
 *     emptied exactly as mlh_local_map_clear empties them. The next mlh_local_map_assemble rebuilds: it re-associates the erased keyframes from the store in its one
 *     batch, appended in search order behind the survivors. With *n_changed == 0 nothing is touched: the filtered clouds stay and the next assemble returns
 *     rebuilt = 0. CHOSEN: changed entries are not re-associated in place (after a real correction nearly every cached keyframe has changed, and it would need a
 *     second definition of the cache order);
 *   CHOSEN the global map: the clouds of (f7) are left as they are -- STALE until the next mlh_global_map_assemble, which transforms every selected keyframe with
 *     its stored pose on every call anyway.
 * mlh_keyframes_update_poses: the update from host arrays. Host memory only: no launch, no host wait. MLH_ERR_INVALID, with nothing changed, for a range outside
 *   the store, n <= 0, NULL poses or n_changed, a non-finite pose (what mlh_keyframe_save refuses), a non-finite covariance. Beside a solve submitted with mlh_*_begin
 *   the rule of mlh_local_map_assemble applies (the call touches nothing a solve reads).
 * mlh_keyframes_update_from_pose_graph: the same update with covs = NULL and the poses taken from pg_ctx's records in HBM (stride 176, pose at offset 0:
 *   mlh_pg_device_poses); pose-graph index first_index + i -> store key first_key + i; n < 0: every pose-graph keyframe from first_index. ONE strided
 *   device-to-pinned-host copy of 56 bytes per keyframe on ctx's stream -- ordered behind pg_ctx's stream by an event when the contexts differ (same device, as
 *   mlh_fuse_add_scan_from) --, ONE host wait, then the host rules. The call returns only after the copy has completed, so no reader event outlives it; the caller
 *   holds whatever lock guards pg_ctx, as publishLoopInfo holds m_keyframelist. MLH_ERR_INVALID, with nothing changed, for a range outside either side or an empty
 *   pose graph; MLH_ERR_STATE while pg_ctx has an uncollected solve, MLH_ERR_UNSUPPORTED when pg_ctx is under a communicator (as (f14)) or on another device.
 * mlh_keyframe_poses: what the store holds for keys first_key .. first_key + n - 1: poses (7 n), covs (36 n), positions (3 n, f32); each may be NULL. Host memory
 *   only, no wait. MLH_ERR_INVALID for a range outside the store (n == 0 is an empty read). */
int mlh_keyframes_update_poses(mlh_ctx *ctx, int32_t first_key, int32_t n, const double *poses /* 7 n */, const double *covs /* 36 n or NULL */, int drift_tail,
                               int32_t *n_changed, double drift_out[7] /* may be NULL */);
int mlh_keyframes_update_from_pose_graph(mlh_ctx *ctx, mlh_ctx *pg_ctx /* may equal ctx */, int32_t first_index, int32_t first_key,
                                         int32_t n /* < 0: all pg keyframes from first_index */, int drift_tail, int32_t *n_changed, double drift_out[7]);
int mlh_keyframe_poses(mlh_ctx *ctx, int32_t first_key, int32_t n, double *poses, double *covs, float *positions /* each may be NULL */);

/* ---------------------------------------------------------------- (f18) pose-graph marginal covariances, on the device
 * What (f14) did not hand back: the uncertainty of the corrected poses. The mapper weighs every keyframe's points by its 6 x 6 pose covariance (f1); after a loop
 * closure the poses of (f15) are consistent while the stored covariances are still what the odometry had accumulated. Nothing in the reference computes this
 * (publishLoopInfo sends the mapper's own cov_ back); every rule is CHOSEN.
 * mlh_pg_marginals(cur_index, form): the 6 x 6 diagonal blocks of H^-1, where H is exactly the matrix mlh_pg_linearize(cur_index) describes -- the problem
 *   first = earliest_loop_index_ .. cur at the STORED poses, the sequential measurements taken from those poses, loop edges Huber-corrected, block `first`
 *   constant, no Levenberg-Marquardt diagonal and no Jacobi scaling, over the tangent of the solver's Plus in the order [rotation 3, translation 3] (CHOSEN: what
 *   ceres::Covariance would give on that problem). The block of `first` is zero: that is the gauge. A stage-style entry: the stored poses, the last poses and
 *   every buffer of (f14) that outlives a call keep their bits; an optimise after it gives the bits of one without it.
 *   - form MLH_PG_COV_LOCAL: the blocks as defined. form MLH_PG_COV_STORE: each block as A Sigma A^T in the keyframe store's convention, the left perturbation
 *     T = exp(xi^) T_bar with xi = [rho, phi] of (f1): A = [[2 [t]x, I], [2 I, 0]] (rows rho, phi; columns rotation, translation; t the keyframe's stored
 *     translation), because Plus turns by the angle 2 |d_r| about d_r on the left and adds d_t: phi = 2 d_r, rho = d_t - phi x t (csrc/pg_marg_host.hpp).
 *     covs (36 M doubles, row-major, may be NULL) <- the blocks of first..cur in the form asked for. Every block is symmetric to the bit (one triangle is
 *     computed, the other copied).
 *   - the method: H = B + W^T W as (f14) splits it; B = L L^T, Y = L^-1 W^T, C = I + Y^T Y and its dense Cholesky by the kernels of (f14), fed S = 1 and a zero
 *     diagonal; then by Woodbury H^-1 = B^-1 - Z C^-1 Z^T with Z = L^-T Y: a selected inversion of the band (Takahashi's recursion, one workgroup, a 5 x 5-block
 *     window in LDS), Z by one lane per column in one backward sweep, Q = L_c^-1 Z^T by a blocked triangular solve whose panel updates run on
 *     v_mfma_f64_16x16x4_f64 (O((6 L)^2 n): where the time goes at large L), and a tail that subtracts each block's 6 x 6 Gram of Q and writes both forms. No
 *     n x n matrix is formed. Launches: 13 + 1 for L <= 128, 13 + 3 ceil(6 L / 64) beyond -- not a function of M (the one exception: cur == first, 4 launches,
 *     the one zero block, ok = 1); ONE host wait. No floating-point atomics: two runs give the same bits.
 *   - memory beyond what an optimise of the same problem holds: 72 M doubles of results, 180 (M - 1) doubles of the band's inverse and, for L <= 128, the packed
 *     dense factor (ceil(6 L / 64) * 64)^2 doubles (at most 4.7 MB; beyond 128 the blocked stage's factor is used in place) -- O(M) in all; Z and Q overwrite Y
 *     (the 0.3 GB per 1000 keyframes at L = 1024 that mlh_pg_reserve states). Allocated by the first call, grown as the others are, counted in mlh_pg_info; a
 *     context that never calls this entry holds what it held before.
 *   *result: ok (0 when a pivot of B or of C was not positive: nothing is published, covs is not written, and no earlier result stays valid), M, L, first,
 *   launches, host waits. Errors as mlh_pg_optimize: MLH_ERR_STATE without a loop, below the earliest index or beside an uncollected solve; MLH_ERR_INVALID for a
 *   cur_index that names no keyframe or an unknown form; MLH_ERR_UNSUPPORTED above the context's loop capacity or under a communicator -- each with nothing
 *   touched, an earlier valid result included.
 * mlh_pg_device_marginals: both forms in HBM for device consumers, 36 doubles per keyframe of first..cur: *cov_local, *cov_store, and the problem they belong to
 *   (*first_index, *n_keyframes; either may be NULL). The result goes stale -- both pointers NULL, *first_index -1, *n_keyframes 0 -- with mlh_pg_optimize /
 *   mlh_pg_optimize_forced, mlh_pg_set_loop, mlh_pg_reset and mlh_session_import of the pose graph; mlh_pg_add_keyframe does not invalidate it. It is not part of
 *   the session image.
 * mlh_keyframes_update_from_pose_graph_cov: mlh_keyframes_update_from_pose_graph with covariances: the strided pose copy plus ONE copy of the store-form blocks
 *   of the range, STILL ONE host wait, then the host rules of mlh_keyframes_update_poses with covs != NULL. CHOSEN rules:
 *     cov_mode MLH_KF_COV_RELATIVE: key i takes its store-form block;
 *     cov_mode MLH_KF_COV_ABSOLUTE: key i takes its block plus the stored covariance of the key that `first` maps to -- with left perturbations a common-mode
 *       error of the anchor is the same world-frame vector on every keyframe, so to first order the sum needs no adjoint (compoundPoseWithCov's method 1 with an
 *       identity transport);
 *     the key of `first` itself keeps its covariance; keys of the range before it, and the keys beyond the range (the drift tail), keep theirs.
 *   MLH_ERR_STATE when pg_ctx holds no valid marginals, or the range reaches beyond their `cur`; MLH_ERR_INVALID for an unknown cov_mode, or with
 *   MLH_KF_COV_ABSOLUTE when `first` maps to no key of the store; the other errors are (f15)'s. */
enum { MLH_PG_COV_LOCAL = 0, MLH_PG_COV_STORE = 1 };
enum { MLH_KF_COV_RELATIVE = 0, MLH_KF_COV_ABSOLUTE = 1 };
typedef struct mlh_pg_marginals_result {
    int32_t ok;                              /* 0: a pivot of B or C was not positive */
    int32_t n_keyframes, n_loops;            /* M, L of the problem */
    int32_t first_index;
    int32_t launches, host_waits;
} mlh_pg_marginals_result;
int mlh_pg_marginals(mlh_ctx *ctx, int32_t cur_index, const mlh_pg_opts *opts, int32_t form, double *covs /* 36 M, row-major, or NULL */,
                     mlh_pg_marginals_result *result);
int mlh_pg_device_marginals(mlh_ctx *ctx, const double **cov_local, const double **cov_store, int32_t *first_index, int32_t *n_keyframes);
int mlh_keyframes_update_from_pose_graph_cov(mlh_ctx *ctx, mlh_ctx *pg_ctx /* may equal ctx */, int32_t first_index, int32_t first_key,
                                             int32_t n /* < 0: all pg keyframes from first_index */, int drift_tail, int32_t cov_mode, int32_t *n_changed,
                                             double drift_out[7]);

/* ---------------------------------------------------------------- (f16) the initial extrinsic calibration, on the device
 * InitialExtrinsics (estimator/src/initial/initial_extrinsics.h:34-40, initial_extrinsics.cpp:20-22, 26-116, 119-241, 243-309) as Estimator::process drives it while
 * ESTIMATE_EXTRINSIC == 2 (estimator/src/estimator/estimator.cpp:437-467): the relative poses of one mlh_track_cloud per LiDAR go to mlh_initext_add_pose, and
 * mlh_initext_calibrate solves the hand-eye problem for every LiDAR that has no rotation yet; what it returns seeds the extrinsics that the window solve of
 * (f8)-(f10) refines. A context keeps in HBM: Q_ (n_lidar x 1200 x 4 f64, row-major), v_pose_ (300 x n_lidar x 7 f64, each pose [t, q(xyzw)]) and one result
 * record per LiDAR (calib_ext_'s q and t, the singular values, the flags); on the host the options, the heap pq_pose_ (std::priority_queue under the reference's own
 * comparator), pose_laser_add_, cov_rot_state_ / cov_pos_state_ and a mirror of calib_ext_. saveStatistics, decomposeE, calibTimeDelay (empty in the reference),
 * evalCalib / computeMeanPose stay with the caller. Eigen is not available to this project: csrc/initext_host.hpp lists what is restated from memory of Eigen 3.3.
 * Quaternions of this section are (x, y, z, w), Eigen's coefficient order.
 * Reproduced (csrc/initext_host.hpp has the list with the lines): rotCmp reads LiDAR 0's w, not idx_ref's; Q_'s block is written only by a rotation stage and only
 *   for the set last accepted; a rotation stage without a new accepted set rewrites that block with the Huber weight of the moment; b and w are not weighted while A
 *   and G are; rot_cov(1) is the second-smallest singular value; the sign rule `if (x[0] < 0) x = -x` acts on the quaternion's x component; a heap smaller than
 *   window_size returns before anything is written.
 * Chosen: abs is the double overload; mlh_initext_reset also empties the heap (the reference's clearState forgets to); non-finite poses are refused; the 4 x 4 block
 *   is computed on the host (so that its bits do not depend on the device's atan2) and travels as a kernel argument; a LiDAR list may not name idx_ref.
 * mlh_initext_opts_default: n_lidar 2, idx_ref 0, planar_movement 0, window_size 4, n_pose 300 (cpp:22), eps_r 0.05, eps_t 0.1 (cpp:20-21), rot_cov_thre 0 (= the
 *   rule of cpp:58: 0.05 planar, 0.25 otherwise), QBL the identity, TBL zero.
 * mlh_initext_reset = clearState + setParameter: validates the options (NULL: the defaults; MLH_ERR_INVALID outside 1 <= n_lidar <= 8, 0 <= idx_ref < n_lidar,
 *   1 <= window_size, 1 <= n_pose <= 300, finite positive eps and finite rot_cov_thre >= 0, finite QBL / TBL with non-zero quaternions), sizes and clears the state.
 *   The only call of this section that allocates; every other one returns MLH_ERR_STATE before it.
 * mlh_initext_add_pose = addPose (cpp:79-102): checkScrewMotion of every LiDAR against idx_ref on the host; an accepted set takes slot pq_pose_.size() or, once
 *   n_pose sets are held, the slot of the heap's top, and goes to HBM as the argument of one small launch (no copy, no host wait). *accepted <- 0 / 1.
 * mlh_initext_calibrate = for each of the n listed LiDARs (distinct, not idx_ref), with stages MLH_INITEXT_ROT: calibExRotation (cpp:119-241); MLH_INITEXT_TRANS:
 *   calibExTranslation (cpp:243-309) with the rotation calib_ext_ holds; both: the call site's nesting -- the translation runs only where this call's rotation
 *   converged, the decision rot_cov(1) > rot_cov_thre_ being taken on the device. ONE launch (one workgroup of 256 per LiDAR), ONE device-to-pinned copy of the
 *   records, ONE host wait, whatever n. Singular values by one-sided (Hestenes) Jacobi on the tall matrices themselves (csrc/svd_dev.hpp), fixed summation order, no
 *   atomics: two runs give the same bits. out[i] describes lidars[i]. While the heap holds fewer than window_size sets a rotation stage does nothing (rot_ran 0; with
 *   nothing else to do the call launches nothing). cov_rot_state_ / cov_pos_state_ follow setCovRotation / setCovTranslation.
 *   MLH_ERR_INVALID, with nothing changed, for a bad list or stages.
 * mlh_initext_info: counts, flags, bytes, allocations since the context was made, launches and host waits of the last add_pose / calibrate.
 * mlh_initext_read_state (tests): Q (n_lidar x 1200 x 4), sets (300 x n_lidar x 7), calib_ext (n_lidar x 7 as [t, q(xyzw)]); each may be NULL. */
enum { MLH_INITEXT_ROT = 1, MLH_INITEXT_TRANS = 2 };
enum { MLH_INITEXT_MAX_LIDAR = 8, MLH_INITEXT_N_POSE = 300 };
typedef struct mlh_initext_opts {
    int32_t n_lidar, idx_ref, planar_movement, window_size;
    int32_t n_pose, reserved;                /* N_POSE (cpp:22) */
    double eps_r, eps_t;                     /* EPSILON_R, EPSILON_T (cpp:20-21) */
    double rot_cov_thre;                     /* 0: cpp:58 */
    double qbl[MLH_INITEXT_MAX_LIDAR][4];    /* QBL (x, y, z, w) */
    double tbl[MLH_INITEXT_MAX_LIDAR][3];    /* TBL */
} mlh_initext_opts;
typedef struct mlh_initext_result {
    double q[4];                             /* calib_ext_[lidar].q_ (x, y, z, w) */
    double t[3];                             /* calib_ext_[lidar].t_ */
    double rot_sv[4];                        /* singular values of Q_[lidar], descending; rot_cov(1) = rot_sv[2] */
    double trans_sv[4];                      /* of A (three; [3] = 0) or G (four), descending */
    int32_t lidar;
    int32_t rot_ran, rot_converged;          /* calibExRotation got past the window check; returned true */
    int32_t trans_solved, trans_rank;        /* calibExTranslation ran; the rank Eigen's solve would use */
    int32_t rot_sweeps, trans_sweeps;        /* Jacobi sweeps, the last (rotation-free) one included */
    int32_t slot;                            /* pose_laser_add_.first the rotation stage wrote (-1: none) */
} mlh_initext_result;
typedef struct mlh_initext_info_t {
    int32_t configured, n_lidar;
    int32_t n_sets, heap_size;               /* v_pose_.size(), pq_pose_.size() */
    int32_t last_slot;                       /* pose_laser_add_.first (-1: nothing accepted yet) */
    int32_t cov_rot_mask, cov_pos_mask;      /* bit n: cov_rot_state_[n], cov_pos_state_[n] */
    int32_t full_cov_rot, full_cov_pos;
    int32_t launches, host_waits;            /* of the last mlh_initext_add_pose / mlh_initext_calibrate */
    int32_t reserved;
    int64_t allocations, bytes_hbm;
    double rot_cov_thre;                     /* rot_cov_thre_ in force */
} mlh_initext_info_t;
void mlh_initext_opts_default(mlh_initext_opts *o);
int mlh_initext_reset(mlh_ctx *ctx, const mlh_initext_opts *opts);
int mlh_initext_add_pose(mlh_ctx *ctx, const double *poses /* n_lidar x 7 */, int32_t *accepted);
int mlh_initext_calibrate(mlh_ctx *ctx, const int32_t *lidars, int32_t n, int32_t stages, mlh_initext_result *out /* n */);
int mlh_initext_info(mlh_ctx *ctx, mlh_initext_info_t *out);
int mlh_initext_read_state(mlh_ctx *ctx, double *Q, double *sets, double *calib_ext);

/* ---------------------------------------------------------------- (f8) the odometry's sliding window on the device
 * The estimator keeps, per LiDAR and kind, a CircularBuffer<PointICloud> of WINDOW_SIZE + 1 slots (surf_points_stack_[n], corner_points_stack_[n]); before every
 * optimizeMap it thins the new scan's features into slot cir_buf_cnt_ (estimator/src/estimator/estimator.cpp:485-496), slides the window (slideWindow,
 * cpp:1521-1536) and rebuilds one local map per LiDAR (buildLocalMap, cpp:1159-1204; buildCalibMap, cpp:1067-1110). Here the stacks live in HBM as float4 records
 * {x, y, z, intensity} (stride 16, intensity offset 12: the layout mlh_fused_cloud hands out) and the maps are built from them in one call.
 * mlh_window_reset: empties the store and sizes it for n_lidar (1..16) LiDARs and window_size (1..16); called again it starts over. mlh_destroy frees it.
 *   Every other window call returns MLH_ERR_STATE before it.
 * mlh_window_set: stack[lidar][slot] = the two clouds (cpp:489, 494, for a caller that thinned them itself); slot is the LOGICAL index 0..window_size, as the
 *   reference's operator[]. Host or device records; n == 0 stores an empty cloud (its pointer may be NULL). A host cloud has been read when the call returns.
 * mlh_window_set_from_scan: cpp:487-495 device to device for the scan `src` holds after mlh_extract_run + mlh_extract_voxel_run (and mlh_scan_undistort, if the
 *   caller ran it): its less-sharp points through pcl::VoxelGrid at leaf_corner (0.2, cpp:74), its voxel-thinned less-flat cloud through pcl::VoxelGrid at
 *   leaf_surf (0.4, cpp:73), the arithmetic of mlh_voxel_grid. src == ctx is the plain case; another context of the same device follows mlh_fuse_add_scan_from's
 *   rules (src idle, ordered by the same two events: whatever rewrites src's scan next waits for this call's reads).
 * mlh_window_slide: slideWindow's stack.push(stack[src_slot]) for every LiDAR and both kinds, with CircularBuffer's semantics (utility/CircularBuffer.h:61-67,
 *   134-137, 186-197), which are not a plain shift: while fewer than window_size + 1 pushes have happened, the copy of logical slot src_slot goes to PHYSICAL slot
 *   `size` and nothing moves; from then on it overwrites the oldest slot and the start advances, so logical i becomes i - 1 and the new last slot is a copy of the
 *   old src_slot. operator[] is (start + i) % capacity throughout. REPRODUCED: the INITIAL phase (cpp:505-513) with its push of a still-empty slot and the state in
 *   which the last two slots hold the same cloud. A slide copies no points: slots name reference-counted ranges of an arena.
 * mlh_window_cloud: logical slot's cloud of `kind` in HBM for mlh_features_set(..., MLH_MEM_DEVICE); *device_points is NULL when *n == 0. Valid until the next
 *   mlh_window_set* / _slide / _reset.
 * mlh_window_info (outputs may be NULL): allocations = device allocations the store and its maps have made since mlh_window_reset; in steady state -- set + slide +
 *   build on clouds no larger than those seen before -- it stops growing. bytes_used: the records the slots name; bytes_reserved: the store's device memory.
 * mlh_window_build_local_map: pose_local = n_lidar x (window_size + 1) x 7 doubles [t, q(xyzw)], the reference's pose_local_[n][i] (cpp:1181: the Pose of
 *   T_pivot^-1 T_i T_ext), computed by the caller; each is used exactly as mlh_transform_point_cloud uses its pose. In the reference's order:
 *   - per LiDAR n and kind, slots 0 .. window_size - 1 (slot window_size is skipped, cpp:1182) of LiDAR n's stacks (source_lidar < 0: buildLocalMap,
 *     cpp:1185-1191) or of LiDAR source_lidar's stacks with ITS pose_local rows, for every n (buildCalibMap, cpp:1095-1101, IDX_REF) are transformed and
 *     appended in slot order to LiDAR n's pre-filter cloud: ONE launch for all n_lidar x window_size x 2 segments (256-point tiles, a tile never straddles a
 *     segment, empty segments have none), the arithmetic of mlh_transform_point_cloud bit for bit, intensity copied, the stacks untouched;
 *   - each of the 2 n_lidar pre-filter clouds through pcl::VoxelGrid<PointI> at its leaf (cpp:1103-1109, 1195-1203), the arithmetic of mlh_voxel_grid; an empty
 *     cloud filters to an empty cloud; a grid of more than 2^31 cells returns the input.
 *   n_pre / n_ds [2 n_lidar] <- the lengths, index 2 n + kind. One transform launch, one upload of all tables and two host waits per call (the clouds' bounds; the
 *   filtered counts), whatever window_size and the clouds' sizes are; 2 n_lidar voxel filters.
 * mlh_window_map_cloud: LiDAR `lidar`'s pre-filter (filtered = 0) or filtered (1) map of `kind` in HBM, for mlh_map_set_pair(..., MLH_MEM_DEVICE); NULL when
 *   *n == 0. Valid until the next build or reset.
 * MLH_ERR_INVALID (text in mlh_last_error) for a LiDAR or slot out of range, bad records, non-finite or non-positive leaves, a source_lidar out of range, a null
 * or non-finite pose_local. A failed call leaves the store as it was. */
typedef struct mlh_window_map_opts {
    int32_t source_lidar;       /* < 0: every LiDAR's map from its own stacks (buildLocalMap); >= 0: every map from this LiDAR's stacks (buildCalibMap's IDX_REF) */
    float leaf_surf[16];        /* per LiDAR, > 0. buildLocalMap: one ratio for all (cpp:1196, 1200); buildCalibMap: 0.4 for IDX_REF, 0.2 for the others (cpp:1103) */
    float leaf_corner[16];
} mlh_window_map_opts;
/* buildLocalMap's values: source_lidar -1, every leaf 0.4 * min(2, max(0.75, n_scans * n_lidar * window_size / 192)) (cpp:1196) */
void mlh_window_map_opts_default(mlh_window_map_opts *o, int n_scans, int n_lidar, int window_size);
int mlh_window_reset(mlh_ctx *ctx, int n_lidar, int window_size);
int mlh_window_set(mlh_ctx *ctx, int lidar, int slot, const void *surf, int n_surf, const void *corner, int n_corner, int stride_bytes, int intensity_offset_bytes,
                   int mem);
int mlh_window_set_from_scan(mlh_ctx *ctx, mlh_ctx *src, int lidar, int slot, float leaf_surf, float leaf_corner);
int mlh_window_slide(mlh_ctx *ctx, int src_slot);
int mlh_window_cloud(mlh_ctx *ctx, int lidar, int slot, int kind, const void **device_points, int32_t *n);
int mlh_window_info(mlh_ctx *ctx, int32_t *n_lidar, int32_t *window_size, int64_t *pushes, int64_t *bytes_used, int64_t *bytes_reserved, int64_t *allocations);
int mlh_window_build_local_map(mlh_ctx *ctx, const double *pose_local, const mlh_window_map_opts *opts, int32_t *n_pre, int32_t *n_ds);
int mlh_window_map_cloud(mlh_ctx *ctx, int lidar, int kind, int filtered, const void **device_points, int32_t *n);

/* ---------------------------------------------------------------- (a5) local map index
 * replaces pcl::KdTreeFLANN<PointT>::setInputCloud(cloud) as used at
 *   estimator/src/lidarMapper/lidar_mapper_keyframe.cpp:433-434 (and estimator.cpp:1095-1109, 1230-1233).
 * Builds a dense cell grid (cell edge just above sqrt(min_match_sq_dis), so the 27-cell neighbourhood is exact for
 * the acceptance test "5th neighbour sq-dist < min_match_sq_dis", feature_extract.hpp:667/814) over the cloud
 * and keeps the points cell-sorted in HBM as float4 {x, y, z, original index}.
 * mlh_map_rebuild re-runs the index build on the resident cloud(s) (the reference rebuilds every frame); kind may be
 * MLH_ALL_KINDS to rebuild both maps in one set of fused launches.
 */
int mlh_map_set(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, float min_match_sq_dis, int mem);
/* the two setInputCloud calls of a mapper frame (lidar_mapper_keyframe.cpp:433-434) in one set of launches and one host hand-shake.
 * The grid box of a kind is laid out with a margin when it is first computed; while later clouds keep fitting it (the local map is a
 * sliding keyframe window) a call costs pack + index build only, and returns as soon as the pack pass has reported that the clouds fit (the index build is still
 * running on the context's stream then; every later call is ordered behind it) -- a cloud that has outgrown the box is detected on the
 * device and takes the bounds pass again. Results never depend on which way a call went (the grid is an acceleration structure only). */
int mlh_map_set_pair(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                     float min_match_sq_dis, int mem);
/* The same, for the NEXT frame while a solve submitted with mlh_gn_solve_begin is still running: the maps are double-buffered, this call stages and indexes
 * into the set the solve does not read, on a second stream, returns when that index is complete and makes the set current -- launches enqueued afterwards (the
 * next mlh_gn_solve_begin) read it; the solve in flight keeps the old one (one solve in flight at this point: collect the older one first). Called a second
 * time beside the SAME uncollected solve, its target is the set that solve reads: the call then waits for the main stream to run dry before it rewrites the set
 * (correct, no longer overlapped).
 * The GPU then builds the next index (a chain of small launches) in the shadow of the current frame's iterations. What the caller must know: in the reference the
 * local map of frame k + 1 depends on frame k's optimised pose in one place -- extractSurroundingKeyFrames (lidar_mapper_keyframe.cpp:254-354) picks the keyframes
 * within a radius of the PREDICTED pose of frame k + 1, which carries frame k's map-to-odometry correction (cpp:145-160). A caller that stages this early selects
 * with the correction of frame k - 1 and re-checks the selection when frame k's pose arrives (a radius test over the keyframe positions on the host); the set
 * changes only when a keyframe sits within the change of the correction (sub-centimetre) of the radius, and then the frame is staged and solved again
 * synchronously. INTEGRATION.md section 2 spells the loop out.
 * Without a solve in flight and with device-resident clouds the same call overlaps the index build with whatever the main stream is doing that reads no map --
 * a frame's own front end: call it after the frame's upload / extraction / fusion have been enqueued and before the first call that waits for them
 * (mlh_fused_cloud); the host then waits for the build instead of for the front end, and scan2MapOptimization finds the index ready (the local map is made of
 * earlier keyframes: it does not depend on the scan being processed). Without a solve in flight and with host-resident clouds: mlh_map_set_pair. */
int mlh_map_set_pair_overlapped(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                                float min_match_sq_dis, int mem);
int mlh_map_rebuild(mlh_ctx *ctx, int kind);
/* diagnostics of the resident index (no reference counterpart: pcl::KdTreeFLANN exposes nothing of the kind): points, non-empty grid
 * cells, the population of the cell an average map point lives in (sum of squared cell populations / n), and the lanes per query the
 * correspondence kernel will use for this kind with the staged feature sets (8 or 16; chosen from the launch size and that density --
 * a tuning decision, results do not depend on it). Any output pointer may be null. */
int mlh_map_info(mlh_ctx *ctx, int kind, int32_t *n_points, int32_t *occupied_cells, double *mean_cell_population, int32_t *knn_lanes);
/* k-NN against the resident map (pcl::KdTreeFLANN::nearestKSearch role; feature_extract.hpp:666, 813):
 * queries are xyz triples (HOST), outputs idx[nq*k] (original map indices, ascending distance, ties by index) and
 * sqdist[nq*k]; slots beyond the number of points found inside the 27-cell neighbourhood are -1 / +inf. k = 5.
 * EXACT ONLY INSIDE THE ACCEPTANCE RADIUS: the search covers the 27 cells around the query (cell edge 1.001 * sqrt(min_match_sq_dis)),
 * so indices and distances equal a kd-tree's for every neighbour with sqdist < min_match_sq_dis -- all the mapper looks at
 * (sq_dis[k-1] < MIN_MATCH_SQ_DIS, hpp:667/814). A returned neighbour with sqdist >= min_match_sq_dis may be farther than a map
 * point just outside the 27 cells; a caller that needs exact neighbours beyond that radius must stage the map with a larger
 * min_match_sq_dis. */
int mlh_knn(mlh_ctx *ctx, int kind, const float *queries_xyz, int nq, int k, int32_t *idx, float *sqdist);

/* ---------------------------------------------------------------- scan features (the cloud_data / laser_cloud argument)
 * stages a feature cloud (PointIWithCov role). cov_offset_bytes: byte offset of cov_vec[6] (cxx cxy cxz cyy cyz czz, f32)
 * inside a record, or -1 when the records carry no covariance (then trace = 0 -> weight 1, lidar_map_factor.hpp:41).
 * intensity_offset_bytes: byte offset of the f32 intensity (= LiDAR index, visualization.cpp:48), or -1.
 */
int mlh_features_set(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, int intensity_offset_bytes,
                     int cov_offset_bytes, int mem);

/* Pose blocks (a19, BASELINE config 4: online extrinsic calibration). The estimator's calibration problem
 * (estimator.cpp:656-780, buildCalibMap :1067-1157) gives every LiDAR its own 7-parameter block: the reference LiDAR's features
 * constrain the body pose (LidarPureOdom* blocks with the pivot and the reference extrinsic held constant), LiDAR n's features
 * constrain its extrinsic alone (LidarOnlineCalib{PlaneNorm,Edge}Factor, lidar_online_calib_factor.hpp:24-165 -- the same
 * residual/Jacobian form as the map factors with sqrt_info = 1). Stage the feature cloud of block 0, 1, ... in ascending order;
 * every block starts on a 256-feature boundary in HBM so that a workgroup never straddles two pose blocks. */
int mlh_features_set_block(mlh_ctx *ctx, int kind, int block, const void *points, int stride_bytes, int n, int cov_offset_bytes, int mem);

/* ---------------------------------------------------------------- (a4, a6-a11, a15) match + linearise + reduce
 * replaces, for every staged feature of `kind`, at pose `pose`:
 *   pointAssociateToMap                         estimator/src/utility/utility.h:103-117
 *   FeatureExtract::match{Surf,Corner}PointFromMap / match{Surf,Corner}FromMap   feature_extract.hpp:379-883
 *   LidarMapPlaneNormFactor / LidarMapEdgeFactor ctor + Evaluate                  lidar_map_factor.hpp:28-71, 132-174
 *   ActiveFeatureSelection::evaluateFeatJacobianMatching                           lidar_mapper.h:130-174
 *   the J^T J / J^T r accumulation of evalHessian / Ceres' evaluator              lidar_mapper_keyframe.cpp:575-581, 1160-1169
 * Dense outputs (HOST, nullable), in feature order:
 *   valid[m]  1 when the feature found a correspondence (the bool return of match*PointFromMap)
 *   coeffs[m*6]  PointPlaneFeature::coeffs_ : surf = (n_hat, d, 0, 0); corner = (X1, X2)
 *   r[m], J[m*6] the factor's residual and first 6 Jacobian columns (weighted by sqrt_info, NOT loss-corrected)
 * Reduced outputs (HOST, nullable): JtJ[36] row-major, Jtr[6], cost (sum 0.5*rho), n_valid -- rows are Huber-corrected
 * as Ceres' ResidualBlock::Evaluate does (huber_delta <= 0 or MLH_FLAG_NO_LOSS: trivial loss).
 */
int mlh_match_linearize(mlh_ctx *ctx, int kind, const double pose[7], int k_neigh, uint32_t flags,
                        float min_match_sq_dis, float min_plane_dis, double huber_delta, double cov_measurement_trace,
                        uint8_t *valid, double *coeffs, double *r, double *J,
                        double *JtJ, double *Jtr, double *cost, int32_t *n_valid);

/* Re-linearise the correspondences found by the last mlh_match_linearize of `kind` at a new pose
 * (what ceres::Solve does on every LM iteration: CostFunction::Evaluate on fixed factors). Same outputs. */
int mlh_linearize(mlh_ctx *ctx, int kind, const double pose[7], uint32_t flags, double huber_delta, double cov_measurement_trace,
                  double *r, double *J, double *JtJ, double *Jtr, double *cost, int32_t *n_valid);

/* the correspondences of `kind` currently live on the device (after mlh_match_linearize, or -- only the selected ones -- after
 * mlh_good_feature_matching): valid[m], coeffs[m x 6] (PointPlaneFeature::coeffs_: plane n, d / line X1, X2; zeros where invalid) */
int mlh_match_coeffs(mlh_ctx *ctx, int kind, uint8_t *valid, double *coeffs, int32_t *n_valid);
/* Test and diagnosis aid, no reference counterpart: the neighbour records the most recent correspondence launch of `kind` left on the device (after
 * mlh_match_linearize, mlh_gn_solve*, mlh_scan2map*: the LAST iteration's search), copied as they stand. records_out (HOST, may be NULL to ask for the stride
 * only): m x stride records of four floats {x, y, z, squared distance} -- the K nearest map points of feature slot f at records_out[(f * stride + t) * 4],
 * t = 0 .. K - 1 ascending by (squared distance, map index), {0, 0, 0, +inf} where the search left none (a feature with fewer than K points in its 27 cells has
 * none at all). *k_stride_out (may be NULL) <- stride, the records per feature slot (5, or 10 once a launch asked for K = 10). Slots t >= K of a feature, the
 * padding slots between pose blocks and the features this rank does not own hold whatever was there before. Waits for the context's stream, then copies:
 * no launch, nothing on a hot path. MLH_ERR_STATE when no correspondence launch of this kind has run since its map or features were last staged. */
int mlh_match_neighbours(mlh_ctx *ctx, int kind, float *records_out, int32_t *k_stride_out);

/* ---------------------------------------------------------------- (a13) good-feature selection
 * replaces ActiveFeatureSelection::goodFeatureMatching (estimator/src/lidarMapper/lidar_mapper.h:229-573).
 * ALL features of `kind` are matched and their weighted, un-corrected 1x6 Jacobians evaluated on the GPU in one pass
 * (what match*PointFromMap + evaluateFeatJacobianMatching produce one feature at a time, lidar_mapper.h:130-174, 483-521); the
 * inherently sequential draw loops -- rnd, stochastic-greedy logdet (gd_fix, gd_float) -- then run on the host
 * over those rows with the reference's draw sequence (std::mt19937 + uniform_int_distribution, common/random_generator.hpp:53;
 * the MAX_FEATURE_SELECT_TIME wall-clock cut-off is not applied); fps draws one number (its starting point) and its
 * farthest-point arg-max loop runs on the device for up to 16384 features (same f32 arithmetic, lowest index among equal
 * distances; a round re-measures only the buckets of points the new pick can change -- the same picks, 1 us per round; inside
 * mlh_scan2map the two kinds' loops run side by side), the host replaying selection list and information matrix along the visiting order. sub_mat_H must come in as the reference initialises it
 * (1e-6 * I, cpp:505/520) and returns H + sum j^T j of the selected rows. On return only the selected features stay valid
 * on the device, so mlh_linearize / the LM of mlh_scan2map see exactly the residual blocks the reference would add.
 * fps asked for more features than match (gf_ratio * n above the number of matching features): the reference's loop has no "every point visited" exit
 * (lidar_mapper.h:391-399), so once everything has been visited it matches feature 1 again on every further round and -- when that feature matches -- appends it,
 * with its J^T J, until the count is reached. Reproduced: sel_out then ends in repeats of index 1, sub_mat_H holds its outer product as many times, and on the
 * device the feature weighs as that many residual blocks. (When feature 1 does not match, the reference spins into its 20 ms cut-off and returns what it has: the
 * same list, without the wait.) */
enum { MLH_GF_WO = 0, MLH_GF_RND = 1, MLH_GF_FPS = 2, MLH_GF_GD_FIX = 3, MLH_GF_GD_FLOAT = 4 };
int mlh_good_feature_matching(mlh_ctx *ctx, int kind, const double pose[7], int gf_method, double gf_ratio, uint64_t seed,
                              float min_match_sq_dis, float min_plane_dis, int32_t *sel_idx, int32_t *n_sel,
                              double sub_mat_H[36], uint8_t *matched);

/* ---------------------------------------------------------------- (a16, a17) device-resident solvers
 * Common options. */
typedef struct mlh_solver_opts {
    float min_match_sq_dis;          /* MIN_MATCH_SQ_DIS, parameters.cpp:232 */
    float min_plane_dis;             /* MIN_PLANE_DIS,    parameters.cpp:233 */
    double huber_delta;              /* ceres::HuberLoss(0.1), lidar_mapper_keyframe.cpp:443 */
    double map_eig_thre;             /* MAP_EIG_THRE, evalDegenracy, lidar_mapper_keyframe.cpp:1178-1189 */
    double cov_measurement_trace;    /* trace(COV_MEASUREMENT) used when with_ua is off (cpp:543-544) */
    uint32_t flags;                  /* MLH_FLAG_WITH_UA | MLH_FLAG_CHECK_FOV | MLH_FLAG_POSE_COV (the mlh_scan2map* entry points only: mlh_scan2map_cov). CHECK_FOV applies to mlh_gn_solve* (estimator.cpp:1142, 1149 pass it); the mlh_scan2map*
                                      * entry points ignore it, as scan2MapOptimization does: its matching goes through goodFeatureMatching, which hard-codes
                                      * n_neigh = 5 and CHECK_FOV = false (lidar_mapper.h:256-283) */
    int max_outer;                   /* max_iter = 2, cpp:439 */
    int max_lm_iterations;           /* options.max_num_iterations = 30, cpp:590 */
    int gf_method;                   /* FLAGS_gf_method: MLH_GF_* (lidar_mapper.h:89); mlh_scan2map only */
    double gf_ratio;                 /* gf_ratio_cur (cpp:474-492) */
    uint64_t gf_seed;                /* the reference seeds its mt19937 from std::random_device; fixed here */
} mlh_solver_opts;
void mlh_solver_opts_default(mlh_solver_opts *o);

/* per-iteration record written by the solvers (HOST array provided by the caller) */
typedef struct mlh_iter_stat {
    int32_t n_surf, n_corner;        /* matched features of each kind */
    int32_t is_degenerate;
    int32_t lm_iterations;           /* scan2map only */
    int32_t successful_steps;        /* scan2map only */
    int32_t termination;             /* scan2map only: 0 max-iters 1 gradient 2 parameter 3 function 4 failure */
    double cost;                     /* cost at the linearisation point (GN) / initial cost (scan2map) */
    double final_cost;               /* scan2map only */
    double eigval[6];
    double H[36];                    /* J^T J at the start of the iteration (evalHessian) */
    double g[6];
    double pose_after[7];
} mlh_iter_stat;

/* n_iters Gauss-Newton iterations, entirely on the device (no host round trip inside): per iteration re-match both
 * kinds at the current pose, linearise with Huber correction, reduce J^T J / J^T r, evalDegenracy
 * (lidar_mapper_keyframe.cpp:1172-1204), solve H d = -g, pose <- PoseLocalParameterization::Plus(pose, V_update d)
 * (pose_local_parameterization.cpp:26-45). This is BASELINE.json's "GN iteration". stats may be NULL. */
int mlh_gn_solve(mlh_ctx *ctx, double pose_inout[7], int n_iters, const mlh_solver_opts *opts, mlh_iter_stat *stats);
/* How the iterations of mlh_gn_solve / mlh_gn_solve_begin* are laid out on the device. Neither switch changes a result (same arithmetic in the same order; the
 * tests compare the variants bit for bit); they exist for A/B measurements and as the reference forms in the tests. This call is the only way to set them.
 *   deferred_finish 1 (default): on one GPU, without per-iteration statistics and for frame-sized launches (at most 160 fit tiles = 40 960 feature slots; larger
 *       launches keep the classic form, where the redundant sums would cost more than the serial tail they replace), every iteration but the last leaves the J^T J / J^T r records of its tiles in HBM and
 *       the NEXT iteration's correspondence launch starts by summing them, solving and applying Plus in every workgroup redundantly (the kernel boundary is the only
 *       synchronisation); 0: the fit kernel's last-arriving workgroup finishes every iteration (evalHessian + evalDegenracy + solve + Plus,
 *       lidar_mapper_keyframe.cpp:575-596, 1160-1204) while the other compute units wait.
 *   final_in_successor 1 (default; needs deferred_finish): a solve submitted with mlh_gn_solve_begin* leaves its LAST iteration as records too. The next
 *       mlh_gn_solve_begin_chained completes it in its first correspondence launch -- sum, solve, Plus, the pose published to that solve's host record and stored as the
 *       state's pose from there, then this frame's chained start pose (lidar_mapper_keyframe.cpp:145-160) computed in the same prologue: neither the serial finish nor
 *       the chain launch stand between two frames. mlh_gn_solve_end, or any other solver call, completes a solve no successor took with a one-workgroup launch.
 *       0: the last iteration finishes and publishes in its own fit launch.
 *   knn_warm_start 1 (default): iterations >= 1 bound the 5-NN search of a feature by the distances from its new position to the five neighbours the previous
 *       iteration found (an upper bound of the fifth-neighbour distance: the search stays exact, feature_extract.hpp:666/813); 0: every iteration searches cold. */
int mlh_set_gn_schedule(mlh_ctx *ctx, int deferred_finish, int knn_warm_start, int final_in_successor);
/* The same solve submitted and collected separately (one GPU, or several ranks joined by the mailbox communicator -- not under RCCL; no statistics): _begin enqueues the n_iters iterations and returns at once, _end waits for the
 * pose. Between the two the caller may stage the NEXT frame's maps (mlh_map_set_pair): those launches queue up behind the solve on the context's stream, so the
 * GPU does not idle through the host's turn-around at the frame boundary (bench.py submits its frames this way). At most two solves in flight per context
 * (frame k + 1 may be submitted before frame k's pose is collected); mlh_gn_solve_end returns them in submission order. */
int mlh_gn_solve_begin(mlh_ctx *ctx, const double pose_in[7], int n_iters, const mlh_solver_opts *opts);
/* Frame k + 1 submitted while frame k is still being solved: its start pose is the reference's -- transformUpdate() with frame k's RESULT and odometry pose, then
 * transformAssociateToMap() with frame k + 1's odometry pose (lidar_mapper_keyframe.cpp:145-160: pose_wmap_wodom = pose_wmap_curr * pose_wodom_curr.inverse();
 * pose_wmap_curr = pose_wmap_wodom * pose_wodom_curr; Pose::operator* and Pose::inverse as pose.cpp:99-113) -- computed ON THE DEVICE from the pose the previous
 * solve leaves there, by a one-lane launch in front of the iterations. wodom_prev / wodom_cur: [t, q] of the odometry poses of frame k and frame k + 1. The data
 * dependency between consecutive frames stays where the data is; the host never needs frame k's pose to submit frame k + 1. */
int mlh_gn_solve_begin_chained(mlh_ctx *ctx, const double wodom_prev[7], const double wodom_cur[7], int n_iters, const mlh_solver_opts *opts);
int mlh_gn_solve_end(mlh_ctx *ctx, double pose_out[7]);

/* Per-block options of mlh_gn_solve_blocks. k_neigh: N_NEIGH of the block's correspondences (5 for the reference LiDAR, 10 for
 * the others in buildCalibMap, estimator.cpp:1135); eig_thre / freeze: degeneracy handling -- freeze = 0 projects the weak
 * directions out (evalDegenracy, estimator.cpp:1608-1636), freeze = 1 leaves the block untouched when lambda_min < eig_thre
 * (the extrinsic branch, estimator.cpp:1662-1676, without its frame-count state). */
typedef struct mlh_block_opts {
    int n_blocks;
    int k_neigh[8];
    double eig_thre[8];
    int freeze[8];
} mlh_block_opts;
/* n_iters GN iterations on n_blocks independent pose blocks (poses_inout: n_blocks x 7), one correspondence + one fit launch
 * per iteration for all blocks and both feature kinds. stats: n_iters x n_blocks records (iteration-major), may be NULL;
 * termination = 1 in a record marks a frozen block. Multi-LiDAR features must have been staged with mlh_features_set_block (a block of one kind may be empty,
 * n = 0: a LiDAR without corner features in this frame; any subset of the blocks solved by itself returns the bits those blocks have among all of them). */
int mlh_gn_solve_blocks(mlh_ctx *ctx, double *poses_inout, int n_iters, const mlh_solver_opts *opts, const mlh_block_opts *block_opts,
                        mlh_iter_stat *stats);

/* scan2MapOptimization(): max_outer x { goodFeatureMatching (corner, then surf; wo_gf = all matched features),
 * evalHessian + evalDegenracy, Levenberg-Marquardt (Ceres trust-region semantics, <= max_lm_iterations) on the selected,
 * fixed correspondences }. Device-resident for wo_gf; the other gf methods add one host round trip per outer iteration for
 * the selection loop. replaces lidar_mapper_keyframe.cpp:423-599 and 628-639; with MLH_FLAG_POSE_COV in opts->flags also :600-606 and what :632 stores
 * (mlh_scan2map_cov below). stats: max_outer records, or NULL (then evalDegenracy takes
 * the eigen-decomposition only when H - thre*I is not positive definite, i.e. when something IS degenerate). */
int mlh_scan2map(mlh_ctx *ctx, double pose_inout[7], const mlh_solver_opts *opts, mlh_iter_stat *stats);
/* scan2MapOptimization submitted and collected separately (lidar_mapper_keyframe.cpp:423-599 and 628-639 -- :600-606 with MLH_FLAG_POSE_COV -- as the mapper's per-frame call, :145-160 for the chained start pose):
 * mlh_scan2map_begin enqueues the whole solve and returns. lm_lookahead = 0 (automatic): per outer iteration the match launch and ONE launch that runs the
 * Levenberg-Marquardt loop to its end on the device -- nothing to overflow -- wherever that launch applies (one GPU, at most mlh_get_info's loop_max_tiles fit
 * tiles: 160 = 40 960 feature slots on a whole MI355X, fewer on a part of one);
 * otherwise, and with lm_lookahead > 0: per outer iteration the match launch and that many LM launches (automatic: the previous collected frame's longest LM loop + 2,
 * 10 before any; at most max_lm_iterations), launches behind the LM loop's termination find `done` on the device and leave. The caller stages the NEXT frame's maps
 * (mlh_map_set_pair_overlapped) and submits the next frame (mlh_scan2map_begin_chained: start pose = transformUpdate + transformAssociateToMap on the pose the
 * previous solve leaves on the device) before it collects this one's pose with mlh_scan2map_end. Up to two solves in flight, in submission order, shared with
 * mlh_gn_solve_begin / _end (each collected by its own _end). One GPU or the mailbox communicator; gf_method MLH_GF_WO (a selection runs host loops between launches).
 * status_out (nullable):
 *   0  the LM loops terminated inside the look-ahead: pose_out is bit for bit what mlh_scan2map returns on the same inputs;
 *   2  a loop needed more LM iterations than were enqueued -- or a one-launch loop gave its in-kernel barrier up (its workgroups were not all resident at once:
 *      mlh_get_info counts it and lowers the context's gate); nothing had been restaged and no younger solve was chained behind, so the frame was solved again
 *      synchronously from its start pose inside this call (after a barrier given up on: through the launch-per-iteration form): pose_out is mlh_scan2map's;
 *   1  the same, but the inputs of the frame are no longer staged (or a younger solve continues from this one's unfinished pose): pose_out is the frame's START
 *      pose; the caller solves the frame with mlh_scan2map on its inputs and resubmits what was chained behind it;
 *   3  this frame was chained behind a frame that ended with status 1 (or 3, or with an error): it began from that frame's unfinished pose, so pose_out -- whatever
 *      its own loops did, finished or not -- is not the mapper's; resubmit it after the predecessor has been solved.
 * With status_out == NULL the statuses 1 and 3 are returned as MLH_ERR_INCOMPLETE (pose_out is still filled in): a pose that is not a result never comes back
 * under a success code the caller cannot tell apart. */
int mlh_scan2map_begin(mlh_ctx *ctx, const double pose_in[7], const mlh_solver_opts *opts, int lm_lookahead);
int mlh_scan2map_begin_chained(mlh_ctx *ctx, const double wodom_prev[7], const double wodom_cur[7], const mlh_solver_opts *opts, int lm_lookahead);
int mlh_scan2map_end(mlh_ctx *ctx, double pose_out[7], int32_t *status_out);
/* The pose covariance of the most recently COLLECTED scan2map solve -- mlh_scan2map or mlh_downsample_scan2map has returned, or mlh_scan2map_end has returned that
 * solve -- whose options carried MLH_FLAG_POSE_COV (lidar_mapper_keyframe.cpp:600-622 and the assignment at :632):
 *   H_final_out (nullable)  evalHessian at the returned pose: J^T J, Huber-corrected, over the residual blocks of the last outer iteration (problem.Evaluate at the
 *                           pose the last ceres::Solve returned, cpp:600-605);
 *   cov_out                 its inverse (cov_mapping = mat_H.inverse(), cpp:606), computed as Eigen's fixed-size inverse is: LU with partial pivoting, solved against
 *                           the identity. A singular H gives the inf / NaN that gives; nothing is special-cased.
 * Both row-major 6 x 6 in the order of the pose's tangent [t, theta], like mlh_iter_stat::H. No evaluation launch and no host wait are added: when the
 * Levenberg-Marquardt loop ends, its state's record at the current pose IS that Hessian (the record is replaced by the candidate's exactly when a step is accepted),
 * so the wavefront that publishes the pose inverts it and stores both matrices in front of the pose. They are copied out of the pinned record when the solve is
 * collected: two solves in flight do not overwrite each other's, and every form the solve's launches can take delivers the same bits. A local map below
 * scan2MapOptimization's minimum (cpp:429: nothing is optimised) gives two zero matrices (cpp:637).
 * The rule of cpp:607-608 -- cov_mapping is ZERO while the mapper holds at most 10 keyframes -- is the caller's: the library does not know the mapper's keyframe
 * count at this call (the facade's scan2MapOptimization applies it). With with_ua_flag off the reference stores zero as well (cpp:621).
 * MLH_ERR_STATE (with a text): nothing collected yet, the collected solve did not set the flag, or its pose_out was not a result (mlh_scan2map_end statuses 1, 3;
 * a call that returned an error -- a frame whose thinning kept no feature of a kind among them, which mlh_downsample_scan2map reports as MLH_ERR_STATE like
 * mlh_scan2map does an empty feature set: there is no record to invert, and nothing is delivered).
 * Under an RCCL or mailbox communicator a flagged solve is refused with MLH_ERR_UNSUPPORTED before anything is enqueued. */
int mlh_scan2map_cov(mlh_ctx *ctx, double cov_out[36], double H_final_out[36]);
/* downsampleCurrentScan (both kinds) and scan2MapOptimization back to back WITHOUT the host reading what the thinning kept (lidar_mapper_keyframe.cpp:356-421 ->
 * :423-639, as process() calls them one after the other, cpp:1000-1112): the solve's launches are sized for an upper bound (the input clouds) and take the feature
 * counts from device memory; the counts come back with the pose. Same results as mlh_downsample_current_scan_pair followed by mlh_scan2map(stats = NULL), bit for
 * bit -- and exactly those two calls wherever the fused form does not apply (clouds that are not the context's fused clouds, a good-feature selection, several
 * ranks, a local map below scan2MapOptimization's minimum, more than 131 072 input points). pose_inout is written on success only. */
int mlh_downsample_scan2map(mlh_ctx *ctx, const void *surf_points, int n_surf, const void *corner_points, int n_corner, int stride_bytes,
                            int intensity_offset_bytes, int mem, float leaf_surf, float leaf_corner, const double *ext_poses, const double *ext_covs,
                            int n_lidar, const double cov_measurement[9], int with_ua, double trace_threshold, double pose_inout[7],
                            const mlh_solver_opts *opts, int32_t *n_surf_features, int32_t *n_corner_features);

/* ---------------------------------------------------------------- (f4) scan-to-scan odometry: LidarTracker::trackCloud
 * replaces lidar_tracker.cpp:23-129 and the functions it drives: matchCornerFromScan / matchSurfFromScan
 * (feature_extract.hpp:132-376; kd-tree 1-NN within DISTANCE_SQ_THRESHOLD, then the walks over the neighbouring scan lines),
 * TransformToStart without distortion (utility.h:55-77), LidarScanPlaneNormFactor / LidarScanEdgeFactorVector
 * (lidar_scan_factor.hpp:24-64, 236-279) under HuberLoss(0.1), ceres::Solve with max_num_iterations = 4, two rounds.
 * kind MLH_CORNER: previous = "corner_points_less_sharp", current = "corner_points_sharp";
 * kind MLH_SURF:   previous = "surf_points_less_flat",    current = "surf_points_flat"   (lidar_tracker.cpp:30-38).
 * Previous-frame clouds must be ordered by ring id = int(intensity) (as extractCloud emits them); 0 <= id <= 255. */
typedef struct mlh_track_opts {
    float distance_sq_threshold;     /* DISTANCE_SQ_THRESHOLD, config distance_sq_threshold (25) */
    float nearby_scan;               /* NEARBY_SCAN, config nearby_scan (2.5) */
    double huber_delta;              /* ceres::HuberLoss(0.1), lidar_tracker.cpp:45 */
    int32_t max_outer;               /* 2, cpp:42 */
    int32_t max_lm_iterations;       /* options.max_num_iterations = 4, cpp:113 */
} mlh_track_opts;
void mlh_track_opts_default(mlh_track_opts *o);
/* stage the previous frame's cloud of one kind and build its index (pcl::KdTreeFLANN::setInputCloud, cpp:33-34) */
int mlh_track_set_prev(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int n, int intensity_offset_bytes, int mem,
                       float distance_sq_threshold);
/* stage the current frame's features of one kind */
int mlh_track_set_cur(mlh_ctx *ctx, int kind, const void *points, int stride_bytes, int m, int intensity_offset_bytes, int mem);
/* device-to-device hand-over from the extractor of the SAME context (after mlh_extract_run, and mlh_extract_voxel_run for which = 1):
 * which = 0: the scan's sharp corners / flat surfs become the current frame; which = 1: its less-sharp corners / voxel-thinned
 * less-flat surfs become the previous frame (call it after mlh_track_cloud, for the next frame). The scan must have been uploaded
 * with its intensity (ring id) field. */
int mlh_track_set_from_scan(mlh_ctx *ctx, int which, float distance_sq_threshold);
/* pcl::VoxelGrid<PointXYZI>::filter (PCL 1.8.0 filters/impl/voxel_grid.hpp) over a whole cloud: one centroid per occupied voxel, x, y, z
 * AND intensity averaged, ascending voxel index; a grid of more than 2^31 cells returns the input unchanged ("leaf size is too small").
 * Estimator::buildLocalMap / buildCalibMap thin the window's clouds with it (estimator/src/estimator/estimator.cpp:1124-1130,
 * 1194-1203). out: same record layout as the input (fields other than x, y, z, intensity zeroed). Host or device buffers. */
int mlh_voxel_grid(mlh_ctx *ctx, const void *points, int stride_bytes, int n, int intensity_offset_bytes, float leaf, void *out,
                   int32_t *n_out, int mem);
/* pcl::transformPointCloud(cloud, cloud, pose.T_.cast<float>()) in place (estimator.cpp:1185-1192: the window clouds moved into
 * the pivot frame): x, y, z <- R p + t in single precision, the other fields kept. pose = [t(3), q(xyzw)]. */
int mlh_transform_point_cloud(mlh_ctx *ctx, void *points, int stride_bytes, int n, const double pose[7], int mem);
/* TransformToEnd (estimator/src/utility/utility.h:79-100; TransformToStart :55-77) over n records, in place: p_end = T^-1 T(s) p with
 * T(s) = (Identity.slerp(s, q), s t), s = (intensity - int(intensity)) / scan_period when b_distortion (the intensity field carries
 * ring id + time inside the sweep), else 1. f64 arithmetic, the intermediate and final points rounded to f32 as the reference's
 * float points do. pose = [t(3), q(xyzw)]. Host (copied in and out) or device buffers. */
int mlh_transform_to_end(mlh_ctx *ctx, void *points, int stride_bytes, int n, int intensity_offset_bytes, const double pose[7],
                         int b_distortion, float scan_period, int mem);
/* Estimator::undistortMeasurements (estimator.cpp:376-410, DISTORTION = 1) for the scan the context holds: TransformToEnd(...,
 * true, scan_period) on all its points (laser_cloud; the less-sharp corner list indexes them) and on its voxel-thinned less-flat
 * cloud, in place on the device. Order as in Estimator::process (estimator.cpp:532-586): the tracker consumes this scan's sharp /
 * flat features and mlh_track_set_from_scan(1) copies the (still distorted) less-sharp / less-flat clouds to the previous frame
 * first; then this call; then mlh_fuse_add_scan hands the undistorted clouds to the mapper. */
int mlh_scan_undistort(mlh_ctx *ctx, const double pose_undist[7], float scan_period);

/* The mapper's input clouds without leaving HBM. transformCloudFeature (estimator/src/utility/visualization.cpp:39-51) moves every
 * LiDAR's features into the body frame and overwrites intensity with the LiDAR index before they are published to the mapper;
 * mlh_fuse_add_scan does that for the scan the context holds (after mlh_extract_run + mlh_extract_voxel_run): its voxel-thinned
 * less-flat points are appended to the fused SURF cloud, its less-sharp points to the fused CORNER cloud (float32: (r0 x + r1 y)
 * + r2 z + t per row, R rounded once from the double quaternion). mlh_fused_cloud hands out the device pointer (float4 records
 * {x,y,z,lidar}: stride 16, intensity offset 12) for mlh_downsample_current_scan(..., MLH_MEM_DEVICE); it stays valid until the
 * next mlh_fuse_add_*. ext_pose = [t(3), q(xyzw)] of the LiDAR in the body frame. mlh_fuse_add_rings takes rings [ring_begin,
 * ring_end) of the scan only: several LiDARs uploaded as ONE scan (their rings back to back, one launch set for all of them)
 * are appended one ring range at a time, each with its own extrinsic. The appends never wait for the host: the record counts live
 * on the device and mlh_fused_cloud fetches them once. */
int mlh_fuse_reset(mlh_ctx *ctx);
int mlh_fuse_add_scan(mlh_ctx *ctx, int lidar_idx, const double ext_pose[7]);
int mlh_fuse_add_rings(mlh_ctx *ctx, int ring_begin, int ring_end, int lidar_idx, const double ext_pose[7]);
/* mlh_fuse_add_scan with the scan ANOTHER context (src, same device) holds -- estimator.cpp:248-263 runs every LiDAR's segmentCloud -> extractCloud on a thread of its
 * own; with a context per thread (the host-side cluster searches of the LiDARs side by side) this gathers their mapping features in ONE context's fused clouds
 * without a host hop. Ordered on the device in both directions: ctx's stream waits for what src's stream has been given so far, and whatever rewrites src's scan
 * next (mlh_scan_upload, mlh_segment_cloud, mlh_extract_run, mlh_extract_voxel_run, mlh_scan_undistort) waits for this append. src must be idle while this
 * call runs (its last call has returned, none is running: the calling thread touches src's bookkeeping). */
int mlh_fuse_add_scan_from(mlh_ctx *ctx, mlh_ctx *src, int lidar_idx, const double ext_pose[7]);
int mlh_fused_cloud(mlh_ctx *ctx, int kind, const void **device_points, int32_t *n);
/* match*FromScan at `pose`: valid[m] and coeffs[m x 6] ('c': closest point, second point; 's': w, negative_OA_dot_norm, 0, 0); either may be NULL */
int mlh_track_match(mlh_ctx *ctx, int kind, const double pose[7], const mlh_track_opts *opts, uint8_t *valid, double *coeffs);
/* trackCloud: pose_inout = pose_ini -> pose_prev_cur; stats: max_outer records (n_surf / n_corner = residual blocks) or NULL */
int mlh_track_cloud(mlh_ctx *ctx, double pose_inout[7], const mlh_track_opts *opts, mlh_iter_stat *stats);

/* ---------------------------------------------------------------- (e) multi-GPU: map shards + one all-reduce per iteration
 * One process (context) per GPU. The local map is partitioned spatially: rank g stages only the map points of its
 * region plus a halo >= sqrt(min_match_sq_dis) (mlh_map_set on that subset), and OWNS the features whose map-frame
 * position p = pointAssociateToMap(feature) satisfies  lo.xyz . p + lo.w >= 0  and  hi.xyz . p + hi.w < 0
 * (either plane may be NULL = unbounded; evaluated in f32 as ((a*x + b*y) + c*z) + d, so neighbouring ranks that share a
 * plane take complementary decisions and every feature has exactly one owner). Features a rank does not own contribute
 * nothing on that rank. Because every map point within the acceptance radius of an owned feature is local, the 5-NN /
 * gate decisions are identical to the unsharded ones.
 * mlh_comm_init joins the ranks (RCCL, dlopen'ed): the device-resident solvers then sum the packed normal equations
 * (32 doubles: 21 J^T J + 6 J^T r + cost + counts) with ONE ncclAllReduce per evaluation on the context's stream, and
 * every rank applies the identical 6x6 solve / Plus redundantly (no pose broadcast). */
int mlh_shard_set(mlh_ctx *ctx, const float *lo_plane4, const float *hi_plane4);
/* The balanced alternative of SURVEY 8(e): every rank stages the WHOLE map (4 M points are 64 MB of 288 GB) and owns the features whose
 * slot index f satisfies f % n_ranks == rank -- no halo, equal shares whatever the scene, the same one all-reduce per evaluation. The index
 * build is then replicated instead of divided, which is the price. n_ranks = 1 switches it off; it combines with mlh_shard_set (both tests
 * must hold) but is meant to be used instead of it. */
int mlh_shard_set_features(mlh_ctx *ctx, int n_ranks, int rank);
int mlh_comm_unique_id(void *out_128_bytes);
int mlh_comm_init(mlh_ctx *ctx, int n_ranks, int rank, const void *unique_id_128_bytes);
/* The same join WITHOUT a collective library -- the mailbox communicator: the path's one collective is a few hundred bytes per evaluation, i.e. pure latency,
 * and a library all-reduce (protocol selection, proxy threads, a ring over the ranks) costs tens of microseconds there. mlh_p2p_mailbox allocates this rank's
 * mailbox in device memory and returns its 64-byte hipIpc handle; the caller exchanges the handles out of band (one all-gather of 64 bytes: MPI, torch.distributed,
 * a file ...) and hands all n_ranks of them, in rank order, to mlh_p2p_comm_init, which maps the peers' mailboxes (peer access over xGMI between GPUs; ranks may
 * also share a GPU). Every all-reduce of the solvers (and mlh_allreduce_f64, up to 512 doubles) is then ONE single-workgroup kernel per rank on the context's stream:
 * store my record into my slot of every mailbox, publish a sequence number, wait for the n sequence numbers in my own mailbox, add the n slots in rank order --
 * every rank ends with the same bits. A peer that never shows up raises an error on the next call instead of hanging the GPU (5 s bound). <= 16 ranks. */
int mlh_p2p_mailbox(mlh_ctx *ctx, void *ipc_handle_64_bytes);
int mlh_p2p_comm_init(mlh_ctx *ctx, int n_ranks, int rank, const void *ipc_handles /* n_ranks x 64 bytes, rank order */);
/* drops the communicator (either kind): the context is single-GPU again */
int mlh_comm_finalize(mlh_ctx *ctx);
/* in-place sum of n doubles (HOST buffer, any n) over the ranks -- the standalone "mlh_allreduce_normal_eq" of SURVEY 8b */
int mlh_allreduce_f64(mlh_ctx *ctx, double *host_inout, int n);

/* ---------------------------------------------------------------- (f17) the session image: a mapping session saved and restored
 * What PoseGraph::savePoseGraph (mloam_loop/src/pose_graph.cpp:655-694) and loadPoseGraph (cpp:696-781, through loadKeyFrame, cpp:225-279, and addKeyFrameIntoDB,
 * cpp:77-90) keep over a restart: every keyframe with its clouds, the place index and the pose graph. Here: one versioned, checksummed, canonical byte image of
 * the keyframe store of (f5) / (f7) / (f15), the Scan Context store of (f11) and the pose graph of (f14); csrc/session_host.hpp states the format.
 * Reproduced: what the reference's files carry per keyframe -- pose, the clouds, the loop edge (index and relative pose) -- and that a loaded map answers like the
 *   one that was saved: after an import every entry point of (f5) .. (f15) gives the bits it gave on the exporting context.
 * CHOSEN: one binary image instead of pose_graph.txt + four .pcd files per keyframe; the format is this project's own. The image also carries what the reference
 *   recomputes on load: the Scan Context entries with the period counter and the searched prefix (a loaded store answers mlh_sc_detect as the saved one would
 *   have, stale prefix included), and each keyframe's covariance. A caller that wants the index rebuilt instead -- other num_ring / num_sector, or an image
 *   without the SC section -- imports KEYFRAMES | PG, calls mlh_sc_reset and mlh_sc_add_keyframes(0, K): loadPoseGraph's addKeyFrameIntoDB loop in one call.
 * CHOSEN: the image is CANONICAL: the clouds are stored key by key (surf, corner, outlier) whatever order the store's arena got them in (outlier clouds are
 *   attached later), and the local-map cache, the map clouds and all scratch stay out, so two contexts with the same content give the same bytes whatever their
 *   call histories, and export(import(image)) == image. (The SC section carries the store's statistics counters; last_host_decided / last_skipped are those of the
 *   last add, so a store filled by mlh_sc_add_keyframes and one filled by single adds differ in those two words and in nothing else.)
 * DEPARTURE: not in the image, because transient: the odometry window, the calibration store, the marginalisation prior, the initial-extrinsics state. No PCD or
 *   text formats, no compression, little-endian hosts only, no import from another context's device memory.
 * Checksum of a section of u32 words w_i: sum (w_i XOR 0x9E3779B9) (2 i + 1) mod 2^64 -- an integer sum, taken on the device in any order with the same bits.
 * mlh_session_export_size: the bytes an export of `sections` (an OR of MLH_SESSION_*; KEYFRAMES stands for the keyframes and their points) takes now.
 * mlh_session_export: the image into dst (`mem`: MLH_MEM_HOST or MLH_MEM_DEVICE), *written <- its length. capacity too small: MLH_ERR_INVALID, *written <- the
 *   length needed, nothing touched. MLH_SESSION_SC before the first mlh_sc_reset: MLH_ERR_STATE. ONE pack launch whatever the number of keyframes: 256-record
 *   tiles that never straddle a cloud; a thread moves one 16-byte record from the store's arena to its canonical place in a staging image and adds its four
 *   checksum terms, the workgroup's sum goes to the section's word by one 64-bit integer atomic add (order-independent: no float atomics). The SC and PG
 *   sections are copied into the staging image device to device (a fixed number of copies) and checksummed there by the same launch. Then one copy to dst and ONE
 *   host wait (for a device dst one more, behind the 208-byte header, which is written last from the read-back checksums). Beside a solve submitted with
 *   mlh_*_begin: correct, but enqueued behind the solve on the context's stream, as mlh_local_map_assemble.
 * An export refuses what no import would take: 2^31 or more stored points is MLH_ERR_UNSUPPORTED before anything runs; an image written into host memory is held
 *   to the import's validation before the call returns (a pose graph with a non-finite pose: MLH_ERR_STATE); a device destination is not read back. The staging
 *   image belongs to the call: neither an export nor an import leaves an image-sized buffer in the context.
 * mlh_session_inspect: host only, no context: validates the header, the section table and every section's contents (bounds, overlaps, record sizes, counts
 *   against lengths, n[] >= 0, finite poses, the SC options as mlh_sc_reset does, loop indices, max_loops <= MLH_PG_LOOPS_LIMIT, every padding byte zero) AND the payload checksums.
 * mlh_session_import: the same validation on the host before the context is touched (the payload checksums excepted), the requested sections uploaded into NEW
 *   buffers, their checksums taken on the device by the pack kernel; only if every one matches are the buffers swapped into the stores: the keyframe store as
 *   mlh_keyframes_reset followed by the saves would leave it (offsets = the prefix sums, cache and map clouds empty); the SC store with its options, entries,
 *   positions, period counter, searched prefix and counters; the pose graph with count, earliest loop and the loop indices, max_loops raised as by mlh_pg_reserve
 *   when the image's is larger. Any failure -- a corrupt image is MLH_ERR_INVALID with the reason in mlh_last_error -- leaves the context exactly as it was; a
 *   requested section the image lacks is MLH_ERR_INVALID; stores not named in `sections` are untouched. ONE host wait, launches independent of the keyframes.
 * mlh_session_last_info: the last successful export or import of the context (zeroes before). */
enum { MLH_SESSION_KEYFRAMES = 1, MLH_SESSION_SC = 2, MLH_SESSION_PG = 4 };
typedef struct mlh_session_info {
    uint32_t version;
    uint32_t sections;               /* MLH_SESSION_* the image holds (import: those imported) */
    int32_t launches, host_waits;    /* of the export / import (mlh_session_inspect: 0) */
    int64_t total_bytes;
    int64_t count[4];                /* per stored section -- keyframes, points, Scan Context entries, pose-graph keyframes --: elements, */
    int64_t bytes[4];                /* ... bytes, */
    uint64_t checksum[4];            /* ... checksum; zero for an absent section */
} mlh_session_info;
int mlh_session_export_size(mlh_ctx *ctx, uint32_t sections, size_t *bytes);
int mlh_session_export(mlh_ctx *ctx, uint32_t sections, void *dst, size_t capacity, int mem, size_t *written);
int mlh_session_inspect(const void *image, size_t bytes, mlh_session_info *out);
int mlh_session_import(mlh_ctx *ctx, const void *image, size_t bytes, uint32_t sections, mlh_session_info *out);
int mlh_session_last_info(mlh_ctx *ctx, mlh_session_info *out);

/* host-side helpers mirroring the reference's small functions (no GPU work) */
/* PoseLocalParameterization::Plus with V_update_ (row-major 6x6; NULL = identity) */
int mlh_pose_plus(const double x[7], const double delta[6], const double *V_update, double x_plus_delta[7]);
/* evalDegenracy: eigenvalues ascending, V_update = (V_f^T)^-1 V_p^T, returns 1 when degenerate */
int mlh_eval_degeneracy(const double H[36], double eig_thre, double eigval[6], double V_update[36]);

#ifdef __cplusplus
}
#endif
#endif /* MLOAM_HIP_H */
