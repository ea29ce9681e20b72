"""m-loam_amd -- MI355X-native (gfx950) scan-to-map hot path of M-LOAM.

The product is ``lib/libmloam_hip.so`` (hand-written HIP kernels behind the C-ABI of ``include/mloam_hip.h``) plus the
C++ facade under ``host/`` that mirrors the reference's ``FeatureExtract`` / factor / ``PoseLocalParameterization``
interfaces. This module is the thin ctypes harness the tests and ``bench.py`` use to call through that C-ABI; it
contains no compute and no CPU fallback: if the HIP library is missing or no GPU is visible it raises.

Import with ``importlib.import_module("m-loam_amd")`` (the directory name carries a hyphen).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLOAM_HIP_LIB") or os.path.join(_HERE, "lib", "libmloam_hip.so")   # override: instrumented debug builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mloam_hip.h")

SURF, CORNER = 0, 1
cd_ = C.c_double
ALL_KINDS = -1
MEM_HOST, MEM_DEVICE = 0, 1
FLAG_CHECK_FOV, FLAG_WITH_UA, FLAG_NO_LOSS, FLAG_POSE_COV = 1, 2, 4, 8
GF_METHODS = {"wo_gf": 0, "rnd": 1, "fps": 2, "gd_fix": 3, "gd_float": 4}
K_KNN, K_FIT, K_LINEARIZE, K_SOLVE, K_GRID_BUILD, K_EXTRACT, K_ALLREDUCE, K_KNN_PRE, K_KNN_FIRST = range(9)
K_ALL = 0x1FF
THIN_NONE, THIN_SORT_FIRST, THIN_SHARED_GRID, THIN_SINGLE_CALLS = range(4)


class MlhError(RuntimeError):
    pass


class SolverOpts(C.Structure):
    _fields_ = [("min_match_sq_dis", C.c_float), ("min_plane_dis", C.c_float), ("huber_delta", C.c_double),
                ("map_eig_thre", C.c_double), ("cov_measurement_trace", C.c_double), ("flags", C.c_uint32),
                ("max_outer", C.c_int), ("max_lm_iterations", C.c_int), ("gf_method", C.c_int), ("gf_ratio", C.c_double),
                ("gf_seed", C.c_uint64)]


class BlockOpts(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("k_neigh", C.c_int * 8), ("eig_thre", C.c_double * 8), ("freeze", C.c_int * 8)]


class LocalMapOpts(C.Structure):
    """mlh_local_map_opts: extractSurroundingKeyFrames' parameters"""
    _fields_ = [("surrounding_kf_radius", C.c_float), ("map_sur_kf_res", C.c_float), ("leaf_surf", C.c_float), ("leaf_corner", C.c_float),
                ("trace_threshold", C.c_double), ("with_ua", C.c_int), ("cov_measurement", C.c_double * 9)]


def local_map_opts(surrounding_kf_radius=50.0, map_sur_kf_res=1.0, leaf_surf=0.4, leaf_corner=0.2, trace_threshold=0.6, with_ua=True, cov_measurement=None):
    o = LocalMapOpts()
    o.surrounding_kf_radius, o.map_sur_kf_res, o.leaf_surf, o.leaf_corner = surrounding_kf_radius, map_sur_kf_res, leaf_surf, leaf_corner
    o.trace_threshold, o.with_ua = trace_threshold, int(bool(with_ua))
    cm = np.diag([0.0025] * 3) if cov_measurement is None else np.asarray(cov_measurement, np.float64)
    for i, v in enumerate(np.ascontiguousarray(cm, np.float64).reshape(9)):
        o.cov_measurement[i] = float(v)
    return o


class GlobalMapOpts(C.Structure):
    """mlh_global_map_opts: pubGlobalMap's / saveGlobalMap's parameters"""
    _fields_ = [("kf_radius", C.c_float), ("kf_res", C.c_float), ("leaf", C.c_float), ("split", C.c_int32), ("trace_threshold", C.c_double),
                ("with_ua", C.c_int), ("cov_measurement", C.c_double * 9)]


def global_map_opts(for_save=False, **kw) -> GlobalMapOpts:
    """mlh_global_map_opts_default (for_save: saveGlobalMap's values, else pubGlobalMap's), then the given fields"""
    o = GlobalMapOpts()
    load_library().mlh_global_map_opts_default(C.byref(o), int(bool(for_save)))
    for k, v in kw.items():
        if k == "cov_measurement":
            for i, x in enumerate(np.ascontiguousarray(v, np.float64).reshape(9)):
                o.cov_measurement[i] = float(x)
        elif k == "with_ua":
            o.with_ua = int(bool(v))
        else:
            setattr(o, k, v)
    return o


class WindowMapOpts(C.Structure):
    """mlh_window_map_opts: buildLocalMap's / buildCalibMap's parameters"""
    _fields_ = [("source_lidar", C.c_int32), ("leaf_surf", C.c_float * 16), ("leaf_corner", C.c_float * 16)]


def window_map_opts(n_scans=16, n_lidar=1, window_size=3, source_lidar=-1, leaf_surf=None, leaf_corner=None) -> WindowMapOpts:
    """mlh_window_map_opts_default (buildLocalMap's ratio for every LiDAR), then source_lidar and the given per-LiDAR leaves (a number = the same for all)"""
    o = WindowMapOpts()
    load_library().mlh_window_map_opts_default(C.byref(o), int(n_scans), int(n_lidar), int(window_size))
    o.source_lidar = int(source_lidar)
    for name, v in (("leaf_surf", leaf_surf), ("leaf_corner", leaf_corner)):
        if v is not None:
            arr = getattr(o, name)
            for i, x in enumerate(np.full(n_lidar, v, np.float32) if np.ndim(v) == 0 else np.asarray(v, np.float32)):
                arr[i] = float(x)
    return o


def global_map_select(positions_xyz, center, kf_radius, kf_res):
    """mlh_global_map_select (host arithmetic): the keyframes the global map is made of, in the order their clouds are appended"""
    pos = np.ascontiguousarray(positions_xyz, np.float32).reshape(-1, 3)
    c = None if center is None else np.ascontiguousarray(center, np.float32).reshape(3)
    ids = np.zeros(max(len(pos), 1), np.int32)
    n = C.c_int32(0)
    rc = load_library().mlh_global_map_select(_p(pos) if len(pos) else None, len(pos), _p(c), float(kf_radius), float(kf_res), _p(ids), C.byref(n))
    if rc != 0:
        raise MlhError(f"mlh_global_map_select failed ({rc})")
    return ids[:n.value].copy()


class WindowPriorInfo(C.Structure):
    """mlh_window_prior_info"""
    _fields_ = [("valid", C.c_int32), ("n_keep", C.c_int32), ("n", C.c_int32), ("kept_mm", C.c_int32), ("kept_rr", C.c_int32), ("sweeps_mm", C.c_int32),
                ("sweeps_rr", C.c_int32), ("reserved", C.c_int32), ("min_kept_mm", cd_), ("max_dropped_mm", cd_), ("min_kept_rr", cd_), ("max_dropped_rr", cd_)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class CalibStoreInfo(C.Structure):
    """mlh_calib_store_info"""
    _fields_ = [("n_appends", C.c_int32), ("n_tiles", C.c_int32), ("n_slots", C.c_int32), ("n_valid", C.c_int32), ("max_ext", C.c_int32), ("in_use", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ScOpts(C.Structure):
    """mlh_sc_opts"""
    _fields_ = [("lidar_height", cd_), ("num_ring", C.c_int32), ("num_sector", C.c_int32), ("max_radius", cd_), ("num_exclude_recent", C.c_int32),
                ("num_candidates", C.c_int32), ("search_ratio", cd_), ("dist_thres", cd_), ("tree_making_period", C.c_int32), ("reserved", C.c_int32),
                ("loop_distance_threshold", cd_)]


class ScResult(C.Structure):
    """mlh_sc_result"""
    _fields_ = [("match_index", C.c_int32), ("nearest_index", C.c_int32), ("shift", C.c_int32), ("n_candidates_scored", C.c_int32),
                ("rejected_by_distance", C.c_int32), ("yaw_diff_rad", C.c_float), ("score", cd_)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ScStoreInfo(C.Structure):
    """mlh_sc_store_info"""
    _fields_ = [("n_entries", C.c_int32), ("searched_prefix", C.c_int32), ("period_counter", C.c_int32), ("desc_tile_points", C.c_int32),
                ("desc_wrap_points", C.c_int32), ("last_host_decided", C.c_int32), ("last_skipped", C.c_int32), ("reserved", C.c_int32),
                ("points_host_decided", C.c_int64), ("points_skipped", C.c_int64), ("bytes_hbm", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class ScBatchInfo(C.Structure):
    """mlh_sc_batch_info"""
    _fields_ = [("n_entries", C.c_int32), ("n_chunks", C.c_int32), ("launches", C.c_int32), ("host_waits", C.c_int32), ("first_index", C.c_int32),
                ("chunk_points", C.c_int32), ("max_chunks_per_entry", C.c_int32), ("target_workgroups", C.c_int32),
                ("n_points", C.c_int64), ("points_host_decided", C.c_int64), ("points_skipped", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SESSION_KEYFRAMES, SESSION_SC, SESSION_PG = 1, 2, 4
SESSION_ALL = SESSION_KEYFRAMES | SESSION_SC | SESSION_PG


class SessionInfo(C.Structure):
    """mlh_session_info; the arrays are per stored section: keyframes, points, Scan Context entries, pose-graph keyframes"""
    _fields_ = [("version", C.c_uint32), ("sections", C.c_uint32), ("launches", C.c_int32), ("host_waits", C.c_int32), ("total_bytes", C.c_int64),
                ("count", C.c_int64 * 4), ("bytes", C.c_int64 * 4), ("checksum", C.c_uint64 * 4)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k in ("count", "bytes", "checksum") else getattr(self, k)) for k, _ in self._fields_}


def session_inspect(image) -> dict:
    """the header and section table of a session image (bytes or a uint8 array), validated on the host, payload checksums included (mlh_session_inspect)"""
    buf = np.frombuffer(bytes(image), np.uint8) if not isinstance(image, np.ndarray) else np.ascontiguousarray(image, np.uint8)
    info = SessionInfo()
    rc = load_library().mlh_session_inspect(buf.ctypes.data_as(C.c_void_p) if len(buf) else None, len(buf), C.byref(info))
    if rc != 0:
        raise MlhError(f"mlh error {rc}: not a valid session image")
    return info.as_dict()


def sc_opts(**kw) -> ScOpts:
    """mlh_sc_opts_default (config_loop_realvehicle.yaml), then the given fields"""
    o = ScOpts()
    load_library().mlh_sc_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class LoopOpts(C.Structure):
    """mlh_loop_opts"""
    _fields_ = [("leaf_surf", C.c_float), ("leaf_corner", C.c_float), ("history_search_num", C.c_int32), ("max_outer", C.c_int32), ("max_lm_iterations", C.c_int32),
                ("reserved", C.c_int32), ("local_registration_threshold", cd_), ("huber_delta", cd_), ("match_sq_dis_surf", C.c_float),
                ("match_sq_dis_corner", C.c_float), ("plane_dis", cd_), ("line_eig_ratio", C.c_float), ("reserved2", C.c_int32), ("min_match_ratio", cd_)]


class LoopOuterStat(C.Structure):
    """mlh_loop_outer_stat"""
    _fields_ = [("entered", C.c_int32), ("ran", C.c_int32), ("surf_num", C.c_int32), ("corner_num", C.c_int32), ("lm_iterations", C.c_int32),
                ("successful_steps", C.c_int32), ("termination", C.c_int32), ("reserved", C.c_int32), ("initial_cost", cd_), ("final_cost", cd_)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class LoopResult(C.Structure):
    """mlh_loop_result"""
    _fields_ = [("T_relative", cd_ * 16), ("para_pose", cd_ * 7), ("opti_cost", cd_), ("accepted", C.c_int32), ("n_outer", C.c_int32), ("outer", LoopOuterStat * 8)]

    def as_dict(self):
        return dict(T_relative=np.array(self.T_relative).reshape(4, 4), para_pose=np.array(self.para_pose), opti_cost=self.opti_cost, accepted=bool(self.accepted),
                    n_outer=self.n_outer, outer=[self.outer[i].as_dict() for i in range(self.n_outer)])


class LoopInfo(C.Structure):
    """mlh_loop_info"""
    _fields_ = [("n_pre", C.c_int32 * 4), ("n_ds", C.c_int32 * 4), ("allocations", C.c_int64), ("bytes_hbm", C.c_int64)]


def loop_opts(**kw) -> LoopOpts:
    """mlh_loop_opts_default (pose_graph.cpp:33-34, loop_registration.cpp, feature_extract.hpp), then the given fields"""
    o = LoopOpts()
    load_library().mlh_loop_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


LOOP_MODEL_SURF, LOOP_MODEL_CORNER, LOOP_DATA_SURF, LOOP_DATA_CORNER = 0, 1, 2, 3


class FgrOpts(C.Structure):
    """mlh_fgr_opts"""
    _fields_ = [("normal_radius", C.c_float), ("fpfh_radius", C.c_float), ("div_factor", cd_), ("use_absolute_scale", C.c_int32), ("iteration_number", C.c_int32),
                ("max_corr_dist", cd_), ("tuple_scale", C.c_float), ("tuple_max_cnt", C.c_int32), ("global_registration_threshold", cd_), ("seed", C.c_uint64)]


class FgrResult(C.Structure):
    """mlh_fgr_result"""
    _fields_ = [("T_relative", cd_ * 16), ("final_cost_normalize", cd_), ("final_cost", cd_), ("global_scale", cd_), ("start_scale", cd_), ("means", cd_ * 6),
                ("accepted", C.c_int32), ("swapped", C.c_int32), ("n_mutual", C.c_int32), ("n_tuples", C.c_int32), ("n_corres", C.c_int32), ("n_trials", C.c_int32),
                ("host_waits", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("reserved", "T_relative", "means", "accepted", "swapped")}
        d.update(T_relative=np.array(self.T_relative).reshape(4, 4), means=np.array(self.means).reshape(2, 3), accepted=bool(self.accepted), swapped=bool(self.swapped))
        return d


class FgrInfo(C.Structure):
    """mlh_fgr_info_t"""
    _fields_ = [("n", C.c_int32 * 2), ("have_normals", C.c_int32 * 2), ("have_spfh", C.c_int32 * 2), ("have_features", C.c_int32 * 2), ("launches", C.c_int32),
                ("host_waits", C.c_int32), ("allocations", C.c_int64), ("bytes_hbm", C.c_int64)]


def fgr_opts(**kw) -> FgrOpts:
    """mlh_fgr_opts_default (config_loop_realvehicle.yaml; seed 1), then the given fields"""
    o = FgrOpts()
    load_library().mlh_fgr_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


FGR_NORMALS, FGR_SPFH, FGR_FPFH = 0, 1, 2


class PgOpts(C.Structure):
    """mlh_pg_opts"""
    _fields_ = [("max_num_iterations", C.c_int32), ("n_sequential", C.c_int32), ("t_var", cd_), ("q_var", cd_), ("huber_delta", cd_)]


class PgResult(C.Structure):
    """mlh_pg_result"""
    _fields_ = [("num_iterations", C.c_int32), ("num_successful_steps", C.c_int32), ("termination", C.c_int32), ("n_keyframes", C.c_int32), ("n_loops", C.c_int32),
                ("first_index", C.c_int32), ("launches", C.c_int32), ("host_waits", C.c_int32), ("initial_cost", cd_), ("final_cost", cd_), ("final_radius", cd_),
                ("drift", cd_ * 7), ("solve_radius", cd_)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "drift"}
        d["drift"] = np.array(self.drift)
        return d


class PgInfo(C.Structure):
    """mlh_pg_info_t"""
    _fields_ = [("n_keyframes", C.c_int32), ("n_loops", C.c_int32), ("earliest_loop_index", C.c_int32), ("max_loops", C.c_int32), ("allocations", C.c_int64),
                ("bytes_hbm", C.c_int64)]


PG_LOOPS_LIMIT = 1024          # MLH_PG_LOOPS_LIMIT
PG_COV_LOCAL, PG_COV_STORE = 0, 1          # MLH_PG_COV_*: the solver's tangent [rotation, translation] / the keyframe store's left perturbation [rho, phi]
KF_COV_RELATIVE, KF_COV_ABSOLUTE = 0, 1    # MLH_KF_COV_*


class PgMarginalsResult(C.Structure):
    """mlh_pg_marginals_result"""
    _fields_ = [("ok", C.c_int32), ("n_keyframes", C.c_int32), ("n_loops", C.c_int32), ("first_index", C.c_int32), ("launches", C.c_int32), ("host_waits", C.c_int32)]


def pg_opts(**kw) -> PgOpts:
    """mlh_pg_opts_default (pose_graph.cpp:522, 525, 555, 566), then the given fields"""
    o = PgOpts()
    load_library().mlh_pg_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class InitExtOpts(C.Structure):
    """mlh_initext_opts"""
    _fields_ = [("n_lidar", C.c_int32), ("idx_ref", C.c_int32), ("planar_movement", C.c_int32), ("window_size", C.c_int32), ("n_pose", C.c_int32), ("reserved", C.c_int32),
                ("eps_r", cd_), ("eps_t", cd_), ("rot_cov_thre", cd_), ("qbl", (cd_ * 4) * 8), ("tbl", (cd_ * 3) * 8)]


class InitExtResult(C.Structure):
    """mlh_initext_result"""
    _fields_ = [("q", cd_ * 4), ("t", cd_ * 3), ("rot_sv", cd_ * 4), ("trans_sv", cd_ * 4), ("lidar", C.c_int32), ("rot_ran", C.c_int32), ("rot_converged", C.c_int32),
                ("trans_solved", C.c_int32), ("trans_rank", C.c_int32), ("rot_sweeps", C.c_int32), ("trans_sweeps", C.c_int32), ("slot", C.c_int32)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, t in self._fields_ if t is C.c_int32}
        d.update(q=np.array(self.q), t=np.array(self.t), rot_sv=np.array(self.rot_sv), trans_sv=np.array(self.trans_sv))
        return d


class InitExtInfo(C.Structure):
    """mlh_initext_info_t"""
    _fields_ = [("configured", C.c_int32), ("n_lidar", C.c_int32), ("n_sets", C.c_int32), ("heap_size", C.c_int32), ("last_slot", C.c_int32), ("cov_rot_mask", C.c_int32),
                ("cov_pos_mask", C.c_int32), ("full_cov_rot", C.c_int32), ("full_cov_pos", C.c_int32), ("launches", C.c_int32), ("host_waits", C.c_int32),
                ("reserved", C.c_int32), ("allocations", C.c_int64), ("bytes_hbm", C.c_int64), ("rot_cov_thre", cd_)]


INITEXT_ROT, INITEXT_TRANS = 1, 2


def initext_opts(qbl=None, tbl=None, **kw) -> InitExtOpts:
    """mlh_initext_opts_default (initial_extrinsics.cpp:20-22, 58), then the given fields; qbl (n, 4) as (x, y, z, w), tbl (n, 3)"""
    o = InitExtOpts()
    load_library().mlh_initext_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    for name, src in (("qbl", qbl), ("tbl", tbl)):
        if src is not None:
            for i, row in enumerate(np.asarray(src, np.float64)):
                for j, v in enumerate(row):
                    getattr(o, name)[i][j] = float(v)
    return o


class SegmentParams(C.Structure):
    _fields_ = [("vertical_scans", C.c_int32), ("horizon_scans", C.c_int32), ("min_cluster_size", C.c_int32), ("segment_valid_point_num", C.c_int32),
                ("segment_valid_line_num", C.c_int32), ("segment_theta", C.c_float), ("roi_range", C.c_double), ("segment_flag", C.c_int32)]


class TrackOpts(C.Structure):
    _fields_ = [("distance_sq_threshold", C.c_float), ("nearby_scan", C.c_float), ("huber_delta", C.c_double),
                ("max_outer", C.c_int32), ("max_lm_iterations", C.c_int32)]


class IterStat(C.Structure):
    _fields_ = [("n_surf", C.c_int32), ("n_corner", C.c_int32), ("is_degenerate", C.c_int32), ("lm_iterations", C.c_int32),
                ("successful_steps", C.c_int32), ("termination", C.c_int32), ("cost", C.c_double), ("final_cost", C.c_double),
                ("eigval", C.c_double * 6), ("H", C.c_double * 36), ("g", C.c_double * 6), ("pose_after", C.c_double * 7)]

    def as_dict(self):
        return dict(n_surf=self.n_surf, n_corner=self.n_corner, is_degenerate=bool(self.is_degenerate),
                    lm_iterations=self.lm_iterations, successful_steps=self.successful_steps, termination=self.termination,
                    cost=self.cost, final_cost=self.final_cost, eigval=np.array(self.eigval), H=np.array(self.H).reshape(6, 6),
                    g=np.array(self.g), pose_after=np.array(self.pose_after))


class DeviceInfo(C.Structure):
    """mlh_device_info (include/mloam_hip.h)."""
    _fields_ = [("cu_count", C.c_int32), ("cu_solver", C.c_int32), ("loop_blocks_per_cu", C.c_int32 * 3), ("loop_max_tiles", C.c_int32 * 3),
                ("scan_uploads_from_ahead", C.c_int32), ("loop_launches", C.c_uint64), ("loop_timeouts", C.c_uint64), ("loop_fallbacks", C.c_uint64)]

    def as_dict(self):
        return dict(cu_count=self.cu_count, cu_solver=self.cu_solver, loop_blocks_per_cu=list(self.loop_blocks_per_cu),
                    loop_max_tiles=list(self.loop_max_tiles), loop_launches=int(self.loop_launches), loop_timeouts=int(self.loop_timeouts),
                    loop_fallbacks=int(self.loop_fallbacks), scan_uploads_from_ahead=int(self.scan_uploads_from_ahead))


class ThinInfo(C.Structure):
    """mlh_thin_info_t (include/mloam_hip.h)."""
    _fields_ = [("path", C.c_int32), ("n_in", C.c_int32 * 2), ("reserved", C.c_int32)]


_lib = None


def load_library():
    """Loads libmloam_hip.so; raises MlhError when it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MlhError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    lib = C.CDLL(LIB_PATH)
    vp, ci, cf, cd = C.c_void_p, C.c_int, C.c_float, C.c_double
    lib.mlh_create.argtypes = [C.POINTER(vp), ci]
    lib.mlh_destroy.argtypes = [vp]
    lib.mlh_destroy.restype = None
    lib.mlh_last_error.argtypes = [vp]
    lib.mlh_last_error.restype = C.c_char_p
    lib.mlh_version.restype = C.c_char_p
    lib.mlh_stream.argtypes = [vp]
    lib.mlh_stream.restype = vp
    lib.mlh_synchronize.argtypes = [vp]
    lib.mlh_get_info.argtypes = [vp, C.POINTER(DeviceInfo)]
    lib.mlh_profile_enable.argtypes = [vp, ci]
    lib.mlh_comm_finalize.argtypes = [vp]
    lib.mlh_profile_sample.argtypes = [vp, ci]
    lib.mlh_profile_reset.argtypes = [vp]
    lib.mlh_profile_get.argtypes = [vp, ci, C.POINTER(cd), C.POINTER(C.c_longlong)]
    lib.mlh_scan_upload.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, ci]
    lib.mlh_scan_upload_ahead.argtypes = [vp, vp, ci, ci]
    lib.mlh_segment_params_default.argtypes = [C.POINTER(SegmentParams)]
    lib.mlh_segment_params_default.restype = None
    lib.mlh_segment_cloud.argtypes = [vp, vp, ci, ci, ci, ci, C.POINTER(SegmentParams), vp, C.POINTER(C.c_int32), vp, vp, vp, ci, C.POINTER(C.c_int32)]
    lib.mlh_extract_run.argtypes = [vp]
    lib.mlh_extract_fetch.argtypes = [vp, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_int32)]
    lib.mlh_extract_voxel_run.argtypes = [vp, cf]
    lib.mlh_extract_fetch_voxel.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_point_uncertainty.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, vp, cd, vp, vp]
    dp = C.POINTER(C.c_double)
    lib.mlh_cloud_uct_associate_to_map.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, ci, cd, vp, C.POINTER(C.c_int32), ci]
    lib.mlh_compound_pose_with_cov.argtypes = [vp, vp, vp, vp, vp, vp]
    i32p = C.POINTER(C.c_int32)
    lib.mlh_keyframes_reset.argtypes = [vp]
    lib.mlh_keyframe_save.argtypes = [vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, i32p]
    lib.mlh_keyframe_save_staged.argtypes = [vp, vp, vp, i32p]
    lib.mlh_local_map_assemble.argtypes = [vp, vp, vp, vp, ci, C.POINTER(LocalMapOpts), i32p, i32p, i32p, i32p, i32p]
    lib.mlh_local_map_clear.argtypes = [vp]
    lib.mlh_local_map_cloud.argtypes = [vp, ci, ci, C.POINTER(vp), i32p]
    lib.mlh_local_map_info.argtypes = [vp, i32p, i32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.mlh_keyframe_attach_outlier.argtypes = [vp, C.c_int32, vp, ci, ci, ci, ci]
    lib.mlh_global_map_opts_default.argtypes = [C.POINTER(GlobalMapOpts), ci]
    lib.mlh_global_map_opts_default.restype = None
    lib.mlh_global_map_assemble.argtypes = [vp, vp, vp, vp, ci, C.POINTER(GlobalMapOpts), i32p, i32p, i32p, i32p]
    lib.mlh_global_map_cloud.argtypes = [vp, ci, ci, C.POINTER(vp), i32p]
    lib.mlh_global_map_release.argtypes = [vp]
    lib.mlh_global_map_select.argtypes = [vp, ci, vp, cf, cf, vp, i32p]
    lib.mlh_keyframes_update_poses.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, ci, i32p, vp]
    lib.mlh_keyframes_update_from_pose_graph.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, ci, i32p, vp]
    lib.mlh_keyframes_update_from_pose_graph_cov.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, ci, C.c_int32, i32p, vp]
    lib.mlh_keyframe_poses.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    i64p = C.POINTER(C.c_int64)
    lib.mlh_window_map_opts_default.argtypes = [C.POINTER(WindowMapOpts), ci, ci, ci]
    lib.mlh_window_map_opts_default.restype = None
    lib.mlh_window_reset.argtypes = [vp, ci, ci]
    lib.mlh_window_set.argtypes = [vp, ci, ci, vp, ci, vp, ci, ci, ci, ci]
    lib.mlh_window_set_from_scan.argtypes = [vp, vp, ci, ci, cf, cf]
    lib.mlh_window_slide.argtypes = [vp, ci]
    lib.mlh_window_cloud.argtypes = [vp, ci, ci, ci, C.POINTER(vp), i32p]
    lib.mlh_window_info.argtypes = [vp, i32p, i32p, i64p, i64p, i64p, i64p]
    lib.mlh_window_build_local_map.argtypes = [vp, vp, C.POINTER(WindowMapOpts), i32p, i32p]
    lib.mlh_window_map_cloud.argtypes = [vp, ci, ci, ci, C.POINTER(vp), i32p]
    lib.mlh_downsample_current_scan.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, vp, vp, ci, vp, ci, cd, vp, C.POINTER(C.c_int32)]
    lib.mlh_track_opts_default.argtypes = [vp]
    lib.mlh_track_opts_default.restype = None
    lib.mlh_track_set_prev.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf]
    lib.mlh_track_set_cur.argtypes = [vp, ci, vp, ci, ci, ci, ci]
    lib.mlh_track_set_from_scan.argtypes = [vp, ci, cf]
    lib.mlh_downsample_current_scan_pair.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, cf, cf, vp, vp, ci, vp, ci, C.c_double, vp, vp]
    lib.mlh_downsample_scan2map.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, cf, cf, vp, vp, ci, vp, ci, C.c_double, vp, vp, vp, vp]
    lib.mlh_features_fetch.argtypes = [vp, ci, vp, ci, C.POINTER(C.c_int32)]
    lib.mlh_thin_info.argtypes = [vp, C.POINTER(ThinInfo)]
    lib.mlh_voxel_grid.argtypes = [vp, vp, ci, ci, ci, cf, vp, vp, ci]
    lib.mlh_transform_point_cloud.argtypes = [vp, vp, ci, ci, vp, ci]
    lib.mlh_transform_to_end.argtypes = [vp, vp, ci, ci, ci, vp, ci, cf, ci]
    lib.mlh_scan_undistort.argtypes = [vp, vp, cf]
    lib.mlh_fuse_reset.argtypes = [vp]
    lib.mlh_fuse_add_scan.argtypes = [vp, ci, vp]
    lib.mlh_fuse_add_scan_from.argtypes = [vp, vp, ci, vp]
    lib.mlh_fuse_add_rings.argtypes = [vp, ci, ci, ci, vp]
    lib.mlh_fused_cloud.argtypes = [vp, ci, vp, vp]
    lib.mlh_track_match.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.mlh_track_cloud.argtypes = [vp, vp, vp, vp]
    lib.mlh_pure_odom_set.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    lib.mlh_pure_odom_evaluate.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp]
    lib.mlh_pure_odom_normal_eq.argtypes = [vp, vp, vp, ci, vp, ci, cd, vp, vp, C.POINTER(cd), C.POINTER(C.c_int32)]
    lib.mlh_pure_odom_gn_solve.argtypes = [vp, vp, vp, ci, vp, ci, cd, ci, C.c_uint32, vp, C.POINTER(cd), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mlh_window_prior_set.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.mlh_window_prior_get.argtypes = [vp, C.POINTER(WindowPriorInfo), vp, vp, vp, vp]
    lib.mlh_window_prior_clear.argtypes = [vp]
    lib.mlh_window_prior_evaluate.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, C.POINTER(cd)]
    lib.mlh_window_ext_prior_set.argtypes = [vp, ci, vp, C.c_uint32]
    lib.mlh_window_marginalize.argtypes = [vp, vp, vp, ci, vp, ci, cd, C.POINTER(WindowPriorInfo)]
    lib.mlh_voxel_filter.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, vp, C.POINTER(C.c_int32), ci]
    lib.mlh_map_set.argtypes = [vp, ci, vp, ci, ci, cf, ci]
    lib.mlh_map_set_pair.argtypes = [vp, vp, ci, vp, ci, ci, cf, ci]
    lib.mlh_map_set_pair_overlapped.argtypes = [vp, vp, ci, vp, ci, ci, cf, ci]
    lib.mlh_map_rebuild.argtypes = [vp, ci]
    lib.mlh_map_info.argtypes = [vp, ci, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(cd), C.POINTER(C.c_int32)]
    lib.mlh_set_voxel_member_order.argtypes = [vp, ci]
    lib.mlh_set_extract_tie_order.argtypes = [vp, ci]
    lib.mlh_set_gn_schedule.argtypes = [vp, ci, ci, ci]
    lib.mlh_scan2map_begin.argtypes = [vp, vp, C.POINTER(SolverOpts), ci]
    lib.mlh_scan2map_begin_chained.argtypes = [vp, vp, vp, C.POINTER(SolverOpts), ci]
    lib.mlh_scan2map_end.argtypes = [vp, vp, vp]
    lib.mlh_scan2map_cov.argtypes = [vp, vp, vp]
    lib.mlh_std_sort_permutation.argtypes = [vp, vp, ci, ci, vp, ci]
    lib.mlh_debug_bad_launch.argtypes = [vp]
    lib.mlh_pure_odom_begin.argtypes = [vp]
    lib.mlh_calib_accumulate.argtypes = [vp, ci, vp, ci, C.c_uint32, cf, cf, ci]
    lib.mlh_calib_add.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    lib.mlh_calib_use.argtypes = [vp, ci]
    lib.mlh_calib_clear.argtypes = [vp]
    lib.mlh_calib_info.argtypes = [vp, C.POINTER(CalibStoreInfo)]
    lib.mlh_calib_evaluate.argtypes = [vp, vp, ci, vp, vp]
    lib.mlh_sc_opts_default.argtypes = [C.POINTER(ScOpts)]
    lib.mlh_sc_opts_default.restype = None
    lib.mlh_sc_reset.argtypes = [vp, C.POINTER(ScOpts)]
    lib.mlh_sc_add.argtypes = [vp, vp, vp, ci, ci, ci, vp, C.POINTER(C.c_int32)]
    lib.mlh_sc_add_keyframe.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.mlh_sc_add_keyframes.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.mlh_sc_last_batch.argtypes = [vp, C.POINTER(ScBatchInfo)]
    lib.mlh_session_export_size.argtypes = [vp, C.c_uint32, C.POINTER(C.c_size_t)]
    lib.mlh_session_export.argtypes = [vp, C.c_uint32, vp, C.c_size_t, ci, C.POINTER(C.c_size_t)]
    lib.mlh_session_inspect.argtypes = [vp, C.c_size_t, C.POINTER(SessionInfo)]
    lib.mlh_session_import.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.POINTER(SessionInfo)]
    lib.mlh_session_last_info.argtypes = [vp, C.POINTER(SessionInfo)]
    lib.mlh_sc_detect.argtypes = [vp, C.c_int32, C.POINTER(ScResult)]
    lib.mlh_sc_candidates.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_sc_distance.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(cd), C.POINTER(C.c_int32)]
    lib.mlh_sc_fetch.argtypes = [vp, C.c_int32, vp, vp, vp]
    lib.mlh_sc_info.argtypes = [vp, C.POINTER(ScStoreInfo)]
    lib.mlh_loop_opts_default.argtypes = [C.POINTER(LoopOpts)]
    lib.mlh_loop_opts_default.restype = None
    lib.mlh_loop_build_clouds.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.POINTER(LoopOpts), vp, vp]
    lib.mlh_loop_set_clouds.argtypes = [vp, vp, vp, ci, ci, ci]
    lib.mlh_loop_cloud.argtypes = [vp, ci, ci, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    lib.mlh_loop_info_get.argtypes = [vp, C.POINTER(LoopInfo)]
    lib.mlh_loop_match.argtypes = [vp, ci, vp, C.POINTER(LoopOpts), vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_loop_evaluate.argtypes = [vp, vp, vp, C.POINTER(LoopOpts), vp, vp, C.POINTER(cd), vp]
    lib.mlh_loop_register.argtypes = [vp, vp, C.POINTER(LoopOpts), C.POINTER(LoopResult)]
    lib.mlh_fgr_opts_default.argtypes = [C.POINTER(FgrOpts)]
    lib.mlh_fgr_opts_default.restype = None
    for fn in (lib.mlh_fgr_features, lib.mlh_fgr_spfh, lib.mlh_fgr_fpfh):
        fn.argtypes = [vp, ci, C.POINTER(FgrOpts)]
    lib.mlh_fgr_fetch.argtypes = [vp, ci, ci, vp, vp]
    lib.mlh_fgr_set_normals.argtypes = [vp, ci, C.c_int32, vp]
    lib.mlh_fgr_set_spfh.argtypes = [vp, ci, C.c_int32, vp, vp]
    lib.mlh_fgr_set_features.argtypes = [vp, ci, C.c_int32, vp]
    lib.mlh_fgr_match.argtypes = [vp, C.POINTER(FgrOpts), vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.mlh_fgr_register.argtypes = [vp, C.POINTER(FgrOpts), C.POINTER(FgrResult)]
    lib.mlh_fgr_register_device.argtypes = [vp, C.POINTER(FgrOpts), C.POINTER(FgrResult)]
    lib.mlh_fgr_tail_tuple_test.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(FgrOpts), vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mlh_fgr_tail_optimize.argtypes = [vp, vp, C.c_int32, C.c_double, C.POINTER(FgrOpts), vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_fgr_info.argtypes = [vp, C.POINTER(FgrInfo)]
    lib.mlh_pg_opts_default.argtypes = [C.POINTER(PgOpts)]
    lib.mlh_pg_opts_default.restype = None
    lib.mlh_pg_reset.argtypes = [vp]
    lib.mlh_pg_info.argtypes = [vp, C.POINTER(PgInfo)]
    lib.mlh_pg_reserve.argtypes = [vp, C.c_int32]
    lib.mlh_pg_add_keyframe.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_pg_set_loop.argtypes = [vp, C.c_int32, C.c_int32, vp]
    lib.mlh_pg_optimize.argtypes = [vp, C.c_int32, C.POINTER(PgOpts), C.POINTER(PgResult)]
    lib.mlh_pg_poses.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    lib.mlh_pg_device_poses.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mlh_pg_linearize.argtypes = [vp, C.c_int32, C.POINTER(PgOpts), C.POINTER(C.c_int32), vp, vp, vp, vp, C.POINTER(cd_), vp, vp]
    lib.mlh_pg_solve_step.argtypes = [vp, C.c_int32, C.POINTER(PgOpts), cd_, vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_pg_time_stages.argtypes = [vp, C.c_int32, C.POINTER(PgOpts), C.POINTER(PgResult), vp]
    lib.mlh_pg_optimize_forced.argtypes = [vp, C.c_int32, C.POINTER(PgOpts), C.c_uint32, C.POINTER(PgResult)]
    lib.mlh_pg_marginals.argtypes = [vp, C.c_int32, C.POINTER(PgOpts), C.c_int32, vp, C.POINTER(PgMarginalsResult)]
    lib.mlh_pg_device_marginals.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mlh_initext_opts_default.argtypes = [C.POINTER(InitExtOpts)]
    lib.mlh_initext_opts_default.restype = None
    lib.mlh_initext_reset.argtypes = [vp, C.POINTER(InitExtOpts)]
    lib.mlh_initext_add_pose.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_initext_calibrate.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(InitExtResult)]
    lib.mlh_initext_info.argtypes = [vp, C.POINTER(InitExtInfo)]
    lib.mlh_initext_read_state.argtypes = [vp, vp, vp, vp]
    lib.mlh_pure_odom_add_matches.argtypes = [vp, ci, vp, ci, C.c_uint32, cf, cf, ci, ci]
    lib.mlh_pure_odom_add_matches_gf.argtypes = [vp, ci, vp, vp, vp, vp, ci, C.c_uint32, cf, cf, ci, ci, cf, C.c_uint64, vp, C.POINTER(C.c_int32)]
    lib.mlh_knn.argtypes = [vp, ci, vp, ci, ci, vp, vp]
    lib.mlh_features_set.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci]
    lib.mlh_features_set_block.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci]
    lib.mlh_gn_solve_blocks.argtypes = [vp, vp, ci, C.POINTER(SolverOpts), C.POINTER(BlockOpts), vp]
    lib.mlh_match_linearize.argtypes = [vp, ci, vp, ci, C.c_uint32, cf, cf, cd, cd, vp, vp, vp, vp, vp, vp, C.POINTER(cd), C.POINTER(C.c_int32)]
    lib.mlh_match_coeffs.argtypes = [vp, ci, vp, vp, C.POINTER(C.c_int32)]
    lib.mlh_match_neighbours.argtypes = [vp, ci, vp, C.POINTER(C.c_int32)]
    lib.mlh_linearize.argtypes = [vp, ci, vp, C.c_uint32, cd, cd, vp, vp, vp, vp, C.POINTER(cd), C.POINTER(C.c_int32)]
    lib.mlh_good_feature_matching.argtypes = [vp, ci, vp, ci, cd, C.c_uint64, cf, cf, vp, C.POINTER(C.c_int32), vp, vp]
    lib.mlh_solver_opts_default.argtypes = [C.POINTER(SolverOpts)]
    lib.mlh_solver_opts_default.restype = None
    lib.mlh_gn_solve.argtypes = [vp, vp, ci, C.POINTER(SolverOpts), vp]
    lib.mlh_gn_solve_begin.argtypes = [vp, vp, ci, C.POINTER(SolverOpts)]
    lib.mlh_features_copy.argtypes = [vp, vp, ci]
    lib.mlh_gn_solve_begin_chained.argtypes = [vp, vp, vp, ci, C.POINTER(SolverOpts)]
    lib.mlh_gn_solve_end.argtypes = [vp, vp]
    lib.mlh_scan2map.argtypes = [vp, vp, C.POINTER(SolverOpts), vp]
    lib.mlh_shard_set.argtypes = [vp, vp, vp]
    lib.mlh_shard_set_features.argtypes = [vp, ci, ci]
    lib.mlh_comm_unique_id.argtypes = [vp]
    lib.mlh_comm_init.argtypes = [vp, ci, ci, vp]
    lib.mlh_p2p_mailbox.argtypes = [vp, vp]
    lib.mlh_p2p_comm_init.argtypes = [vp, ci, ci, vp]
    lib.mlh_allreduce_f64.argtypes = [vp, vp, ci]
    lib.mlh_pose_plus.argtypes = [vp, vp, vp, vp]
    lib.mlh_eval_degeneracy.argtypes = [vp, cd, vp, vp]
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "mlh_create", "mlh_destroy", "mlh_last_error", "mlh_version", "mlh_stream", "mlh_synchronize", "mlh_get_info",
    "mlh_comm_finalize", "mlh_profile_enable", "mlh_profile_sample", "mlh_profile_reset", "mlh_profile_get",
    "mlh_segment_params_default", "mlh_segment_cloud", "mlh_scan_upload", "mlh_scan_upload_ahead", "mlh_extract_run", "mlh_extract_fetch", "mlh_extract_voxel_run", "mlh_extract_fetch_voxel",
    "mlh_point_uncertainty", "mlh_downsample_current_scan", "mlh_voxel_filter", "mlh_pure_odom_set", "mlh_pure_odom_evaluate", "mlh_pure_odom_normal_eq", "mlh_track_opts_default", "mlh_track_set_prev", "mlh_track_set_cur",
    "mlh_track_set_from_scan", "mlh_downsample_current_scan_pair", "mlh_downsample_scan2map", "mlh_features_fetch", "mlh_thin_info", "mlh_voxel_grid", "mlh_transform_point_cloud", "mlh_transform_to_end", "mlh_scan_undistort", "mlh_fuse_reset", "mlh_fuse_add_scan", "mlh_fuse_add_scan_from", "mlh_fuse_add_rings", "mlh_fused_cloud", "mlh_track_match", "mlh_track_cloud", "mlh_cloud_uct_associate_to_map", "mlh_compound_pose_with_cov",
    "mlh_map_set", "mlh_map_set_pair", "mlh_map_set_pair_overlapped", "mlh_map_rebuild", "mlh_map_info", "mlh_set_voxel_member_order", "mlh_debug_bad_launch", "mlh_set_extract_tie_order", "mlh_set_gn_schedule", "mlh_std_sort_permutation", "mlh_pure_odom_begin", "mlh_pure_odom_add_matches", "mlh_pure_odom_add_matches_gf", "mlh_pure_odom_gn_solve", "mlh_knn", "mlh_features_set", "mlh_features_set_block", "mlh_gn_solve_blocks",
    "mlh_match_linearize", "mlh_match_coeffs", "mlh_match_neighbours", "mlh_linearize", "mlh_good_feature_matching", "mlh_solver_opts_default", "mlh_gn_solve", "mlh_gn_solve_begin", "mlh_gn_solve_begin_chained", "mlh_gn_solve_end", "mlh_features_copy", "mlh_scan2map", "mlh_scan2map_begin", "mlh_scan2map_begin_chained", "mlh_scan2map_end", "mlh_scan2map_cov",
    "mlh_shard_set", "mlh_shard_set_features", "mlh_comm_unique_id", "mlh_comm_init", "mlh_p2p_mailbox", "mlh_p2p_comm_init", "mlh_allreduce_f64",
    "mlh_pose_plus", "mlh_eval_degeneracy",
    "mlh_keyframes_reset", "mlh_keyframe_save", "mlh_keyframe_save_staged", "mlh_local_map_assemble", "mlh_local_map_clear", "mlh_local_map_cloud", "mlh_local_map_info",
    "mlh_keyframe_attach_outlier", "mlh_global_map_opts_default", "mlh_global_map_assemble", "mlh_global_map_cloud", "mlh_global_map_release", "mlh_global_map_select",
    "mlh_keyframes_update_poses", "mlh_keyframes_update_from_pose_graph", "mlh_keyframes_update_from_pose_graph_cov", "mlh_keyframe_poses",
    "mlh_initext_opts_default", "mlh_initext_reset", "mlh_initext_add_pose", "mlh_initext_calibrate", "mlh_initext_info", "mlh_initext_read_state",
    "mlh_window_map_opts_default", "mlh_window_reset", "mlh_window_set", "mlh_window_set_from_scan", "mlh_window_slide", "mlh_window_cloud", "mlh_window_info",
    "mlh_window_build_local_map", "mlh_window_map_cloud",
    "mlh_window_prior_set", "mlh_window_prior_get", "mlh_window_prior_clear", "mlh_window_prior_evaluate", "mlh_window_ext_prior_set", "mlh_window_marginalize",
    "mlh_calib_accumulate", "mlh_calib_add", "mlh_calib_use", "mlh_calib_clear", "mlh_calib_info", "mlh_calib_evaluate",
    "mlh_sc_opts_default", "mlh_sc_reset", "mlh_sc_add", "mlh_sc_add_keyframe", "mlh_sc_add_keyframes", "mlh_sc_last_batch", "mlh_sc_detect", "mlh_sc_candidates", "mlh_sc_distance", "mlh_sc_fetch", "mlh_sc_info",
    "mlh_loop_opts_default", "mlh_loop_build_clouds", "mlh_loop_set_clouds", "mlh_loop_cloud", "mlh_loop_info_get", "mlh_loop_match", "mlh_loop_evaluate", "mlh_loop_register",
    "mlh_fgr_opts_default", "mlh_fgr_features", "mlh_fgr_spfh", "mlh_fgr_fpfh", "mlh_fgr_fetch", "mlh_fgr_set_normals", "mlh_fgr_set_spfh", "mlh_fgr_set_features",
    "mlh_fgr_match", "mlh_fgr_register", "mlh_fgr_register_device", "mlh_fgr_tail_tuple_test", "mlh_fgr_tail_optimize", "mlh_fgr_info",
    "mlh_pg_opts_default", "mlh_pg_reset", "mlh_pg_info", "mlh_pg_add_keyframe", "mlh_pg_set_loop", "mlh_pg_optimize", "mlh_pg_poses", "mlh_pg_device_poses",
    "mlh_pg_linearize", "mlh_pg_solve_step", "mlh_pg_time_stages", "mlh_pg_optimize_forced", "mlh_pg_reserve", "mlh_pg_marginals", "mlh_pg_device_marginals",
    "mlh_session_export_size", "mlh_session_export", "mlh_session_inspect", "mlh_session_import", "mlh_session_last_info",
]


_hip = None


def _hip_runtime():
    """the HIP runtime the library is linked against (already mapped into the process by load_library)"""
    global _hip
    if _hip is None:
        load_library()
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", os.path.join("/opt/rocm/lib", "libamdhip64.so")):
            try:
                _hip = C.CDLL(name)
                break
            except OSError:
                continue
        if _hip is None:
            raise MlhError("the HIP runtime library could not be loaded")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class DeviceCloud:
    """A device-resident cloud owned by the library (mlh_fused_cloud): pointer, record count, record stride in bytes."""
    def __init__(self, ptr, n, stride=16):
        self.ptr, self.n, self.stride = ptr, n, stride


def _src(points):
    """(pointer, stride_bytes, n, mem, keepalive) for a numpy array (host), a torch CUDA tensor or a DeviceCloud (device)."""
    if isinstance(points, DeviceCloud):
        return C.c_void_p(points.ptr), points.stride, points.n, MEM_DEVICE, points
    if isinstance(points, np.ndarray):
        a = np.ascontiguousarray(points, np.float32)
        return a.ctypes.data_as(C.c_void_p), a.shape[1] * 4, a.shape[0], MEM_HOST, a
    # torch tensor on the GPU
    t = points.contiguous()
    assert t.is_cuda and t.dtype.itemsize == 4
    return C.c_void_p(t.data_ptr()), t.shape[1] * 4, t.shape[0], MEM_DEVICE, t


def default_track_opts(**kw) -> TrackOpts:
    o = TrackOpts()
    load_library().mlh_track_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_opts(pose_cov: bool = False, **kw) -> SolverOpts:
    """mlh_solver_opts_default, then the given fields; pose_cov=True adds FLAG_POSE_COV to whatever `flags` says (Context.scan2map_cov reads the result)"""
    o = SolverOpts()
    load_library().mlh_solver_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    if pose_cov:
        o.flags |= FLAG_POSE_COV
    return o


class Context:
    """One mlh_ctx (one HIP stream, device-resident buffers)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.mlh_create(C.byref(h), device)
        if rc != 0:
            raise MlhError(f"mlh_create failed ({rc}): no usable HIP device {device}")
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.lib.mlh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise MlhError(f"mlh error {rc}: {self.lib.mlh_last_error(self.h).decode()}")

    def stream(self):
        return self.lib.mlh_stream(self.h)

    def synchronize(self):
        self._ck(self.lib.mlh_synchronize(self.h))

    def info(self) -> dict:
        """mlh_get_info: compute units, the in-kernel loops' residency gates and what became of them (launches / timeouts / fallbacks)."""
        di = DeviceInfo()
        self._ck(self.lib.mlh_get_info(self.h, C.byref(di)))
        return di.as_dict()

    # ---- profiling
    def profile_enable(self, kernel_mask=K_ALL):
        """kernel_mask: bit k brackets launches of kernel id k with HIP events (0/False = off, True = all)."""
        if kernel_mask is True:
            kernel_mask = K_ALL
        self._ck(self.lib.mlh_profile_enable(self.h, int(kernel_mask)))

    def profile_sample(self, every_n=1):
        self._ck(self.lib.mlh_profile_sample(self.h, int(every_n)))

    def profile_reset(self):
        self._ck(self.lib.mlh_profile_reset(self.h))

    def profile_get(self, kernel_id):
        ms, n = C.c_double(0), C.c_longlong(0)
        self._ck(self.lib.mlh_profile_get(self.h, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- extraction
    def scan_upload(self, points, scan_start, scan_end):
        ptr, stride, n, mem, keep = _src(points)
        if mem == MEM_HOST:
            ss = np.ascontiguousarray(scan_start, np.int32)
            se = np.ascontiguousarray(scan_end, np.int32)
            self._ck(self.lib.mlh_scan_upload(self.h, ptr, stride, 12 if stride >= 16 else -1, n, _p(ss), _p(se), len(ss), mem))
        else:
            ss, se = scan_start.contiguous(), scan_end.contiguous()
            self._ck(self.lib.mlh_scan_upload(self.h, ptr, stride, 12 if stride >= 16 else -1, n, C.c_void_p(ss.data_ptr()), C.c_void_p(se.data_ptr()), ss.numel(), mem))
        self._scan_n = n

    def scan_upload_ahead(self, points):
        """mlh_scan_upload_ahead: the NEXT scan's points (a HOST array, kept alive and unchanged by the caller until the scan_upload that names it) go to the device
        now, beside the kernels of the current scan."""
        ptr, stride, n, mem, keep = _src(points)
        if mem != MEM_HOST:
            raise ValueError("scan_upload_ahead takes a host array")
        self._ck(self.lib.mlh_scan_upload_ahead(self.h, ptr, stride, n))

    def segment_cloud(self, points4, fetch=True, outlier_capacity=None, **kw):
        """ImageSegmenter::segmentCloud: unordered cloud (n, 4) [x y z intensity] (numpy or torch CUDA) -> the context's scan (ring-major, on the
        device) and, with fetch, the ring-major cloud / ScanInfo arrays / outlier cloud. kw: fields of SegmentParams."""
        prm = SegmentParams()
        self.lib.mlh_segment_params_default(C.byref(prm))
        for k, v in kw.items():
            setattr(prm, k, v)
        ptr, stride, n, mem, keep = _src(points4)
        vs = prm.vertical_scans
        out = np.zeros((max(n, 1), 4), np.float32) if fetch else None
        cap = min(n, vs * ((prm.horizon_scans + 4) // 5)) + 1 if outlier_capacity is None else int(outlier_capacity)
        outl = np.zeros((max(cap, 1), 4), np.float32) if fetch else None
        ss = np.zeros(vs, np.int32); se = np.zeros(vs, np.int32)
        no, nl = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_segment_cloud(self.h, ptr, stride, 12 if stride >= 16 else -1, n, mem, C.byref(prm), _p(out) if fetch else None, C.byref(no),
                                            _p(ss), _p(se), _p(outl) if fetch else None, cap, C.byref(nl)))
        self._scan_n = no.value
        return dict(cloud=out[:no.value].copy() if fetch else None, outlier=outl[:min(nl.value, cap)].copy() if fetch else None, n_outlier=nl.value, scan_start=ss, scan_end=se, n=no.value)

    def extract_run(self):
        self._ck(self.lib.mlh_extract_run(self.h))

    def extract_fetch(self):
        n = self._scan_n
        label = np.zeros(n, np.int32)
        curv = np.zeros(n, np.float32)
        picked = np.zeros(n, np.int32)
        lists = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        ptrs = (C.c_void_p * 4)(*[l.ctypes.data_as(C.c_void_p) for l in lists])
        cnt = (C.c_int32 * 4)()
        self._ck(self.lib.mlh_extract_fetch(self.h, _p(label), _p(curv), _p(picked), ptrs, cnt))
        names = ["sharp", "less_sharp", "flat", "less_flat_raw"]
        out = dict(label=label, curvature=curv, picked=picked)
        for i, nm in enumerate(names):
            out[nm] = lists[i][:cnt[i]].copy()
        return out

    def extract(self, points, scan_start, scan_end, voxel_leaf=None):
        self.scan_upload(points, scan_start, scan_end)
        self.extract_run()
        out = self.extract_fetch()
        if voxel_leaf:
            out["less_flat_ds"] = self.extract_voxel(voxel_leaf)
        return out

    def extract_voxel_run(self, leaf=0.2):
        """The per-ring VoxelGrid of the less-flat points, result kept on the device (for fuse_add_scan / track_set_from_scan)."""
        self._ck(self.lib.mlh_extract_voxel_run(self.h, leaf))

    def extract_voxel(self, leaf=0.2):
        """surf_points_less_flat after the per-ring VoxelGrid (feature_extract.cpp:266-271)."""
        self._ck(self.lib.mlh_extract_voxel_run(self.h, leaf))
        buf = np.zeros((max(self._scan_n, 1), 4), np.float32)
        n = C.c_int32(0)
        self._ck(self.lib.mlh_extract_fetch_voxel(self.h, _p(buf), C.byref(n)))
        return buf[:n.value].copy()

    def point_uncertainty(self, points, ext_poses, ext_covs, cov_measurement, trace_threshold=0.0):
        """points (n, >=4) [x y z lidar-id ...] -> (cov_vec (n, 6) f32, keep (n,) bool)."""
        ptr, stride, n, mem, keep = _src(points)
        ep = np.ascontiguousarray(ext_poses, np.float64).reshape(-1, 7)
        ec = np.ascontiguousarray(ext_covs, np.float64).reshape(-1, 36)
        cm = np.ascontiguousarray(cov_measurement, np.float64).reshape(9)
        cov = np.zeros((n, 6), np.float32)
        kp = np.zeros(n, np.int32)
        self._ck(self.lib.mlh_point_uncertainty(self.h, ptr, stride, n, 12, mem, _p(ep), _p(ec), ep.shape[0], _p(cm), trace_threshold, _p(cov), _p(kp)))
        return cov, kp.astype(bool)

    # ---- scan-to-scan odometry (LidarTracker)
    def track_set_prev(self, kind, points4, distance_sq_threshold=25.0):
        ptr, stride, n, mem, keep = _src(points4)
        self._ck(self.lib.mlh_track_set_prev(self.h, kind, ptr, stride, n, 12, mem, distance_sq_threshold))

    def track_set_cur(self, kind, points4):
        ptr, stride, n, mem, keep = _src(points4)
        self._ck(self.lib.mlh_track_set_cur(self.h, kind, ptr, stride, n, 12, mem))
        self._m_track = getattr(self, "_m_track", {})
        self._m_track[kind] = n

    def track_set_from_scan(self, which, distance_sq_threshold=25.0):
        """which = 0: current frame <- this context's scan (sharp / flat); 1: previous frame <- (less sharp / thinned less flat)."""
        self._ck(self.lib.mlh_track_set_from_scan(self.h, which, distance_sq_threshold))

    def voxel_grid(self, points4, leaf):
        """pcl::VoxelGrid<PointXYZI> over rows [x y z intensity] -> centroids (all four fields averaged), ascending voxel index."""
        ptr, stride, n, mem, keep = _src(points4)
        assert stride == 16 and mem == MEM_HOST
        out = np.zeros((n, 4), np.float32)
        cnt = C.c_int32(0)
        self._ck(self.lib.mlh_voxel_grid(self.h, ptr, 16, n, 12, float(leaf), _p(out), C.byref(cnt), MEM_HOST))
        return out[:cnt.value].copy()

    def transform_point_cloud(self, points4, pose):
        """pcl::transformPointCloud with the float 4x4 of `pose` (host array in, transformed copy out; intensity kept)."""
        a = np.array(points4, np.float32, order="C", copy=True)
        ps = np.ascontiguousarray(pose, np.float64).reshape(7)
        self._ck(self.lib.mlh_transform_point_cloud(self.h, _p(a), a.shape[1] * 4, a.shape[0], _p(ps), MEM_HOST))
        return a

    def transform_to_end(self, points4, pose, distortion=True, scan_period=0.1):
        """TransformToEnd over rows [x y z intensity] (host array in, transformed copy out)."""
        a = np.array(points4, np.float32, order="C", copy=True)
        assert a.shape[1] == 4
        ps = np.ascontiguousarray(pose, np.float64).reshape(7)
        self._ck(self.lib.mlh_transform_to_end(self.h, _p(a), 16, a.shape[0], 12, _p(ps), int(bool(distortion)), float(scan_period), MEM_HOST))
        return a

    def scan_undistort(self, pose_undist, scan_period=0.1):
        """Estimator::undistortMeasurements on the scan this context holds (in place, on the device)."""
        ps = np.ascontiguousarray(pose_undist, np.float64).reshape(7)
        self._ck(self.lib.mlh_scan_undistort(self.h, _p(ps), float(scan_period)))

    def fuse_reset(self):
        self._ck(self.lib.mlh_fuse_reset(self.h))

    def fuse_add_scan(self, lidar_idx, ext_pose):
        """transformCloudFeature for the scan this context holds: append its mapping features, in the body frame, to the fused clouds."""
        e = np.ascontiguousarray(ext_pose, np.float64).reshape(7)
        self._ck(self.lib.mlh_fuse_add_scan(self.h, int(lidar_idx), _p(e)))

    def fuse_add_scan_from(self, src, lidar_idx, ext_pose):
        """The same for the scan ANOTHER context of this device holds (extracted + voxel-thinned there): device to device, ordered by events."""
        e = np.ascontiguousarray(ext_pose, np.float64).reshape(7)
        self._ck(self.lib.mlh_fuse_add_scan_from(self.h, src.h, int(lidar_idx), _p(e)))

    def fuse_add_rings(self, ring_begin, ring_end, lidar_idx, ext_pose):
        """The same for rings [ring_begin, ring_end) of a scan that holds several LiDARs back to back."""
        e = np.ascontiguousarray(ext_pose, np.float64).reshape(7)
        self._ck(self.lib.mlh_fuse_add_rings(self.h, int(ring_begin), int(ring_end), int(lidar_idx), _p(e)))

    def fused_cloud(self, kind) -> "DeviceCloud":
        ptr, n = C.c_void_p(), C.c_int32(0)
        self._ck(self.lib.mlh_fused_cloud(self.h, kind, C.byref(ptr), C.byref(n)))
        return DeviceCloud(ptr.value, n.value)

    def track_match(self, kind, pose, opts=None):
        opts = opts or default_track_opts()
        pose = np.ascontiguousarray(pose, np.float64)
        m = self._m_track[kind]
        valid = np.zeros(m, np.uint8); coeffs = np.zeros((m, 6))
        self._ck(self.lib.mlh_track_match(self.h, kind, _p(pose), C.byref(opts), _p(valid), _p(coeffs)))
        return valid, coeffs

    def track_cloud(self, pose_ini, opts=None, want_stats=True):
        opts = opts or default_track_opts()
        pose = np.ascontiguousarray(pose_ini, np.float64).copy()
        if not want_stats:
            self._ck(self.lib.mlh_track_cloud(self.h, _p(pose), C.byref(opts), None))
            return pose, None
        stats = (IterStat * opts.max_outer)()
        self._ck(self.lib.mlh_track_cloud(self.h, _p(pose), C.byref(opts), C.cast(stats, C.c_void_p)))
        return pose, [s.as_dict() for s in stats]

    def pure_odom_set(self, types, points, coeffs, frame_idx, ext_idx, sqrt_info=None):
        t = np.ascontiguousarray(types, np.int32); fi = np.ascontiguousarray(frame_idx, np.int32); ei = np.ascontiguousarray(ext_idx, np.int32)
        p = np.ascontiguousarray(points, np.float64); c = np.ascontiguousarray(coeffs, np.float64)
        assert p.shape == (len(t), 3) and c.shape == (len(t), 6)
        si = None if sqrt_info is None else np.ascontiguousarray(sqrt_info, np.float64)
        self._ck(self.lib.mlh_pure_odom_set(self.h, len(t), _p(t), _p(p), _p(c), _p(si) if si is not None else None, _p(fi), _p(ei)))
        self._n_odom = len(t)

    def pure_odom_begin(self):
        """start a device-resident LidarPureOdom factor table (filled by pure_odom_add_matches)"""
        self._ck(self.lib.mlh_pure_odom_begin(self.h))
        self._n_odom = 0

    def pure_odom_add_matches(self, kind, rel_pose, frame_idx, ext_idx, k_neigh=5, flags=0, min_match_sq_dis=1.0, min_plane_dis=0.2):
        """match the staged features of `kind` at rel_pose = T_pivot^-1 T_frame T_ext and append the valid ones as factors, all on the device"""
        p = np.ascontiguousarray(rel_pose, np.float64)
        self._ck(self.lib.mlh_pure_odom_add_matches(self.h, kind, _p(p), int(k_neigh), int(flags), float(min_match_sq_dis), float(min_plane_dis),
                                                    int(frame_idx), int(ext_idx)))

    def pure_odom_add_matches_gf(self, kind, rel_pose, pivot, pose_i, ext, frame_idx, ext_idx, gf_ratio=0.8, seed=0, k_neigh=5, flags=0, min_match_sq_dis=1.0,
                                 min_plane_dis=0.2):
        """pure_odom_add_matches behind the odometry's good-feature selection (Estimator::goodFeatureMatching, estimator.cpp:1347-1517) -> the selected feature
        indices in selection order; only they are appended as factors"""
        a = [np.ascontiguousarray(x, np.float64) for x in (rel_pose, pivot, pose_i, ext)]
        sel = np.zeros(max(self._m[kind], 1), np.int32)
        n = C.c_int32(0)
        self._ck(self.lib.mlh_pure_odom_add_matches_gf(self.h, kind, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), int(k_neigh), int(flags), float(min_match_sq_dis),
                                                       float(min_plane_dis), int(frame_idx), int(ext_idx), float(gf_ratio), int(seed), _p(sel), C.byref(n)))
        return sel[:n.value].copy()

    def pure_odom_evaluate(self, pivot, frames, exts, want_jacobians=True):
        pv = np.ascontiguousarray(pivot, np.float64); fr = np.ascontiguousarray(frames, np.float64).reshape(-1, 7)
        ex = np.ascontiguousarray(exts, np.float64).reshape(-1, 7)
        r = np.zeros(self._n_odom); J = np.zeros((self._n_odom, 3, 7)) if want_jacobians else None
        self._ck(self.lib.mlh_pure_odom_evaluate(self.h, _p(pv), _p(fr), len(fr), _p(ex), len(ex), _p(r), _p(J) if J is not None else None))
        return r, J

    def pure_odom_normal_eq(self, pivot, frames, exts, huber_delta=1.0):
        """J^T J, J^T r, cost, count of the coupled window problem over [pivot | frames | extrinsics] (6 local parameters each)."""
        pv = np.ascontiguousarray(pivot, np.float64); fr = np.ascontiguousarray(frames, np.float64).reshape(-1, 7)
        ex = np.ascontiguousarray(exts, np.float64).reshape(-1, 7)
        D = 6 * (1 + len(fr) + len(ex))
        H = np.zeros((D, D)); g = np.zeros(D); cost = C.c_double(0); cnt = C.c_int32(0)
        self._ck(self.lib.mlh_pure_odom_normal_eq(self.h, _p(pv), _p(fr), len(fr), _p(ex), len(ex), float(huber_delta), _p(H), _p(g), C.byref(cost), C.byref(cnt)))
        return dict(H=H, g=g, cost=cost.value, count=cnt.value)

    def pure_odom_gn_solve(self, pivot, frames, exts, n_iters=5, huber_delta=1.0, const_blocks=None, V_update=None):
        """the coupled window problem [pivot | frames | extrinsics] solved on the device (mlh_pure_odom_gn_solve): n_iters Gauss-Newton iterations on the staged
        factor table; const_blocks: indices into [pivot, frames..., exts...] held constant (default: the pivot and extrinsic 0, as Estimator::optimizeMap does)."""
        pv = np.ascontiguousarray(pivot, np.float64)
        fr = np.ascontiguousarray(frames, np.float64).reshape(-1, 7).copy(); ex = np.ascontiguousarray(exts, np.float64).reshape(-1, 7).copy()
        nb = 1 + len(fr) + len(ex)
        const_blocks = [0, 1 + len(fr)] if const_blocks is None else list(const_blocks)
        mask = 0
        for b in const_blocks:
            mask |= 1 << int(b)
        V = None if V_update is None else np.ascontiguousarray(V_update, np.float64).reshape(nb, 36)
        cost, n, st = C.c_double(0), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_pure_odom_gn_solve(self.h, _p(pv), _p(fr), len(fr), _p(ex), len(ex), float(huber_delta), int(n_iters), mask, _p(V), C.byref(cost), C.byref(n), C.byref(st)))
        return dict(frames=fr, exts=ex, cost=cost.value, count=n.value, status=st.value)

    @staticmethod
    def _window_poses(pivot, frames, exts):
        return (np.ascontiguousarray(pivot, np.float64), np.ascontiguousarray(frames, np.float64).reshape(-1, 7), np.ascontiguousarray(exts, np.float64).reshape(-1, 7))

    def window_prior_set(self, block_ids, x0, J0, r0):
        """install a window prior (mlh_window_prior_set): kept block k -> window block block_ids[k], linearisation points, linearized_jacobians / _residuals"""
        ids = np.ascontiguousarray(block_ids, np.int32); nk = len(ids)
        x = np.ascontiguousarray(x0, np.float64).reshape(nk, 7); J = np.ascontiguousarray(J0, np.float64).reshape(6 * nk, 6 * nk)
        r = np.ascontiguousarray(r0, np.float64).reshape(6 * nk)
        self._ck(self.lib.mlh_window_prior_set(self.h, nk, _p(ids), _p(x), _p(J), _p(r)))

    def window_prior_info(self):
        info = WindowPriorInfo()
        self._ck(self.lib.mlh_window_prior_get(self.h, C.byref(info), None, None, None, None))
        return info.as_dict()

    def window_prior_get(self):
        """the installed prior (mlh_window_prior_get) or None"""
        info = self.window_prior_info()
        if not info["valid"]:
            return None
        nk, n = info["n_keep"], info["n"]
        ids = np.zeros(nk, np.int32); x0 = np.zeros((nk, 7)); J0 = np.zeros((n, n)); r0 = np.zeros(n)
        self._ck(self.lib.mlh_window_prior_get(self.h, None, _p(ids), _p(x0), _p(J0), _p(r0)))
        return dict(info=info, block_ids=ids, x0=x0, J0=J0, r0=r0)

    def window_prior_clear(self):
        self._ck(self.lib.mlh_window_prior_clear(self.h))

    def window_prior_evaluate(self, pivot, frames, exts):
        """MarginalizationFactor::Evaluate at a state (mlh_window_prior_evaluate): residuals, H, g, cost"""
        pv, fr, ex = self._window_poses(pivot, frames, exts)
        D = 6 * (1 + len(fr) + len(ex)); n = self.window_prior_info()["n"]
        res = np.zeros(n); H = np.zeros((D, D)); g = np.zeros(D); cost = C.c_double(0)
        self._ck(self.lib.mlh_window_prior_evaluate(self.h, _p(pv), _p(fr), len(fr), _p(ex), len(ex), _p(res), _p(H), _p(g), C.byref(cost)))
        return dict(residuals=res, H=H, g=g, cost=cost.value)

    def window_ext_prior_set(self, rows, in_marginalization=True, in_solve=False):
        """the extrinsics' PriorFactor (mlh_window_ext_prior_set): rows (n_ext, 9) = t, q(xyzw), pos_scale, rot_scale; None / empty removes them"""
        r = np.zeros((0, 9)) if rows is None else np.ascontiguousarray(rows, np.float64).reshape(-1, 9)
        self._ck(self.lib.mlh_window_ext_prior_set(self.h, len(r), _p(r) if len(r) else None, (1 if in_marginalization else 0) | (2 if in_solve else 0)))

    def window_marginalize(self, pivot, frames, exts, huber_delta=1.0):
        """marginalise the pivot at the given state (mlh_window_marginalize); the result replaces the installed prior -> info"""
        pv, fr, ex = self._window_poses(pivot, frames, exts)
        info = WindowPriorInfo()
        self._ck(self.lib.mlh_window_marginalize(self.h, _p(pv), _p(fr), len(fr), _p(ex), len(ex), float(huber_delta), C.byref(info)))
        return info.as_dict()

    def calib_add(self, types, points, coeffs, ext_idx, sqrt_info=None):
        """append LidarOnlineCalib factors to the context's calibration store from host lists (mlh_calib_add); ext_idx is per factor"""
        t = np.ascontiguousarray(types, np.int32); ei = np.ascontiguousarray(ext_idx, np.int32)
        p = np.ascontiguousarray(points, np.float64); c = np.ascontiguousarray(coeffs, np.float64)
        assert p.shape == (len(t), 3) and c.shape == (len(t), 6) and ei.shape == (len(t),)
        si = None if sqrt_info is None else np.ascontiguousarray(sqrt_info, np.float64)
        self._ck(self.lib.mlh_calib_add(self.h, len(t), _p(t), _p(p), _p(c), _p(si), _p(ei)))

    def calib_accumulate(self, kind, rel_pose, ext_idx, k_neigh=10, flags=FLAG_CHECK_FOV, min_match_sq_dis=1.0, min_plane_dis=0.2):
        """match the staged features of `kind` (LiDAR ext_idx's pivot-frame features) against the resident map (buildCalibMap's) at rel_pose and append the valid
        correspondences to the calibration store, all on the device (mlh_calib_accumulate)"""
        p = np.ascontiguousarray(rel_pose, np.float64)
        self._ck(self.lib.mlh_calib_accumulate(self.h, kind, _p(p), int(k_neigh), int(flags), float(min_match_sq_dis), float(min_plane_dis), int(ext_idx)))

    def calib_use(self, on=True):
        """whether the store's factors enter pure_odom_normal_eq / pure_odom_gn_solve / window_marginalize (the frame_cnt % N_CUMU_FEATURE == 0 gate)"""
        self._ck(self.lib.mlh_calib_use(self.h, 1 if on else 0))

    def calib_clear(self):
        self._ck(self.lib.mlh_calib_clear(self.h))

    def calib_info(self):
        info = CalibStoreInfo()
        self._ck(self.lib.mlh_calib_info(self.h, C.byref(info)))
        return info.as_dict()

    def calib_evaluate(self, exts, want_jacobians=True):
        """per-factor residual and 1 x 7 Jacobian row of a store made by calib_add, in the order given (mlh_calib_evaluate)"""
        ex = np.ascontiguousarray(exts, np.float64).reshape(-1, 7)
        n = self.calib_info()["n_valid"]
        r = np.zeros(n); J = np.zeros((n, 7)) if want_jacobians else None
        self._ck(self.lib.mlh_calib_evaluate(self.h, _p(ex), len(ex), _p(r), _p(J)))
        return r, J

    # ---- Scan Context place recognition (SCManager + detectLoop's distance rejection on the device)
    def sc_reset(self, opts: ScOpts = None):
        """setParameter: empties the store and zeroes the period counter (mlh_sc_reset); None: the shipped configuration"""
        self._sc_opts = opts if opts is not None else sc_opts()
        self._ck(self.lib.mlh_sc_reset(self.h, C.byref(self._sc_opts)))

    def sc_add(self, clouds, position=None):
        """makeAndSaveScancontextAndKeys of the concatenation of up to three clouds ((n, >= 3) float32 arrays, torch CUDA tensors or device clouds, all of one
        stride and memory kind; a single cloud may be given bare) -> the entry's index (mlh_sc_add)"""
        if not isinstance(clouds, (list, tuple)):
            clouds = [clouds]
        src = [_src(c) for c in clouds]
        live = [s for s in src if s[2] > 0] or src[:1]
        stride, mem = (live[0][1], live[0][3]) if live else (16, MEM_HOST)
        assert all(s[1] == stride and s[3] == mem for s in live), "the clouds share record stride and memory kind"
        ptrs = (C.c_void_p * max(len(src), 1))(*[(s[0] if s[2] > 0 else None) for s in src])
        ns = (C.c_int32 * max(len(src), 1))(*[s[2] for s in src])
        pos = None if position is None else np.ascontiguousarray(position, np.float64).reshape(3)
        idx = C.c_int32(-1)
        self._ck(self.lib.mlh_sc_add(self.h, ptrs, ns, len(src), stride, mem, _p(pos), C.byref(idx)))
        return idx.value

    def sc_add_keyframe(self, key):
        """the same from keyframe `key` of the mapper's store: its surf, corner and outlier clouds device to device, its stored translation (mlh_sc_add_keyframe)"""
        idx = C.c_int32(-1)
        self._ck(self.lib.mlh_sc_add_keyframe(self.h, int(key), C.byref(idx)))
        return idx.value

    def sc_add_keyframes(self, first_key, n):
        """keyframes [first_key, first_key + n) of the mapper's store as n entries, in a fixed number of launches: what n sc_add_keyframe calls leave -> the first
        entry's index (mlh_sc_add_keyframes)"""
        idx = C.c_int32(-1)
        self._ck(self.lib.mlh_sc_add_keyframes(self.h, int(first_key), int(n), C.byref(idx)))
        return idx.value

    def sc_last_batch(self) -> dict:
        """launches, host waits, chunks and point counts of the last sc_add_keyframes (mlh_sc_last_batch)"""
        info = ScBatchInfo()
        self._ck(self.lib.mlh_sc_last_batch(self.h, C.byref(info)))
        return info.as_dict()

    def sc_detect(self, que_index) -> dict:
        """detectLoopClosureID + detectLoop's distance rejection (mlh_sc_detect)"""
        r = ScResult()
        self._ck(self.lib.mlh_sc_detect(self.h, int(que_index), C.byref(r)))
        return r.as_dict()

    def sc_candidates(self, que_index, prefix):
        """the candidate search alone: (indices in scoring order, squared key distances) among entries [0, prefix) (mlh_sc_candidates)"""
        k = self._sc_opts.num_candidates
        idx, d2, n = np.zeros(k, np.int32), np.zeros(k, np.float32), C.c_int32(0)
        self._ck(self.lib.mlh_sc_candidates(self.h, int(que_index), int(prefix), _p(idx), _p(d2), C.byref(n)))
        return idx[:n.value].copy(), d2[:n.value].copy()

    def sc_distance(self, i, j):
        """distanceBtnScanContext(descriptor i, descriptor j) -> (distance, shift) (mlh_sc_distance)"""
        d, s = C.c_double(0.0), C.c_int32(0)
        self._ck(self.lib.mlh_sc_distance(self.h, int(i), int(j), C.byref(d), C.byref(s)))
        return d.value, s.value

    def sc_fetch(self, index):
        """entry `index` -> (descriptor (num_ring, num_sector) float64, ring key float32, sector key float64) (mlh_sc_fetch)"""
        R, S = self._sc_opts.num_ring, self._sc_opts.num_sector
        desc, rk, sk = np.zeros((S, R)), np.zeros(R, np.float32), np.zeros(S)
        self._ck(self.lib.mlh_sc_fetch(self.h, int(index), _p(desc), _p(rk), _p(sk)))
        return np.ascontiguousarray(desc.T), rk, sk

    def sc_info(self) -> dict:
        info = ScStoreInfo()
        self._ck(self.lib.mlh_sc_info(self.h, C.byref(info)))
        return info.as_dict()

    # ---- the session image (row f17): the keyframe store, the Scan Context store and the pose graph saved and restored
    def session_export_size(self, sections=SESSION_ALL) -> int:
        n = C.c_size_t(0)
        self._ck(self.lib.mlh_session_export_size(self.h, int(sections), C.byref(n)))
        return n.value

    def session_export(self, sections=SESSION_ALL) -> bytes:
        """the canonical byte image of the named stores (mlh_session_export into host memory)"""
        buf = np.zeros(max(self.session_export_size(sections), 1), np.uint8)
        n = C.c_size_t(0)
        self._ck(self.lib.mlh_session_export(self.h, int(sections), _p(buf), buf.nbytes, MEM_HOST, C.byref(n)))
        return buf[:n.value].tobytes()

    def session_import(self, image, sections=SESSION_ALL) -> dict:
        """the named sections of an image into this context's stores; a refused image leaves the context as it was (mlh_session_import)"""
        buf = np.frombuffer(bytes(image), np.uint8)
        info = SessionInfo()
        self._ck(self.lib.mlh_session_import(self.h, buf.ctypes.data_as(C.c_void_p) if len(buf) else None, len(buf), int(sections), C.byref(info)))
        # the bindings' copy of the SC options (sc_fetch and sc_candidates size their outputs by it)
        if int(sections) & SESSION_SC:
            at = int(np.frombuffer(bytes(image)[128:136], "<u8")[0])          # the SC section's offset: the third slot of the section table
            self._sc_opts = ScOpts.from_buffer_copy(bytes(image)[at:at + C.sizeof(ScOpts)])
        return info.as_dict()

    def session_last_info(self) -> dict:
        info = SessionInfo()
        self._ck(self.lib.mlh_session_last_info(self.h, C.byref(info)))
        return info.as_dict()

    # ---- loop-closure local registration (constructLocalMap + performLocalRegistration on the device)
    def loop_build_clouds(self, data, model, opts: LoopOpts = None):
        """constructLocalMap: data / model = lists of (keyframe key, 4 x 4 float32 matrix) -> (n_pre[4], n_ds[4]) in the order model surf, model corner, data surf,
        data corner (mlh_loop_build_clouds)"""
        def pack(lst):
            keys = np.ascontiguousarray([k for k, _ in lst], np.int32)
            mats = np.ascontiguousarray([np.asarray(m, np.float32).reshape(16) for _, m in lst], np.float32).reshape(-1, 16)
            return keys, mats
        dk, dm = pack(data)
        mk, mm = pack(model)
        n_pre, n_ds = np.zeros(4, np.int32), np.zeros(4, np.int32)
        self._ck(self.lib.mlh_loop_build_clouds(self.h, _p(dk), _p(dm), len(dk), _p(mk), _p(mm), len(mk), C.byref(opts) if opts is not None else None, _p(n_pre), _p(n_ds)))
        return n_pre, n_ds

    def loop_set_clouds(self, model_surf, model_corner, data_surf, data_corner):
        """the four filtered clouds given directly: (n, 4) float32 arrays {x, y, z, intensity} or torch CUDA tensors, all of one kind (mlh_loop_set_clouds)"""
        src = [_src(c) for c in (model_surf, model_corner, data_surf, data_corner)]
        mem = src[0][3]
        assert all(s[3] == mem and s[1] == 16 for s in src), "four (n, 4) clouds of one memory kind"
        ptrs = (C.c_void_p * 4)(*[(s[0] if s[2] > 0 else None) for s in src])
        ns = (C.c_int32 * 4)(*[s[2] for s in src])
        self._ck(self.lib.mlh_loop_set_clouds(self.h, ptrs, ns, 16, 12, mem))

    def loop_cloud(self, which, filtered=True, fetch=True):
        """cloud `which` (LOOP_MODEL_SURF ..), pre-filter or filtered: a DeviceCloud, or with fetch its (n, 4) float32 copy (mlh_loop_cloud)"""
        ptr, n = C.c_void_p(), C.c_int32(0)
        self._ck(self.lib.mlh_loop_cloud(self.h, int(which), int(bool(filtered)), C.byref(ptr), C.byref(n)))
        if not fetch:
            return DeviceCloud(ptr.value, n.value, 16)
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            self.synchronize()
            assert _hip_runtime().hipMemcpy(_p(out), ptr, out.nbytes, 2) == 0
        return out

    def loop_info(self) -> dict:
        info = LoopInfo()
        self._ck(self.lib.mlh_loop_info_get(self.h, C.byref(info)))
        return dict(n_pre=list(info.n_pre), n_ds=list(info.n_ds), allocations=int(info.allocations), bytes_hbm=int(info.bytes_hbm))

    def loop_match(self, kind, T, opts: LoopOpts = None):
        """matchSurfFromMap / matchCornerFromMap of the filtered data cloud at T (4 x 4) -> (valid (m,), coeffs (m, 4) or (m, 2, 4), features.size()) (mlh_loop_match)"""
        m = self.loop_info()["n_ds"][2 + kind]
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        valid = np.zeros(m, np.uint8)
        coeffs = np.zeros((m, 4) if kind == SURF else (m, 2, 4))
        n = C.c_int32(0)
        self._ck(self.lib.mlh_loop_match(self.h, int(kind), _p(T), C.byref(opts) if opts is not None else None, _p(valid), _p(coeffs), C.byref(n)))
        return valid.astype(bool), coeffs, n.value

    def loop_evaluate(self, T_match, pose, opts: LoopOpts = None) -> dict:
        """both matches at T_match, then one evaluation of every residual block at pose [t, q(xyzw)] -> H, g, cost, counts (mlh_loop_evaluate)"""
        T = np.ascontiguousarray(T_match, np.float64).reshape(16)
        x = np.ascontiguousarray(pose, np.float64).reshape(7)
        H, g, cost, counts = np.zeros((6, 6)), np.zeros(6), cd_(0.0), np.zeros(2, np.int32)
        self._ck(self.lib.mlh_loop_evaluate(self.h, _p(T), _p(x), C.byref(opts) if opts is not None else None, _p(H), _p(g), C.byref(cost), _p(counts)))
        return dict(H=H, g=g, cost=cost.value, counts=counts)

    def loop_register(self, T_ini, opts: LoopOpts = None) -> dict:
        """performLocalRegistration(the four filtered clouds, T_ini) (mlh_loop_register)"""
        T = np.ascontiguousarray(T_ini, np.float64).reshape(16)
        r = LoopResult()
        self._ck(self.lib.mlh_loop_register(self.h, _p(T), C.byref(opts) if opts is not None else None, C.byref(r)))
        return r.as_dict()

    # ---- FPFH + Fast Global Registration over the loop store's two surf clouds (performGlobalRegistration on the device)
    def fgr_info(self) -> dict:
        info = FgrInfo()
        self._ck(self.lib.mlh_fgr_info(self.h, C.byref(info)))
        return dict(n=list(info.n), have_normals=list(info.have_normals), have_spfh=list(info.have_spfh), have_features=list(info.have_features),
                    launches=info.launches, host_waits=info.host_waits, allocations=int(info.allocations), bytes_hbm=int(info.bytes_hbm))

    def fgr_features(self, which, opts: FgrOpts = None, first=FGR_NORMALS):
        """normals + SPFH + FPFH of cloud `which` (LOOP_MODEL_SURF / LOOP_DATA_SURF); first = FGR_SPFH / FGR_FPFH: from the normals / the SPFH counts in place
        (mlh_fgr_features, mlh_fgr_spfh, mlh_fgr_fpfh)"""
        fn = (self.lib.mlh_fgr_features, self.lib.mlh_fgr_spfh, self.lib.mlh_fgr_fpfh)[first]
        self._ck(fn(self.h, int(which), C.byref(opts) if opts is not None else None))

    def fgr_fetch(self, which, what):
        """FGR_NORMALS -> (n, 4) float32; FGR_SPFH -> ((n, 33) int32 counts, (n,) int32 neighbour counts); FGR_FPFH -> (n, 33) float32 (mlh_fgr_fetch)"""
        n = self.fgr_info()["n"][which >> 1] if what == FGR_FPFH else self.loop_info()["n_ds"][which]
        if what == FGR_SPFH:
            out, k = np.zeros((n, 33), np.int32), np.zeros(n, np.int32)
            self._ck(self.lib.mlh_fgr_fetch(self.h, int(which), what, _p(out), _p(k)))
            return out, k
        out = np.zeros((n, 4 if what == FGR_NORMALS else 33), np.float32)
        self._ck(self.lib.mlh_fgr_fetch(self.h, int(which), what, _p(out), None))
        return out

    def fgr_set_normals(self, which, normals4):
        a = np.ascontiguousarray(normals4, np.float32).reshape(-1, 4)
        self._ck(self.lib.mlh_fgr_set_normals(self.h, int(which), len(a), _p(a)))

    def fgr_set_spfh(self, which, counts, k):
        a, b = np.ascontiguousarray(counts, np.int32).reshape(-1, 33), np.ascontiguousarray(k, np.int32).reshape(-1)
        assert len(a) == len(b)
        self._ck(self.lib.mlh_fgr_set_spfh(self.h, int(which), len(a), _p(a), _p(b)))

    def fgr_set_features(self, which, features):
        a = np.ascontiguousarray(features, np.float32).reshape(-1, 33)
        self._ck(self.lib.mlh_fgr_set_features(self.h, int(which), len(a), _p(a)))

    def fgr_match(self, opts: FgrOpts = None):
        """AdvancedMatching up to the cross check on the two feature sets -> (m, 2) int32 (model index, data index) in ascending i (mlh_fgr_match)"""
        cap = max(1, min(self.fgr_info()["n"]))
        out, n = np.zeros((cap, 2), np.int32), C.c_int32(0)
        self._ck(self.lib.mlh_fgr_match(self.h, C.byref(opts) if opts is not None else None, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def fgr_register(self, opts: FgrOpts = None) -> dict:
        """performGlobalRegistration(model surf cloud, data surf cloud) (mlh_fgr_register)"""
        r = FgrResult()
        self._ck(self.lib.mlh_fgr_register(self.h, C.byref(opts) if opts is not None else None, C.byref(r)))
        return r.as_dict()

    def fgr_register_device(self, opts: FgrOpts = None) -> dict:
        """fgr_register with the tuple test and OptimizePairwise on the device: the same tuples, one 136-byte record to the host, one wait
        (mlh_fgr_register_device)"""
        r = FgrResult()
        self._ck(self.lib.mlh_fgr_register_device(self.h, C.byref(opts) if opts is not None else None, C.byref(r)))
        return r.as_dict()

    def fgr_tail_tuple_test(self, pq, swapped=False, opts: FgrOpts = None, capacity_tuples=None):
        """the device tuple test on host records pq (n, 6) = (p, q) -> ((k, 3) int32 indices into the records, n_trials). capacity_tuples: the rows of the output
        (default: min(tuple_max_cnt, 100 n), the least the call accepts) (mlh_fgr_tail_tuple_test)"""
        a = np.ascontiguousarray(pq, np.float32).reshape(-1, 6)
        o = opts if opts is not None else fgr_opts()
        cap = min(int(o.tuple_max_cnt), 100 * len(a)) if capacity_tuples is None else int(capacity_tuples)
        out, k, t = np.zeros((max(cap, 1), 3), np.int32), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_fgr_tail_tuple_test(self.h, _p(a), len(a), int(bool(swapped)), C.byref(o), _p(out), cap, C.byref(k), C.byref(t)))
        return out[:k.value].copy(), int(t.value)

    def fgr_tail_optimize(self, pq, start_scale=1.0, opts: FgrOpts = None):
        """the device OptimizePairwise on host records pq (n, 6), every record one correspondence -> (trans (4, 4) float32, (final_cost, final_cost_normalize),
        optimised) (mlh_fgr_tail_optimize)"""
        a = np.ascontiguousarray(pq, np.float32).reshape(-1, 6)
        trans, cost, ran = np.zeros(16, np.float32), np.zeros(2, np.float64), C.c_int32(0)
        self._ck(self.lib.mlh_fgr_tail_optimize(self.h, _p(a), len(a), float(start_scale), C.byref(opts) if opts is not None else None, _p(trans), _p(cost), C.byref(ran)))
        return trans.reshape(4, 4), (float(cost[0]), float(cost[1])), bool(ran.value)

    # ---- pose-graph optimisation (PoseGraph::addKeyFrame's bookkeeping, updateLoopInfo, optimizePoseGraph on the device)
    def pg_reset(self):
        self._ck(self.lib.mlh_pg_reset(self.h))

    def pg_info(self) -> dict:
        info = PgInfo()
        self._ck(self.lib.mlh_pg_info(self.h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in info._fields_}

    def pg_reserve(self, max_loops):
        """the context's capacity of loop edges of one problem, 128 .. PG_LOOPS_LIMIT; allocates nothing, survives pg_reset (mlh_pg_reserve)"""
        self._ck(self.lib.mlh_pg_reserve(self.h, int(max_loops)))

    def pg_add_keyframe(self, pose) -> int:
        """the keyframe's index (mlh_pg_add_keyframe); pose [t, q(xyzw)]"""
        p, idx = np.ascontiguousarray(pose, np.float64).reshape(7), C.c_int32(-1)
        self._ck(self.lib.mlh_pg_add_keyframe(self.h, _p(p), C.byref(idx)))
        return idx.value

    def pg_set_loop(self, index, loop_index, rel_pose):
        """KeyFrame::updateLoopInfo + the earliest-index rule (mlh_pg_set_loop)"""
        p = np.ascontiguousarray(rel_pose, np.float64).reshape(7)
        self._ck(self.lib.mlh_pg_set_loop(self.h, int(index), int(loop_index), _p(p)))

    def pg_optimize(self, cur_index, opts: PgOpts = None) -> dict:
        """one pass of optimizePoseGraph's body for cur_index (mlh_pg_optimize)"""
        r = PgResult()
        self._ck(self.lib.mlh_pg_optimize(self.h, int(cur_index), C.byref(opts) if opts is not None else None, C.byref(r)))
        return r.as_dict()

    def pg_optimize_forced(self, cur_index, fail_mask, opts: PgOpts = None) -> dict:
        """pg_optimize with the linear solve of iteration k + 1 declared failed for every set bit k of fail_mask (mlh_pg_optimize_forced: a test entry)"""
        r = PgResult()
        self._ck(self.lib.mlh_pg_optimize_forced(self.h, int(cur_index), C.byref(opts) if opts is not None else None, int(fail_mask), C.byref(r)))
        return r.as_dict()

    def pg_poses(self, first=0, n=None, last=False):
        """(n, 7) poses from `first`; with last: (poses, last poses) (mlh_pg_poses)"""
        n = self.pg_info()["n_keyframes"] - first if n is None else n
        a, b = np.zeros((n, 7)), np.zeros((n, 7))
        self._ck(self.lib.mlh_pg_poses(self.h, int(first), int(n), _p(a), _p(b) if last else None))
        return (a, b) if last else a

    def pg_device_poses(self):
        """(device pointer or None, stride in bytes, count) of the keyframe records in HBM (mlh_pg_device_poses)"""
        ptr, stride, cnt = C.c_void_p(None), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_pg_device_poses(self.h, C.byref(ptr), C.byref(stride), C.byref(cnt)))
        return ptr.value, stride.value, cnt.value

    def pg_linearize(self, cur_index, opts: PgOpts = None, dense=True) -> dict:
        """the problem's edges at the stored poses -> dict(ij (E, 2), r (E, 6), Ji, Jj (E, 6, 6), cost, H (n, n), g (n,)) (mlh_pg_linearize)"""
        info = self.pg_info()
        M = max(1, cur_index - max(info["earliest_loop_index"], 0) + 1)
        n = 6 * (M - 1)
        ij, r, Ji, Jj = np.zeros((5 * M, 2), np.int32), np.zeros((5 * M, 6)), np.zeros((5 * M, 6, 6)), np.zeros((5 * M, 6, 6))
        H, g = (np.zeros((n, n)), np.zeros(n)) if dense else (None, None)
        ne, cost = C.c_int32(0), cd_(0.0)
        self._ck(self.lib.mlh_pg_linearize(self.h, int(cur_index), C.byref(opts) if opts is not None else None, C.byref(ne), _p(ij), _p(r), _p(Ji), _p(Jj), C.byref(cost),
                                           _p(H) if dense else None, _p(g) if dense else None))
        e = ne.value
        return dict(ij=ij[:e].copy(), r=r[:e].copy(), Ji=Ji[:e].copy(), Jj=Jj[:e].copy(), cost=cost.value, H=H, g=g)

    def pg_solve_step(self, cur_index, radius, opts: PgOpts = None) -> dict:
        """one linear solve at the stored poses with the given radius -> dict(step, delta, ok) (mlh_pg_solve_step)"""
        info = self.pg_info()
        n = 6 * max(0, cur_index - max(info["earliest_loop_index"], 0))
        step, delta, ok = np.zeros(n), np.zeros(n), C.c_int32(0)
        self._ck(self.lib.mlh_pg_solve_step(self.h, int(cur_index), C.byref(opts) if opts is not None else None, float(radius), _p(step), _p(delta), C.byref(ok)))
        return dict(step=step, delta=delta, ok=bool(ok.value))

    PG_STAGE_NAMES = ("linearize", "assemble", "band_factor", "substitution", "gram", "dense_solve", "back_substitution", "lm_bookkeeping")

    def pg_marginals(self, cur_index, opts: PgOpts = None, form=PG_COV_LOCAL) -> dict:
        """the 6 x 6 diagonal blocks of H^-1 of the problem first..cur at the stored poses -> dict(cov (M, 6, 6) in `form`, ok, n_keyframes, n_loops, first_index,
        launches, host_waits); with ok == 0 cov is None (mlh_pg_marginals)"""
        info = self.pg_info()
        r = PgMarginalsResult()
        cov = np.zeros((max(info["n_keyframes"], 1), 6, 6))
        self._ck(self.lib.mlh_pg_marginals(self.h, int(cur_index), C.byref(opts) if opts is not None else None, int(form), _p(cov), C.byref(r)))
        out = {k: getattr(r, k) for k, _ in r._fields_}
        out["cov"] = cov[:r.n_keyframes].copy() if r.ok else None
        return out

    def pg_device_marginals(self):
        """(device pointer of the local form or None, of the store form or None, first_index, n_keyframes) of the valid marginals in HBM (mlh_pg_device_marginals)"""
        a, b, first, n = C.c_void_p(), C.c_void_p(), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_pg_device_marginals(self.h, C.byref(a), C.byref(b), C.byref(first), C.byref(n)))
        return a.value, b.value, first.value, n.value

    def pg_time_stages(self, cur_index, opts: PgOpts = None):
        """the launches of pg_optimize without the write-back, timed per stage -> (result dict, {stage: ms}) (mlh_pg_time_stages)"""
        r, ms = PgResult(), np.zeros(8)
        self._ck(self.lib.mlh_pg_time_stages(self.h, int(cur_index), C.byref(opts) if opts is not None else None, C.byref(r), _p(ms)))
        return r.as_dict(), dict(zip(self.PG_STAGE_NAMES, ms.tolist()))

    # ---- the initial extrinsic calibration (InitialExtrinsics: addPose, calibExRotation, calibExTranslation on the device)
    def initext_reset(self, opts: InitExtOpts = None):
        """clearState + setParameter (mlh_initext_reset)"""
        self._ck(self.lib.mlh_initext_reset(self.h, C.byref(opts) if opts is not None else None))

    def initext_add_pose(self, poses) -> bool:
        """addPose for one set of relative poses (n_lidar, 7) as [t, q(xyzw)] (mlh_initext_add_pose)"""
        p, acc = np.ascontiguousarray(poses, np.float64), C.c_int32(0)
        if p.size != 7 * self.initext_info()["n_lidar"]:
            raise ValueError("poses must be (n_lidar, 7)")
        self._ck(self.lib.mlh_initext_add_pose(self.h, _p(p), C.byref(acc)))
        return bool(acc.value)

    def initext_calibrate(self, lidars, stages=INITEXT_ROT | INITEXT_TRANS) -> list:
        """calibExRotation and / or calibExTranslation for the listed LiDARs in one launch -> one dict per LiDAR (mlh_initext_calibrate)"""
        ls = np.ascontiguousarray(lidars, np.int32).reshape(-1)
        out = (InitExtResult * max(1, len(ls)))()
        self._ck(self.lib.mlh_initext_calibrate(self.h, _p(ls), len(ls), int(stages), out))
        return [out[i].as_dict() for i in range(len(ls))]

    def initext_info(self) -> dict:
        info = InitExtInfo()
        self._ck(self.lib.mlh_initext_info(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    def initext_read_state(self) -> dict:
        """Q (n_lidar, 1200, 4), the stored sets (300, n_lidar, 7) and calib_ext_ (n_lidar, 7) (mlh_initext_read_state: a test entry)"""
        n = self.initext_info()["n_lidar"]
        Q, sets, ext = np.zeros((max(n, 1), 1200, 4)), np.zeros((300, max(n, 1), 7)), np.zeros((max(n, 1), 7))
        self._ck(self.lib.mlh_initext_read_state(self.h, _p(Q), _p(sets), _p(ext)))
        return dict(Q=Q, sets=sets, calib_ext=ext)

    def downsample_current_scan(self, kind, points4, leaf, ext_poses, ext_covs, cov_measurement, with_ua=True, trace_threshold=0.6, fetch=True):
        """downsampleCurrentScan for one kind; the result becomes the kind's feature set and, with fetch, is also returned (m, 11)
        (without: the number of features; nothing leaves the device)."""
        ptr, stride, n, mem, keep = _src(points4)
        ep = np.ascontiguousarray(ext_poses, np.float64).reshape(-1, 7)
        ec = np.ascontiguousarray(ext_covs, np.float64).reshape(-1, 36)
        cm = np.ascontiguousarray(cov_measurement, np.float64).reshape(9)
        out = np.zeros((n, 11), np.float32) if fetch else None
        cnt = C.c_int32(0)
        self._ck(self.lib.mlh_downsample_current_scan(self.h, kind, ptr, stride, n, 12, mem, leaf, _p(ep), _p(ec), len(ep), _p(cm), int(bool(with_ua)),
                                                      float(trace_threshold), _p(out) if fetch else None, C.byref(cnt)))
        self._m = getattr(self, "_m", {})
        self._m[kind] = cnt.value
        return out[:cnt.value].copy() if fetch else cnt.value

    def downsample_current_scan_pair(self, surf4, corner4, leaf_surf, leaf_corner, ext_poses, ext_covs, cov_measurement, with_ua=True, trace_threshold=0.6):
        """downsampleCurrentScan for both kinds in one call (one thinning pipeline for the two fused clouds) -> (n_surf_features, n_corner_features)."""
        ps, ss, ns, ms, ks = _src(surf4)
        pc, sc, nc, mc, kc = _src(corner4)
        assert ss == sc and ms == mc
        ep = np.ascontiguousarray(ext_poses, np.float64).reshape(-1, 7)
        ec = np.ascontiguousarray(ext_covs, np.float64).reshape(-1, 36)
        cm = np.ascontiguousarray(cov_measurement, np.float64).reshape(9)
        a, b = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_downsample_current_scan_pair(self.h, ps, ns, pc, nc, ss, 12, ms, float(leaf_surf), float(leaf_corner), _p(ep), _p(ec), len(ep), _p(cm),
                                                           int(bool(with_ua)), float(trace_threshold), C.byref(a), C.byref(b)))
        self._m = getattr(self, "_m", {})
        self._m[SURF], self._m[CORNER] = a.value, b.value
        return a.value, b.value

    def downsample_scan2map(self, surf4, corner4, leaf_surf, leaf_corner, ext_poses, ext_covs, cov_measurement, pose, opts=None, with_ua=True, trace_threshold=0.6):
        """downsampleCurrentScan (both kinds) + scan2MapOptimization with no host read between them (mlh_downsample_scan2map) -> (pose, (n_surf_features, n_corner_features))."""
        opts = opts or default_opts()
        ps, ss, ns, ms, ks = _src(surf4)
        pc, sc, nc, mc, kc = _src(corner4)
        assert ss == sc and ms == mc
        ep = np.ascontiguousarray(ext_poses, np.float64).reshape(-1, 7)
        ec = np.ascontiguousarray(ext_covs, np.float64).reshape(-1, 36)
        cm = np.ascontiguousarray(cov_measurement, np.float64).reshape(9)
        x = np.ascontiguousarray(pose, np.float64).copy()
        a, b = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_downsample_scan2map(self.h, ps, ns, pc, nc, ss, 12, ms, float(leaf_surf), float(leaf_corner), _p(ep), _p(ec), len(ep), _p(cm),
                                                  int(bool(with_ua)), float(trace_threshold), _p(x), C.byref(opts), C.byref(a), C.byref(b)))
        self._m = getattr(self, "_m", {})
        self._m[SURF], self._m[CORNER] = a.value, b.value
        return x, (a.value, b.value)

    def features_fetch(self, kind) -> np.ndarray:
        """the staged feature set of `kind` as the solver will read it -> (n, 7) f32 [x y z intensity cxx cyy czz] (mlh_features_fetch)"""
        n = C.c_int32(0)
        rc = self.lib.mlh_features_fetch(self.h, kind, None, 0, C.byref(n))       # the count first: a set with records answers a capacity of 0 with "invalid"
        if rc != 0 and not (rc == -1 and n.value > 0):
            self._ck(rc)
        out = np.zeros((n.value, 7), np.float32)
        if n.value:
            self._ck(self.lib.mlh_features_fetch(self.h, kind, _p(out), n.value, C.byref(n)))
        return out

    THIN_PATH_NAMES = ("none", "sort-first", "shared-grid", "single-calls")

    def thin_info(self) -> dict:
        """the form the most recent downsample_current_scan_pair / downsample_scan2map took -> dict(path, n_in) (mlh_thin_info)"""
        t = ThinInfo()
        self._ck(self.lib.mlh_thin_info(self.h, C.byref(t)))
        return dict(path=self.THIN_PATH_NAMES[t.path], n_in=(int(t.n_in[0]), int(t.n_in[1])))

    def cloud_uct_associate_to_map(self, points11, pose_global, cov_global, ext, ext_cov, cov_meas, with_ua, trace_threshold):
        """cloudUCTAssociateToMap on (n, 11) records [x y z i cov6 trace] -> kept, transformed records in input order."""
        a = np.ascontiguousarray(points11, np.float32)
        assert a.shape[1] == 11
        pg, cg = np.ascontiguousarray(pose_global, np.float64), np.ascontiguousarray(cov_global, np.float64)
        e, ec = np.ascontiguousarray(ext, np.float64), np.ascontiguousarray(ext_cov, np.float64)
        cm = np.ascontiguousarray(cov_meas, np.float64)
        out = np.zeros_like(a)
        cnt = C.c_int32(0)
        self._ck(self.lib.mlh_cloud_uct_associate_to_map(self.h, _p(a), 44, a.shape[0], 12, 16, 40, _p(pg), _p(cg), _p(e), _p(ec), e.shape[0],
                                                         _p(cm), int(bool(with_ua)), float(trace_threshold), _p(out), C.byref(cnt), MEM_HOST))
        return out[:cnt.value].copy()

    def cloud_uct_associate_to_map_device(self, d_points11, d_out, pose_global, cov_global, ext, ext_cov, cov_meas, with_ua, trace_threshold):
        """Device-resident variant: d_points11 / d_out are torch CUDA float32 tensors (n, 11); returns the number of records written."""
        ptr, stride, n, mem, keep = _src(d_points11)
        optr, ostride, on, omem, okeep = _src(d_out)
        assert mem == MEM_DEVICE and omem == MEM_DEVICE and stride == 44 and ostride == 44 and on >= n
        pg, cg = np.ascontiguousarray(pose_global, np.float64), np.ascontiguousarray(cov_global, np.float64)
        e, ec = np.ascontiguousarray(ext, np.float64), np.ascontiguousarray(ext_cov, np.float64)
        cm = np.ascontiguousarray(cov_meas, np.float64)
        cnt = C.c_int32(0)
        self._ck(self.lib.mlh_cloud_uct_associate_to_map(self.h, ptr, 44, n, 12, 16, 40, _p(pg), _p(cg), _p(e), _p(ec), e.shape[0], _p(cm),
                                                         int(bool(with_ua)), float(trace_threshold), optr, C.byref(cnt), MEM_DEVICE))
        return cnt.value

    def voxel_filter_device(self, d_points, d_out, leaf, trace_threshold=0.0):
        """Device-resident VoxelGridCovarianceMLOAM: torch CUDA float32 (n, 4) or (n, 11) in, same layout out; returns the count."""
        ptr, stride, n, mem, keep = _src(d_points)
        optr, ostride, on, omem, okeep = _src(d_out)
        assert mem == MEM_DEVICE and omem == MEM_DEVICE and stride == ostride and on >= n
        ncol = stride // 4
        cov_off, tr_off = (16, 40) if ncol >= 11 else (-1, -1)
        cnt = C.c_int32(0)
        self._ck(self.lib.mlh_voxel_filter(self.h, ptr, stride, n, 12 if ncol >= 4 else -1, cov_off, tr_off, leaf, trace_threshold, optr, C.byref(cnt), MEM_DEVICE))
        return cnt.value

    def voxel_filter(self, points, leaf, trace_threshold=0.0):
        """VoxelGridCovarianceMLOAM: points (n, 4) [x y z intensity] -> plain branch; (n, 11) [x y z i cov6 trace] -> covariance branch."""
        a = np.ascontiguousarray(points, np.float32)
        n, ncol = a.shape
        out = np.zeros_like(a)
        cnt = C.c_int32(0)
        cov_off, tr_off = (16, 40) if ncol >= 11 else (-1, -1)
        self._ck(self.lib.mlh_voxel_filter(self.h, _p(a), ncol * 4, n, 12 if ncol >= 4 else -1, cov_off, tr_off, leaf, trace_threshold, _p(out), C.byref(cnt), MEM_HOST))
        return out[:cnt.value].copy()

    # ---- keyframe store + local map (saveKeyframe / extractSurroundingKeyFrames / clearCloud on the device)
    def keyframes_reset(self):
        self._ck(self.lib.mlh_keyframes_reset(self.h))

    def keyframe_save(self, pose, cov, surf, corner):
        """saveKeyframe's store: pose [t, q(xyzw)], its 6x6 cov, the surf / corner clouds ((n, >= 4) [x y z lidar ...] arrays or device clouds) -> key"""
        p = np.ascontiguousarray(pose, np.float64).reshape(7)
        c = np.ascontiguousarray(cov, np.float64).reshape(36)
        (ps, ss, ns, ms, ks), (pc, sc, nc, mc, kc) = _src(surf), _src(corner)
        if ns == 0:
            ss, ms = sc, mc
        if nc == 0:
            sc, mc = ss, ms
        assert ss == sc and ms == mc and ss >= 16, "both clouds share record stride (>= 4 floats) and memory kind"
        key = C.c_int32(-1)
        self._ck(self.lib.mlh_keyframe_save(self.h, _p(p), _p(c), ps, ns, pc, nc, ss, 12, ms, C.byref(key)))
        return key.value

    def keyframe_save_staged(self, pose, cov):
        """saveKeyframe with the context's staged feature sets (device to device) -> key"""
        p = np.ascontiguousarray(pose, np.float64).reshape(7)
        c = np.ascontiguousarray(cov, np.float64).reshape(36)
        key = C.c_int32(-1)
        self._ck(self.lib.mlh_keyframe_save_staged(self.h, _p(p), _p(c), C.byref(key)))
        return key.value

    def local_map_assemble(self, pose_cur, ext_poses, ext_covs, opts: LocalMapOpts):
        """extractSurroundingKeyFrames -> dict(rebuilt, n_surf_ds, n_corner_ds, kf_ids (the ids appended this call, in order))"""
        p = np.ascontiguousarray(pose_cur, np.float64).reshape(7)
        ep = np.ascontiguousarray(ext_poses, np.float64).reshape(-1, 7)
        ec = None if ext_covs is None else np.ascontiguousarray(ext_covs, np.float64).reshape(-1, 36)
        nk = C.c_int32(0)
        self._ck(self.lib.mlh_local_map_info(self.h, C.byref(nk), None, None, None))
        ids = np.zeros(max(nk.value, 1), np.int32)
        rb, a, b, n = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mlh_local_map_assemble(self.h, _p(p), _p(ep), _p(ec), len(ep), C.byref(opts), C.byref(rb), C.byref(a), C.byref(b),
                                                 ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        return dict(rebuilt=bool(rb.value), n_surf_ds=a.value, n_corner_ds=b.value, kf_ids=ids[:n.value].copy())

    def local_map_cloud(self, kind, filtered=True) -> "DeviceCloud":
        """the local map cloud of `kind` in HBM (48-byte PointIWithCov records): filtered = the _ds cloud, else the pre-filter one"""
        ptr, n = C.c_void_p(), C.c_int32(0)
        self._ck(self.lib.mlh_local_map_cloud(self.h, kind, int(bool(filtered)), C.byref(ptr), C.byref(n)))
        return DeviceCloud(ptr.value, n.value, 48)

    def _fetch48(self, dc):
        if dc.n == 0:
            return np.zeros((0, 11), np.float32)
        self.synchronize()
        out = np.zeros((dc.n, 12), np.float32)
        e = _hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dc.ptr), C.c_size_t(dc.n * 48), 2)   # hipMemcpyDeviceToHost
        if e != 0:
            raise MlhError(f"hipMemcpy of a map cloud failed ({e})")
        return out[:, :11].copy()

    def local_map_fetch(self, kind, filtered=True):
        """the same cloud copied to the host as (n, 11) float32 [x y z i cov6 trace]"""
        return self._fetch48(self.local_map_cloud(kind, filtered))

    def local_map_clear(self):
        """clearCloud: the four map clouds (the cache and the store stay)"""
        self._ck(self.lib.mlh_local_map_clear(self.h))

    def local_map_info(self) -> dict:
        a, b, c, d = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.mlh_local_map_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(n_keyframes=a.value, n_cached=b.value, store_bytes=c.value, cache_bytes=d.value)

    # ---- the global map (pubGlobalMap / saveGlobalMap on the device)
    def keyframe_attach_outlier(self, key, outlier):
        """saveKeyframe's third cloud ((n, >= 4) [x y z lidar ...] array or device cloud), attached to the saved keyframe `key`"""
        po, so, no, mo, ko = _src(outlier)
        self._ck(self.lib.mlh_keyframe_attach_outlier(self.h, int(key), po, no, so, 12, mo))

    def global_map_assemble(self, pose_cur, ext_poses, ext_covs, opts: GlobalMapOpts):
        """pubGlobalMap / saveGlobalMap -> dict(n_pre, n_ds (two clouds each), kf_ids (the keyframes the map is made of, in append order))"""
        p = None if pose_cur is None else np.ascontiguousarray(pose_cur, np.float64).reshape(7)
        ep = np.ascontiguousarray(ext_poses, np.float64).reshape(-1, 7)
        ec = None if ext_covs is None else np.ascontiguousarray(ext_covs, np.float64).reshape(-1, 36)
        nk = C.c_int32(0)
        self._ck(self.lib.mlh_local_map_info(self.h, C.byref(nk), None, None, None))
        ids = np.zeros(max(nk.value, 1), np.int32)
        n_pre, n_ds, n = (C.c_int32 * 2)(), (C.c_int32 * 2)(), C.c_int32(0)
        self._ck(self.lib.mlh_global_map_assemble(self.h, _p(p), _p(ep), _p(ec), len(ep), C.byref(opts), n_pre, n_ds, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  C.byref(n)))
        return dict(n_pre=[n_pre[0], n_pre[1]], n_ds=[n_ds[0], n_ds[1]], kf_ids=ids[:n.value].copy())

    def global_map_cloud(self, which=0, filtered=True) -> "DeviceCloud":
        """global map cloud `which` in HBM (48-byte PointIWithCov records): filtered = the _ds cloud, else the pre-filter one"""
        ptr, n = C.c_void_p(), C.c_int32(0)
        self._ck(self.lib.mlh_global_map_cloud(self.h, which, int(bool(filtered)), C.byref(ptr), C.byref(n)))
        return DeviceCloud(ptr.value, n.value, 48)

    def global_map_fetch(self, which=0, filtered=True):
        """the same cloud copied to the host as (n, 11) float32 [x y z i cov6 trace]"""
        return self._fetch48(self.global_map_cloud(which, filtered))

    def global_map_release(self):
        self._ck(self.lib.mlh_global_map_release(self.h))

    # ---- loop-corrected poses into the keyframe store (updateKeyframe, a stub in the reference)
    def keyframes_update_poses(self, first_key, poses, covs=None, drift_tail=False) -> dict:
        """keys first_key .. take poses (n, 7) [t, q(xyzw)] and, when given, covs (n, 6, 6) -> dict(n_changed, drift (7,)) (mlh_keyframes_update_poses)"""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        c = None if covs is None else np.ascontiguousarray(covs, np.float64).reshape(-1, 36)
        assert c is None or len(c) == len(p), "one covariance per pose"
        nc, drift = C.c_int32(0), np.zeros(7)
        self._ck(self.lib.mlh_keyframes_update_poses(self.h, int(first_key), len(p), _p(p) if len(p) else None, _p(c), int(bool(drift_tail)), C.byref(nc), _p(drift)))
        return dict(n_changed=nc.value, drift=drift)

    def keyframes_update_from_pose_graph(self, pg_ctx=None, first_index=0, first_key=0, n=-1, drift_tail=False) -> dict:
        """the same update with the poses of pg_ctx's pose-graph records in HBM (None: this context's); n < 0: every pose-graph keyframe from first_index
        -> dict(n_changed, drift (7,)) (mlh_keyframes_update_from_pose_graph)"""
        src = self if pg_ctx is None else pg_ctx
        nc, drift = C.c_int32(0), np.zeros(7)
        self._ck(self.lib.mlh_keyframes_update_from_pose_graph(self.h, src.h, int(first_index), int(first_key), int(n), int(bool(drift_tail)), C.byref(nc), _p(drift)))
        return dict(n_changed=nc.value, drift=drift)

    def keyframes_update_from_pose_graph_cov(self, pg_ctx=None, first_index=0, first_key=0, n=-1, drift_tail=False, cov_mode=KF_COV_RELATIVE) -> dict:
        """keyframes_update_from_pose_graph with the store-form marginal covariances of pg_ctx's last pg_marginals; cov_mode KF_COV_RELATIVE / KF_COV_ABSOLUTE
        -> dict(n_changed, drift (7,)) (mlh_keyframes_update_from_pose_graph_cov)"""
        src = self if pg_ctx is None else pg_ctx
        nc, drift = C.c_int32(0), np.zeros(7)
        self._ck(self.lib.mlh_keyframes_update_from_pose_graph_cov(self.h, src.h, int(first_index), int(first_key), int(n), int(bool(drift_tail)), int(cov_mode), C.byref(nc),
                                                                   _p(drift)))
        return dict(n_changed=nc.value, drift=drift)

    def keyframe_poses(self, first_key=0, n=None) -> dict:
        """what the store holds -> dict(poses (n, 7), covs (n, 6, 6), positions (n, 3) float32) (mlh_keyframe_poses)"""
        n = self.local_map_info()["n_keyframes"] - first_key if n is None else n
        poses, covs, pos = np.zeros((max(n, 0), 7)), np.zeros((max(n, 0), 6, 6)), np.zeros((max(n, 0), 3), np.float32)
        self._ck(self.lib.mlh_keyframe_poses(self.h, int(first_key), int(n), _p(poses), _p(covs), _p(pos)))
        return dict(poses=poses, covs=covs, positions=pos)

    # ---- the odometry's sliding window + its local maps (surf / corner_points_stack_, slideWindow, buildLocalMap / buildCalibMap on the device)
    def window_reset(self, n_lidar, window_size):
        self._ck(self.lib.mlh_window_reset(self.h, int(n_lidar), int(window_size)))

    def window_set(self, lidar, slot, surf, corner):
        """stack[lidar][slot] = the two clouds ((n, >= 4) [x y z intensity ...] arrays or device clouds; an empty array stores an empty cloud)"""
        (ps, ss, ns, ms, ks), (pc, sc, nc, mc, kc) = _src(surf), _src(corner)
        if ns == 0:
            ss, ms = sc, mc
        if nc == 0:
            sc, mc = ss, ms
        assert ss == sc and ms == mc, "both clouds share record stride and memory kind"
        self._ck(self.lib.mlh_window_set(self.h, int(lidar), int(slot), ps if ns else None, ns, pc if nc else None, nc, ss, 12, ms))

    def window_set_from_scan(self, lidar, slot, src=None, leaf_surf=0.4, leaf_corner=0.2):
        """estimator.cpp:487-495 for the scan `src` (default: this context) holds after extract_run + extract_voxel_run, device to device"""
        self._ck(self.lib.mlh_window_set_from_scan(self.h, (src or self).h, int(lidar), int(slot), float(leaf_surf), float(leaf_corner)))

    def window_slide(self, src_slot):
        """slideWindow: stack.push(stack[src_slot]) for every LiDAR and both kinds (CircularBuffer::push)"""
        self._ck(self.lib.mlh_window_slide(self.h, int(src_slot)))

    def window_cloud(self, lidar, slot, kind) -> "DeviceCloud":
        ptr, n = C.c_void_p(), C.c_int32(0)
        self._ck(self.lib.mlh_window_cloud(self.h, int(lidar), int(slot), int(kind), C.byref(ptr), C.byref(n)))
        return DeviceCloud(ptr.value, n.value)

    def _fetch16(self, dc):
        if dc.n == 0:
            return np.zeros((0, 4), np.float32)
        self.synchronize()
        out = np.zeros((dc.n, 4), np.float32)
        e = _hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dc.ptr), C.c_size_t(dc.n * 16), 2)   # hipMemcpyDeviceToHost
        if e != 0:
            raise MlhError(f"hipMemcpy of a window cloud failed ({e})")
        return out

    def window_fetch(self, lidar, slot, kind):
        """the slot's cloud copied to the host as (n, 4) float32 [x y z intensity]"""
        return self._fetch16(self.window_cloud(lidar, slot, kind))

    def window_info(self) -> dict:
        a, b = C.c_int32(0), C.c_int32(0)
        v = [C.c_int64(0) for _ in range(4)]
        self._ck(self.lib.mlh_window_info(self.h, C.byref(a), C.byref(b), *[C.byref(x) for x in v]))
        return dict(n_lidar=a.value, window_size=b.value, pushes=v[0].value, bytes_used=v[1].value, bytes_reserved=v[2].value, allocations=v[3].value)

    def window_build_local_map(self, pose_local, opts: WindowMapOpts):
        """buildLocalMap / buildCalibMap from the store: pose_local (n_lidar, window_size + 1, 7) -> dict(n_pre, n_ds), each (n_lidar, 2) [surf, corner]"""
        info = self.window_info()
        p = np.ascontiguousarray(pose_local, np.float64)
        assert p.size == info["n_lidar"] * (info["window_size"] + 1) * 7
        n_pre, n_ds = np.zeros(2 * info["n_lidar"], np.int32), np.zeros(2 * info["n_lidar"], np.int32)
        i32p = C.POINTER(C.c_int32)
        self._ck(self.lib.mlh_window_build_local_map(self.h, _p(p), C.byref(opts), n_pre.ctypes.data_as(i32p), n_ds.ctypes.data_as(i32p)))
        return dict(n_pre=n_pre.reshape(-1, 2), n_ds=n_ds.reshape(-1, 2))

    def window_map_cloud(self, lidar, kind, filtered=True) -> "DeviceCloud":
        ptr, n = C.c_void_p(), C.c_int32(0)
        self._ck(self.lib.mlh_window_map_cloud(self.h, int(lidar), int(kind), int(bool(filtered)), C.byref(ptr), C.byref(n)))
        return DeviceCloud(ptr.value, n.value)

    def window_map_fetch(self, lidar, kind, filtered=True):
        """LiDAR `lidar`'s local map of `kind` copied to the host as (n, 4) float32 [x y z intensity]"""
        return self._fetch16(self.window_map_cloud(lidar, kind, filtered))

    # ---- map / features
    def map_set(self, kind, points, min_match_sq_dis=1.0):
        ptr, stride, n, mem, keep = _src(points)
        self._ck(self.lib.mlh_map_set(self.h, kind, ptr, stride, n, min_match_sq_dis, mem))

    def map_set_pair(self, surf_points, corner_points, min_match_sq_dis=1.0):
        """both setInputCloud calls of a frame in one set of launches (same memory space and record stride for the two clouds)"""
        ps, ss, ns, ms, ks = _src(surf_points)
        pc, sc, nc, mc, kc = _src(corner_points)
        assert ss == sc and ms == mc
        self._ck(self.lib.mlh_map_set_pair(self.h, ps, ns, pc, nc, ss, min_match_sq_dis, ms))

    def map_set_pair_overlapped(self, surf_points, corner_points, min_match_sq_dis=1.0):
        """stage the NEXT frame's maps while a submitted solve still runs (double-buffered map sets, second stream); see mlh_map_set_pair_overlapped"""
        ps, ss, ns, mems, _k1 = _src(surf_points)
        pc, sc, nc, memc, _k2 = _src(corner_points)
        assert ss == sc and mems == memc
        self._ck(self.lib.mlh_map_set_pair_overlapped(self.h, ps, ns, pc, nc, ss, min_match_sq_dis, mems))

    def map_rebuild(self, kind):
        self._ck(self.lib.mlh_map_rebuild(self.h, kind))

    def set_extract_tie_order(self, reference=True):
        """extractCloud, equal curvatures inside a sector: True = the order the reference's std::sort leaves (default), False = (curvature, index)"""
        self._ck(self.lib.mlh_set_extract_tie_order(self.h, 1 if reference else 0))

    def set_gn_schedule(self, deferred_finish=True, knn_warm_start=True, final_in_successor=True):
        """layout of a Gauss-Newton solve's iterations on the device (mlh_set_gn_schedule): results do not depend on it"""
        self._ck(self.lib.mlh_set_gn_schedule(self.h, 1 if deferred_finish else 0, 1 if knn_warm_start else 0, 1 if final_in_successor else 0))

    def debug_bad_launch(self):
        """one launch with an impossible configuration: raises under MLH_CHECK_LAUNCH=1 (naming the kernel), returns otherwise"""
        self._ck(self.lib.mlh_debug_bad_launch(self.h))

    def set_voxel_member_order(self, mode):
        """voxel filters of this context, members of a voxel: True / 1 = in libstdc++'s std::sort order (the reference's), produced on the
        device (the default); 2 or "host" = the same through a host pass with the platform's own std::sort; False / 0 = by point index
        (a voxel that mixes LiDAR ids may keep another id)"""
        mode = 2 if mode == "host" else int(mode)
        self._ck(self.lib.mlh_set_voxel_member_order(self.h, mode))

    def std_sort_permutation(self, keys, n0=None, mode=1):
        """the permutation std::sort (comparator on the key only) leaves for keys[:n0] and keys[n0:]; mode 1 device, 2 host"""
        keys = np.ascontiguousarray(keys, np.int32)
        n = len(keys)
        perm = np.zeros(n, np.int32)
        self._ck(self.lib.mlh_std_sort_permutation(self.h, _p(keys), n if n0 is None else int(n0), n, _p(perm), int(mode)))
        return perm

    def map_info(self, kind):
        n, occ, lanes, pop = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._ck(self.lib.mlh_map_info(self.h, kind, C.byref(n), C.byref(occ), C.byref(pop), C.byref(lanes)))
        return dict(n=n.value, occupied_cells=occ.value, mean_cell_population=round(pop.value, 2), knn_lanes=lanes.value)

    def knn(self, kind, queries, k=5):
        q = np.ascontiguousarray(queries[:, :3], np.float32)
        idx = np.zeros((q.shape[0], k), np.int32)
        d2 = np.zeros((q.shape[0], k), np.float32)
        self._ck(self.lib.mlh_knn(self.h, kind, _p(q), q.shape[0], k, _p(idx), _p(d2)))
        return idx, d2

    def features_set(self, kind, points):
        """points: (m, 4) [x y z intensity] or (m, 11) [x y z intensity cov6 trace] (compact PointXYZIWithCov)."""
        ptr, stride, n, mem, keep = _src(points)
        ncol = stride // 4
        self._ck(self.lib.mlh_features_set(self.h, kind, ptr, stride, n, 12 if ncol >= 4 else -1, 16 if ncol >= 10 else -1, mem))
        self._m = getattr(self, "_m", {})
        self._m[kind] = n

    def features_set_blocks(self, kind, clouds):
        """clouds: list of (m_b, >=3) arrays, one per pose block (block 0 = body pose, block n = extrinsic of LiDAR n)."""
        for b, pts in enumerate(clouds):
            ptr, stride, n, mem, keep = _src(pts)
            self._ck(self.lib.mlh_features_set_block(self.h, kind, b, ptr, stride, n, 16 if stride // 4 >= 10 else -1, mem))

    def gn_solve_blocks(self, poses, n_iters, k_neigh, eig_thre, freeze, opts: SolverOpts | None = None, want_stats=True):
        opts = opts or default_opts()
        poses = np.ascontiguousarray(poses, np.float64).copy().reshape(-1, 7)
        nb = poses.shape[0]
        bo = BlockOpts()
        bo.n_blocks = nb
        for b in range(nb):
            bo.k_neigh[b] = int(k_neigh[b]); bo.eig_thre[b] = float(eig_thre[b]); bo.freeze[b] = int(freeze[b])
        stats = (IterStat * (n_iters * nb))() if want_stats else None
        self._ck(self.lib.mlh_gn_solve_blocks(self.h, _p(poses), n_iters, C.byref(opts), C.byref(bo), C.cast(stats, C.c_void_p) if want_stats else None))
        st = [[stats[it * nb + b].as_dict() for b in range(nb)] for it in range(n_iters)] if want_stats else None
        return poses, st

    # ---- multi-GPU
    def comm_finalize(self):
        self._ck(self.lib.mlh_comm_finalize(self.h))

    def shard_set(self, lo_plane=None, hi_plane=None):
        lo = None if lo_plane is None else np.ascontiguousarray(lo_plane, np.float32)
        hi = None if hi_plane is None else np.ascontiguousarray(hi_plane, np.float32)
        self._ck(self.lib.mlh_shard_set(self.h, _p(lo), _p(hi)))

    def shard_set_features(self, n_ranks, rank):
        """replicated map, features dealt round-robin: slot f is owned iff f % n_ranks == rank"""
        self._ck(self.lib.mlh_shard_set_features(self.h, int(n_ranks), int(rank)))

    def comm_init(self, n_ranks, rank, unique_id: bytes):
        _torch_rccl_first()
        buf = C.create_string_buffer(unique_id, 128)
        self._ck(self.lib.mlh_comm_init(self.h, n_ranks, rank, C.cast(buf, C.c_void_p)))

    def p2p_mailbox(self) -> bytes:
        """this rank's mailbox of the mailbox communicator: its 64-byte hipIpc handle, to be all-gathered by the caller (mlh_p2p_mailbox)"""
        buf = C.create_string_buffer(64)
        self._ck(self.lib.mlh_p2p_mailbox(self.h, C.cast(buf, C.c_void_p)))
        return buf.raw

    def p2p_comm_init(self, n_ranks, rank, handles):
        """handles: the n_ranks 64-byte handles in rank order (mlh_p2p_comm_init)"""
        blob = b"".join(handles)
        assert len(blob) == 64 * n_ranks
        buf = C.create_string_buffer(blob, len(blob))
        self._ck(self.lib.mlh_p2p_comm_init(self.h, n_ranks, rank, C.cast(buf, C.c_void_p)))

    def allreduce_f64(self, arr):
        a = np.ascontiguousarray(arr, np.float64).copy()
        self._ck(self.lib.mlh_allreduce_f64(self.h, _p(a), a.size))
        return a

    # ---- host-driven evaluation
    def match_linearize(self, kind, pose, flags=0, min_match_sq_dis=1.0, min_plane_dis=0.2, huber_delta=0.1,
                        cov_measurement_trace=0.0075, dense=True, k_neigh=5):
        m = self._m[kind]
        pose = np.ascontiguousarray(pose, np.float64)
        valid = np.zeros(m, np.uint8)
        coeffs = np.zeros((m, 6), np.float64)
        r = np.zeros(m) if dense else None
        J = np.zeros((m, 6)) if dense else None
        H = np.zeros((6, 6))
        g = np.zeros(6)
        cost, cnt = C.c_double(0), C.c_int32(0)
        self._ck(self.lib.mlh_match_linearize(self.h, kind, _p(pose), int(k_neigh), flags, min_match_sq_dis, min_plane_dis, huber_delta,
                                              cov_measurement_trace, _p(valid), _p(coeffs), _p(r), _p(J), _p(H), _p(g),
                                              C.byref(cost), C.byref(cnt)))
        return dict(valid=valid, coeffs=coeffs, r=r, J=J, H=H, g=g, cost=cost.value, count=cnt.value)

    def match_coeffs(self, kind):
        """mlh_match_coeffs: validity and coefficients of the correspondences the last launch that matched `kind` left on the device -> valid (m,), coeffs (m, 6), count"""
        m = self._m[kind]
        valid = np.zeros(m, np.uint8)
        coeffs = np.zeros((m, 6), np.float64)
        n = C.c_int32(0)
        self._ck(self.lib.mlh_match_coeffs(self.h, kind, _p(valid), _p(coeffs), C.byref(n)))
        return dict(valid=valid, coeffs=coeffs, count=n.value)

    def match_neighbours(self, kind):
        """mlh_match_neighbours: the neighbour records of the last correspondence launch of `kind` -> (m, stride, 4) float32 [x y z squared distance]"""
        stride = C.c_int32(0)
        self._ck(self.lib.mlh_match_neighbours(self.h, kind, None, C.byref(stride)))
        rec = np.zeros((self._m[kind], stride.value, 4), np.float32)
        self._ck(self.lib.mlh_match_neighbours(self.h, kind, _p(rec), C.byref(stride)))
        return rec

    def linearize(self, kind, pose, flags=0, huber_delta=0.1, cov_measurement_trace=0.0075, dense=True):
        m = self._m[kind]
        pose = np.ascontiguousarray(pose, np.float64)
        r = np.zeros(m) if dense else None
        J = np.zeros((m, 6)) if dense else None
        H = np.zeros((6, 6))
        g = np.zeros(6)
        cost, cnt = C.c_double(0), C.c_int32(0)
        self._ck(self.lib.mlh_linearize(self.h, kind, _p(pose), flags, huber_delta, cov_measurement_trace, _p(r), _p(J), _p(H), _p(g),
                                        C.byref(cost), C.byref(cnt)))
        return dict(r=r, J=J, H=H, g=g, cost=cost.value, count=cnt.value)

    def good_feature_matching(self, kind, pose, gf_method="gd_fix", gf_ratio=0.2, seed=0, min_match_sq_dis=1.0, min_plane_dis=0.2):
        m = self._m[kind]
        pose = np.ascontiguousarray(pose, np.float64)
        sel = np.zeros(max(m, 1), np.int32)
        n_sel = C.c_int32(0)
        H = np.eye(6) * 1e-6
        matched = np.zeros(m, np.uint8)
        self._ck(self.lib.mlh_good_feature_matching(self.h, kind, _p(pose), GF_METHODS[gf_method], gf_ratio, seed, min_match_sq_dis,
                                                    min_plane_dis, _p(sel), C.byref(n_sel), _p(H), _p(matched)))
        return dict(sel=sel[:n_sel.value].copy(), H=H, matched=matched)

    # ---- device-resident solvers
    def gn_solve(self, pose, n_iters, opts: SolverOpts | None = None, want_stats=True):
        opts = opts or default_opts()
        pose = np.ascontiguousarray(pose, np.float64).copy()
        stats = (IterStat * n_iters)() if want_stats else None
        self._ck(self.lib.mlh_gn_solve(self.h, _p(pose), n_iters, C.byref(opts), C.cast(stats, C.c_void_p) if want_stats else None))
        return pose, ([s.as_dict() for s in stats] if want_stats else None)

    def features_copy_from(self, src: "Context", kind):
        """this context's feature set of `kind` <- the one staged in `src` (same GPU), device to device (mlh_features_copy)"""
        self._ck(self.lib.mlh_features_copy(self.h, src.h, kind))

    def gn_solve_begin(self, pose, n_iters, opts: SolverOpts | None = None):
        """submit the solve and return at once (mlh_gn_solve_begin); collect the pose with gn_solve_end. One in flight per context."""
        self._opts_keep = opts or default_opts()
        pose = np.ascontiguousarray(pose, np.float64)
        self._ck(self.lib.mlh_gn_solve_begin(self.h, _p(pose), n_iters, C.byref(self._opts_keep)))

    def gn_solve_begin_chained(self, wodom_prev, wodom_cur, n_iters, opts: SolverOpts | None = None):
        """submit the next frame's solve; its start pose is made on the device from the previous solve's result (transformUpdate +
        transformAssociateToMap, lidar_mapper_keyframe.cpp:145-160) -- mlh_gn_solve_begin_chained."""
        self._opts_keep2 = opts or default_opts()
        a = np.ascontiguousarray(wodom_prev, np.float64)
        b = np.ascontiguousarray(wodom_cur, np.float64)
        self._ck(self.lib.mlh_gn_solve_begin_chained(self.h, _p(a), _p(b), n_iters, C.byref(self._opts_keep2)))

    def gn_solve_end(self):
        pose = np.zeros(7)
        self._ck(self.lib.mlh_gn_solve_end(self.h, _p(pose)))
        return pose

    def scan2map_begin(self, pose, opts: SolverOpts | None = None, lm_lookahead=0):
        """submit scan2MapOptimization for the staged frame and return (mlh_scan2map_begin); collect with scan2map_end"""
        opts = opts or default_opts()
        p = np.ascontiguousarray(pose, np.float64)
        self._ck(self.lib.mlh_scan2map_begin(self.h, _p(p), C.byref(opts), int(lm_lookahead)))

    def scan2map_begin_chained(self, wodom_prev, wodom_cur, opts: SolverOpts | None = None, lm_lookahead=0):
        opts = opts or default_opts()
        a, b = np.ascontiguousarray(wodom_prev, np.float64), np.ascontiguousarray(wodom_cur, np.float64)
        self._ck(self.lib.mlh_scan2map_begin_chained(self.h, _p(a), _p(b), C.byref(opts), int(lm_lookahead)))

    def scan2map_end(self):
        """-> (pose, status): 0 = converged inside the look-ahead, 2 = re-solved synchronously inside the call, 1 = the caller must re-solve (pose = start pose)"""
        p = np.zeros(7, np.float64)
        st = C.c_int32(0)
        self._ck(self.lib.mlh_scan2map_end(self.h, _p(p), C.byref(st)))
        return p, int(st.value)

    def scan2map_cov(self):
        """-> (cov, H_final), 6 x 6 each in the tangent's order [t, theta]: evalHessian at the pose the most recently collected scan2map solve returned and its
        inverse (mlh_scan2map_cov; the solve's options must carry FLAG_POSE_COV)"""
        cov, H = np.zeros((6, 6)), np.zeros((6, 6))
        self._ck(self.lib.mlh_scan2map_cov(self.h, _p(cov), _p(H)))
        return cov, H

    def scan2map(self, pose, opts: SolverOpts | None = None, want_stats=True):
        opts = opts or default_opts()
        pose = np.ascontiguousarray(pose, np.float64).copy()
        if not want_stats:
            self._ck(self.lib.mlh_scan2map(self.h, _p(pose), C.byref(opts), None))
            return pose, None
        stats = (IterStat * opts.max_outer)()
        self._ck(self.lib.mlh_scan2map(self.h, _p(pose), C.byref(opts), C.cast(stats, C.c_void_p)))
        return pose, [s.as_dict() for s in stats]


def compound_pose_with_cov(pose1, cov1, pose2, cov2):
    a = [np.ascontiguousarray(x, np.float64) for x in (pose1, cov1, pose2, cov2)]
    pose_cp, cov_cp = np.zeros(7), np.zeros((6, 6))
    rc = load_library().mlh_compound_pose_with_cov(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(pose_cp), _p(cov_cp))
    if rc:
        raise MlhError(f"mlh_compound_pose_with_cov -> {rc}")
    return pose_cp, cov_cp


def _torch_rccl_first():
    """A Python host that also uses torch.distributed ends up with torch's bundled librccl mapped; import torch BEFORE the library
    binds RCCL so that both use that one copy (the library binds an already-mapped librccl, see csrc/comm.hip)."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def comm_unique_id() -> bytes:
    _torch_rccl_first()
    buf = C.create_string_buffer(128)
    rc = load_library().mlh_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc:
        raise MlhError(f"mlh_comm_unique_id failed ({rc}): librccl not loadable?")
    return buf.raw


def pose_plus(x, delta, V_update=None):
    x = np.ascontiguousarray(x, np.float64)
    d = np.ascontiguousarray(delta, np.float64)
    V = None if V_update is None else np.ascontiguousarray(V_update, np.float64)
    out = np.zeros(7)
    rc = load_library().mlh_pose_plus(_p(x), _p(d), _p(V), _p(out))
    if rc:
        raise MlhError(f"mlh_pose_plus failed ({rc})")
    return out


def eval_degeneracy(H, eig_thre=100.0):
    H = np.ascontiguousarray(H, np.float64)
    ev = np.zeros(6)
    V = np.zeros((6, 6))
    deg = load_library().mlh_eval_degeneracy(_p(H), eig_thre, _p(ev), _p(V))
    return dict(eigval=ev, V_update=V, is_degenerate=bool(deg))
