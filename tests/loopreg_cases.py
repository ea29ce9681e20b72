"""Cases and plumbing shared by tests/test_loopreg_cases.py (CPU) and tests/test_gpu_loopreg.py (GPU): the C++ restatement of the loop closure's local registration
(tests/host/loopreg_ref.cpp, compiled with plain g++ into a shared object and called through ctypes), the crafted scene -- a floor, two perpendicular walls and six
vertical poles seen from five keyframe positions 1 m apart and seen again displaced by 25 degrees of yaw and (0.6, -0.4, 0.1) m --, the crafted match decisions with
their margins, and a Python transcription of PoseGraph::constructLocalMap's keyframe windows (mloam_loop/src/pose_graph.cpp:374-410). Computed once per process and
shared: do not modify what these functions return."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = np.zeros((0, 4), np.float32)
LEAF = 0.4
TRUTH_YAW_DEG, TRUTH_T = 25.0, (0.6, -0.4, 0.1)
MARGIN = 1e-3                    # every crafted decision stays this far (relative) from its threshold


class Opts(C.Structure):
    """lr_opts of loopreg_ref.cpp"""
    _fields_ = [("max_outer", C.c_int), ("max_lm_iterations", C.c_int), ("huber_delta", C.c_double), ("min_match_ratio", C.c_double), ("threshold", C.c_double),
                ("sq_surf", C.c_float), ("sq_corner", C.c_float), ("plane_dis", C.c_double), ("eig_ratio", C.c_float), ("pad", C.c_int)]


class Outer(C.Structure):
    _fields_ = [("entered", C.c_int), ("ran", C.c_int), ("surf_num", C.c_int), ("corner_num", C.c_int), ("lm_iterations", C.c_int), ("successful_steps", C.c_int),
                ("termination", C.c_int), ("outside", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double)]


class Result(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("para_pose", C.c_double * 7), ("opti_cost", C.c_double), ("accepted", C.c_int), ("n_outer", C.c_int), ("outer", Outer * 8)]


def opts(**kw):
    o = Opts(2, 5, 1.0, 0.2, 2000.0, 2.0, 5.0, 0.2, 3.0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


_BUILD_DIR = None


@functools.lru_cache(maxsize=None)
def ref():
    """the restatement, compiled once per process into a directory of its own"""
    global _BUILD_DIR
    _BUILD_DIR = tempfile.TemporaryDirectory(prefix="loopreg_ref_")
    so = os.path.join(_BUILD_DIR.name, "libloopreg_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"),
           os.path.join(ROOT, "tests", "host", "loopreg_ref.cpp"), "-o", so]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    lib = C.CDLL(so)
    vp, ci, cf, cd = C.c_void_p, C.c_int, C.c_float, C.c_double
    lib.lr_transform.argtypes = [vp, ci, vp, vp]
    lib.lr_match_surf.argtypes = [vp, ci, vp, ci, vp, cf, cd, vp, vp, vp]
    lib.lr_match_corner.argtypes = [vp, ci, vp, ci, vp, cf, cf, vp, vp, vp]
    lib.lr_factor.argtypes = [vp, vp, vp, vp, vp]
    lib.lr_mat_to_quat.argtypes = [vp, vp]
    lib.lr_quat_to_mat.argtypes = [vp, vp]
    lib.lr_evaluate.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, C.POINTER(Opts), vp, vp, vp, vp, vp]
    lib.lr_register.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, C.POINTER(Opts), C.POINTER(Result)]
    for f in (lib.lr_transform, lib.lr_factor, lib.lr_mat_to_quat, lib.lr_quat_to_mat, lib.lr_evaluate, lib.lr_register):
        f.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f4(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 2 and a.shape[1] == 4
    return a


def _Tf(T):
    return np.ascontiguousarray(np.asarray(T, np.float64).astype(np.float32).reshape(16))      # Matrix4d::cast<float>()


def transform(pts, Tf):
    pts = _f4(pts)
    Tf = np.ascontiguousarray(Tf, np.float32).reshape(16)
    out = np.zeros_like(pts)
    ref().lr_transform(_p(pts), len(pts), _p(Tf), _p(out))
    return out


def match_surf(map_s, data_s, T, o=None):
    """-> dict(valid (m,), coeffs (m, 4), n features.size(), sq4 (m,), maxres (m,))"""
    o = o or opts()
    map_s, data_s, Tf = _f4(map_s), _f4(data_s), _Tf(T)
    m = len(data_s)
    valid, coeffs, dbg = np.zeros(m, np.uint8), np.zeros((m, 4)), np.zeros((m, 2), np.float32)
    n = ref().lr_match_surf(_p(map_s), len(map_s), _p(data_s), m, _p(Tf), o.sq_surf, o.plane_dis, _p(valid), _p(coeffs), _p(dbg))
    return dict(valid=valid.astype(bool), coeffs=coeffs, n=n, sq4=dbg[:, 0].copy(), maxres=dbg[:, 1].copy())


def match_corner(map_c, data_c, T, o=None):
    """-> dict(valid (m,), coeffs (m, 2, 4), n features.size(), w1, w2 (m, 3), ld_p (m, 2), eig (m, 3), sq4 (m,))"""
    o = o or opts()
    map_c, data_c, Tf = _f4(map_c), _f4(data_c), _Tf(T)
    m = len(data_c)
    valid, coeffs, dbg = np.zeros(m, np.uint8), np.zeros((m, 2, 4)), np.zeros((m, 12), np.float32)
    n = ref().lr_match_corner(_p(map_c), len(map_c), _p(data_c), m, _p(Tf), o.sq_corner, o.eig_ratio, _p(valid), _p(coeffs), _p(dbg))
    return dict(valid=valid.astype(bool), coeffs=coeffs, n=n, w1=dbg[:, 0:3].copy(), w2=dbg[:, 3:6].copy(), ld_p=dbg[:, 6:8].copy(), eig=dbg[:, 8:11].copy(),
                sq4=dbg[:, 11].copy())


def factor(point, coeff, pose):
    point, coeff, pose = (np.ascontiguousarray(v, np.float64) for v in (point, coeff, pose))
    r, J = np.zeros(3), np.zeros((3, 7))
    ref().lr_factor(_p(point), _p(coeff), _p(pose), _p(r), _p(J))
    return r, J


def mat_to_quat(T):
    T = np.ascontiguousarray(T, np.float64).reshape(16)
    q = np.zeros(4)
    ref().lr_mat_to_quat(_p(T), _p(q))
    return q


def quat_to_mat(q):
    q = np.ascontiguousarray(q, np.float64)
    R = np.zeros(9)
    ref().lr_quat_to_mat(_p(q), _p(R))
    return R.reshape(3, 3)


def pose_of(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.concatenate([T[:3, 3], mat_to_quat(T)])


def evaluate(clouds, T_match, pose, o=None):
    """clouds = (model surf, model corner, data surf, data corner) -> dict(H, g, cost, counts, outside)"""
    o = o or opts()
    c = [_f4(x) for x in clouds]
    Tf, x = _Tf(T_match), np.ascontiguousarray(pose, np.float64)
    H, g, cost, counts, outside = np.zeros((6, 6)), np.zeros(6), np.zeros(1), np.zeros(2, np.int32), np.zeros(1, np.int32)
    ref().lr_evaluate(_p(c[0]), len(c[0]), _p(c[1]), len(c[1]), _p(c[2]), len(c[2]), _p(c[3]), len(c[3]), _p(Tf), _p(x), C.byref(o), _p(H), _p(g), _p(cost), _p(counts),
                      _p(outside))
    return dict(H=H, g=g, cost=float(cost[0]), counts=counts, outside=int(outside[0]))


def register(clouds, T_ini, o=None):
    o = o or opts()
    c = [_f4(x) for x in clouds]
    T = np.ascontiguousarray(T_ini, np.float64).reshape(16)
    r = Result()
    ref().lr_register(_p(c[0]), len(c[0]), _p(c[1]), len(c[1]), _p(c[2]), len(c[2]), _p(c[3]), len(c[3]), _p(T), C.byref(o), C.byref(r))
    outer = [{k: getattr(r.outer[i], k) for k, _ in Outer._fields_} for i in range(r.n_outer)]
    return dict(T_relative=np.array(r.T).reshape(4, 4), para_pose=np.array(r.para_pose), opti_cost=r.opti_cost, accepted=bool(r.accepted), n_outer=r.n_outer, outer=outer)


# ---------------------------------------------------------------- the crafted scene
def yaw_T(deg, t=(0.0, 0.0, 0.0)):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


TRUTH = yaw_T(TRUTH_YAW_DEG, TRUTH_T)
POLES = [(-5.0, -5.0), (-2.0, 5.5), (3.0, -6.0), (6.0, 4.0), (9.5, -3.0), (10.0, 6.5)]


def _sample_keyframe(rng, T_kf, n_surf, n_corner):
    """points of the world (floor z = 0, wall y = 8, wall x = 12, the poles) with 0.02 m jitter, in the keyframe's frame; intensity = a LiDAR id"""
    part = rng.choice(3, n_surf, p=[0.6, 0.2, 0.2])
    u, v = rng.uniform(-8.0, 12.0, n_surf), rng.uniform(-8.0, 8.0, n_surf)
    h = rng.uniform(0.0, 3.0, n_surf)
    surf = np.where(part[:, None] == 0, np.stack([u, v, np.zeros(n_surf)], 1), np.where(part[:, None] == 1, np.stack([u, np.full(n_surf, 8.0), h], 1), np.stack([np.full(n_surf, 12.0), v, h], 1)))
    pole = rng.integers(0, len(POLES), n_corner)
    corner = np.stack([np.array(POLES)[pole, 0], np.array(POLES)[pole, 1], rng.uniform(0.0, 3.0, n_corner)], 1)
    Tinv = np.linalg.inv(T_kf)
    out = []
    for w in (surf, corner):
        w = w + rng.normal(0.0, 0.02, w.shape)
        loc = w @ Tinv[:3, :3].T + Tinv[:3, 3]
        out.append(np.ascontiguousarray(np.concatenate([loc, rng.integers(0, 2, (len(loc), 1)).astype(np.float64)], 1), np.float32))
    return out


@functools.lru_cache(maxsize=None)
def scene():
    """10 keyframes: 0..4 the first pass (1 m apart along x, 1 m above the floor), 5..9 the second pass -- keyframe 5 + i stands where keyframe i stood, displaced by
    TRUTH. The STORED poses of the second pass carry an odometry drift the verification must not see (only relative poses enter constructLocalMap).
    -> dict(poses (10, 4, 4) stored, clouds [(surf, corner)] in keyframe frames, que_index 7, match_index 2, pose_ini I, clouds4 the four filtered clouds as
    constructLocalMap restated makes them, pre4 the pre-filter ones, lists the (key, Matrix4f) lists, truth, T_ini)"""
    import oracle as orc
    orc.build()
    rng = np.random.default_rng(12)
    true, stored, clouds = [], [], []
    drift = yaw_T(3.0, (1.5, -2.0, 0.3))
    for k in range(10):
        base = np.eye(4)
        base[:3, 3] = [float(k % 5), 0.0, 1.0]
        T = base if k < 5 else base @ TRUTH
        true.append(T)
        stored.append(T if k < 5 else drift @ T)
        clouds.append(_sample_keyframe(rng, T, int(rng.integers(300, 601)), int(rng.integers(40, 81))))
    que_index, match_index = 7, 2
    pose_ini = np.eye(4)
    # the two passes as the two lists (the C-ABI takes lists; the windows that choose them in the reference are the facade's, held in test_loopreg_cases.py)
    data_keys, model_keys = [5, 6, 7, 8, 9], [0, 1, 2, 3, 4]
    data = [(k, chain_data(pose_ini, stored[que_index], stored[k])) for k in data_keys]
    model = [(k, chain_model(stored[match_index], stored[k])) for k in model_keys]
    pre4 = []
    for lst in (model, data):
        for kind in (0, 1):
            parts = [transform(clouds[k][kind], Tf) for k, Tf in lst]
            pre4.append(np.concatenate(parts) if parts else EMPTY)
    clouds4 = [orc.voxel_grid(p, LEAF) if len(p) else EMPTY for p in pre4]
    truth = np.linalg.inv(true[match_index]) @ true[que_index]
    T_ini = yaw_T(round(TRUTH_YAW_DEG / 6.0) * 6.0)                      # the Scan Context yaw on the 6-degree sector grid, zero translation
    return dict(poses=np.array(stored), clouds=clouds, que_index=que_index, match_index=match_index, pose_ini=pose_ini, lists=(data, model), pre4=pre4, clouds4=clouds4,
                truth=truth, T_ini=T_ini)


# ---------------------------------------------------------------- constructLocalMap's keyframe windows and matrix chains, transcribed (pose_graph.cpp:374-410)
def data_window(que_index, history, has):
    out = []
    for j in range(-history, 1):
        if que_index + j < 0:
            continue
        if not has(que_index + j):
            continue
        out.append(que_index + j)
    return out


def model_window(que_index, match_index, history, has):
    out = []
    for j in range(-history, history + 1):
        if match_index + j < 0 or match_index + j >= que_index:
            continue
        if not has(match_index + j):
            continue
        out.append(match_index + j)
    return out


def chain_data(T_ini, T_cur, T_kf):
    """T_ini_map_kf.cast<float>() (cpp:381-383)"""
    return (np.asarray(T_ini) @ (np.linalg.inv(T_cur) @ np.asarray(T_kf))).astype(np.float32)


def chain_model(T_old, T_kf):
    """T_relative.cast<float>() (cpp:405-406)"""
    return (np.linalg.inv(T_old) @ np.asarray(T_kf)).astype(np.float32)


# ---------------------------------------------------------------- crafted match decisions
def _group(center, offsets):
    return np.asarray(center, np.float64)[None, :] + np.asarray(offsets, np.float64)


@functools.lru_cache(maxsize=None)
def crafted():
    """Model and data clouds of isolated groups, one data point per group, matched at the identity. The surf groups are horizontal patches stacked 10 m apart above
    the origin: matchSurfFromMap's fit solves n . p = -1 in the algebraic sense, which is a plane fit only while the plane's offset is the dominant coordinate; the
    corner groups stand 40 m apart.
    surf:   0 fifth neighbour just inside 2.0 | 1 just outside | 2 one neighbour 0.25 m off the fitted plane (rejected) | 3 0.15 m off (kept) | 4 three map points only
    corner: 0 fifth neighbour just inside 5.0 | 1 just outside | 2 a blob (ratio < 3, rejected) | 3 a line (kept) | 4 three map points only
    -> dict(clouds4, surf_want, corner_want (the decisions), and the restatement's matches); asserts every decision's margin on the restatement's values"""
    def cloud(groups):
        p = np.concatenate(groups)
        return np.ascontiguousarray(np.concatenate([p, np.zeros((len(p), 1))], 1), np.float32)

    square = [(0.5, 0.4, 0.0), (-0.45, 0.5, 0.0), (-0.5, -0.4, 0.0), (0.4, -0.5, 0.0)]
    o = opts()

    def surf_clouds(lift):
        g, q = [], []
        for k, r5 in enumerate((np.sqrt(2.0 * (1.0 - 4e-3)), np.sqrt(2.0 * (1.0 + 4e-3)))):
            c = (0.0, 0.0, 10.0 * (1 + k))
            g.append(_group(c, square + [(r5, 0.0, 0.0)])); q.append(c)
        for k, h in enumerate(lift):
            c = (0.0, 0.0, 10.0 * (3 + k))
            g.append(_group(c, square + [(0.05, 0.02, h)])); q.append(c)
        c = (0.0, 0.0, 50.0)
        g.append(_group(c, square[:3])); q.append(c)
        return cloud(g), cloud([np.array(q)])

    # the lift that leaves the worst neighbour 0.25 / 0.15 m from the FITTED plane: the residual is close to linear in the lift, two secant steps find it
    lift = [0.3, 0.2]
    for _ in range(4):
        ms, ds = surf_clouds(lift)
        r = match_surf(ms, ds, np.eye(4), o)["maxres"][2:4]
        lift = [lift[0] * 0.25 / float(r[0]), lift[1] * 0.15 / float(r[1])]
    ms, ds = surf_clouds(lift)
    s = match_surf(ms, ds, np.eye(4), o)
    rel = lambda v, thr: abs(float(v) - thr) / thr
    assert rel(s["sq4"][0], 2.0) >= MARGIN and s["sq4"][0] < 2.0 and rel(s["sq4"][1], 2.0) >= MARGIN and s["sq4"][1] > 2.0
    assert abs(s["maxres"][2] - 0.25) < 5e-3 and abs(s["maxres"][3] - 0.15) < 5e-3 and rel(s["maxres"][2], 0.2) >= MARGIN and rel(s["maxres"][3], 0.2) >= MARGIN
    assert rel(s["maxres"][0], 0.2) >= MARGIN and s["maxres"][0] < 0.2
    assert s["sq4"][4] > 100.0                                               # (the fifth nearest point belongs to another group)
    surf_want = [True, False, False, True, False]
    assert s["valid"].tolist() == surf_want and s["n"] == 2

    line = [(0.0, 0.0, -0.8), (0.01, 0.0, -0.4), (0.0, 0.01, 0.0), (-0.01, 0.0, 0.4)]
    g, q = [], []
    for k, r5 in enumerate((np.sqrt(5.0 * (1.0 - 4e-3)), np.sqrt(5.0 * (1.0 + 4e-3)))):
        c = (40.0 * k, -3.0, 1.5)
        g.append(_group(c, line + [(0.3, 0.0, r5)])); q.append((c[0] + 0.3, c[1], c[2]))
    c = (80.0, -3.0, 1.5)
    g.append(_group(c, [(0.5, 0.0, 0.0), (-0.5, 0.1, 0.0), (0.0, 0.5, 0.1), (0.1, -0.5, 0.0), (0.0, 0.1, 0.5)])); q.append((c[0] + 0.1, c[1], c[2]))
    c = (120.0, -3.0, 1.5)
    g.append(_group(c, line + [(0.0, 0.0, 0.8)])); q.append((c[0] + 0.3, c[1] + 0.2, c[2]))
    c = (160.0, -3.0, 1.5)
    g.append(_group(c, line[:3])); q.append(c)
    mc, dc = cloud(g), cloud([np.array(q)])
    cr = match_corner(mc, dc, np.eye(4), o)
    # (the data points stand 0.3 m beside the line; the fifth neighbour is straight above them)
    assert cr["sq4"][0] < 5.0 and rel(cr["sq4"][0], 5.0) >= MARGIN and cr["sq4"][1] > 5.0 and rel(cr["sq4"][1], 5.0) >= MARGIN
    for i in (0, 2, 3):
        ratio = float(cr["eig"][i][2]) / max(float(cr["eig"][i][1]), 1e-30)
        assert rel(ratio, 3.0) >= MARGIN, (i, ratio)
    assert cr["eig"][2][2] < 3.0 * cr["eig"][2][1] and cr["eig"][3][2] > 3.0 * cr["eig"][3][1]
    corner_want = [True, False, False, True, False]
    assert cr["valid"].tolist() == corner_want and cr["n"] == 4
    return dict(clouds4=[ms, mc, ds, dc], surf_want=surf_want, corner_want=corner_want, surf=s, corner=cr)
