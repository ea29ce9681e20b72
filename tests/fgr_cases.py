"""Cases and plumbing shared by tests/test_fgr_cases.py (CPU) and tests/test_gpu_fgr.py (GPU): the C++ restatement of performGlobalRegistration
(tests/host/fgr_ref.cpp, compiled with plain g++ into a shared object and called through ctypes), the test clouds -- a 2 x 2 x 2-cell room (floor, two walls, a box
and a slanted board, 0.02 m of jitter) sampled twice, clouds of 0 to 3 points and one cloud inside a single cell --, the registration scene (a 500-point model and
its copy moved by yaw 0.3 rad and 1.5 m) and the measured tolerances of tests/golden/fgr_tolerances.json (`python tests/fgr_cases.py` measures and rewrites them).
Computed once per process and shared: do not modify what these functions return."""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_PATH = os.path.join(ROOT, "tests", "golden", "fgr_tolerances.json")
DIM, BINS = 33, 11
NORMAL_RADIUS, FPFH_RADIUS = 1.0, 1.5
TRUTH_YAW, TRUTH_T = 0.3, (0.9, -0.8, 0.9)          # |t| = 1.503 m; the data frame's origin stays inside the room, so both clouds' normals face inwards
f32 = np.float32


class Opts(C.Structure):
    """mlh_fgr_opts"""
    _fields_ = [("normal_radius", C.c_float), ("fpfh_radius", C.c_float), ("div_factor", C.c_double), ("use_absolute_scale", C.c_int32), ("iteration_number", C.c_int32),
                ("max_corr_dist", C.c_double), ("tuple_scale", C.c_float), ("tuple_max_cnt", C.c_int32), ("global_registration_threshold", C.c_double), ("seed", C.c_uint64)]


class Result(C.Structure):
    """mlh_fgr_result"""
    _fields_ = [("T_relative", C.c_double * 16), ("final_cost_normalize", C.c_double), ("final_cost", C.c_double), ("global_scale", C.c_double), ("start_scale", C.c_double),
                ("means", C.c_double * 6), ("accepted", C.c_int32), ("swapped", C.c_int32), ("n_mutual", C.c_int32), ("n_tuples", C.c_int32), ("n_corres", C.c_int32),
                ("n_trials", C.c_int32), ("host_waits", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(T_relative=np.array(self.T_relative).reshape(4, 4), final_cost_normalize=self.final_cost_normalize, final_cost=self.final_cost,
                    global_scale=self.global_scale, start_scale=self.start_scale, means=np.array(self.means).reshape(2, 3), accepted=bool(self.accepted),
                    swapped=bool(self.swapped), n_mutual=self.n_mutual, n_tuples=self.n_tuples, n_corres=self.n_corres, n_trials=self.n_trials)


_BUILD_DIR = None


@functools.lru_cache(maxsize=None)
def ref():
    """the restatement, compiled once per process into a directory of its own"""
    global _BUILD_DIR
    _BUILD_DIR = tempfile.TemporaryDirectory(prefix="fgr_ref_")
    so = os.path.join(_BUILD_DIR.name, "libfgr_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "m-loam_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "fgr_ref.cpp"), "-o", so]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    lib = C.CDLL(so)
    vp, ci, cf, cd = C.c_void_p, C.c_int, C.c_float, C.c_double
    lib.fr_normals.argtypes = [vp, ci, cf, vp, vp, vp, vp, vp]
    lib.fr_spfh.argtypes = [vp, ci, vp, cf, vp, vp, vp]
    lib.fr_fpfh.argtypes = [vp, ci, vp, vp, cf, vp]
    lib.fr_match.argtypes = [vp, ci, vp, ci, vp, vp]
    lib.fr_normalize.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp]
    lib.fr_tail.argtypes = [vp, ci, vp, ci, vp, ci, ci, C.POINTER(Opts), C.POINTER(Result)]
    lib.fr_register.argtypes = [vp, ci, vp, ci, C.POINTER(Opts), vp, vp, vp, vp, C.POINTER(Result), vp, vp]
    lib.fr_pair_features.argtypes = [vp, vp, vp, vp, vp]
    lib.fr_bins.argtypes = [vp, vp]
    lib.fr_spfh_value.argtypes = [ci, ci]
    lib.fr_spfh_value.restype = cf
    lib.fr_l2.argtypes = [vp, vp]
    lib.fr_l2.restype = cf
    lib.fr_opts_fault.argtypes = [C.POINTER(Opts)]
    lib.fr_opts_default.argtypes = [C.POINTER(Opts)]
    lib.fr_tuple_test.argtypes = [vp, ci, ci, cf, ci, C.c_uint64, vp, vp]
    lib.fr_rng_draw.argtypes = [C.c_uint64, ci]
    lib.fr_rng_draw.restype = C.c_uint32
    lib.fr_optimize.argtypes = [vp, ci, cd, cd, cd, ci, vp, vp]
    for f in (lib.fr_normals, lib.fr_spfh, lib.fr_fpfh, lib.fr_normalize, lib.fr_tail, lib.fr_register, lib.fr_bins, lib.fr_opts_default):
        f.restype = None
    return lib


def opts(**kw):
    o = Opts()
    ref().fr_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f4(a):
    a = np.ascontiguousarray(a, f32)
    assert a.ndim == 2 and a.shape[1] == 4
    return a


# ---------------------------------------------------------------- the restatement's stages
def normals(cloud, radius=NORMAL_RADIUS):
    c = _f4(cloud)
    n = len(c)
    out = dict(normals=np.zeros((n, 4), f32), normals64=np.zeros((n, 4)), flag_flip=np.zeros(n, np.uint8), flag_gap=np.zeros(n, np.uint8), k=np.zeros(n, np.int32))
    ref().fr_normals(_p(c), n, radius, _p(out["normals"]), _p(out["normals64"]), _p(out["flag_flip"]), _p(out["flag_gap"]), _p(out["k"]))
    out["flagged"] = (out["flag_flip"] | out["flag_gap"]).astype(bool)
    return out


def spfh(cloud, normals4, radius=FPFH_RADIUS):
    c, nm = _f4(cloud), _f4(normals4)
    n = len(c)
    out = dict(counts=np.zeros((n, DIM), np.int32), k=np.zeros(n, np.int32), fragile=np.zeros(n, np.int32))
    ref().fr_spfh(_p(c), n, _p(nm), radius, _p(out["counts"]), _p(out["k"]), _p(out["fragile"]))
    return out


def fpfh(cloud, counts, k, radius=FPFH_RADIUS):
    c = _f4(cloud)
    n = len(c)
    cn, kk = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(k, np.int32)
    out = np.zeros((n, DIM), f32)
    ref().fr_fpfh(_p(c), n, _p(cn), _p(kk), radius, _p(out))
    return out


def features(cloud):
    nm = normals(cloud)["normals"]
    s = spfh(cloud, nm)
    return fpfh(cloud, s["counts"], s["k"])


def match(f0, f1):
    a, b = np.ascontiguousarray(f0, f32).reshape(-1, DIM), np.ascontiguousarray(f1, f32).reshape(-1, DIM)
    pairs = np.zeros((min(len(a), len(b)) + 1, 2), np.int32)
    sw = C.c_int32(0)
    n = ref().fr_match(_p(a), len(a), _p(b), len(b), _p(pairs), C.byref(sw))
    return pairs[:n].copy(), bool(sw.value)


def normalize(c0, c1, use_absolute_scale=1):
    a, b = _f4(c0), _f4(c1)
    np0, np1, means, scales = np.zeros((len(a), 3), f32), np.zeros((len(b), 3), f32), np.zeros(6, f32), np.zeros(2, f32)
    ref().fr_normalize(_p(a), len(a), _p(b), len(b), use_absolute_scale, _p(np0), _p(np1), _p(means), _p(scales))
    return np0, np1, means.reshape(2, 3), scales


def tail(c0, c1, pairs, swapped, o=None):
    a, b, pr = _f4(c0), _f4(c1), np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    r = Result()
    ref().fr_tail(_p(a), len(a), _p(b), len(b), _p(pr), len(pr), int(swapped), C.byref(o if o is not None else opts()), C.byref(r))
    return r.as_dict()


def register(c0, c1, o=None):
    a, b = _f4(c0), _f4(c1)
    r, pairs, n = Result(), np.zeros((min(len(a), len(b)) + 1, 2), np.int32), C.c_int32(0)
    ref().fr_register(_p(a), len(a), _p(b), len(b), C.byref(o if o is not None else opts()), None, None, None, None, C.byref(r), _p(pairs), C.byref(n))
    d = r.as_dict()
    d["pairs"] = pairs[:n.value].copy()
    return d


# ---------------------------------------------------------------- the clouds
MIN_SPACING = 0.15     # as a voxel-filtered cloud has one: two points closer than this share their whole normal_radius neighbourhood, hence (to rounding) their
                       # normal, and every such pair sits on the swap decision of computePairFeatures


def _surface_candidates(rng, n):
    """n candidate points of the room: floor z = -1.2, walls x = -1.4 and y = 1.4, a 0.6 m box on the floor, a board tilted 35 degrees, 0.02 m of jitter;
    everything inside (-1.5, 1.5)^3"""
    share = np.array([0.30, 0.22, 0.22, 0.14, 0.12])
    cnt = np.floor(share * n).astype(int)
    cnt[0] += n - cnt.sum()
    u = lambda m, lo, hi: rng.uniform(lo, hi, m)
    parts = [np.stack([u(cnt[0], -1.4, 1.4), u(cnt[0], -1.4, 1.4), np.full(cnt[0], -1.2)], 1),
             np.stack([np.full(cnt[1], -1.4), u(cnt[1], -1.4, 1.4), u(cnt[1], -1.2, 1.3)], 1),
             np.stack([u(cnt[2], -1.4, 1.4), np.full(cnt[2], 1.4), u(cnt[2], -1.2, 1.3)], 1)]
    m = cnt[3]                                                       # the box: its top and the two faces towards the room
    face = rng.integers(0, 3, m)
    a, b = u(m, 0.0, 0.6), u(m, 0.0, 0.6)
    box = np.where(face[:, None] == 0, np.stack([0.5 + a, -1.3 + b, np.full(m, -0.6)], 1),
                   np.where(face[:, None] == 1, np.stack([np.full(m, 0.5), -1.3 + a, -1.2 + b], 1), np.stack([0.5 + a, np.full(m, -0.7), -1.2 + b], 1)))
    parts.append(box)
    m = cnt[4]                                                       # the board: from (-1.3, -0.9) rising along x
    s, t = u(m, 0.0, 1.0), u(m, 0.0, 0.8)
    ang = np.radians(35.0)
    parts.append(np.stack([-1.3 + s * np.cos(ang), -0.9 + t, -1.1 + s * np.sin(ang)], 1))
    p = np.concatenate(parts) + rng.normal(0.0, 0.02, (n, 3))
    return np.clip(p, -1.49, 1.49)[rng.permutation(n)]


def _thin(cand, n, spacing):
    """the first n candidates that keep `spacing` from everything kept before them"""
    kept = []
    for p in cand:
        if all(np.sum((p - q) ** 2) >= spacing ** 2 for q in kept):
            kept.append(p)
            if len(kept) == n:
                break
    assert len(kept) == n
    return np.array(kept)


def _surfaces(rng, n):
    """n points of the room, no two closer than MIN_SPACING"""
    p = _thin(_surface_candidates(rng, 6 * n), n, MIN_SPACING)
    return np.ascontiguousarray(np.concatenate([p, rng.uniform(0, 1, (n, 1))], 1), f32)


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> (n, 4) float32. room_a / room_b: two samplings (307 and 353 points: no multiple of 16, 64 or 128; more than one workgroup of every kernel;
    about one point in twenty has a pair feature within 1e-5 of a bin edge by chance alone: 3 k features x 2e-4 of the range); one_cell: 97 points of a bowl 1.4 m
    wide, inside one index cell; tiny_0 .. tiny_3: 0 to 3 points 1.2 m apart"""
    rng = np.random.default_rng(1301)
    out = {"room_a": _surfaces(rng, 307), "room_b": _surfaces(rng, 353)}
    one = rng.uniform(0.0, 1.4, (600, 3))                           # a bowl: the neighbour sets, and so the normals, differ from point to point
    one[:, 2] = 0.25 * (one[:, 0] ** 2 + one[:, 1] ** 2) + rng.normal(0, 0.02, 600)
    one = _thin(one, 97, 0.1)
    out["one_cell"] = np.ascontiguousarray(np.concatenate([one, np.zeros((97, 1))], 1), f32)
    # 1.2 m apart: inside each other's fpfh_radius, outside the normal_radius -- NaN normals (fewer than 3 neighbours), pair features that are NaN
    tiny = np.array([[0.6, 0.1, -0.3, 0], [-0.6, 0.1, -0.3, 0], [0.0, 0.1, 0.74, 0]], f32)
    for m in range(4):
        out[f"tiny_{m}"] = np.ascontiguousarray(tiny[:m].reshape(m, 4))
    return out


def truth_T():
    c, s = np.cos(TRUTH_YAW), np.sin(TRUTH_YAW)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = TRUTH_T
    return T


@functools.lru_cache(maxsize=None)
def scene():
    """the registration scene: model = 500 points of the room; data = the same points in a frame moved by truth_T (model = T data), in f32"""
    model = _surfaces(np.random.default_rng(77), 500)
    T = truth_T()
    q = (model[:, :3].astype(np.float64) - T[:3, 3]) @ T[:3, :3]          # R^T (p - t)
    data = np.ascontiguousarray(np.concatenate([q, model[:, 3:4]], 1), f32)
    return dict(model=model, data=data, truth=T)


@functools.lru_cache(maxsize=None)
def scene_reference():
    s = scene()
    return register(s["model"], s["data"])


def angle_between(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.abs(np.sum(a * b, 1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.arccos(np.clip(c, 0.0, 1.0))


# ---------------------------------------------------------------- the measured tolerances
def measure_tolerances():
    """normal_angle: the largest angle between the f32 restatement and the same code in f64 over the unflagged points of the test clouds (the bound is 8 x: two
    libm implementations differ in the trigonometry of computeRoots); register_T: the restatement's own end-to-end error max |T - truth| on the scene (the bound
    is 2 x)"""
    worst = 0.0
    for name, c in clouds().items():
        if len(c) < 3:
            continue
        r = normals(c)
        ok = ~r["flagged"] & np.isfinite(r["normals"][:, 0])
        if ok.any():
            worst = max(worst, float(angle_between(r["normals"][ok, :3], r["normals64"][ok, :3]).max()))
    err = float(np.abs(scene_reference()["T_relative"] - scene()["truth"]).max())
    return {"normal_angle_measured_rad": worst, "normal_angle_bound_rad": 8.0 * worst, "register_T_measured": err, "register_T_bound": 2.0 * err}


def tolerances():
    with open(TOL_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    t = measure_tolerances()
    with open(TOL_PATH, "w") as f:
        json.dump(t, f, indent=1, sort_keys=True)
        f.write("\n")
    print(t)
