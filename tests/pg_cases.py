"""Cases and plumbing shared by tests/test_pg_cases.py (CPU) and tests/test_gpu_posegraph.py (GPU): the C++ restatement of the pose-graph optimisation
(tests/host/pg_ref.cpp, compiled with plain g++ and -ffp-contract=off into a shared object and called through ctypes) and the crafted pose graphs -- 1 m steps on
a gentle curve with small random rotations, an estimate that drifts away from that truth, loop measurements that are the TRUE relative pose plus a stated
perturbation. Computed once per process and shared: do not modify what these functions return (Graph.copy() gives a graph of one's own)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
from scipy.spatial.transform import Rotation as Rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_VAR, Q_VAR, HUBER, MAX_IT = 0.1, 0.01, 1.0, 5
DECISION_MARGIN = 1e-6           # every LM decision of the restatement stays this far (relative) from its threshold on every full-optimise case


class Opts(C.Structure):
    """pgr_opts of pg_ref.cpp"""
    _fields_ = [("max_num_iterations", C.c_int), ("pad", C.c_int), ("t_var", C.c_double), ("q_var", C.c_double), ("huber_delta", C.c_double)]


class Result(C.Structure):
    """pgr_result of pg_ref.cpp"""
    _fields_ = [("num_iterations", C.c_int), ("num_successful_steps", C.c_int), ("termination", C.c_int), ("n_keyframes", C.c_int), ("n_loops", C.c_int),
                ("n_decisions", C.c_int), ("n_rejected", C.c_int), ("n_refused", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("drift", C.c_double * 7), ("min_margin", C.c_double),
                ("margin_relative_decrease", C.c_double), ("margin_function", C.c_double), ("margin_parameter", C.c_double), ("margin_gradient", C.c_double),
                ("margin_model", C.c_double), ("solve_radius", C.c_double)]


def opts(**kw):
    o = Opts(MAX_IT, 0, T_VAR, Q_VAR, HUBER)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


_BUILD_DIR = None


@functools.lru_cache(maxsize=None)
def ref():
    """the restatement, compiled once per process into a directory of its own"""
    global _BUILD_DIR
    _BUILD_DIR = tempfile.TemporaryDirectory(prefix="pg_ref_")
    so = os.path.join(_BUILD_DIR.name, "libpg_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"),
           os.path.join(ROOT, "tests", "host", "pg_ref.cpp"), "-o", so]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    lib = C.CDLL(so)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.pgr_edge.argtypes = [vp, vp, vp, cd, cd, vp, vp, vp]
    lib.pgr_plus.argtypes = [vp, vp, vp]
    lib.pgr_pose_mul.argtypes = [vp, vp, vp]
    lib.pgr_pose_inverse.argtypes = [vp, vp]
    lib.pgr_linearize.argtypes = [vp, vp, vp, ci, ci, C.POINTER(Opts), vp, vp, vp, vp, C.POINTER(cd), vp, vp]
    lib.pgr_solve_step.argtypes = [vp, vp, vp, ci, ci, C.POINTER(Opts), cd, vp, vp]
    lib.pgr_dense_step.argtypes = [vp, vp, ci, cd, vp, vp]
    lib.pgr_optimize.argtypes = [vp, vp, vp, vp, ci, ci, ci, C.POINTER(Opts), C.c_uint, C.POINTER(Result)]
    for f in (lib.pgr_edge, lib.pgr_plus, lib.pgr_pose_mul, lib.pgr_pose_inverse, lib.pgr_optimize):
        f.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def edge(pi, pj, meas, t_var=T_VAR, q_var=Q_VAR):
    """the restatement's uncorrected factor: r (6,), Ji, Jj (6, 6) over [rotation, translation]"""
    pi, pj, meas = (np.ascontiguousarray(a, np.float64).reshape(7) for a in (pi, pj, meas))
    r, Ji, Jj = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    ref().pgr_edge(_p(pi), _p(pj), _p(meas), t_var, q_var, _p(r), _p(Ji), _p(Jj))
    return r, Ji, Jj


def plus(x, delta):
    x, delta, out = np.ascontiguousarray(x, np.float64).reshape(7), np.ascontiguousarray(delta, np.float64).reshape(6), np.zeros(7)
    ref().pgr_plus(_p(x), _p(delta), _p(out))
    return out


def pose_mul(a, b):
    a, b, out = np.ascontiguousarray(a, np.float64).reshape(7), np.ascontiguousarray(b, np.float64).reshape(7), np.zeros(7)
    ref().pgr_pose_mul(_p(a), _p(b), _p(out))
    return out


def pose_inverse(a):
    a, out = np.ascontiguousarray(a, np.float64).reshape(7), np.zeros(7)
    ref().pgr_pose_inverse(_p(a), _p(out))
    return out


def dense_step(H, g, radius):
    """the restatement's one linear solve from given normal equations: dict(step, delta, ok)"""
    H, g = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(g, np.float64)
    n = len(g)
    assert H.shape == (n, n)
    step, delta = np.zeros(n), np.zeros(n)
    ok = ref().pgr_dense_step(_p(H), _p(g), n, float(radius), _p(step), _p(delta))
    return dict(step=step, delta=delta, ok=bool(ok))


def _pose(R, t):
    return np.concatenate([np.asarray(t, np.float64), R.as_quat()])


def _split(p):
    return Rot.from_quat(p[3:]), p[:3]


def relative(pi, pj):
    """T_i^-1 T_j as [t, q(xyzw)] (NumPy / SciPy: used to craft measurements, never as a reference)"""
    Ri, ti = _split(pi)
    Rj, tj = _split(pj)
    return _pose(Ri.inv() * Rj, Ri.inv().apply(tj - ti))


class Graph:
    """a pose graph as the caller holds it: poses, last poses (count, 7), loop_index (count,), loop_rel (count, 7), earliest"""

    def __init__(self, poses):
        self.poses = np.ascontiguousarray(poses, np.float64).copy()
        n = len(self.poses)
        self.last = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n, 1))
        self.loop_index = np.full(n, -1, np.int32)
        self.loop_rel = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n, 1))
        self.earliest = -1

    def copy(self):
        g = Graph(self.poses)
        g.last, g.loop_index, g.loop_rel, g.earliest = self.last.copy(), self.loop_index.copy(), self.loop_rel.copy(), self.earliest
        return g

    def set_loop(self, index, loop_index, rel):
        self.loop_index[index] = loop_index
        self.loop_rel[index] = rel
        if self.earliest > loop_index or self.earliest == -1:
            self.earliest = loop_index

    def n_loops(self, cur):
        return int((self.loop_index[self.earliest:cur + 1] >= 0).sum())

    def upload(self, ctx):
        """the same graph into a context's store (mlh_pg_reset, then adds and set_loops in index order)"""
        ctx.pg_reset()
        for k in range(len(self.poses)):
            assert ctx.pg_add_keyframe(self.poses[k]) == k
        for k in np.nonzero(self.loop_index >= 0)[0]:
            ctx.pg_set_loop(int(k), int(self.loop_index[k]), self.loop_rel[k])

    # ---- the restatement
    def linearize(self, cur, dense=True):
        M = cur - self.earliest + 1
        n = 6 * (M - 1)
        ij, r, Ji, Jj = np.zeros((5 * M, 2), np.int32), np.zeros((5 * M, 6)), np.zeros((5 * M, 6, 6)), np.zeros((5 * M, 6, 6))
        H, g, cost = np.zeros((n, n)), np.zeros(n), C.c_double(0.0)
        o = opts()
        e = ref().pgr_linearize(_p(self.poses), _p(self.loop_index), _p(self.loop_rel), self.earliest, cur, C.byref(o), _p(ij), _p(r), _p(Ji), _p(Jj), C.byref(cost),
                                _p(H) if dense else None, _p(g) if dense else None)
        return dict(ij=ij[:e].copy(), r=r[:e].copy(), Ji=Ji[:e].copy(), Jj=Jj[:e].copy(), cost=cost.value, H=H, g=g)

    def solve_step(self, cur, radius):
        n = 6 * (cur - self.earliest)
        step, delta = np.zeros(n), np.zeros(n)
        o = opts()
        ok = ref().pgr_solve_step(_p(self.poses), _p(self.loop_index), _p(self.loop_rel), self.earliest, cur, C.byref(o), float(radius), _p(step), _p(delta))
        return dict(step=step, delta=delta, ok=bool(ok))

    def optimize(self, cur, fail_mask=0, **kw):
        """one pass of optimizePoseGraph's body on a COPY: -> (the graph after it, the restatement's result). fail_mask: bit k set refuses the linear solve of
        iteration k + 1, as a non-positive pivot would (the solver's invalid-step branch)"""
        g = self.copy()
        res, o = Result(), opts(**kw)
        ref().pgr_optimize(_p(g.poses), _p(g.last), _p(g.loop_index), _p(g.loop_rel), len(g.poses), g.earliest, cur, C.byref(o), int(fail_mask), C.byref(res))
        return g, res


def trajectory(n, seed, drift_t=2e-3, drift_r=2e-4):
    """(truth, estimate), each (n, 7): 1 m steps along a heading that turns 0.02 rad per step, a small random rotation on every pose; the estimate chains the true
    relative motions with noise of drift_t metres / drift_r radians per step"""
    rng = np.random.default_rng(seed)
    truth = []
    pos = np.zeros(3)
    for k in range(n):
        yaw = 0.02 * k
        if k:
            pos = pos + np.array([np.cos(yaw), np.sin(yaw), 0.01 * np.sin(0.3 * k)])
        R = Rot.from_euler("z", yaw) * Rot.from_rotvec(rng.normal(size=3) * 0.02)
        truth.append(_pose(R, pos))
    truth = np.array(truth)
    est = [truth[0].copy()]
    for k in range(1, n):
        rel = relative(truth[k - 1], truth[k])
        Rr, tr = _split(rel)
        Rr = Rr * Rot.from_rotvec(rng.normal(size=3) * drift_r)
        tr = tr + rng.normal(size=3) * drift_t
        Rp, tp = _split(est[-1])
        est.append(_pose(Rp * Rr, tp + Rp.apply(tr)))
    return truth, np.array(est)


def loop_measurement(truth, index, loop_index, pert_t=(0, 0, 0), pert_rotvec=(0, 0, 0)):
    """the true relative pose T_loop^-1 T_index with pert_t added to its translation and exp(pert_rotvec) multiplied onto its rotation from the right"""
    rel = relative(truth[loop_index], truth[index])
    R, t = _split(rel)
    return _pose(R * Rot.from_rotvec(np.asarray(pert_rotvec, np.float64)), t + np.asarray(pert_t, np.float64))


def make_graph(n, loops, seed, **kw):
    """loops: (index, loop_index) or (index, loop_index, pert_t, pert_rotvec); the default perturbation is 1 cm / 1 mrad"""
    truth, est = trajectory(n, seed, **kw)
    g = Graph(est)
    for spec in loops:
        j, i = spec[0], spec[1]
        pt = spec[2] if len(spec) > 2 else (0.01, -0.01, 0.005)
        pr = spec[3] if len(spec) > 3 else (0.001, 0.0005, -0.001)
        g.set_loop(j, i, loop_measurement(truth, j, i, pt, pr))
    return g


# ---- the crafted graphs (each built once)
@functools.lru_cache(maxsize=None)
def graph_linearize():
    """one graph, first = 0, read at cur = 1 (M = 2: one free block, a loop onto the constant block), 4 (M = 5: band not yet full), 5 (M = 6: first full band) and
    69 (M = 70). Loops: 1 -> 0 and 4 -> 0 end on the constant block; 3 -> 1, 5 -> 2 and 69 -> 66 have both ends inside the band (Huber inactive: little drift over
    three steps, a 1 cm / 1 mrad perturbation); 40 -> 10 and 60 -> 3 are perturbed by decimetres and hundredths of a radian (Huber active)."""
    far = ((0.3, -0.2, 0.1), (0.01, 0.0, 0.02))
    return make_graph(75, [(1, 0), (3, 1), (4, 0), (5, 2), (40, 10) + far, (60, 3) + far, (69, 66)], seed=11, drift_t=5e-3, drift_r=5e-4)


LINEARIZE_CURS = (1, 4, 5, 69)


@functools.lru_cache(maxsize=None)
def graph_step(name):
    """graphs for one linear solve: (graph, cur). L0: no loop edge inside first..cur; L1; L3: 30 -> 5 and 25 -> 10 nested, 35 -> 20 crossing both; L24: 6 L + 1 = 145
    columns (past 128 lanes, and C past the dense stage's LDS image); M130: 130 keyframes."""
    if name == "L0":
        return make_graph(30, [(28, 2)], seed=21), 20
    if name == "L1":
        return make_graph(22, [(19, 1)], seed=22), 21
    if name == "L3":
        return make_graph(42, [(30, 5), (25, 10), (35, 20)], seed=23), 40
    if name == "L24":
        return make_graph(62, [(k, k - 28) for k in range(30, 54)], seed=24), 60
    if name == "M130":
        return make_graph(131, [(40, 1), (70, 20), (100, 50), (125, 3), (129, 90)], seed=25), 130
    raise KeyError(name)


STEP_CASES = ("L0", "L1", "L3", "L24", "M130")
STEP_RADIUS = 1e4


@functools.lru_cache(maxsize=None)
def graph_optimize(name):
    """graphs for a full optimise: (graph, cur). converge: first = 5 > 0, five keyframes after cur; rejected: one loop measurement rotated by 170 degrees about z
    from the truth (in the restatement its second iteration ends on the function tolerance: num_successful_steps 1 < num_iterations 2); L0: a loop exists (50 -> 4)
    but none inside first..cur = 4..20."""
    if name == "converge":
        return make_graph(40, [(30, 5), (34, 8)], seed=31, drift_t=5e-3, drift_r=5e-4), 34
    if name == "rejected":
        return make_graph(32, [(25, 3, (0.0, 0.0, 0.0), (0.0, 0.0, np.deg2rad(170.0)))], seed=32, drift_t=5e-3, drift_r=5e-4), 27
    if name == "L0":
        return make_graph(52, [(50, 4)], seed=33), 20
    raise KeyError(name)


OPTIMIZE_CASES = ("converge", "rejected", "L0")


@functools.lru_cache(maxsize=None)
def optimized(name):
    """the restatement's pass over graph_optimize(name): (graph after, Result)"""
    g, cur = graph_optimize(name)
    return g.optimize(cur)


@functools.lru_cache(maxsize=None)
def second_pass():
    """after the `converge` pass: a loop 38 -> 12 is added and cur = 38 optimised: (graph before the second pass, graph after, Result)"""
    g1, _ = optimized("converge")
    g = g1.copy()
    truth, _ = trajectory(40, 31, drift_t=5e-3, drift_r=5e-4)
    g.set_loop(38, 12, loop_measurement(truth, 38, 12, (0.01, -0.01, 0.005), (0.001, 0.0005, -0.001)))
    g2, res = g.optimize(38)
    return g, g2, res


# ---- forced invalid steps: no crafted graph makes the solver turn a step down on its own (under Huber(1) this problem's steps are well behaved), so the branch is
# driven by refusing chosen linear solves, on the device (mlh_pg_optimize_forced) and in the restatement (Graph.optimize(fail_mask=...)) alike
FORCED_CASES = {"first_two": (0b00011, 8), "middle": (0b00110, 8), "five_in_a_row": (0b111110, 8), "all": (0xFF, 8)}


@functools.lru_cache(maxsize=None)
def forced(name):
    """the restatement's pass over the `converge` graph with FORCED_CASES[name] = (fail_mask, max_num_iterations): (graph after, Result)"""
    g, cur = graph_optimize("converge")
    mask, max_it = FORCED_CASES[name]
    return g.optimize(cur, fail_mask=mask, max_num_iterations=max_it)
