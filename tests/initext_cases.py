"""Cases and plumbing shared by tests/test_initext_cases.py (CPU) and tests/test_gpu_initext.py (GPU): a NumPy transcription of InitialExtrinsics
(estimator/src/initial/initial_extrinsics.cpp:79-309) with np.linalg.svd in the place of Eigen's JacobiSVD -- LAPACK is the independent reference for the device's
one-sided Jacobi -- and crafted motion sequences built from a KNOWN extrinsic. NumPy only. Computed once per process and shared: do not modify what these functions
return.

Conventions: a pose is [t, q(xyzw)]; quaternions are (x, y, z, w). With the extrinsic X = (q_e, t_e) of a LiDAR and the reference LiDAR's motion (q_a, t_a), the
LiDAR's own motion is q_b = q_e^-1 q_a q_e, t_b = R_e^T ((R_a - I) t_e + t_a): exactly what calibExRotation (q_a = q_e q_b q_e^-1) and calibExTranslationNonPlanar
((R_a - I) x = q_e t_b - t_a) invert.

The first calibration of a run sees ONE block in Q_ (sets accepted before the heap reached WINDOW_SIZE never enter it), whose null space is two-dimensional: that
call's null vector is not unique, and the next block's Huber weight reads it. Every sequence therefore starts with rotation steps of 2 degrees: two such rotations
are at most 4 degrees apart whatever the estimate, below the 5 degrees at which the weight leaves 1, so Q_ does not depend on a non-unique vector. Later steps are
3 degrees; by then the estimate is unique."""
import functools
import heapq

import numpy as np

N_POSE, WINDOW_SIZE = 300, 4
EPS_R, EPS_T = 0.05, 0.1
DECISION_MARGIN = 1e-6           # every decision of the transcription stays this far from its threshold on every case (tests/test_initext_cases.py)
ROT, TRANS = 1, 2
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------- quaternions (x, y, z, w)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qrotm(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qaxis(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(angle / 2) * a, [np.cos(angle / 2)]])


def angle_axis(q):
    """Eigen: AngleAxisd(Quaterniond)"""
    n = np.linalg.norm(q[:3])
    if n != 0.0:
        ang = 2.0 * np.arctan2(n, abs(q[3]))
        if q[3] < 0:
            n = -n
        return ang, q[:3] / n
    return 0.0, np.array([1.0, 0.0, 0.0])


def angular_distance(a, b):
    d = qmul(a, qconj(b))
    return 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def pose_make(q, t):
    """Pose(q, t): q_.normalize()"""
    return np.concatenate([np.asarray(t, np.float64), np.asarray(q, np.float64) / np.linalg.norm(q)])


def screw_distances(pr, pd):
    ar, xr = angle_axis(pr[3:])
    ad, xd = angle_axis(pd[3:])
    return abs(ar - ad), abs(pr[:3] @ xr - pd[:3] @ xd)


def rot_block(pr, pd, ext):
    """huber (L - R) of cpp:128-153 -> (block 4 x 4, the angular distance in degrees)"""
    r1 = pr[3:]
    qe = ext[3:]
    qinv = qconj(qe) / (qe @ qe)
    qinv = qinv / np.linalg.norm(qinv)
    r2 = qmul(qmul(qe, pd[3:]), qinv)
    ad = 180 / np.pi * angular_distance(r1, r2)
    huber = 5.0 / ad if ad > 5.0 else 1.0
    L, R = np.zeros((4, 4)), np.zeros((4, 4))
    w, q = pr[6], pr[3:6]
    L[:3, :3] = w * np.eye(3) + skew(q); L[:3, 3] = q; L[3, :3] = -q; L[3, 3] = w
    w, q = pd[6], pd[3:6]
    R[:3, :3] = w * np.eye(3) - skew(q); R[:3, 3] = q; R[3, :3] = -q; R[3, 3] = w
    return huber * (L - R), ad


def svd_solve(A, b):
    """JacobiSVD::solve with Eigen's default threshold -> (x, singular values, rank, the smallest relative distance of a singular value from the threshold)"""
    if A.shape[0] == 0:
        return np.zeros(A.shape[1]), np.zeros(A.shape[1]), 0, np.inf
    U, S, Vt = np.linalg.svd(A, full_matrices=False)
    thr = min(A.shape) * EPS * S[0]
    keep = S > thr
    x = np.zeros(A.shape[1])
    for j in np.nonzero(keep)[0]:
        x += Vt[j] * ((U[:, j] @ b) / S[j])
    margin = np.inf if S[0] == 0 else float(np.min(np.abs(S - thr)) / S[0])
    return x, S, int(keep.sum()), margin


class RefInitExt:
    """The transcription: the same interface as the device wrapper of tests/test_gpu_initext.py (add_pose / calibrate / info), plus the margins of its decisions"""

    def __init__(self, n_lidar=2, idx_ref=0, planar_movement=0, window_size=WINDOW_SIZE, n_pose=N_POSE, eps_r=EPS_R, eps_t=EPS_T, rot_cov_thre=0.0, qbl=None, tbl=None):
        self.n, self.ref, self.planar, self.window, self.n_pose, self.eps_r, self.eps_t = n_lidar, idx_ref, planar_movement, window_size, n_pose, eps_r, eps_t
        self.thre = rot_cov_thre if rot_cov_thre > 0 else (0.05 if planar_movement else 0.25)
        qbl = np.tile([0.0, 0, 0, 1], (n_lidar, 1)) if qbl is None else np.asarray(qbl, np.float64)
        tbl = np.zeros((n_lidar, 3)) if tbl is None else np.asarray(tbl, np.float64)
        self.calib_ext = np.array([pose_make(qbl[i], tbl[i]) for i in range(n_lidar)])
        self.cov_rot = [i == idx_ref for i in range(n_lidar)]
        self.cov_pos = [i == idx_ref for i in range(n_lidar)]
        self.Q = np.zeros((n_lidar, 4 * N_POSE, 4))
        self.heap = []               # (-w of LiDAR 0, slot): the top is the largest w, as under rotCmp
        self.v_pose = []
        self.add = None              # pose_laser_add_
        self.margins = dict(screw=np.inf, sigma=np.inf, huber_rot=np.inf, huber_trans=np.inf, rank=np.inf, sign=np.inf)
        self.heap_keys = []

    def _margin(self, name, value):
        self.margins[name] = min(self.margins[name], float(value))

    def add_pose(self, poses):
        poses = np.asarray(poses, np.float64).reshape(self.n, 7)
        ok = True
        for i in range(self.n):
            r_dis, t_dis = screw_distances(poses[self.ref], poses[i])
            self._margin("screw", min(abs(r_dis - self.eps_r), abs(t_dis - self.eps_t)))
            ok = ok and (r_dis < self.eps_r) and (t_dis < self.eps_t)
        if ok:
            w0 = poses[0, 6]
            self.heap_keys.append(w0)
            if len(self.heap) < self.n_pose:
                slot = len(self.heap)
                self.v_pose.append(poses.copy())
                heapq.heappush(self.heap, (-w0, slot))
            else:
                slot = self.heap[0][1]
                self.v_pose[slot] = poses.copy()
                heapq.heapreplace(self.heap, (-w0, slot))
            self.add = (slot, poses.copy())
        return ok

    def _rotation(self, l, r):
        if len(self.heap) < self.window or self.add is None:
            return
        slot, poses = self.add
        blk, ad = rot_block(poses[self.ref], poses[l], self.calib_ext[l])
        self._margin("huber_rot", abs(ad - 5.0) / 5.0)
        self.Q[l, 4 * slot:4 * slot + 4] = blk
        _, S, Vt = np.linalg.svd(self.Q[l], full_matrices=False)
        x = Vt[3].copy()
        if x[0] < 0:
            x = -x
        self.calib_ext[l, 3:] = x
        r.update(rot_ran=1, rot_sv=S, slot=slot, rot_converged=int(S[2] > self.thre))
        self._margin("sigma", abs(S[2] - self.thre) / self.thre)
        if r["rot_converged"]:
            self._margin("sign", abs(x[0]))
            self.cov_rot[l] = True

    def _translation(self, l, r):
        q = self.calib_ext[l, 3:].copy()
        N = len(self.v_pose)
        rows, rhs = [], []
        for s in range(N):
            pr, pd = self.v_pose[s][self.ref], self.v_pose[s][l]
            _, t_dis = screw_distances(pr, pd)
            self._margin("huber_trans", abs(t_dis - 0.04) / 0.04)
            huber = 0.04 / t_dis if t_dis > 0.04 else 1.0
            Rr = qrotm(pr[3:])
            if not self.planar:
                rows.append(huber * (Rr - np.eye(3)))
                rhs.append(qrotm(q) @ pd[:3] - pr[:3])
            else:
                J = Rr[:2, :2] - np.eye(2)
                n = qrotm(q)[2]
                p = qrotm(q) @ (pd[:3] - (pd[:3] @ n) * n)
                K = np.array([[p[0], -p[1]], [p[1], p[0]]])
                rows.append(huber * np.hstack([J, K]))
                rhs.append(pr[:2])
        nc = 4 if self.planar else 3
        A = np.vstack(rows) if rows else np.zeros((0, nc))
        b = np.concatenate(rhs) if rhs else np.zeros(0)
        x, S, rank, margin = svd_solve(A, b)
        self._margin("rank", margin)
        if not self.planar:
            self.calib_ext[l] = pose_make(q, x)
        else:
            yaw = np.arctan2(x[3], x[2])
            self.calib_ext[l] = pose_make(qmul(qaxis([0, 0, 1], yaw), q), [-x[0], -x[1], 0.0])
        sv = np.zeros(4)
        sv[:nc] = S
        r.update(trans_solved=1, trans_rank=rank, trans_sv=sv)
        self.cov_pos[l] = True

    def calibrate(self, lidars, stages=ROT | TRANS):
        out = []
        for l in lidars:
            r = dict(lidar=l, rot_ran=0, rot_converged=0, trans_solved=0, trans_rank=0, slot=-1, rot_sv=None, trans_sv=np.zeros(4))
            if stages & ROT:
                self._rotation(l, r)
            if (stages & TRANS) and (not (stages & ROT) or r["rot_converged"]):
                self._translation(l, r)
            r["q"], r["t"] = self.calib_ext[l, 3:].copy(), self.calib_ext[l, :3].copy()
            out.append(r)
        return out

    def info(self):
        return dict(n_sets=len(self.v_pose), heap_size=len(self.heap), last_slot=-1 if self.add is None else self.add[0],
                    cov_rot_mask=sum(int(b) << i for i, b in enumerate(self.cov_rot)), cov_pos_mask=sum(int(b) << i for i, b in enumerate(self.cov_pos)),
                    full_cov_rot=int(all(self.cov_rot)), full_cov_pos=int(all(self.cov_pos)))


# ---------------------------------------------------------------- the drivers: the same calls against the transcription and against the device
def run(api, case):
    """Feeds case["frames"] to `api` the way case["mode"] says and returns one record per frame: dict(accepted, info, results = [calibrate outputs ...]).
    callsite / callsite_staged: estimator.cpp:437-467 -- after an accepted set, every LiDAR without a rotation is calibrated, fused (ROT | TRANS in one call) or
      stage by stage (ROT for all of them, then TRANS for those that converged);
    every: after EVERY frame, accepted or not, ROT for all LiDARs but the reference; on the frames listed in case["trans_at"] also TRANS alone."""
    n, ref = case["opts"]["n_lidar"], case["opts"]["idx_ref"]
    others = [l for l in range(n) if l != ref]
    records = []
    for k, poses in enumerate(case["frames"]):
        acc = bool(api.add_pose(poses))
        results = []
        if case["mode"] in ("callsite", "callsite_staged"):
            todo = [l for l in others if not (api.info()["cov_rot_mask"] >> l) & 1]
            if acc and todo:
                if case["mode"] == "callsite":
                    results.append(api.calibrate(todo, ROT | TRANS))
                else:
                    r = api.calibrate(todo, ROT)
                    results.append(r)
                    conv = [x["lidar"] for x in r if x["rot_converged"]]
                    if conv:
                        results.append(api.calibrate(conv, TRANS))
        else:
            results.append(api.calibrate(others, ROT))
            if k in case.get("trans_at", ()):
                results.append(api.calibrate(others, TRANS))
        records.append(dict(accepted=acc, info=api.info(), results=results))
    return records


# ---------------------------------------------------------------- crafted sequences
def lidar_motion(ext, pa):
    """the motion a LiDAR with extrinsic `ext` sees while the reference LiDAR moves by `pa`"""
    qe, te = ext[3:], ext[:3]
    qb = qmul(qmul(qconj(qe), pa[3:]), qe)
    if qb[3] < 0:
        qb = -qb
    tb = qrotm(qe).T @ ((qrotm(pa[3:]) - np.eye(3)) @ te + pa[:3])
    return np.concatenate([tb, qb])


def make_frames(exts, idx_ref, n_frames, seed, planar=0.0, small=6, pure_translation=False, step_deg=3.0, t_max=0.2):
    """n_frames pose sets (n_lidar, 7): the reference LiDAR turns by `step_deg` (+ up to 0.5, every frame its own angle, so that the heap's keys are distinct; the
    first `small` frames by 2 + up to 0.3) about a random axis -- with planar > 0 about z tilted by up to `planar` radians, planar < 0 exactly about z -- and moves by
    up to t_max (planar: in the xy plane)"""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(n_frames):
        if planar < 0:
            axis = np.array([0.0, 0.0, 1.0])
        elif planar > 0:
            tilt = rng.uniform(-planar, planar, 2)
            axis = np.array([tilt[0], tilt[1], 1.0])
        else:
            axis = rng.normal(size=3)
        ang = np.deg2rad((2.0 + 0.3 * rng.uniform()) if k < small else (step_deg + 0.5 * rng.uniform()))
        t = rng.uniform(-t_max, t_max, 3)
        if planar:
            t[2] = 0.0 if planar < 0 else 0.01 * t[2]
        qa = np.array([0.0, 0, 0, 1]) if pure_translation else qaxis(axis, ang)
        pa = np.concatenate([t, qa])
        # the reference LiDAR's own motion is `pa`; the others see it through their extrinsic RELATIVE to the reference LiDAR
        frames.append(np.array([pa if l == idx_ref else lidar_motion(exts[l], pa) for l in range(len(exts))]))
    return frames


def ext_pose(axis, deg, t):
    return np.concatenate([np.asarray(t, np.float64), qaxis(axis, np.deg2rad(deg))])


EXT_MAIN = ext_pose([0.2, -0.5, 1.0], 40.0, [0.3, -0.2, 0.1])          # sigma_3 passes 0.25 between N = 20 and N = 40 (tests/test_initext_cases.py holds it)
IDENT = ext_pose([0, 0, 1], 0.0, [0, 0, 0])
SWEEP_CHECKPOINTS = (5, 20, 40, 63, 64, 65, 300, 320)                   # accepted sets


def _bad_rotation(frame, l):
    """LiDAR l's angle off by 0.06 rad: rejected by the first half of the screw test"""
    f = frame.copy()
    ang, ax = angle_axis(f[l, 3:])
    f[l, 3:] = qaxis(ax, ang + 0.06)
    return f


def _bad_translation(frame, l):
    """LiDAR l moved by 0.15 m along its own axis: rejected by the second half"""
    f = frame.copy()
    _, ax = angle_axis(f[l, 3:])
    f[l, :3] = f[l, :3] + 0.15 * ax
    return f


def _outlier(frame, l, seed):
    """LiDAR l turns by its own angle about ANOTHER axis (nearly the opposite one) and keeps its screw translation: accepted by the screw test (which compares angles and pitches only), and
    once the estimate is good more than 5 degrees from the reference LiDAR's rotation: the block's Huber weight is active and reads the estimate"""
    f = frame.copy()
    rng = np.random.default_rng(seed)
    ang, ax = angle_axis(f[l, 3:])
    new_ax = -ax + 0.3 * rng.normal(size=3)
    new_ax /= np.linalg.norm(new_ax)
    pitch = f[l, :3] @ ax
    f[l, 3:] = qaxis(new_ax, ang)
    f[l, :3] = pitch * new_ax
    return f


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(opts, frames, mode[, trans_at])"""
    out = {}
    # general motion, every stage after every frame: N = 5 .. 300 accepted sets, then 20 more that replace slots; a frame rejected by each half of the screw test
    # (the rotation stage then runs WITHOUT a new set: early, at frame 6, behind the outlier, and late); an accepted outlier whose weight reads the estimate
    f = make_frames([IDENT, EXT_MAIN], 0, 325, seed=4)
    f[6] = _bad_rotation(f[6], 1)
    f[100] = _bad_translation(f[100], 1)
    f[30] = _outlier(f[30], 1, seed=5)
    f[31] = _bad_rotation(f[31], 1)          # rejected: the rotation stage rewrites the OUTLIER's block, with the weight the new estimate gives it
    f[200] = _bad_rotation(f[200], 1)
    f[310] = _bad_translation(f[310], 1)
    acc_index, n_acc = {}, 0
    for k in range(len(f)):
        if k not in (6, 31, 100, 200, 310):
            n_acc += 1
            acc_index[n_acc] = k
    out["sweep"] = dict(opts=dict(n_lidar=2, idx_ref=0, planar_movement=0), frames=f, mode="every", trans_at=tuple(acc_index[n] for n in SWEEP_CHECKPOINTS))
    # the call site, fused and stage by stage, n_lidar = 2
    f = make_frames([IDENT, EXT_MAIN], 0, 45, seed=9)
    f[10] = _bad_rotation(f[10], 1)
    f[11] = _bad_translation(f[11], 1)
    for mode in ("callsite", "callsite_staged"):
        out[mode + "_2"] = dict(opts=dict(n_lidar=2, idx_ref=0, planar_movement=0), frames=f, mode=mode)
    # n_lidar = 4, idx_ref = 2, steps of 9 degrees; LiDAR 3's sets are outliers on frames 6 .. 19 (down-weighted, its estimate being unique by then), so its
    # rotation converges a dozen frames after the others' -- to whatever those sets make of it; rotCmp still reads LiDAR 0
    exts = [ext_pose([1, 0.3, -0.2], 25.0, [0.5, 0.1, -0.3]), EXT_MAIN, IDENT, ext_pose([-0.4, 1, 0.6], 110.0, [-0.2, 0.4, 0.2])]
    f = make_frames(exts, 2, 40, seed=3, step_deg=9.0)
    for k in range(6, 20):
        f[k] = _outlier(f[k], 3, seed=100 + k)
    out["callsite_4"] = dict(opts=dict(n_lidar=4, idx_ref=2, planar_movement=0), frames=f, mode="callsite")
    # planar motion: exactly about z with planar_movement = 0 (the null space stays two-dimensional: nothing ever converges; 2-degree steps throughout, see above)
    f = make_frames([IDENT, EXT_MAIN], 0, 24, seed=4, planar=-1.0, small=24)
    out["planar_z_0"] = dict(opts=dict(n_lidar=2, idx_ref=0, planar_movement=0), frames=f, mode="every")
    # ... and about a z axis that wobbles by up to 0.25 rad with planar_movement = 1 (threshold 0.05; the planar translation system)
    ext_p = ext_pose([0.1, -0.05, 1.0], 35.0, [0.3, -0.2, 0.0])
    f = make_frames([ext_p, IDENT], 1, 60, seed=6, planar=0.25)
    out["planar_wobble_1"] = dict(opts=dict(n_lidar=2, idx_ref=1, planar_movement=1), frames=f, mode="callsite")
    # pure translation: Q_ stays zero, the result is the identity quaternion
    f = make_frames([IDENT, EXT_MAIN], 0, 8, seed=7, pure_translation=True, t_max=0.02)
    out["pure_translation"] = dict(opts=dict(n_lidar=2, idx_ref=0, planar_movement=0), frames=f, mode="every")
    return out


EXTRINSICS = {"sweep": {1: EXT_MAIN}, "callsite_2": {1: EXT_MAIN}, "callsite_staged_2": {1: EXT_MAIN}}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(records of the transcription, the transcription after the run) for a case -- shared: do not modify"""
    c = cases()[name]
    api = RefInitExt(**c["opts"])
    return run(api, c), api
