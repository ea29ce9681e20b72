"""Crafted odometry windows and an f64 NumPy restatement of the reference's window prior, shared by tests/test_marg_cases.py (CPU) and
tests/test_gpu_window_prior.py (GPU).

Restated lines: MarginalizationInfo::marginalize (marginalization_factor.cpp:189-319, with numpy.linalg.eigh where it has SelfAdjointEigenSolver),
MarginalizationFactor::Evaluate (cpp:358-410), PriorFactor::Evaluate (prior_factor.hpp:36-72, LeftQuatMatrix of common/algos/math.hpp:77-87), and the way
Estimator::optimizeMap puts them together (estimator.cpp:658-685, 871-1063). The feature factors come from the oracle (orc.pure_odom_normal_eq), whose Huber
correction is the one ResidualBlockInfo::Evaluate applies to a scalar residual (cpp:50-81: rho[2] <= 0, the sqrt(rho[1]) branch).

Poses are [t, qx qy qz qw]; the window layout is [pivot | frames 0.. | extrinsics 0..], 6 local parameters per block."""
import functools

import numpy as np

EPS = 1e-8          # marginalization_factor.h: eps
HUBER = 1.0         # estimator.cpp:602


# ---------------------------------------------------------------- quaternions / poses
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qinv(q):        # Eigen: conjugate / squaredNorm
    return np.array([-q[0], -q[1], -q[2], q[3]]) / float(q @ q)


def qrot_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_mat(p):
    T = np.eye(4)
    T[:3, :3] = qrot_mat(p[3:] / np.linalg.norm(p[3:]))
    T[:3, 3] = p[:3]
    return T


def rotvec_quat(v):
    a = np.linalg.norm(v)
    if a < 1e-300:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(a / 2) * v / a, [np.cos(a / 2)]])


def pose_compose(a, b):      # T_a T_b
    return np.concatenate([a[:3] + qrot_mat(a[3:]) @ b[:3], qmul(a[3:], b[3:])])


def perturb(p, rng, dt=0.03, drot_deg=0.3):
    d = rng.normal(size=3); d *= dt / np.linalg.norm(d)
    w = rng.normal(size=3); w *= np.deg2rad(drot_deg) / np.linalg.norm(w)
    q = qmul(p[3:], rotvec_quat(w))
    return np.concatenate([p[:3] + d, q / np.linalg.norm(q)])


def pose_plus(x, d):         # PoseLocalParameterization::Plus with V_update = I
    q = qmul(x[3:], np.array([d[3] / 2, d[4] / 2, d[5] / 2, 1.0]))
    return np.concatenate([x[:3] + d[:3], q / np.linalg.norm(q)])


# ---------------------------------------------------------------- generator
def random_pose(rng, extent, max_deg=25.0):
    w = rng.normal(size=3); w *= np.deg2rad(rng.uniform(0, max_deg)) / np.linalg.norm(w)
    return np.concatenate([rng.uniform(-extent, extent, 3), rotvec_quat(w)])


def make_factors(rng, pivot, frames, exts, counts, extent=20.0, single_normal=None):
    """counts[i][e] factors for (frame i, extrinsic e): half planes, half lines in the pivot frame (planes only with single_normal: all of them share that normal),
    a point sampled on each and taken into the LiDAR frame through (T_pivot^-1 T_i T_ext)^-1, 1 cm noise"""
    types, points, coeffs, fi, ei = [], [], [], [], []
    Tp_inv = np.linalg.inv(pose_mat(pivot))
    for i in range(len(frames)):
        for e in range(len(exts)):
            T = Tp_inv @ pose_mat(frames[i]) @ pose_mat(exts[e])
            Ti = np.linalg.inv(T)
            for k in range(int(counts[i][e])):
                x = rng.uniform(-extent, extent, 3)                  # the sampled point, pivot frame
                if single_normal is not None or k % 2 == 0:
                    nrm = np.asarray(single_normal, float) if single_normal is not None else rng.normal(size=3)
                    nrm = nrm / np.linalg.norm(nrm)
                    co = np.array([nrm[0], nrm[1], nrm[2], -float(nrm @ x), 0.0, 0.0])
                    ty = 0
                else:
                    v = rng.normal(size=3); v /= np.linalg.norm(v)
                    s = rng.uniform(-0.05, 0.05)
                    co = np.concatenate([x + (s + 0.1) * v, x + (s - 0.1) * v])
                    ty = 1
                p = Ti[:3, :3] @ x + Ti[:3, 3] + rng.normal(size=3) * 0.01
                types.append(ty); points.append(p); coeffs.append(co); fi.append(i); ei.append(e)
    return dict(types=np.array(types, np.int32), points=np.array(points, np.float64).reshape(-1, 3), coeffs=np.array(coeffs, np.float64).reshape(-1, 6),
                fi=np.array(fi, np.int32), ei=np.array(ei, np.int32))


def make_window(n_frames, n_ext, counts, seed, extent=20.0, single_normal=None):
    """a window: true poses inside +-extent, factors made at them, then the frames and the extrinsics beyond the first perturbed by 3 cm / 0.3 degrees"""
    rng = np.random.default_rng(seed)
    counts = np.broadcast_to(np.asarray(counts), (n_frames, n_ext))
    pivot = random_pose(rng, extent * 0.25)
    frames_gt = np.stack([pose_compose(pivot, np.concatenate([[0.4 * (i + 1), 0.05 * i, 0.01], rotvec_quat(np.deg2rad([0.3, -0.2, 1.0 + i]))])) for i in range(n_frames)])
    exts_gt = np.stack([np.array([0, 0, 0, 0, 0, 0, 1.0])] + [random_pose(rng, 0.5, 20.0) for _ in range(n_ext - 1)])
    w = make_factors(rng, pivot, frames_gt, exts_gt, counts, extent, single_normal)
    w.update(pivot=pivot, frames_gt=frames_gt, exts_gt=exts_gt, frames=np.stack([perturb(p, rng) for p in frames_gt]),
             exts=np.stack([exts_gt[0]] + [perturb(p, rng) for p in exts_gt[1:]]), n_frames=n_frames, n_ext=n_ext)
    return w


# the shapes of tests/test_gpu_window_prior.py: name -> (n_frames, n_ext, counts, seed, extent, single_normal)
_C32 = [[14, 300], [0, 12], [16, 13]]          # one empty (frame, extrinsic) group, one that ends in a partial 256-factor tile
SHAPES = {
    "1x1": (1, 1, 40, 11, 20.0, None),
    "1x4": (1, 4, 30, 12, 20.0, None),
    "3x2": (3, 2, _C32, 13, 20.0, None),
    "rank_deficient": (1, 2, 30, 14, 5.0, (0.2, -0.3, 0.9)),
    "limit": (11, 10, 4, 15, 20.0, None),
}


@functools.lru_cache(maxsize=None)
def shape_window(name):
    nf, ne, counts, seed, extent, normal = SHAPES[name]
    return make_window(nf, ne, counts, seed, extent, normal)


# ---------------------------------------------------------------- restatement
def feature_system(orc, w, pivot, frames, exts, huber=HUBER):
    """the table's loss-corrected normal equations over all blocks: A (D x D), b (D), cost"""
    D = 6 * (1 + len(frames) + len(exts))
    if len(w["types"]) == 0:
        return np.zeros((D, D)), np.zeros(D), 0.0
    ne = orc.pure_odom_normal_eq(w["types"], w["points"], w["coeffs"], None, w["fi"], w["ei"], pivot, frames, exts, huber)
    return ne["H"].copy(), ne["g"].copy(), ne["cost"]


def prior_dx(prior, poses):
    """marginalization_factor.cpp:371-388 (Utility::positify returns its argument, utility.h:198-205: the sign is the `if`'s)"""
    dx = np.zeros(6 * len(prior["block_ids"]))
    for k, b in enumerate(prior["block_ids"]):
        x, x0 = poses[b], prior["x0"][k]
        dq = qmul(qinv(x0[3:]), x[3:])
        dx[6 * k:6 * k + 3] = x[:3] - x0[:3]
        dx[6 * k + 3:6 * k + 6] = 2.0 * dq[:3]
        if not dq[3] >= 0:
            dx[6 * k + 3:6 * k + 6] = 2.0 * -dq[:3]
    return dx


def prior_evaluate(prior, pivot, frames, exts):
    """MarginalizationFactor::Evaluate + its share of the D x D normal equations: residuals, H, g, cost"""
    poses = np.vstack([np.asarray(pivot)[None, :], frames, exts])
    D = 6 * len(poses)
    res = prior["r0"] + prior["J0"] @ prior_dx(prior, poses)
    rows = np.concatenate([np.arange(6 * b, 6 * b + 6) for b in prior["block_ids"]])
    H = np.zeros((D, D)); g = np.zeros(D)
    H[np.ix_(rows, rows)] = prior["J0"].T @ prior["J0"]
    g[rows] = prior["J0"].T @ res
    return dict(residuals=res, H=H, g=g, cost=0.5 * float(res @ res))


def ext_prior_evaluate(row, x):
    """PriorFactor::Evaluate (prior_factor.hpp:36-72): 6 residuals, 6 x 6 Jacobian (the one the reference's comment calls wrong, as written)"""
    t, rot, ps, rs = row[:3], row[3:7], row[7], row[8]
    r = np.concatenate([ps * (x[:3] - t), rs * 2.0 * qmul(qinv(rot), x[3:])[:3]])
    l = qmul(qinv(x[3:]), rot)
    skew = np.array([[0, -l[2], l[1]], [l[2], 0, -l[0]], [-l[1], l[0], 0]])
    J = np.zeros((6, 6))
    J[:3, :3] = ps * np.eye(3)
    J[3:, 3:] = rs * (l[3] * np.eye(3) + skew)
    return r, J


def add_ext_prior(A, b, rows, exts, n_frames):
    cost = 0.0
    for e, row in enumerate(rows):
        r, J = ext_prior_evaluate(row, exts[e])
        s = slice(6 * (1 + n_frames + e), 6 * (2 + n_frames + e))
        A[s, s] += J.T @ J
        b[s] += J.T @ r
        cost += 0.5 * float(r @ r)
    return cost


def marginalize(A, b, m=6, eps=EPS):
    """marginalization_factor.cpp:286-313 on the assembled system, the first m parameters marginalised"""
    Amm = 0.5 * (A[:m, :m] + A[:m, :m].T)
    lm, Vm = np.linalg.eigh(Amm)
    Amm_inv = Vm @ np.diag(np.where(lm > eps, 1.0 / np.where(lm > eps, lm, 1.0), 0.0)) @ Vm.T
    Amr, Arm, Arr = A[:m, m:], A[m:, :m], A[m:, m:]
    S = Arr - Arm @ Amm_inv @ Amr
    bs = b[m:] - Arm @ Amm_inv @ b[:m]
    lr, Vr = np.linalg.eigh(S)
    keep = lr > eps
    Sv = np.where(keep, lr, 0.0)
    Sinv = np.where(keep, 1.0 / np.where(keep, lr, 1.0), 0.0)
    J0 = np.diag(np.sqrt(Sv)) @ Vr.T
    r0 = np.diag(np.sqrt(Sinv)) @ Vr.T @ bs
    return dict(J0=J0, r0=r0, S=S, bs=bs, eig_mm=lm, eig_rr=lr, kept_mm=int((lm > eps).sum()), kept_rr=int(keep.sum()))


def window_system(orc, w, pivot, frames, exts, prior=None, ext_rows=None, huber=HUBER):
    """what mlh_window_marginalize assembles / what the solve factorises: table + prior term + extrinsic prior rows"""
    A, b, cost = feature_system(orc, w, pivot, frames, exts, huber)
    if prior is not None:
        p = prior_evaluate(prior, pivot, frames, exts)
        A += p["H"]; b += p["g"]; cost += p["cost"]
    if ext_rows is not None:
        cost += add_ext_prior(A, b, ext_rows, exts, len(frames))
    return A, b, cost


def marginalize_window(orc, w, pivot, frames, exts, prior=None, ext_rows=None, huber=HUBER):
    """estimator.cpp:871-1063: the new prior (block map slid as addr_shift does) or None when nothing touches the pivot"""
    n_frames, n_ext = len(frames), len(exts)
    if len(w["types"]) == 0 and (prior is None or 0 not in list(prior["block_ids"])):
        return None
    A, b, _ = window_system(orc, w, pivot, frames, exts, prior, ext_rows, huber)
    out = marginalize(A, b)
    out.update(block_ids=np.array(list(range(n_frames)) + [1 + n_frames + e for e in range(n_ext)], np.int32), x0=np.vstack([frames, exts]).copy(), A=A, b=b)
    return out


def gn_solve(orc, w, pivot, frames, exts, n_iters, const_blocks, prior=None, ext_rows=None, huber=HUBER):
    """mlh_pure_odom_gn_solve's iterations with the prior's term (and ext_rows, the online-calibration form) in every one"""
    fr, ex = np.array(frames, float), np.array(exts, float)
    nb = 1 + len(fr) + len(ex)
    free = np.concatenate([np.arange(6 * b, 6 * b + 6) for b in range(nb) if b not in const_blocks])
    for _ in range(n_iters):
        A, b, _ = window_system(orc, w, pivot, fr, ex, prior, ext_rows, huber)
        step = np.zeros(6 * nb)
        step[free] = np.linalg.solve(A[np.ix_(free, free)], -b[free])
        for i in range(len(fr)):
            if 1 + i not in const_blocks:
                fr[i] = pose_plus(fr[i], step[6 * (1 + i):6 * (2 + i)])
        for e in range(len(ex)):
            if 1 + len(fr) + e not in const_blocks:
                ex[e] = pose_plus(ex[e], step[6 * (1 + len(fr) + e):6 * (2 + len(fr) + e)])
    return fr, ex


# ---------------------------------------------------------------- the chain of test 4
CHAIN_SHAPES = ((1, 2), (3, 2))
CHAIN_WINDOWS = 4
CHAIN_PRIOR_SCALES = (5.0, 10.0)       # PRIOR_FACTOR_POS / PRIOR_FACTOR_ROT


@functools.lru_cache(maxsize=None)
def chain_inputs(n_frames, n_ext):
    """four consecutive windows of a trajectory: per window the factors (made at the true poses) and the new frame's perturbed first estimate"""
    rng = np.random.default_rng(100 + 10 * n_frames + n_ext)
    step = np.concatenate([[0.4, 0.03, 0.01], rotvec_quat(np.deg2rad([0.2, -0.1, 1.2]))])
    traj = [random_pose(rng, 3.0)]
    for _ in range(CHAIN_WINDOWS + n_frames):
        traj.append(pose_compose(traj[-1], step))
    exts_gt = np.stack([np.array([0, 0, 0, 0, 0, 0, 1.0])] + [random_pose(rng, 0.5, 20.0) for _ in range(n_ext - 1)])
    windows = []
    for k in range(CHAIN_WINDOWS):
        f = make_factors(rng, traj[k], np.stack(traj[k + 1:k + 1 + n_frames]), exts_gt, np.full((n_frames, n_ext), 40), 20.0)
        f["new_frame"] = perturb(traj[k + n_frames], rng)
        windows.append(f)
    first = dict(pivot=traj[0], frames=np.stack([perturb(p, rng) for p in traj[1:n_frames]] + [windows[0]["new_frame"]]) if n_frames > 1 else windows[0]["new_frame"][None, :],
                 exts=np.stack([exts_gt[0]] + [perturb(p, rng) for p in exts_gt[1:]]))
    ext_rows = np.hstack([exts_gt, np.tile(CHAIN_PRIOR_SCALES, (n_ext, 1))])
    return dict(windows=windows, first=first, ext_rows=ext_rows)


def chain_run(n_frames, n_ext, solve, marg):
    """the loop of test 4: solve(w, pivot, frames, exts) -> (frames, exts); marg(w, pivot, frames, exts) -> anything. Per window: 5 iterations with the pivot and
    extrinsic 0 constant, marginalise, slide (frame 0 becomes the pivot), append the new perturbed frame. Returns per window (pivot, frames, exts, marg's result)."""
    ci = chain_inputs(n_frames, n_ext)
    pivot, frames, exts = ci["first"]["pivot"], ci["first"]["frames"].copy(), ci["first"]["exts"].copy()
    out = []
    for k, w in enumerate(ci["windows"]):
        if k > 0:
            frames = np.vstack([frames[1:], w["new_frame"][None, :]])
        fr, ex = solve(w, pivot, frames, exts)
        m = marg(w, pivot, fr, ex)
        out.append((pivot.copy(), fr.copy(), ex.copy(), m))
        pivot, frames, exts = fr[0].copy(), fr, ex
    return out


@functools.lru_cache(maxsize=None)
def chain_reference(n_frames, n_ext):
    """the NumPy loop (computed once, shared)"""
    import oracle as orc
    orc.build()
    ci = chain_inputs(n_frames, n_ext)
    state = {"prior": None}
    const = (0, 1 + n_frames)

    def solve(w, pivot, frames, exts):
        return gn_solve(orc, w, pivot, frames, exts, 5, const, state["prior"])

    def marg(w, pivot, frames, exts):
        state["prior"] = marginalize_window(orc, w, pivot, frames, exts, state["prior"], ci["ext_rows"])
        return state["prior"]

    return chain_run(n_frames, n_ext, solve, marg)


def decomposed_spectra(orc):
    """(label, eigenvalues) of every matrix the GPU tests have decomposed on both sides: condition (c) of tests/test_marg_cases.py"""
    out = []
    for name in SHAPES:
        w = shape_window(name)
        m = marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
        out += [(name + " Amm", m["eig_mm"]), (name + " Schur", m["eig_rr"])]
    for nf, ne in CHAIN_SHAPES:
        for k, (_, _, _, m) in enumerate(chain_reference(nf, ne)):
            out += [(f"chain {nf}x{ne} window {k} Amm", m["eig_mm"]), (f"chain {nf}x{ne} window {k} Schur", m["eig_rr"])]
    return out
