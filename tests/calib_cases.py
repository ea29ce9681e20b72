"""Crafted calibration-feature stores and an f64 NumPy restatement of the reference's one-block online-calibration factors, shared by
tests/test_calib_cases.py (CPU) and tests/test_gpu_calib_store.py (GPU).

Restated lines: LidarOnlineCalibPlaneNormFactor::Evaluate (lidar_online_calib_factor.hpp:35-62), LidarOnlineCalibEdgeFactor::Evaluate (:135-165), the Huber
correction Ceres applies to a scalar residual (rho[2] <= 0: the sqrt(rho[1]) branch, as tests/marg_cases.py has it for the window factors), and the way
Estimator::optimizeMap adds them to the window's problem and to its marginalisation on calibration frames (estimator.cpp:714-735, 762-780, 921-938, 960-977).

A calibration factor lives on ONE block, the extrinsic of its LiDAR: its point is a pivot-frame feature of that LiDAR, its coefficients a plane / line of that
LiDAR's calibration map in the pivot frame. tests/marg_cases.py's make_factors with identity pivot and frame makes exactly that (its T is then T_ext)."""
import functools

import numpy as np

import marg_cases as mc

IDENT = np.array([0.0, 0, 0, 0, 0, 0, 1.0])
OUTLIER_FRACTION = 0.05


# ---------------------------------------------------------------- generator
def make_calib(rng, exts_gt, counts, outlier_fraction=OUTLIER_FRACTION):
    """counts[e] factors on extrinsic e, made at exts_gt; about outlier_fraction of the points are then moved 2-3 m off their plane / line, so that both branches of
    HuberLoss(1.0) occur when the factors are evaluated near exts_gt"""
    f = mc.make_factors(rng, IDENT, IDENT[None, :], np.asarray(exts_gt), [list(counts)])
    n = len(f["types"])
    out = dict(types=f["types"], points=f["points"].copy(), coeffs=f["coeffs"], ei=f["ei"])
    if n == 0:
        return out
    for i in rng.choice(n, max(1, int(round(outlier_fraction * n))), replace=False):
        co = f["coeffs"][i]
        if f["types"][i] == 0:
            u = co[:3]
        else:
            v = (co[:3] - co[3:]) / np.linalg.norm(co[:3] - co[3:])
            u = rng.normal(size=3); u -= (u @ v) * v; u /= np.linalg.norm(u)
        d = rng.uniform(2.0, 3.0) * (1.0 if rng.random() < 0.5 else -1.0)
        out["points"][i] += mc.qrot_mat(exts_gt[f["ei"][i]][3:]).T @ (d * u)
    return out


def concat(parts):
    parts = [p for p in parts if p is not None and len(p["types"])]
    if not parts:
        return dict(types=np.zeros(0, np.int32), points=np.zeros((0, 3)), coeffs=np.zeros((0, 6)), ei=np.zeros(0, np.int32))
    return {k: np.concatenate([p[k] for p in parts]) for k in ("types", "points", "coeffs", "ei")}


# ---------------------------------------------------------------- restatement
def calib_eval(cal, exts, sqrt_info=None):
    """residuals (n) and 1 x 7 Jacobian rows (n, 7; 7th column zero), without the loss correction"""
    exts = np.asarray(exts, float).reshape(-1, 7)
    ty, p, co, ei = cal["types"], cal["points"], cal["coeffs"], cal["ei"]
    n = len(ty)
    s = np.ones(n) if sqrt_info is None else np.asarray(sqrt_info, float)
    R = np.stack([mc.qrot_mat(e[3:]) for e in exts])[ei] if n else np.zeros((0, 3, 3))
    t = exts[ei, :3]
    lp = np.einsum("nij,nj->ni", R, p) + t
    r = np.zeros(n); J = np.zeros((n, 7))
    pl = ty == 0
    # plane: r = w . lp + d; [w^T | -w^T R [p]x]   (a^T [v]x = a x v)
    w = co[pl, :3]
    r[pl] = np.einsum("ni,ni->n", w, lp[pl]) + co[pl, 3]
    J[pl, :3] = w
    J[pl, 3:6] = -np.cross(np.einsum("ni,nij->nj", w, R[pl]), p[pl])
    # edge: r = |nu| / |de|; [-eta [de]x | eta [de]x R [p]x], eta = nu.normalized()^T / |de| (the zero vector stays zero)
    ed = ~pl
    la, lb = co[ed, :3], co[ed, 3:]
    nu = np.cross(lp[ed] - la, lp[ed] - lb)
    de = la - lb
    nn, dn = np.linalg.norm(nu, axis=1), np.linalg.norm(de, axis=1)
    r[ed] = nn / dn
    eta = np.where(nn[:, None] > 0, nu / np.where(nn > 0, nn, 1.0)[:, None], nu) / dn[:, None]
    k = np.cross(eta, de)
    J[ed, :3] = -k
    J[ed, 3:6] = np.cross(np.einsum("ni,nij->nj", k, R[ed]), p[ed])
    return s * r, s[:, None] * J


def calib_system(cal, exts, n_frames, huber=mc.HUBER):
    """the store's loss-corrected share of the window's normal equations: A (D x D), b (D), cost, count, and how many factors took the |r| > delta branch"""
    exts = np.asarray(exts, float).reshape(-1, 7)
    D = 6 * (1 + n_frames + len(exts))
    A = np.zeros((D, D)); b = np.zeros(D)
    r, J = calib_eval(cal, exts)
    sq = r * r
    outer = (sq > huber * huber) if huber > 0 else np.zeros(len(r), bool)
    rho0 = np.where(outer, 2.0 * huber * np.sqrt(sq) - huber * huber, sq)
    sc = np.sqrt(np.where(outer, huber / np.where(outer, np.sqrt(sq), 1.0), 1.0))
    Jc, rc = J[:, :6] * sc[:, None], r * sc
    for e in range(len(exts)):
        m = cal["ei"] == e
        if m.any():
            s = slice(6 * (1 + n_frames + e), 6 * (2 + n_frames + e))
            A[s, s] += Jc[m].T @ Jc[m]
            b[s] += Jc[m].T @ rc[m]
    return A, b, 0.5 * float(rho0.sum()), len(r), int(outer.sum())


def window_system(orc, w, cal, pivot, frames, exts, prior=None, ext_rows=None, huber=mc.HUBER):
    """what the solve factorises / the marginalisation assembles with a store in use: marg_cases' system + the store's term (cal None: not in use)"""
    A, b, cost = mc.window_system(orc, w, pivot, frames, exts, prior, ext_rows, huber)
    if cal is not None and len(cal["types"]):
        Ac, bc, cc, _, _ = calib_system(cal, exts, len(frames), huber)
        A += Ac; b += bc; cost += cc
    return A, b, cost


def gn_solve(orc, w, cal, pivot, frames, exts, n_iters, const_blocks, prior=None, ext_rows=None, huber=mc.HUBER):
    """marg_cases.gn_solve with the store's term in every iteration"""
    fr, ex = np.array(frames, float), np.array(exts, float)
    nb = 1 + len(fr) + len(ex)
    free = np.concatenate([np.arange(6 * b, 6 * b + 6) for b in range(nb) if b not in const_blocks])
    for _ in range(n_iters):
        A, b, _ = window_system(orc, w, cal, pivot, fr, ex, prior, ext_rows, huber)
        step = np.zeros(6 * nb)
        step[free] = np.linalg.solve(A[np.ix_(free, free)], -b[free])
        for i in range(len(fr)):
            if 1 + i not in const_blocks:
                fr[i] = mc.pose_plus(fr[i], step[6 * (1 + i):6 * (2 + i)])
        for e in range(len(ex)):
            if 1 + len(fr) + e not in const_blocks:
                ex[e] = mc.pose_plus(ex[e], step[6 * (1 + len(fr) + e):6 * (2 + len(fr) + e)])
    return fr, ex


def marginalize_window(orc, w, cal, pivot, frames, exts, prior=None, ext_rows=None, huber=mc.HUBER):
    """estimator.cpp:871-1063 with the calibration factors of cpp:921-938, 960-977 (they never touch the pivot: Arr only)"""
    n_frames, n_ext = len(frames), len(exts)
    if len(w["types"]) == 0 and (prior is None or 0 not in list(prior["block_ids"])):
        return None
    A, b, _ = window_system(orc, w, cal, pivot, frames, exts, prior, ext_rows, huber)
    out = mc.marginalize(A, b)
    out.update(block_ids=np.array(list(range(n_frames)) + [1 + n_frames + e for e in range(n_ext)], np.int32), x0=np.vstack([frames, exts]).copy(), A=A, b=b)
    return out


# ---------------------------------------------------------------- the windows of the GPU tests
def ref_only(w):
    """a marg_cases window with only its extrinsic-0 factors kept: the reference LiDAR's window factors of the calibration problem"""
    m = w["ei"] == 0
    out = dict(w)
    for k in ("types", "points", "coeffs", "fi", "ei"):
        out[k] = w[k][m]
    return out


# test 2: per window shape, the store's counts per extrinsic for each of three interleaved appends (tile edges 1, 255, 256, 257; an extrinsic with none; the
# second append large enough to outgrow the buffers the first one allocated)
STORE_COUNTS = {
    "1x4": ((0, 1, 0, 255), (0, 2600, 0, 2500), (0, 256, 0, 257)),          # extrinsic 2 has none; totals 2857 / 3012
    "3x2": ((0, 257), (0, 5200), (0, 255)),
}


@functools.lru_cache(maxsize=None)
def store_case(name):
    w = mc.shape_window(name)
    rng = np.random.default_rng(500 + len(name) + w["n_ext"])
    parts = [make_calib(rng, w["exts_gt"], c) for c in STORE_COUNTS[name]]
    # every append arrives in no particular order of extrinsics
    for p in parts:
        perm = rng.permutation(len(p["types"]))
        for k in p:
            p[k] = p[k][perm]
    return dict(window=ref_only(w) if name == "1x4" else w, parts=parts, all=concat(parts))


# test 5 / the CPU check against the reference's optimizeMap: (1 frame, 3 extrinsics), window factors on extrinsic 0 only
@functools.lru_cache(maxsize=None)
def calib_problem(seed=21):
    w = mc.make_window(1, 3, [[60, 0, 0]], seed)
    rng = np.random.default_rng(seed + 1000)
    return dict(window=w, cal=make_calib(rng, w["exts_gt"], (0, 150, 97)))


# ---------------------------------------------------------------- the chain of test 6
CHAIN_SHAPES = ((1, 3), (3, 2))
CHAIN_WINDOWS = 4
CHAIN_CALIB_COUNTS = (0, 150, 97)
CHAIN_SEEDS = {(1, 3): 713, (3, 2): 732}


def chain_uses_store(k):
    """the frame_cnt % N_CUMU_FEATURE == 0 gate of the chain: every 2nd window"""
    return k % 2 == 1


@functools.lru_cache(maxsize=None)
def chain_inputs(n_frames, n_ext):
    """four consecutive windows: window factors of the reference LiDAR (40 per frame, extrinsic 0), the calibration factors every window accumulates for the
    other LiDARs, the new frame's perturbed first estimate; extrinsic PriorFactor rows as marg_cases.chain_inputs has them"""
    rng = np.random.default_rng(CHAIN_SEEDS[(n_frames, n_ext)])
    step = np.concatenate([[0.4, 0.03, 0.01], mc.rotvec_quat(np.deg2rad([0.2, -0.1, 1.2]))])
    traj = [mc.random_pose(rng, 3.0)]
    for _ in range(CHAIN_WINDOWS + n_frames):
        traj.append(mc.pose_compose(traj[-1], step))
    exts_gt = np.stack([IDENT] + [mc.random_pose(rng, 0.5, 20.0) for _ in range(n_ext - 1)])
    counts = np.zeros((n_frames, n_ext), int); counts[:, 0] = 40
    windows = []
    for k in range(CHAIN_WINDOWS):
        f = mc.make_factors(rng, traj[k], np.stack(traj[k + 1:k + 1 + n_frames]), exts_gt, counts, 20.0)
        f["new_frame"] = mc.perturb(traj[k + n_frames], rng)
        f["cal"] = make_calib(rng, exts_gt, CHAIN_CALIB_COUNTS[:n_ext])
        windows.append(f)
    first = dict(pivot=traj[0], frames=np.stack([mc.perturb(p, rng) for p in traj[1:n_frames]] + [windows[0]["new_frame"]]) if n_frames > 1 else windows[0]["new_frame"][None, :],
                 exts=np.stack([exts_gt[0]] + [mc.perturb(p, rng) for p in exts_gt[1:]]))
    ext_rows = np.hstack([exts_gt, np.tile(mc.CHAIN_PRIOR_SCALES, (n_ext, 1))])
    return dict(windows=windows, first=first, ext_rows=ext_rows)


def chain_const_blocks(n_frames, n_ext, k):
    """pivot and extrinsic 0 are constant; on the other windows evalDegenracy freezes every extrinsic (V_update_ = 0, estimator.cpp:1671-1676): held constant"""
    if chain_uses_store(k):
        return (0, 1 + n_frames)
    return (0,) + tuple(1 + n_frames + e for e in range(n_ext))


def chain_run(n_frames, n_ext, accumulate, solve, marg, clear):
    """per window: accumulate(cal); solve(k, w, pivot, frames, exts, use) -> (frames, exts); marg(k, w, pivot, frames, exts, use) -> anything; clear() after a
    window that used the store; slide. Returns per window (pivot, frames, exts, marg's result)."""
    ci = chain_inputs(n_frames, n_ext)
    pivot, frames, exts = ci["first"]["pivot"], ci["first"]["frames"].copy(), ci["first"]["exts"].copy()
    out = []
    for k, w in enumerate(ci["windows"]):
        if k > 0:
            frames = np.vstack([frames[1:], w["new_frame"][None, :]])
        use = chain_uses_store(k)
        accumulate(w["cal"])
        fr, ex = solve(k, w, pivot, frames, exts, use)
        m = marg(k, w, pivot, fr, ex, use)
        if use:
            clear()
        out.append((pivot.copy(), fr.copy(), ex.copy(), m))
        pivot, frames, exts = fr[0].copy(), fr, ex
    return out


@functools.lru_cache(maxsize=None)
def chain_reference(n_frames, n_ext, with_store=True):
    """the NumPy loop (computed once, shared); with_store False: the same chain without the store's term, the other extrinsics free on the same windows"""
    import oracle as orc
    orc.build()
    ci = chain_inputs(n_frames, n_ext)
    state = {"prior": None, "store": []}

    def accumulate(cal):
        state["store"].append(cal)

    def term(use):
        return concat(state["store"]) if (use and with_store) else None

    def solve(k, w, pivot, frames, exts, use):
        return gn_solve(orc, w, term(use), pivot, frames, exts, 5, chain_const_blocks(n_frames, n_ext, k), state["prior"])

    def marg(k, w, pivot, frames, exts, use):
        state["prior"] = marginalize_window(orc, w, term(use), pivot, frames, exts, state["prior"], ci["ext_rows"])
        return state["prior"]

    def clear():
        state["store"] = []

    return chain_run(n_frames, n_ext, accumulate, solve, marg, clear)


def decomposed_spectra():
    """(label, eigenvalues) of every matrix tests/test_gpu_calib_store.py decomposes on both sides"""
    out = []
    for nf, ne in CHAIN_SHAPES:
        for k, (_, _, _, m) in enumerate(chain_reference(nf, ne)):
            out += [(f"chain {nf}x{ne} window {k} Amm", m["eig_mm"]), (f"chain {nf}x{ne} window {k} Schur", m["eig_rr"])]
    return out
