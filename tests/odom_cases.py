"""Crafted odometry windows and their float64 reference, shared by tests/test_odom_cases.py (CPU) and tests/test_gpu_odom_cases.py (GPU): the coupled window solve of
odom.hip -- odom_ne_kernel, odom_ne_finish_kernel, odom_window_solve_kernel behind mlh_pure_odom_set / _normal_eq / _gn_solve.

The cases are parameters, not arrays. box_window makes "box" windows: points on the six walls of a 16 m cube and on its twelve edges, plane coefficients (w, d) and
line point pairs given in the pivot frame, every point moved into its LiDAR's frame by the exact inverse of T_pivot^-1 T_i T_ext plus 1 cm of noise. The pivot is a
random rigid pose within +-5 m of the origin, the frames lie within 0.5 m / 0.05 rad of it, extrinsic 0 is the identity and the others are random up to 0.5 m /
0.5 rad; the linearisation point is off the truth by N(0, 3 cm) per translation component and N(0, 5 mrad) per rotation-vector component, every fourth factor of a
group is an edge factor and the table comes shuffled. Such windows have cond(H_free) of 5e2 .. 3e3 (3.5e4 under the nf = 132 case's prior), first steps of
0.03 .. 0.07 and costs that fall by a factor of 20 to 60 in the first iteration (tests/test_odom_cases.py prints and asserts them).

The reference: window_system takes the per-factor residuals and Jacobians from oracle.pure_odom_eval_batch (pinned to the reference's own lines by
tests/test_oracle_ref_pin.py) and does everything else in NumPy: Ceres' Huber correction (rows scaled by sqrt(rho1), cost rho0 / 2), the scatter of a factor's 18
entries to [pivot | frame f | extrinsic e], and every entry of H, g and the cost summed with math.fsum -- exactly rounded sums of the rounded products, so the
reference has no summation-order error of its own. Beside g it returns each entry's sum of absolute terms (g cancels: its bar is held against that). window_gn
iterates it: numpy.linalg.solve on the free rows, + 1e-6 I on all of them when a free diagonal entry is exactly zero (the kernel's second attempt), Plus through the
package's host function pose_plus(x, d, V). A window prior's term is tests/marg_cases.py's restatement.

Both functions take a `mutant` for tests/test_odom_cases.py's mutation check: the wrong implementations the GPU file's bars have to tell.
Computed once per process and shared: do not modify what the cached functions return."""
import functools
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import marg_cases as mc  # noqa: E402

# the bars tests/test_gpu_odom_cases.py holds the device to (H, cost and poses: the project's window bars of tests/test_gpu_parity.py, applied per block)
H_BAR = G_BAR = COST_BAR = POSE_BAR = 1e-9
# the conditions the pose bar rests on, asserted at every iterate of the reference: a backward-stable Cholesky leaves about cond * eps * |step| per iteration
MAX_COND, MAX_STEP = 1e6, 0.2
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
DBL_MIN = sys.float_info.min


def _oracle():
    import oracle as O
    O.build()
    return O


def _mla():
    return importlib.import_module("m-loam_amd")


# ---------------------------------------------------------------- generator
def _small_pose(rng, dt, drot):
    w = rng.normal(size=3)
    w *= rng.uniform(0, drot) / np.linalg.norm(w)
    return np.concatenate([rng.uniform(-dt, dt, 3), mc.rotvec_quat(w)])


def _perturb(p, rng, dt=0.03, drot=0.005):
    """the linearisation point of a block: N(0, dt) on every translation component, N(0, drot) on every component of the rotation vector"""
    q = mc.qmul(p[3:], mc.rotvec_quat(rng.normal(size=3) * drot))
    return np.concatenate([p[:3] + rng.normal(size=3) * dt, q / np.linalg.norm(q)])


def box_window(n_frames, n_ext, counts, seed, pivot=None, frame0_rel=None, frame0_start=None):
    """counts[i][e] factors for (frame i, extrinsic e), shuffled. pivot: a pose instead of the random one; frame0_rel: frame 0's true pose relative to the pivot
    instead of a random one; frame0_start: frame 0's linearisation point instead of the perturbed truth."""
    rng = np.random.default_rng(seed)
    counts = np.broadcast_to(np.asarray(counts), (n_frames, n_ext))
    q = rng.normal(size=4)
    rand_pivot = np.concatenate([rng.uniform(-5, 5, 3), q / np.linalg.norm(q)])
    pivot = rand_pivot if pivot is None else np.array(pivot, np.float64)
    rel = [_small_pose(rng, 0.5, 0.05) for _ in range(n_frames)]
    if frame0_rel is not None:
        rel[0] = np.array(frame0_rel, np.float64)
    frames_gt = np.stack([mc.pose_compose(pivot, r) for r in rel])
    exts_gt = np.stack([IDENT] + [_small_pose(rng, 0.5, 0.5) for _ in range(n_ext - 1)])
    Tp_inv = np.linalg.inv(mc.pose_mat(pivot))
    types, points, coeffs, fi, ei = [], [], [], [], []
    for i in range(n_frames):
        for e in range(n_ext):
            Ti = np.linalg.inv(Tp_inv @ mc.pose_mat(frames_gt[i]) @ mc.pose_mat(exts_gt[e]))
            for k in range(int(counts[i][e])):
                x = rng.uniform(-8, 8, 3)
                a = int(rng.integers(3))
                if k % 4 != 3:                                          # a wall: x_a = +-8
                    s = 1.0 if rng.integers(2) else -1.0
                    x[a] = 8.0 * s
                    wn = np.zeros(3); wn[a] = -s
                    co = np.array([wn[0], wn[1], wn[2], -float(wn @ x), 0.0, 0.0])
                    ty = 0
                else:                                                   # an edge of the cube along axis a
                    for b in range(3):
                        if b != a:
                            x[b] = 8.0 if rng.integers(2) else -8.0
                    v = np.zeros(3); v[a] = 1.0
                    s = rng.uniform(-0.05, 0.05)
                    co = np.concatenate([x + (s + 0.1) * v, x + (s - 0.1) * v])
                    ty = 1
                p = Ti[:3, :3] @ x + Ti[:3, 3] + rng.normal(size=3) * 0.01
                types.append(ty); points.append(p); coeffs.append(co); fi.append(i); ei.append(e)
    frames = np.stack([_perturb(p, rng) for p in frames_gt])
    exts = np.stack([exts_gt[0]] + [_perturb(p, rng) for p in exts_gt[1:]])
    if frame0_start is not None:
        frames[0] = np.array(frame0_start, np.float64)
    perm = rng.permutation(len(types))
    w = dict(types=np.array(types, np.int32)[perm], points=np.array(points, np.float64).reshape(-1, 3)[perm], coeffs=np.array(coeffs, np.float64).reshape(-1, 6)[perm],
             fi=np.array(fi, np.int32)[perm], ei=np.array(ei, np.int32)[perm])
    w.update(sqrt_info=np.ones(len(perm)), pivot=pivot, frames_gt=frames_gt, exts_gt=exts_gt, frames=frames, exts=exts, n_frames=n_frames, n_ext=n_ext)
    return w


TABLE_KEYS = ("types", "points", "coeffs", "fi", "ei", "sqrt_info")


def reordered(w, order):
    """the same factors in another table order: 'shuffled' (as generated), 'sorted' (by group, stable), 'reversed'"""
    n = len(w["types"])
    idx = {"shuffled": np.arange(n), "sorted": np.lexsort((np.arange(n), w["ei"], w["fi"])), "reversed": np.arange(n)[::-1]}[order]
    out = dict(w)
    for k in TABLE_KEYS:
        out[k] = np.ascontiguousarray(w[k][idx])
    return out


def table(w):
    """the arguments of Context.pure_odom_set"""
    return (w["types"], w["points"], w["coeffs"], w["fi"], w["ei"], w["sqrt_info"])


# ---------------------------------------------------------------- the committed windows
RAGGED_COUNTS = ((1, 255), (256, 257))            # one factor, a tile less one, a whole tile, a tile and one
RAGGED3_COUNTS = ((1, 255), (256, 513))           # ... and two tiles and one: three tiles of one group
HUBER_DELTA = 0.05


@functools.lru_cache(maxsize=None)
def ragged(three_tiles=False):
    return box_window(2, 2, RAGGED3_COUNTS if three_tiles else RAGGED_COUNTS, 3 if three_tiles else 1)


@functools.lru_cache(maxsize=None)
def sparse_ext():
    """factors name extrinsics 0 and 2 only; the pose arrays hold four extrinsics"""
    w = box_window(2, 4, ((40, 0, 40, 0), (40, 0, 40, 0)), 4)
    assert sorted(set(w["ei"].tolist())) == [0, 2]
    return w


@functools.lru_cache(maxsize=None)
def huber():
    """The ragged shape under huber_delta = 0.05, with the pivot and frame 0's linearisation point AT THE IDENTITY and two more factors in group (0, 0): with
    identity transforms the moved point is the table's point bit for bit on both sides, which is what a residual that is EXACTLY zero needs (under a general pose
    the two sides' moved points differ in the last bit, and a point "on" its line then has a cross product of rounding size and direction). Planted rows -> `planted`:
    on_plane, on_line (group (0, 0)), far (a residual of about 1e6 delta), w0 / w_small / w_large (sqrt_info 0, 1e-3, 1e3)."""
    w = box_window(2, 2, ((3, 255), (256, 257)), 3, pivot=IDENT, frame0_rel=np.concatenate([[0.04, -0.03, 0.035], mc.rotvec_quat(np.array([0.006, -0.005, 0.004]))]),
                   frame0_start=IDENT)
    for k in TABLE_KEYS:
        w[k] = w[k].copy()
    g00 = np.flatnonzero((w["fi"] == 0) & (w["ei"] == 0))
    assert len(g00) == 3
    a, b = int(g00[0]), int(g00[1])
    w["types"][a] = 0; w["points"][a] = [1.5, -2.25, 3.0]; w["coeffs"][a] = [0.0, 0.0, 1.0, -3.0, 0.0, 0.0]                 # z = 3
    w["types"][b] = 1; w["points"][b] = [1.0, 2.125, -3.0]; w["coeffs"][b] = [1.0, 2.0, -3.0, 1.0, 2.25, -3.0]              # the line x = 1, z = -3
    planes = [int(i) for i in np.flatnonzero((w["types"] == 0) & (w["fi"] == 1)) if i not in (a, b)]
    far, w0, ws, wl = planes[:4]
    w["coeffs"][far, 3] += 1e6 * HUBER_DELTA
    w["sqrt_info"][w0], w["sqrt_info"][ws], w["sqrt_info"][wl] = 0.0, 1e-3, 1e3
    w["planted"] = dict(on_plane=a, on_line=b, far=far, w0=w0, w_small=ws, w_large=wl)
    return w


@functools.lru_cache(maxsize=None)
def poses(variant):
    """'plain'; 'half_turn': frame 0 is rotated 180 degrees from an identity pivot, its linearisation point has q.w = 0 exactly; 'frame_is_pivot': frame 0's
    linearisation point is the pivot, with the identity extrinsic 0"""
    if variant == "half_turn":
        return box_window(2, 2, 24, 6, pivot=IDENT, frame0_rel=[0.2, -0.1, 0.05, 0, 0, 1.0, 0], frame0_start=[0.22, -0.08, 0.03, 0, 0, 1.0, 0])
    w = box_window(2, 2, 24, 6)
    if variant == "frame_is_pivot":
        w = box_window(2, 2, 24, 6, frame0_rel=np.concatenate([[0.02, -0.01, 0.015], mc.rotvec_quat(np.array([0.002, -0.003, 0.001]))]), frame0_start=w["pivot"])
    return w


def negated(w):
    """every block's quaternion replaced by its negative: the same rotations"""
    out = dict(w)
    for k in ("pivot", "frames", "exts"):
        out[k] = w[k].copy()
        out[k][..., 3:] *= -1.0
    return out


@functools.lru_cache(maxsize=None)
def max_window():
    """10 frames x 11 extrinsics, 24 factors per group: 22 blocks, D = 132, 110 tiles, 2 640 factors"""
    return box_window(10, 11, 24, 4)


def max_window_prior(w):
    """J0 = 10 I, r0 = 0, x0 = the start, on blocks 0 and 1 + n_frames: what makes the window positive definite with nothing held constant"""
    return dict(block_ids=np.array([0, 1 + w["n_frames"]], np.int32), x0=np.stack([w["pivot"], w["exts"][0]]), J0=10.0 * np.eye(12), r0=np.zeros(12))


MASK_CONST = (0, 2, 5)                             # the pivot, frame 1 and extrinsic 1: two constant blocks in the middle of the free set


@functools.lru_cache(maxsize=None)
def masks_and_V():
    w = box_window(3, 3, 24, 7)
    w["V"] = np.random.default_rng(70).uniform(-1, 1, (7, 6, 6))
    return w


@functools.lru_cache(maxsize=None)
def empty_frame():
    return box_window(3, 2, ((24, 24), (0, 0), (24, 24)), 8)


@functools.lru_cache(maxsize=None)
def non_finite():
    w = dict(ragged())
    w["points"] = w["points"].copy()
    w["points"][100, 0] = np.nan
    return w


# ---------------------------------------------------------------- reference
SYSTEM_MUTANTS = ("rows_by_rho1", "outlier_cost_sq", "offsets_swapped", "tile_dropped")
GN_MUTANTS = ("V_transposed", "plus_offset_6b", "no_regularisation")


def huber_rho(sq, delta, mutant=None):
    """ceres::HuberLoss(delta) at the squared residuals (delta <= 0: no loss) -> rho0, rho1, outlier mask"""
    sq = np.asarray(sq, np.float64)
    rho0, rho1 = sq.copy(), np.ones_like(sq)
    out = np.zeros(sq.shape, bool)
    if delta > 0.0:
        out = sq > delta * delta
        rr = np.sqrt(sq[out])
        rho0[out] = 2.0 * delta * rr - delta * delta
        rho1[out] = np.maximum(DBL_MIN, delta / rr)
        if mutant == "outlier_cost_sq":
            rho0[out] = sq[out]
    return rho0, rho1, out


def _fsum_block(A, B):
    """(m, 6), (m, 6) -> (6, 6) exactly rounded sums of the rounded products A[:, a] * B[:, b], and the sums of their absolute values"""
    T = A[:, :, None] * B[:, None, :]
    S = np.array([[math.fsum(T[:, a, b]) for b in range(6)] for a in range(6)])
    return S, np.abs(T).sum(0)


def window_system(w, pivot, frames, exts, huber_delta, mutant=None):
    """-> dict(H (D, D), g (D,), cost, count, H_abs, g_abs, r, outlier): the loss-corrected normal equations of the table over [pivot | frames | extrinsics]"""
    O = _oracle()
    frames, exts = np.asarray(frames, np.float64).reshape(-1, 7), np.asarray(exts, np.float64).reshape(-1, 7)
    n_frames, n_ext = len(frames), len(exts)
    D = 6 * (1 + n_frames + n_ext)
    r, J = O.pure_odom_eval_batch(w["types"], w["points"], w["coeffs"], w["sqrt_info"], w["fi"], w["ei"], pivot, frames, exts)
    keep = np.ones(len(r), bool)
    if mutant == "tile_dropped":                                        # the 257th factor of the largest group: alone in its last tile
        key = w["fi"].astype(np.int64) * n_ext + w["ei"]
        big = np.bincount(key).argmax()
        members = np.flatnonzero(key == big)
        assert len(members) % 256 == 1
        keep[members[-1]] = False
    rho0, rho1, outlier = huber_rho(r * r, huber_delta, mutant)
    sc = rho1 if mutant == "rows_by_rho1" else np.sqrt(rho1)
    v = (J[:, :, :6] * sc[:, None, None])[keep]
    rs = (r * sc)[keep]
    fi, ei = w["fi"][keep].astype(np.int64), w["ei"][keep].astype(np.int64)
    blocks = np.stack([np.zeros(len(fi), np.int64), 1 + fi, 1 + n_frames + ei], 1)
    if mutant == "offsets_swapped":
        blocks = np.stack([np.zeros(len(fi), np.int64), 1 + n_frames + ei, 1 + fi], 1)
    H, Ha, g, ga = np.zeros((D, D)), np.zeros((D, D)), np.zeros(D), np.zeros(D)
    for s1 in range(3):
        for s2 in range(s1, 3):
            pair = blocks[:, s1] * 64 + blocks[:, s2]
            for p in np.unique(pair):
                sel = pair == p
                b1, b2 = int(p) // 64, int(p) % 64
                S, A = _fsum_block(v[sel, s1], v[sel, s2])
                H[6 * b1:6 * b1 + 6, 6 * b2:6 * b2 + 6] = S; Ha[6 * b1:6 * b1 + 6, 6 * b2:6 * b2 + 6] = A
                if b1 != b2:
                    H[6 * b2:6 * b2 + 6, 6 * b1:6 * b1 + 6] = S.T; Ha[6 * b2:6 * b2 + 6, 6 * b1:6 * b1 + 6] = A.T
        for b in np.unique(blocks[:, s1]):
            sel = blocks[:, s1] == b
            T = v[sel, s1] * rs[sel, None]
            g[6 * b:6 * b + 6] = [math.fsum(T[:, a]) for a in range(6)]
            ga[6 * b:6 * b + 6] = np.abs(T).sum(0)
    return dict(H=H, g=g, cost=math.fsum(0.5 * rho0[keep]), count=int(keep.sum()), H_abs=Ha, g_abs=ga, r=r, outlier=outlier)


def window_gn(w, n_iters, huber_delta, const_blocks=None, V=None, prior=None, mutant=None):
    """mlh_pure_odom_gn_solve's iterations -> dict(pivot, frames, exts, status, cost (of the last linearisation), count, iters=[dict(cond, step, cost, regularised)]).
    const_blocks None: the pivot and extrinsic 0. V: (n_blocks, 6, 6) or None. The pivot block moves too when it is free (the entry point does not return it)."""
    mla = _mla()
    pv, fr, ex = np.array(w["pivot"], np.float64), np.array(w["frames"], np.float64), np.array(w["exts"], np.float64)
    n_frames, n_ext = len(fr), len(ex)
    nb = 1 + n_frames + n_ext
    const = (0, 1 + n_frames) if const_blocks is None else tuple(const_blocks)
    free_blocks = [b for b in range(nb) if b not in const]
    free = np.concatenate([np.arange(6 * b, 6 * b + 6) for b in free_blocks])
    status, iters, cost, count = 0, [], None, 0
    for _ in range(n_iters):
        s = window_system(w, pv, fr, ex, huber_delta, mutant if mutant in SYSTEM_MUTANTS else None)
        H, g, cost, count = s["H"].copy(), s["g"].copy(), s["cost"], s["count"]
        if prior is not None:
            p = mc.prior_evaluate(prior, pv, fr, ex)
            H += p["H"]; g += p["g"]; cost += p["cost"]
        Hf, gf = H[np.ix_(free, free)], g[free]
        rec = dict(cond=np.inf, step=0.0, cost=cost, regularised=False)
        iters.append(rec)
        if not (np.isfinite(Hf).all() and np.isfinite(gf).all()):
            status = 2
            continue
        zero = np.diag(Hf) == 0.0
        live = ~zero
        rec["cond"] = float(np.linalg.cond(Hf[np.ix_(live, live)]))    # (an exactly zero block is decoupled: the condition number of the rest)
        if zero.any():
            if mutant == "no_regularisation":
                status = 2
                continue
            Hf = Hf + 1e-6 * np.eye(len(free))
            status = max(status, 1)
            rec["regularised"] = True
        d = np.linalg.solve(Hf, -gf)
        rec["step"] = float(np.abs(d).max())
        dpad = np.concatenate([d, np.zeros(6 * nb)])
        poses = [pv] + list(fr) + list(ex)
        for k, b in enumerate(free_blocks):
            off = 6 * b if mutant == "plus_offset_6b" else 6 * k
            Vb = None if V is None else (V[b].T if mutant == "V_transposed" else V[b])
            poses[b] = mla.pose_plus(poses[b], dpad[off:off + 6], Vb)
        pv, fr, ex = poses[0], np.stack(poses[1:1 + n_frames]), np.stack(poses[1 + n_frames:])
    return dict(pivot=pv, frames=fr, exts=ex, status=status, cost=cost, count=count, iters=iters)


# ---------------------------------------------------------------- the bars
def measure_system(got, ref):
    """got: dict(H, g, cost, count) -> dict of (value, bar) pairs, every value scaled so that it is held to its bar as it stands.
    H per 6 x 6 block against the largest |ref| of that block; a block that is exactly zero in the reference is exactly zero in `got` (bar 0 on its largest
    entry). g per entry against the largest sum of absolute terms among the six entries of its block. cost relative. count equal. H bit-symmetric."""
    D = len(ref["g"])
    nb = D // 6
    h = hz = gv = gz = 0.0
    for a in range(nb):
        sa = slice(6 * a, 6 * a + 6)
        for b in range(nb):
            sb = slice(6 * b, 6 * b + 6)
            sc = float(np.abs(ref["H"][sa, sb]).max())
            err = float(np.abs(got["H"][sa, sb] - ref["H"][sa, sb]).max())
            if sc == 0.0:
                hz = max(hz, float(np.abs(got["H"][sa, sb]).max()))
            else:
                h = max(h, err / sc) if np.isfinite(err) else np.inf
        sc = float(ref["g_abs"][sa].max())
        err = float(np.abs(got["g"][sa] - ref["g"][sa]).max())
        if sc == 0.0:
            gz = max(gz, float(np.abs(got["g"][sa]).max()))
        else:
            gv = max(gv, err / sc) if np.isfinite(err) else np.inf
    dc = abs(got["cost"] - ref["cost"]) / abs(ref["cost"]) if ref["cost"] != 0 else abs(got["cost"])
    return {"H per block": (h, H_BAR), "H zero blocks": (hz, 0.0), "g per block": (gv, G_BAR), "g zero blocks": (gz, 0.0), "cost": (dc, COST_BAR),
            "count difference": (float(abs(int(got["count"]) - int(ref["count"]))), 0.0),
            "H asymmetry": (float(np.abs(got["H"] - got["H"].T).max()), 0.0)}


def measure_poses(got, ref):
    """got, ref: dict(frames, exts) -> {name: (value, bar)}: the largest absolute difference of a pose entry"""
    return {"poses": (max(float(np.abs(got["frames"] - ref["frames"]).max()), float(np.abs(got["exts"] - ref["exts"]).max())), POSE_BAR)}


def within(measured):
    return all(v <= bar for v, bar in measured.values())


# ---------------------------------------------------------------- what the two test files run
# name -> (window, huber_delta): mlh_pure_odom_normal_eq at the linearisation point ("poses negated" is evaluated at negated(window) and held to the window's own reference)
SYSTEMS = {
    "ragged": (ragged, 1.0), "ragged three tiles": (functools.partial(ragged, True), 1.0), "sparse_ext": (sparse_ext, 1.0), "huber": (huber, HUBER_DELTA),
    "huber on ragged": (ragged, HUBER_DELTA),                                          # (the ragged window itself, general poses, without planted rows)
    "poses plain": (functools.partial(poses, "plain"), 1.0), "poses negated": (functools.partial(poses, "plain"), 1.0),
    "poses half_turn": (functools.partial(poses, "half_turn"), 1.0), "poses frame_is_pivot": (functools.partial(poses, "frame_is_pivot"), 1.0),
    "max_window": (max_window, 1.0), "masks_and_V": (masks_and_V, 1.0), "empty_frame": (empty_frame, 1.0),
}
# name -> (window, n_iters, const_blocks (None: the pivot and extrinsic 0), dense V, window prior, expected status): mlh_pure_odom_gn_solve, huber_delta = 1.0
SOLVES = {
    "ragged": (ragged, 4, None, False, False, 0),
    "ragged three tiles": (functools.partial(ragged, True), 3, None, False, False, 0),
    "sparse_ext": (sparse_ext, 3, (0, 3, 4, 6), False, False, 0),                      # the pivot, extrinsic 0 and the two extrinsics without factors
    "poses plain": (functools.partial(poses, "plain"), 3, None, False, False, 0),
    "poses half_turn": (functools.partial(poses, "half_turn"), 3, None, False, False, 0),
    "poses frame_is_pivot": (functools.partial(poses, "frame_is_pivot"), 3, None, False, False, 0),
    "max_window nf 120": (max_window, 3, None, False, False, 0),
    "max_window nf 132 one iteration": (max_window, 1, (), False, True, 0),
    "max_window nf 132": (max_window, 3, (), False, True, 0),
    "masks": (masks_and_V, 3, MASK_CONST, False, False, 0),
    "masks dense V": (masks_and_V, 2, MASK_CONST, True, False, 0),                      # (a random V is no descent direction: two iterations, the cost is not held to fall)
    "empty_frame": (empty_frame, 3, None, False, False, 1),
}


def solve_args(name):
    """-> dict(w, n_iters, const_blocks, V, prior, status)"""
    fn, n_iters, const, dense, with_prior, status = SOLVES[name]
    w = fn()
    return dict(w=w, n_iters=n_iters, const_blocks=const, V=w["V"] if dense else None, prior=max_window_prior(w) if with_prior else None, status=status)


@functools.lru_cache(maxsize=None)
def system_reference(name):
    fn, hd = SYSTEMS[name]
    w = fn()
    return window_system(w, w["pivot"], w["frames"], w["exts"], hd)


@functools.lru_cache(maxsize=None)
def solve_reference(name, mutant=None):
    a = solve_args(name)
    return window_gn(a["w"], a["n_iters"], 1.0, a["const_blocks"], a["V"], a["prior"], mutant)
