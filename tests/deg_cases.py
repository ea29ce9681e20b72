"""Cases and the float64 reference shared by tests/test_deg_cases.py (CPU) and tests/test_gpu_deg_cases.py (GPU): evalDegenracy's verdict and projector at every
rank -- zero to six discarded directions of the 6-dof update -- in every form the solver tail takes on the device (solver_dev.hpp: eval_degeneracy_mem under
gn_finish_wave, eval_degeneracy_reg under gn_finish2<true> and the three LM begins, and the Cholesky shortcut in front of each of them).

Plain module: NumPy and the oracle only, nothing collected, results cached -- do not modify what these functions return.

reference_tail is the REFERENCE: numpy.linalg.eigh, the rule of lidar_mapper_keyframe.cpp:1172-1204 (the leading eigenvalues below the threshold are discarded, the
scan stops at the first one that is not), P = Q_kept Q_kept^T, numpy.linalg.solve and Plus restated. No oracle in it: the oracle's cyclic Jacobi and Cholesky are
what the kernels restate, so they are held to this reference like the kernels (tests/test_deg_cases.py; the constants of the bars are measured there).

A THRESHOLD is a position in the reference's own spectrum, never a literal (the quantile gates of tests/thin_cases.py): between(j) is the geometric mean of
lam[j - 1] and lam[j] of the oracle's H at the case's start pose (between(0) = lam[0] / 2, between(6) = 2 lam[5]); just_below(j) / just_above(j) are
lam[j] -/+ MARGIN_ABS. MARGIN_ABS = 100 x 6 x 1e-8 x max|H| is derived, not tuned: the device's H is held to the oracle's at rtol 1e-8 per entry
(test_gn_solve_parity; its atol of 1e-6 is nothing beside these H), so by Weyl's inequality the two spectra differ by at most |dH|_2 <= 6 x 1e-8 x max|H|; the factor
100 is the margin. For every case and every iteration no eigenvalue of the oracle's H lies within MARGIN_ABS of the threshold -- a condition, asserted on the CPU; a
case that breaks it gets another seed or start pose (`python tests/deg_cases.py search` prints the spectra, margins and bite of candidates), it is not dropped.
The one threshold that is not a position is nothing_matches': six eigenvalues that are exactly 0 leave no gap to stand in, so it takes the option's default, 100.

What cannot be pinned this way: the 1e-9 band itself. The shortcut -- "H - thre (1 + 1e-9) I has a Cholesky factor => nothing is degenerate, V_update = I" -- fails
for lam[0] inside (thre, thre (1 + 1e-9)] although nothing is degenerate, and the Jacobi path then returns the identity all the same. That band is a hundred
times narrower than what is known of the device's H (1e-8 of the oracle's), so no end-to-end case can be placed in it; shortcut_just_clear and
shortcut_just_caught, MARGIN_ABS either side of lam[0], are the closest legal placements, and MARGIN_ABS is not tightened to get nearer. The tracker passes a
negative threshold: no case here, tests/lm_cases.py's tracker cases run that path."""
import collections
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import lm_cases as lm

EPS = 2.0 ** -52
H_RTOL = 1e-8                                   # test_gn_solve_parity's bar on the device's H
MARGIN_FACTOR = 100.0
POSE_BAR_ORACLE = 1e-7                          # the project's bar on a pose against the oracle's
COMM_POSE_BAR = 1e-13                           # test_rccl_single_rank_path's bar between the fused and the communicator path
BITE = 1000.0
DEFAULT_THRE = 100.0                            # mlh_solver_opts_default's map_eig_thre
FAR = 500.0                                     # nothing_matches: the features moved this far along z (test_fps_selection_on_the_device_ties_and_edge_sizes)


def margin_abs(H):
    return MARGIN_FACTOR * 6.0 * H_RTOL * float(np.abs(H).max())


# ---------------------------------------------------------------- the reference
def plus(x, delta):
    """PoseLocalParameterization::Plus with V_update already applied: t + dt, q (x) [dtheta / 2, 1] normalised. x = [t, qx qy qz qw], delta = [dt, dtheta]"""
    x, d = np.asarray(x, np.float64), np.asarray(delta, np.float64)
    qx, qy, qz, qw = x[3:7]
    dx, dy, dz = d[3:6] / 2.0
    p = np.array([qw * dx + qx + qy * dz - qz * dy,
                  qw * dy - qx * dz + qy + qz * dx,
                  qw * dz + qx * dy - qy * dx + qz,
                  qw - qx * dx - qy * dy - qz * dz])
    return np.concatenate([x[:3] + d[:3], p / np.sqrt(p @ p)])


def projector(Q, k, freeze=False):
    if k == 0:
        return np.eye(6)
    if freeze:
        return np.zeros((6, 6))
    return Q[:, k:] @ Q[:, k:].T


def reference_tail(x, H, g, thre, freeze=False):
    """the tail of one Gauss-Newton iteration in float64 NumPy -> dict(lam, Q, k, P, d, pose, cond2, fallback)"""
    H, g = np.asarray(H, np.float64), np.asarray(g, np.float64)
    lam, Q = np.linalg.eigh(H)
    k = 0
    while k < 6 and lam[k] < thre:
        k += 1
    P = projector(Q, k, freeze)
    fallback = False
    try:
        np.linalg.cholesky(H)
        d = np.linalg.solve(H, -g)
    except np.linalg.LinAlgError:
        fallback = True
        d = np.linalg.solve(H + 1e-6 * np.eye(6), -g)
    cond2 = float(lam[-1] / lam[0]) if lam[0] > 0.0 else np.inf
    return dict(lam=lam, Q=Q, k=k, P=P, d=d, pose=plus(x, P @ d), cond2=cond2, fallback=fallback)


def eig_scale(ref):
    """what c_e multiplies: one float64 rounding of the largest eigenvalue"""
    return EPS * float(ref["lam"][-1])


def pose_scale(ref):
    """what c_t multiplies: 2^-52 (cond2 |d|inf + 1). A step that is exactly zero (nothing_matches) is not amplified by any condition number: the scale is 2^-52"""
    dn = float(np.abs(ref["d"]).max())
    return EPS * ((ref["cond2"] * dn if dn > 0.0 else 0.0) + 1.0)


def shortcut_clear(H, thre):
    """the kernels' shortcut, restated: H - thre (1 + 1e-9) I has a Cholesky factor"""
    try:
        np.linalg.cholesky(np.asarray(H, np.float64) - thre * (1.0 + 1e-9) * np.eye(6))
        return True
    except np.linalg.LinAlgError:
        return False


# ---------------------------------------------------------------- threshold placement
def place(spot, lam, H):
    """(threshold, the rank it is there for) of a placement ("between" | "just_below" | "just_above" | "default", j) in the spectrum lam of H"""
    how, j = spot
    if how == "default":
        return DEFAULT_THRE, int(np.sum(lam < DEFAULT_THRE))
    if how == "between":
        thre = lam[0] / 2.0 if j == 0 else (2.0 * lam[5] if j == 6 else float(np.sqrt(lam[j - 1] * lam[j])))
        return float(thre), j
    if how == "just_below":
        return float(lam[j] - margin_abs(H)), j
    assert how == "just_above", how
    return float(lam[j] + margin_abs(H)), j + 1


def clearance(H, thre):
    """(distance of the nearest eigenvalue of H from the threshold, MARGIN_ABS of H)"""
    lam = np.linalg.eigvalsh(np.asarray(H, np.float64))
    return float(np.abs(lam - thre).min()), margin_abs(H)


def margin_holds(H, thre):
    """the margin condition; a placement that IS lam[j] -/+ MARGIN_ABS stands at the distance itself, to the rounding of that difference"""
    dist, m = clearance(H, thre)
    return dist >= m * (1.0 - 1e-12)


# ---------------------------------------------------------------- the cases
# kind: "gn" (gn_solve), "blocks" (gn_solve_blocks, two blocks, block 1 frozen when degenerate), "lm" (scan2map, max_outer 2)
# spot: the threshold's placement; for "blocks" one (block 0, block 1) pair per phase. rank: the number of discarded directions the case is there for.
Case = collections.namedtuple("Case", "name kind family seed start spot iters rank shift")
PLANE = ("plane", 2, (4, 0.1, 1.0))
BOXES = ("boxes", 11, (12, 0.05, 0.3))


def _gn(name, scene, spot, rank, iters=1, shift=0.0):
    return Case(name, "gn", scene[0], scene[1], scene[2], spot, iters, rank, shift)


CASES = tuple(
    [_gn(f"rank_{j}", PLANE, ("between", j), j) for j in range(7)]
    + [_gn(f"rank_{j}_three_iterations", PLANE, ("between", j), j, iters=3) for j in (1, 3, 5)]
    + [_gn(f"boxes_rank_{j}", BOXES, ("between", j), j) for j in range(4)]
    + [_gn("shortcut_just_clear", PLANE, ("just_below", 0), 0), _gn("shortcut_just_caught", PLANE, ("just_above", 0), 1),
       _gn("boxes_just_below_the_foot", BOXES, ("just_below", 2), 2), _gn("boxes_just_above_the_foot", BOXES, ("just_above", 2), 3),
       _gn("nothing_matches", PLANE, ("default", 0), 6, shift=FAR),
       Case("blocks_freeze", "blocks", PLANE[0], PLANE[1], PLANE[2], ((("between", 1), ("between", 0)), (("between", 1), ("between", 2))), 2, ((1, 0), (1, 2)), 0.0)]
    + [Case(f"lm_rank_{j}", "lm", PLANE[0], PLANE[1], PLANE[2], ("between", j), 2, j, 0.0) for j in range(7)])
BY_NAME = {c.name: c for c in CASES}
REQUIRED_NAMES = tuple([f"rank_{j}" for j in range(7)] + [f"rank_{j}_three_iterations" for j in (1, 3, 5)] + [f"boxes_rank_{j}" for j in range(4)]
                       + ["shortcut_just_clear", "shortcut_just_caught", "boxes_just_below_the_foot", "boxes_just_above_the_foot", "nothing_matches", "blocks_freeze"]
                       + [f"lm_rank_{j}" for j in range(7)])
GN_NAMES = tuple(c.name for c in CASES if c.kind == "gn")
LM_NAMES = tuple(c.name for c in CASES if c.kind == "lm")
BLOCK_FREEZE = (0, 1)
BLOCK_K_NEIGH = (5, 5)


@functools.lru_cache(maxsize=None)
def scene_of(case):
    """the case's scene of lm_cases.SCENES; shift: the features moved along z, away from every map point"""
    sc = lm.SCENES[case.family](case.seed)
    if not case.shift:
        return sc
    move = lambda f: np.ascontiguousarray(f + np.array([0.0, 0.0, case.shift, 0.0], np.float32), np.float32)
    return dict(sc, surf=move(sc["surf"]), corner=move(sc["corner"]))


def start_pose(case):
    return lm.start_pose(lm.Case(case.name, case.family, case.seed, case.start, (), ""))


def block_features(case):
    """[(surf, corner) of block 0, ... of block 1]: the scene's features cut in halves"""
    sc = scene_of(case)
    hs, hc = len(sc["surf"]) // 2, len(sc["corner"]) // 2
    return [(np.ascontiguousarray(sc["surf"][:hs]), np.ascontiguousarray(sc["corner"][:hc])),
            (np.ascontiguousarray(sc["surf"][hs:]), np.ascontiguousarray(sc["corner"][hc:]))]


def _gn_run(case, surf, corner, thre, iters, freeze=False):
    """oracle.gn_iterations with the start pose of every iteration added to its record"""
    O = lm._oracle()
    m = lm.maps_of(case.family, case.seed)
    p0 = start_pose(case)
    res = O.gn_iterations(m[0], m[1], surf, corner, p0, O.mapper_params(map_eig_thre=thre, freeze_when_degenerate=freeze), iters)
    x = p0
    for r in res["iters"]:
        r["x"] = x.copy()
        x = r["pose_after"]
    return res


@functools.lru_cache(maxsize=None)
def spectrum(case, block=None):
    """(lam, H): numpy's eigenvalues of the oracle's H at the case's start pose -- what the thresholds are placed in"""
    sc = scene_of(case)
    surf, corner = (sc["surf"], sc["corner"]) if block is None else block_features(case)[block]
    H = _gn_run(case, surf, corner, DEFAULT_THRE, 1)["iters"][0]["H"]
    return np.linalg.eigvalsh(H), H


@functools.lru_cache(maxsize=None)
def threshold(case, block=None, phase=0):
    spot = case.spot if block is None else case.spot[phase][block]
    return place(spot, *spectrum(case, block))[0]


@functools.lru_cache(maxsize=None)
def solved(case):
    """the oracle's run of a "gn" case at the case's threshold -> dict(thre, pose, iters=[dict(x, H, g, pose_after, n_surf, n_corner, is_degenerate)])"""
    assert case.kind == "gn"
    sc = scene_of(case)
    thre = threshold(case)
    return dict(_gn_run(case, sc["surf"], sc["corner"], thre, case.iters), thre=thre)


@functools.lru_cache(maxsize=None)
def solved_blocks(case):
    """the "blocks" case: [phase][block] -> the oracle's run of that block alone on its half of the features, block 1 frozen when degenerate"""
    assert case.kind == "blocks"
    feats = block_features(case)
    out = []
    for phase in range(len(case.spot)):
        runs = []
        for b, (surf, corner) in enumerate(feats):
            thre = threshold(case, b, phase)
            runs.append(dict(_gn_run(case, surf, corner, thre, case.iters, freeze=bool(BLOCK_FREEZE[b])), thre=thre, freeze=bool(BLOCK_FREEZE[b])))
        out.append(runs)
    return out


@functools.lru_cache(maxsize=None)
def solved_lm(case):
    """oracle.scan2map of an "lm" case at the case's threshold (its outer records carry H0, eigval, is_degenerate) -> its result with thre added"""
    assert case.kind == "lm"
    O = lm._oracle()
    sc = scene_of(case)
    m = lm.maps_of(case.family, case.seed)
    thre = threshold(case)
    res = O.scan2map(m[0], m[1], sc["surf"], sc["corner"], start_pose(case), O.mapper_params(map_eig_thre=thre, max_outer=case.iters))
    return dict(res, thre=thre)


def records(case):
    """every (label, H, thre, rank the case is there for, freeze) the case's oracle run takes a verdict on"""
    if case.kind == "gn":
        s = solved(case)
        return [(f"iteration {i}", r["H"], s["thre"], case.rank, False) for i, r in enumerate(s["iters"])]
    if case.kind == "lm":
        s = solved_lm(case)
        return [(f"outer {i}", o["H0"], s["thre"], case.rank, False) for i, o in enumerate(s["outer"])]
    return [(f"phase {p} block {b} iteration {i}", r["H"], run["thre"], case.rank[p][b], run["freeze"])
            for p, runs in enumerate(solved_blocks(case)) for b, run in enumerate(runs) for i, r in enumerate(run["iters"])]


def gn_records(case):
    """every (label, iteration record, thre, freeze) of a "gn" or "blocks" case: the records that carry x, H, g and the oracle's pose_after"""
    if case.kind == "gn":
        s = solved(case)
        return [(f"iteration {i}", r, s["thre"], False) for i, r in enumerate(s["iters"])]
    return [(f"phase {p} block {b} iteration {i}", r, run["thre"], run["freeze"])
            for p, runs in enumerate(solved_blocks(case)) for b, run in enumerate(runs) for i, r in enumerate(run["iters"])]


def bite(x, ref):
    """the smallest |Plus(x, P_k d) - Plus(x, P_k' d)|inf over the neighbouring ranks k' = k -/+ 1 that exist: what a verdict one direction off moves the pose by"""
    out = np.inf
    for k2 in (ref["k"] - 1, ref["k"] + 1):
        if 0 <= k2 <= 6:
            out = min(out, float(np.abs(ref["pose"] - plus(x, projector(ref["Q"], k2) @ ref["d"])).max()))
    return out


# ---------------------------------------------------------------- the search the cases came from
def search(families=("plane", "boxes"), seeds=range(1, 7), starts=((0.1, 1.0), (0.05, 0.3), (0.3, 3.0)), iters=3):
    """one line per (family, seed, start, iteration): the spectrum, MARGIN_ABS, and per rank the smallest clearance of between(j) and the bite in units of 2^-52
    (cond2 |d| + 1) -- what the committed scenes and start poses were picked from"""
    for family in families:
        for seed in seeds:
            for dt, deg in starts:
                probe = Case("search", "gn", family, seed, (seed + 2, dt, deg), ("between", 0), iters, 0, 0.0)
                lam0, H0 = spectrum(probe)
                for j in range(7):
                    c = probe._replace(spot=("between", j), rank=j)
                    worst, bites = np.inf, []
                    for _, r, thre, _f in gn_records(c):
                        dist, m = clearance(r["H"], thre)
                        ref = reference_tail(r["x"], r["H"], r["g"], thre)
                        worst = min(worst, dist / m)
                        bites.append(bite(r["x"], ref) / pose_scale(ref))
                    print(f"{family} {seed} start ({seed + 2}, {dt}, {deg}) between({j}): clearance / MARGIN_ABS {worst:.1f} bite / scale {min(bites):.2e}", flush=True)
                print(f"{family} {seed} start ({seed + 2}, {dt}, {deg}): lam {np.array2string(lam0, precision=1)} MARGIN_ABS {margin_abs(H0):.2f}", flush=True)


if __name__ == "__main__" and sys.argv[1:2] == ["search"]:
    search()
