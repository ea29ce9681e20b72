"""Cases and plumbing shared by tests/test_lm_cases.py (CPU) and tests/test_gpu_lm_cases.py (GPU): the six-parameter Levenberg-Marquardt loop on starts where it
rejects steps and leaves through its rare exits.

lm_trace is a float64 NumPy restatement of the trust-region iteration (the header of oracle/lm.hpp lists the constants): Jacobi scaling from
the first evaluation, the clamped diagonal and its reuse behind a rejected step, the model cost change, the gradient / parameter / function tolerances in Ceres'
order, the acceptance test rd > 1e-3, the radius update and "five invalid steps in a row". It is the SECOND restatement -- oracle/lm.hpp, in C++, under
oracle.scan2map / oracle.track_cloud is the first -- and it keeps what the first does not report: every iteration's radius, reuse flag, decrease factor and decision
quantities with their distance from the thresholds. The residual blocks, the correspondences, Plus and evalDegenracy stay the oracle's (oracle.linearize,
Map.match, pose_plus, eval_degeneracy): the loop is what is restated here.

The cases are parameters, not arrays: a scene seed, the size of the start error, the options, and the branch the case is there for. They were found by searching
seeds on the CPU with the trace (`python tests/lm_cases.py search`, `... search tracker`, `... search loopreg`); every committed case reaches its branch with every decision quantity of every
iteration at least DECISION_MARGIN (relative) away from its threshold, which tests/test_lm_cases.py asserts. Nothing is larger than conftest's case16 (16 rings,
one LiDAR, the "50k" map). Computed once per process and shared: do not modify what these functions return."""
import collections
import functools
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DECISION_MARGIN = 1e-6           # the convention of tests/pg_cases.py
TRACE = 0.0075                   # cov_measurement_trace of the mapper's blocks without with_ua
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32
FUNCTION_TOL, GRADIENT_TOL, PARAMETER_TOL = 1e-6, 1e-10, 1e-8
MAX_RADIUS, MIN_RADIUS, INITIAL_RADIUS = 1e16, 1e-32, 1e4
NO_CONVERGENCE, GRADIENT, PARAMETER, FUNCTION, FAILURE = 0, 1, 2, 3, 4


def _rel(q, thr):
    return abs(q - thr) / abs(thr)


# ---------------------------------------------------------------- the trace
def lm_trace(evaluate, plus, x0, max_it, min_relative_decrease=1e-3, reuse_diagonal_after_rejection=True):
    """One ceres::Solve on one 6-dof block. evaluate(x) -> dict(H (6, 6), g (6,), cost) of the loss-corrected normal equations; plus(x, delta) -> x (+) delta.
    -> dict(x, iters, summary, margin): iters holds one record per iteration (its fields are the quantities the iteration DECIDED on; a quantity it did not reach is
    None), summary = dict(lm_iterations, successful_steps, evaluations, initial_cost, final_cost, termination), margin = the smallest relative distance of a decision
    quantity from its threshold over the run. The two keyword arguments exist for the mutation test only."""
    x = np.array(x0, np.float64)
    ne = evaluate(x)
    summ = dict(lm_iterations=0, successful_steps=0, evaluations=1, initial_cost=ne["cost"], final_cost=ne["cost"], termination=NO_CONVERGENCE)
    S = 1.0 / (1.0 + np.sqrt(np.diag(ne["H"])))
    radius, decrease_factor, reuse, invalid = INITIAL_RADIUS, 2.0, False, 0
    diag = np.zeros(6)
    gmax_of = lambda e: float(np.abs(x - plus(x, -e["g"])).max())
    gmax = gmax_of(ne)
    iters, margin = [], [np.inf]
    note = lambda v: margin.__setitem__(0, min(margin[0], v))
    it = 0
    while True:
        if it >= max_it:
            summ["termination"] = NO_CONVERGENCE
            break
        note(_rel(gmax, GRADIENT_TOL))
        if gmax <= GRADIENT_TOL:
            summ["termination"] = GRADIENT
            break
        if radius <= MIN_RADIUS:
            summ["termination"] = FAILURE
            break
        it += 1
        summ["lm_iterations"] = it
        rec = dict(radius=radius, reuse_diagonal=reuse, decrease_factor=decrease_factor, gmax=gmax, model_cost_change=None, rd=None, fn_ratio=None, par_ratio=None,
                   valid=False, accepted=False, cost=ne["cost"], candidate_cost=None, candidate=None, candidate_H=None)
        iters.append(rec)
        gs = S * ne["g"]
        A = S[:, None] * ne["H"] * S[None, :]
        if not reuse:
            diag = np.minimum(np.maximum(np.diag(A), MIN_LM_DIAGONAL), MAX_LM_DIAGONAL)
        elif not reuse_diagonal_after_rejection:
            diag = np.minimum(np.maximum(np.diag(A) * 4.0, MIN_LM_DIAGONAL), MAX_LM_DIAGONAL)      # (mutation: a diagonal that is NOT the kept one)
        lhs = A + np.diag(diag / radius)
        reuse = True
        ok = True
        try:
            L = np.linalg.cholesky(lhs)
            y = np.linalg.solve(L.T, np.linalg.solve(L, gs))
            ok = bool(np.isfinite(y).all())
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            step = -y
            sg, sAs = float(step @ gs), float(step @ (A @ step))
            mcc = -(sg + 0.5 * sAs)
            rec["model_cost_change"] = mcc
            note(abs(mcc) / max(abs(sg) + 0.5 * abs(sAs), 1e-300))
            rec["valid"] = mcc > 0.0
        if not rec["valid"]:
            invalid += 1
            if invalid >= 5:
                summ["termination"] = FAILURE
                break
            radius /= decrease_factor
            decrease_factor *= 2.0
            continue
        invalid = 0
        cand = plus(x, step * S)
        ce = evaluate(cand)
        summ["evaluations"] += 1
        rec["candidate_cost"], rec["candidate"], rec["candidate_H"] = ce["cost"], cand, ce["H"]
        step_norm, x_norm = float(np.linalg.norm(x - cand)), float(np.linalg.norm(x))
        pthr = PARAMETER_TOL * (x_norm + PARAMETER_TOL)
        rec["par_ratio"] = step_norm / pthr
        note(_rel(step_norm, pthr))
        if step_norm <= pthr:
            summ["termination"] = PARAMETER
            break
        change = ne["cost"] - ce["cost"]
        fthr = FUNCTION_TOL * ne["cost"]
        rec["fn_ratio"] = abs(change) / ne["cost"] if ne["cost"] > 0 else np.inf
        note(_rel(abs(change), fthr) if fthr > 0 else np.inf)
        if abs(change) <= fthr:
            summ["termination"] = FUNCTION
            break
        rd = change / mcc
        rec["rd"] = rd
        note(_rel(rd, 1e-3))                                            # (the margin is against the REAL threshold whatever the mutation decides with)
        if rd > min_relative_decrease:
            x, ne = cand, ce
            summ["successful_steps"] += 1
            summ["final_cost"] = ne["cost"]
            rec["accepted"] = True
            rec["radius_growth"] = 1.0 / max(1.0 / 3.0, 1.0 - (2.0 * rd - 1.0) ** 3)
            radius = min(MAX_RADIUS, radius * rec["radius_growth"])
            decrease_factor, reuse = 2.0, False
            gmax = gmax_of(ne)
        else:
            radius /= decrease_factor
            decrease_factor *= 2.0
    return dict(x=x, iters=iters, summary=summ, margin=margin[0], last=ne)


def flags(tr):
    """the accept / reject sequence of a trace: 'A' accepted, 'R' rejected (or invalid), 'T' the iteration the loop terminated in"""
    out = ""
    for i, r in enumerate(tr["iters"]):
        last = i == len(tr["iters"]) - 1 and tr["summary"]["termination"] in (PARAMETER, FUNCTION, FAILURE)
        out += "A" if r["accepted"] else ("T" if last else "R")
    return out


# ---------------------------------------------------------------- the mapper's problem under the trace
def _oracle():
    import oracle as O
    O.build()
    return O


def _synth():
    return importlib.import_module("m-loam_amd.synth")


def scan2map_trace(maps, surf, corner, p0, max_outer=2, max_lm_iterations=30, huber_delta=0.1, map_eig_thre=100.0, **mut):
    """scan2MapOptimization with lm_trace as its ceres::Solve: per outer iteration the correspondences are matched once at the start pose (both kinds, 5-NN),
    evalDegenracy of the Hessian there gives V_update, and the trace runs on the fixed correspondences. maps = (oracle.Map surf, oracle.Map corner).
    -> dict(pose, outer=[dict(trace, n_surf, n_corner, is_degenerate, pose_after, V_update)])"""
    O = _oracle()
    x = np.array(p0, np.float64)
    ts, tc = np.full(len(surf), TRACE), np.full(len(corner), TRACE)
    outer = []
    for _ in range(max_outer):
        vs, cs = maps[0].match("s", surf, x)
        vc, cc = maps[1].match("c", corner, x)

        def evaluate(at):
            a = O.linearize("s", surf, ts, at, vs, cs, huber_delta=huber_delta)
            b = O.linearize("c", corner, tc, at, vc, cc, huber_delta=huber_delta)
            return dict(H=a["H"] + b["H"], g=a["g"] + b["g"], cost=a["cost"] + b["cost"], count=a["count"] + b["count"])
        H0 = evaluate(x)["H"] if int(vs.sum()) + int(vc.sum()) else np.zeros((6, 6))
        deg = O.eval_degeneracy(H0, map_eig_thre)
        V = deg["V_update"]
        tr = lm_trace(evaluate, lambda at, d: O.pose_plus(at, d, V), x, max_lm_iterations, **mut)
        x = tr["x"]
        outer.append(dict(trace=tr, n_surf=int(vs.sum()), n_corner=int(vc.sum()), is_degenerate=deg["is_degenerate"], pose_after=x.copy(), V_update=V,
                          valid=(vs, vc), coeffs=(cs, cc)))
    return dict(pose=x, outer=outer)


def _track_rows(O, kind, pts, coeffs, valid, at):
    rows = 1 if kind == "S" else 3
    idx = np.flatnonzero(valid)
    r, J = np.zeros((len(idx), rows)), np.zeros((len(idx), rows, 6))
    for k, i in enumerate(idx):
        ri, Ji = O.scan_factor_eval(kind, pts[i, :3].astype(np.float64), coeffs[i], at, 1.0)
        r[k], J[k] = ri, Ji[:, :6]
    return r, J


def track_trace(tc, pose_ini, max_outer=2, max_lm_iterations=4, huber_delta=0.1, distance_sq_threshold=25.0, **mut):
    """LidarTracker::trackCloud with lm_trace as its ceres::Solve (identity V_update; a round with fewer than 10 correspondences is not solved). tc: conftest's
    track case. The rows are the oracle's scan factors; the Huber correction (rho' scales the block's rows and residuals, cost 0.5 rho) is restated here."""
    O = _oracle()
    x = np.array(pose_ini, np.float64)
    outer = []
    for _ in range(max_outer):
        gate = O.track_params(distance_sq_threshold=distance_sq_threshold)
        vc, cc = O.track_match("c", tc["corner_last"], tc["corner_sharp"], x, gate)
        vs, cs = O.track_match("s", tc["surf_last"], tc["surf_flat"], x, gate)
        n = int(vc.sum()) + int(vs.sum())

        def evaluate(at):
            H, g, cost = np.zeros((6, 6)), np.zeros(6), 0.0
            for kind, pts, co, v in (("S", tc["surf_flat"], cs, vs), ("E", tc["corner_sharp"], cc, vc)):
                r, J = _track_rows(O, kind, pts, co, v, at)
                for rb, Jb in zip(r, J):
                    rho = O.huber(huber_delta, float(rb @ rb))
                    s = np.sqrt(rho[1])
                    cost += 0.5 * rho[0]
                    Jb = Jb * s
                    H += Jb.T @ Jb
                    g += Jb.T @ (rb * s)
            return dict(H=H, g=g, cost=cost, count=n)
        rec = dict(n_corner=int(vc.sum()), n_surf=int(vs.sum()), solved=n >= 10, trace=None)
        if rec["solved"]:
            rec["trace"] = lm_trace(evaluate, lambda at, d: O.pose_plus(at, d), x, max_lm_iterations, **mut)
            x = rec["trace"]["x"]
        rec["pose_after"] = x.copy()
        outer.append(rec)
    return dict(pose=x, outer=outer)


# ---------------------------------------------------------------- scenes (one per seed, cached)
@functools.lru_cache(maxsize=None)
def scene16(seed):
    """conftest's case16 construction for another seed: the "50k" map, one 16-ring scan, the oracle's extraction -> dict(surf_map, corner_map, surf, corner, gt)"""
    import conftest
    O, synth = _oracle(), _synth()
    case = conftest._make_case(synth, "50k", 16, 1, seed=seed)
    surf, corner = conftest.features_from_extraction(synth, case["scans"], lambda s: O.extract(s.points, s.scan_start, s.scan_end))
    return dict(surf_map=case["surf_map"], corner_map=case["corner_map"], surf=surf, corner=corner, gt=case["gt"])


@functools.lru_cache(maxsize=None)
def plane_scene(seed):
    """the degenerate scene of tests/test_gpu_pose_cov.py: a map that is ONE plane and one short vertical line -- evalDegenracy flags it, V_update is a projector"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(-12, 12, 0.4), np.arange(-12, 12, 0.4)), -1).reshape(-1, 2)
    plane = np.concatenate([g + rng.uniform(-0.05, 0.05, g.shape), rng.normal(0, 0.005, (len(g), 1))], 1).astype(np.float32)
    line = np.stack([np.full(200, 3.0), np.full(200, 2.0), np.linspace(0, 4, 200)], 1).astype(np.float32) + rng.normal(0, 0.003, (200, 3)).astype(np.float32)
    surf = np.concatenate([rng.uniform(-8, 8, (3000, 2)), np.zeros((3000, 2))], 1).astype(np.float32)
    corner = np.concatenate([line[::4] + np.float32(0.01), np.zeros((50, 1), np.float32)], 1)
    return dict(surf_map=plane, corner_map=line, surf=surf, corner=corner, gt=np.array([0, 0, 0, 0, 0, 0, 1.0]))


@functools.lru_cache(maxsize=None)
def zero_scene(_seed=0):
    """exact zero residuals at the identity, from f32-representable points on axis planes and axis lines (the constructions of tests/fit_cases.py: p_identical,
    l_feature_on_line). Surf map: stacks of five IDENTICAL points (a keyframe cloud merged five times) on the planes z = -2, x = 4 and y = -4, the in-plane
    coordinates smaller than the offset: the rank-1 fit puts everything on the pivot column and returns n = the axis exactly and d = the offset ONE f32 ULP OUTWARDS
    (2.00000024, 4.00000048: what the QR's Householder arithmetic leaves of 1 / (1 / 2); the oracle and the kernel agree on it bit for bit, test_gpu_fit_cases.py).
    The surf features stand on THAT plane, z = nextafter(-2, -inf) and so on, so n . p + d is 0.0 exactly. Corner map: three lines parallel to the axes on 1/8 m
    steps; the centroid and the direction of five collinear neighbours are exact in the two constant coordinates, and the features lie on the lines. Every residual
    is 0.0 and so is the gradient: the loop ends in its begin on the gradient tolerance, with all its blocks."""
    u = np.arange(-3, 4) / 2.0
    a, b = (w.ravel() for w in np.meshgrid(u, u, indexing="ij"))
    node = lambda x, y, z: np.stack([np.broadcast_to(np.asarray(v, np.float64), a.shape) for v in (x, y, z)], 1)
    nodes = np.concatenate([node(a, b, -2.0), node(4.0, 2 * a, 2 * b), node(2 * a, -4.0, 2 * b)])
    surf_map = np.repeat(nodes, 5, axis=0)
    off = 1.0 / 16
    out = lambda c: float(np.nextafter(np.float32(c), np.float32(np.inf if c > 0 else -np.inf)))
    surf = np.concatenate([node(a + off, b - off, out(-2.0)), node(out(4.0), 2 * a + off, 2 * b + off), node(2 * a - off, out(-4.0), 2 * b + off)])
    t = np.arange(-16, 17) / 8.0
    k = lambda v: np.full(len(t), v)
    lines = np.concatenate([np.stack([t + 1.0, k(3.0), k(1.0)], 1), np.stack([k(-3.0), t, k(2.0)], 1), np.stack([k(2.0), k(-3.0), t + 1.0], 1)])
    tq = np.arange(-12, 12) / 8.0 + 1.0 / 16
    k = lambda v: np.full(len(tq), v)
    corner = np.concatenate([np.stack([tq + 1.0, k(3.0), k(1.0)], 1), np.stack([k(-3.0), tq, k(2.0)], 1), np.stack([k(2.0), k(-3.0), tq + 1.0], 1)])
    f4 = lambda p: np.ascontiguousarray(np.concatenate([p, np.zeros((len(p), 1))], 1), np.float32)
    return dict(surf_map=np.ascontiguousarray(surf_map, np.float32), corner_map=np.ascontiguousarray(lines, np.float32), surf=f4(surf), corner=f4(corner),
                gt=np.array([0, 0, 0, 0, 0, 0, 1.0]))


SCENES = dict(boxes=scene16, plane=plane_scene, zero=zero_scene)

# name, the scene family and seed, the start error (seed, metres, degrees; None = the scene's own pose), solver options, and the branch the case is there for
Case = collections.namedtuple("Case", "name family seed start opts branch")


def start_pose(case):
    sc = SCENES[case.family](case.seed)
    if case.start is None:
        return sc["gt"].copy()
    s, dt, deg = case.start
    return _synth().perturbed_pose(sc["gt"], seed=s, dt=dt, drot_deg=deg)


@functools.lru_cache(maxsize=None)
def maps_of(family, seed):
    O = _oracle()
    sc = SCENES[family](seed)
    return O.Map(sc["surf_map"]), O.Map(sc["corner_map"])


@functools.lru_cache(maxsize=None)
def traced(case, **mut):
    """the trace of a mapper case (cached; the mutated traces of the bar-bites test are cached separately)"""
    sc = SCENES[case.family](case.seed)
    o = dict(case.opts)
    return scan2map_trace(maps_of(case.family, case.seed), sc["surf"], sc["corner"], start_pose(case), max_outer=o.get("max_outer", 2),
                          max_lm_iterations=o.get("max_lm_iterations", 30), huber_delta=o.get("huber_delta", 0.1), **mut)


@functools.lru_cache(maxsize=None)
def oracle_solved(case, **gf):
    """oracle.scan2map on a mapper case; gf: a good-feature selection (gf_method, gf_ratio, seed) in front of every outer iteration"""
    O = _oracle()
    sc = SCENES[case.family](case.seed)
    o = dict(case.opts)
    prm = O.mapper_params(huber_delta=o.get("huber_delta", 0.1), max_outer=o.get("max_outer", 2), max_lm_iterations=o.get("max_lm_iterations", 30), **gf)
    m = maps_of(case.family, case.seed)
    return O.scan2map(m[0], m[1], sc["surf"], sc["corner"], start_pose(case), prm)


# ---------------------------------------------------------------- the committed cases
# Sequences below: one letter per LM iteration of an outer iteration -- A accepted, R rejected, T the iteration the loop terminated in (flags()).
# A start error of 1.5 m / 6 degrees matches about half the features, and evalDegenracy flags most of the outer iterations that begin there: V_update is a
# projector in them. That projection is what makes the loop reject -- the model's decrease lies partly along the direction Plus removes. Over search()'s 360 outer
# iterations 305 of the 342 flagged ones reject at least one step and none of the 18 unflagged ones does (they accept every step at the growth cap instead: case r).
_S = (1.5, 6.0)
CASES = (
    Case("a_single_rejection", "boxes", 11, (12,) + _S, (), "one rejected step between two accepted ones: decrease_factor back to 2, the diagonal recomputed"),
    Case("b_rejections_in_a_row", "plane", 1, (3, 0.3, 3.0), (), "four rejections in a row from the first iteration, then an acceptance: factors 2 4 8 16, the diagonal reused"),
    Case("c_first_iteration_rejected", "plane", 3, (6, 0.3, 3.0), (), "the first LM iteration of outer iteration 1 is rejected: the next proposal is rebuilt from the begin's record"),
    Case("d_budget_ends_on_a_rejection", "boxes", 11, (12,) + _S, (("max_lm_iterations", 13),), "both outer iterations spend their last iteration on a rejected step: termination 0, the last accepted pose"),
    Case("e_termination_after_rejections", "boxes", 10, (11,) + _S, (), "termination 3 at a candidate that follows seven rejections"),
    Case("f_degenerate_with_rejections", "plane", 2, (4, 0.8, 8.0), (), "one plane and one line, V_update a projector, rejections in both outer iterations"),
    Case("g_zero_gradient", "zero", 0, None, (), "exact zero residuals on 219 blocks: termination 1 in the begin, no iteration"),
    Case("p_parameter_tolerance", "boxes", 3, (4, 4.0, 3.0), (), "termination 2: behind seven rejections the step falls under the parameter tolerance before the function tolerance"),
    Case("q_radius_growth_capped", "boxes", 6, (9, 3.0, 12.0), (), "seven accepted steps grow the radius by the cap of 3; the 30-iteration budget ends behind three rejections"),
    Case("r_radius_limit", "boxes", 5, (6,) + _S, (("huber_delta", 0.05),), "outer iteration 1 is not degenerate: 27 accepted steps, every one at the growth cap, 1e4 * 3^26 clamped to the 1e16 limit"),
)
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- the tracker and the loop registration
TrackCase = collections.namedtuple("TrackCase", "name seed sizes start opts branch")


@functools.lru_cache(maxsize=None)
def track_clouds(seed, n_prev_surf, n_prev_corner, n_surf, n_corner):
    """hand-made clouds for trackCloud: points uniform in a 16 m cube, ring ids 0..15 ascending along each cloud (the order the ring-window walks need). With a
    distance gate of 1e4 every feature finds its nearest point and two ring-window partners, so the planes and lines are arbitrary and a dozen of them leave the
    problem strongly curved in the rotation: that curvature, not a projection, is what rejects steps here (V_update is the identity in the tracker)."""
    rng = np.random.default_rng(seed)

    def cloud(n):
        p = np.zeros((n, 4), np.float32)
        p[:, :3] = rng.uniform(-8, 8, (n, 3))
        p[:, 3] = np.sort(rng.integers(0, 16, n))
        return p
    return dict(surf_last=cloud(n_prev_surf), corner_last=cloud(n_prev_corner), surf_flat=cloud(n_surf), corner_sharp=cloud(n_corner))


def track_start(case):
    s, dt, deg = case.start
    return _synth().perturbed_pose(np.array([0, 0, 0, 0, 0, 0, 1.0]), seed=s, dt=dt, drot_deg=deg)


def track_params_of(case):
    o = dict(case.opts)
    return dict(distance_sq_threshold=o.get("distance_sq_threshold", 25.0), huber_delta=o.get("huber_delta", 0.1), max_lm_iterations=o.get("max_lm_iterations", 4))


@functools.lru_cache(maxsize=None)
def track_traced(case, **mut):
    p = track_params_of(case)
    return track_trace(track_clouds(case.seed, *case.sizes), track_start(case), max_lm_iterations=p["max_lm_iterations"], huber_delta=p["huber_delta"],
                       distance_sq_threshold=p["distance_sq_threshold"], **mut)


@functools.lru_cache(maxsize=None)
def track_oracle_solved(case):
    O, tc = _oracle(), track_clouds(case.seed, *case.sizes)
    return O.track_cloud(tc["corner_last"], tc["surf_last"], tc["corner_sharp"], tc["surf_flat"], track_start(case), O.track_params(**track_params_of(case)))


_G = (("distance_sq_threshold", 1e4),)
_TS = (120, 40, 12, 1)           # 120 + 40 previous points, 12 surf features and 1 corner feature: 13 blocks, three more than a round needs
TRACK_CASES = (
    TrackCase("h_rejections_in_a_round", 320, _TS, (320, 1.0, 60.0), _G + (("huber_delta", 1.0), ("max_lm_iterations", 15)),
              "four rejections in a row inside round 0, then eight acceptances to the budget; round 1 ends on the function tolerance"),
    TrackCase("h_first_iteration_rejected", 272, _TS, (272, 1.0, 60.0), _G + (("huber_delta", 100.0), ("max_lm_iterations", 15)),
              "the first three iterations of round 0 are rejected: the proposals are rebuilt from the begin's record"),
    TrackCase("h_default_budget_ends_on_a_rejection", 320, _TS, (320, 1.0, 60.0), _G + (("huber_delta", 1.0), ("max_lm_iterations", 4)),
              "trackCloud's own four iterations end on a rejected step: termination 0, round 1 starts from the last accepted pose"),
    TrackCase("h_budget_ends_on_three_rejections", 320, _TS, (320, 1.0, 60.0), _G + (("huber_delta", 1.0), ("max_lm_iterations", 6)),
              "a budget of six ends behind three rejections in a row"),
)
TRACK_BY_NAME = {c.name: c for c in TRACK_CASES}
# i. tests/loopreg_cases.py's scene rejects nothing: search_loopreg() runs 2 400 solves through loopreg_ref's register() and every one ends with successful_steps ==
# lm_iterations (- 1 on a tolerance exit). That says something about this one scene -- dense, well-conditioned clouds -- and nothing about the kernel; the
# registration's loop is lm_begin_body / lm_step_body, which the host-stepped form of every mapper case above runs. No case i is committed.


def search_tracker(seeds=range(1, 400), sizes=((12, 0), (12, 1)), degrees=(60.0, 120.0, 179.0), deltas=(0.1, 1.0, 100.0), budget=15):
    """hand-made clouds (120 + 40 previous points) through oracle.track_cloud: one line per problem with a rejected step in a round (35 of 7 182 as committed)"""
    O = _oracle()
    n = hits = 0
    for seed in seeds:
        for ns, nc in sizes:
            for deg in degrees:
                for hd in deltas:
                    case = TrackCase("search", seed, (120, 40, ns, nc), (seed, 1.0, deg), (("distance_sq_threshold", 1e4), ("huber_delta", hd), ("max_lm_iterations", budget)), "")
                    res = track_oracle_solved(case)
                    rej = [o["lm_iterations"] - o["successful_steps"] - (o["termination"] in (PARAMETER, FUNCTION)) for o in res["outer"] if o["solved"]]
                    n += 1
                    if any(r > 0 for r in rej):
                        hits += 1
                        print(f"tracker seed {seed} features {ns}+{nc} start {deg} deg delta {hd}: "
                              f"{[(o['n_corner'], o['n_surf'], o['lm_iterations'], o['successful_steps'], o['termination']) for o in res['outer']]}", flush=True)
    print(f"tracker: {hits} of {n} problems reject a step")


def search_loopreg(n=400, deltas=(1.0, 0.1, 0.03), budgets=(5, 12)):
    """tests/loopreg_cases.py's scene from random start transforms (yaw -20 ... 70 degrees around the 25-degree truth, up to 3 m) through loopreg_ref's register()"""
    import loopreg_cases as lc
    s = lc.scene()
    rng = np.random.default_rng(1)
    runs = hits = 0
    for k in range(n):
        yaw, t = float(rng.uniform(-20, 70)), tuple(float(v) for v in rng.uniform(-3, 3, 3) * np.array([1, 1, 0.3]))
        for hd in deltas:
            for mi in budgets:
                r = lc.register(s["clouds4"], lc.yaw_T(yaw, t), lc.opts(huber_delta=hd, max_lm_iterations=mi))
                rej = [o["lm_iterations"] - o["successful_steps"] - (o["termination"] in (PARAMETER, FUNCTION)) for o in r["outer"] if o["ran"]]
                runs += 1
                if any(x > 0 for x in rej):
                    hits += 1
                    print(f"loop registration yaw {yaw:.2f} t {t} delta {hd} budget {mi}: {[(o['lm_iterations'], o['successful_steps'], o['termination']) for o in r['outer']]}", flush=True)
    print(f"loop registration: {hits} of {runs} starts reject a step")


# ---------------------------------------------------------------- the search the cases came from
def search(seeds=range(1, 13), starts=((1.5, 6.0), (3.0, 12.0), (4.0, 3.0)), families=("boxes", "plane")):
    """one line per outer iteration of every (family, seed, start): the accept / reject sequence, the termination, the smallest margin, the steps at the growth
    cap, the radius range and whether the trace and the oracle count the same -- what the committed cases were picked from"""
    for family in families:
        for seed in seeds:
            for k in (1, 2, 3):
                for dt, deg in (starts if family == "boxes" else ((0.3, 3.0), (0.8, 8.0))):
                    case = Case("search", family, seed, (seed + k, dt, deg), (), "")
                    for i, (a, b) in enumerate(zip(traced(case)["outer"], oracle_solved(case)["outer"])):
                        t, s = a["trace"], a["trace"]["summary"]
                        radii = [r["radius"] for r in t["iters"]] or [0.0]
                        same = (s["lm_iterations"], s["successful_steps"], s["termination"], s["evaluations"]) == (b["lm_iterations"], b["successful_steps"], b["termination"], b["evaluations"])
                        print(f"{family} {seed} start ({seed + k}, {dt}, {deg}) outer {i}: {flags(t) or '-'} termination {s['termination']} margin {t['margin']:.1e} "
                              f"capped {sum(1 for r in t['iters'] if r.get('radius_growth') == 3.0)} radius {min(radii):.1e} .. {max(radii):.1e} degenerate {a['is_degenerate']} "
                              f"blocks {a['n_surf']}+{a['n_corner']} oracle {'same' if same else 'DIFFERS'}", flush=True)


if __name__ == "__main__" and sys.argv[1:2] == ["search"]:
    {"tracker": search_tracker, "loopreg": search_loopreg}.get((sys.argv[2:] + [""])[0], search)()
