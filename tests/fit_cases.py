"""Crafted neighbourhoods for the mapper's line and plane fits (dev_math.hpp: plane_fit_qr_f, eig3_largest_f; match.hip: fit_plane, fit_line, fit_feature,
eval_plane, eval_edge), with float64 references that share nothing with the f32 code under test.

Plain module: pure numpy, no fixtures, no GPU, no oracle import, nothing collected.

A SITE is K = 5 or 10 map points plus one query point. All plane sites form ONE surf map and all line sites ONE corner map; the sites are far enough apart that
the K nearest points of a site's query are exactly the site's own (asserted below with knn_cases.brute_knn, at every pose). Most sites sit on the nodes of a 5 m
lattice (about five cells of the 1.001 m index); the near-origin family cannot: a patch 0.3 m and a patch 3 m from the origin are at most 3.3 m apart whatever
one does. So the module asserts what the lattice is for, directly: no foreign point within 2 m of any query, and the K-th distance at most 0.9 of the radius.

Every site names its family, the branch of the f32 code it is built to reach, and its class:
  'f64'   held to the float64 reference under the bars (plane_bar, line_terms): full rank, or the deficient column exactly zero; kappa(A) <= 3e3 for planes
  'bits'  held only to the oracle's / the reference build's bits, with the reason (Eigen's basic solution of a rank-deficient system is not the minimum-norm one
          lstsq returns; a plane through the origin has no finite solution of A n = -1; an isotropic scatter has no direction). At most one site in five.
A DECISION site sits at a stated distance from a gate (min_plane_dis, l2 > 3 l1); the distance of the deciding float64 quantity from the threshold is at
least 20 times the site's bar (asserted by check_margins once the constants of the bars are known).

References (from the f32 coordinates widened to float64):
  plane_ref   n = lstsq(A, -1), n_hat = n / |n|, d = 1 / |n|, kappa(A) from the singular values, max_j |n_hat . p_j + d|
  line_ref    centroid, centred scatter matrix, eigh; valid when l2 > 3 l1; end points c +- 0.1 v (an unordered pair)
  factor_rows residual and 1 x 6 Jacobian of the plane-norm / edge factor at a pose for given coefficients, weighted by sqrt_info_of(trace); normal_eq sums
              them with the Huber weight (rho1 = 1 where r^2 <= delta^2, else delta / |r|) through math.fsum
"""
import math

import numpy as np

import knn_cases as kc

F32 = np.float32
SQ = 1.0                     # min_match_sq_dis
MIN_PLANE_DIS = 0.2
HUBER_DELTA = 0.1
EPS = 2.0 ** -24
KAPPA_MAX = 3.0e3
GAP_MIN = 0.05
TRACES = (0.0075, 1.0 / 9.0, 0.25, 0.0)
QOFF = np.array([0.031, -0.017, 0.023])          # a generic offset of the query from the site's centre: no two neighbours at the same distance


# ---------------------------------------------------------------- poses
def _quat(rotvec):
    rv = np.asarray(rotvec, np.float64)
    a = float(np.linalg.norm(rv))
    if a == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(a / 2) * rv / a, [np.cos(a / 2)]])


def rot_of(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _poses():
    gen = np.concatenate([[0.4, -0.3, 0.2], _quat([0.1, -0.2, 0.3])])
    neg = gen.copy()
    neg[3:] = -neg[3:]
    axis = np.array([0.36, 0.48, 0.8])
    near_pi = np.concatenate([[-0.2, 0.5, 0.1], _quat((np.pi - 5.0e-4) * axis)])
    return dict(identity=np.array([0, 0, 0, 0, 0, 0, 1.0]), generic=gen, q_negated=neg, near_pi=near_pi)


POSES = _poses()
SECOND_POSE = np.concatenate([[0.43, -0.28, 0.17], _quat([0.11, -0.19, 0.32])])      # mlh_linearize re-evaluates the generic pose's correspondences here


def pose_plus(x, delta):
    """PoseLocalParameterization::Plus: t + dt, q * [dtheta / 2, 1] normalised"""
    x, d = np.asarray(x, np.float64), np.asarray(delta, np.float64)
    qx, qy, qz, qw = x[3:]
    dx, dy, dz, dw = d[3] / 2, d[4] / 2, d[5] / 2, 1.0
    p = np.array([qw * dx + qx * dw + qy * dz - qz * dy, qw * dy - qx * dz + qy * dw + qz * dx, qw * dz + qx * dy - qy * dx + qz * dw,
                  qw * dw - qx * dx - qy * dy - qz * dz])
    return np.concatenate([x[:3] + d[:3], p / np.linalg.norm(p)])


def transform(pose, pts):
    pts = np.atleast_2d(np.asarray(pts, np.float64))
    return pts @ rot_of(pose[3:]).T + np.asarray(pose[:3], np.float64)


def inverse_transform(pose, pts):
    pts = np.atleast_2d(np.asarray(pts, np.float64))
    return (pts - np.asarray(pose[:3], np.float64)) @ rot_of(pose[3:])


# ---------------------------------------------------------------- float64 references
def plane_ref(pts):
    """-> dict(n_hat, d, kappa, max_res, valid, rank); pts (K x 3) f32. A zero column is left out of kappa (both solutions put 0 there)."""
    A = np.asarray(pts, np.float64)
    n, _, rank, sv = np.linalg.lstsq(A, -np.ones(len(A)), rcond=1e-12)
    live = np.any(A != 0.0, axis=0)
    svl = np.linalg.svd(A[:, live], compute_uv=False)
    nn = float(np.linalg.norm(n))
    n_hat, d = n / nn, 1.0 / nn
    res = np.abs(A @ n_hat + d)
    return dict(n_hat=n_hat, d=d, kappa=float(svl[0] / svl[-1]) if svl[-1] > 0 else np.inf, max_res=float(res.max()), valid=bool(res.max() <= MIN_PLANE_DIS),
                rank=int(rank), live=live)


def line_ref(pts):
    """-> dict(c, lam (ascending), v (of the largest), gap, extent, valid, ends (2 x 3))"""
    P = np.asarray(pts, np.float64)
    c = P.mean(axis=0)
    D = P - c
    lam, vec = np.linalg.eigh(D.T @ D)
    v = vec[:, 2]
    gap = float((lam[2] - lam[1]) / lam[2]) if lam[2] > 0 else 0.0
    return dict(c=c, lam=lam, v=v, gap=gap, extent=float(np.linalg.norm(D, axis=1).max()), valid=bool(lam[2] > 3.0 * lam[1]),
                ends=np.stack([c + 0.1 * v, c - 0.1 * v]))


def sqrt_info_of(trace):
    with np.errstate(divide="ignore"):
        s = float(np.sqrt(np.float64(1.0) / np.float64(trace)))
    return 1.0 if s >= 3.0 else s / 3.0


def _skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0.0]])


def factor_row(kind, point, coeff, w, pose):
    """residual and 1 x 6 Jacobian [d/dt, d/dtheta] (LidarMapPlaneNormFactor / LidarMapEdgeFactor), all float64"""
    p = np.asarray(point, np.float64)
    c = np.asarray(coeff, np.float64)
    R = rot_of(pose[3:])
    lp = R @ p + np.asarray(pose[:3], np.float64)
    if kind == "s":
        n, d = c[:3], c[3]
        return w * (float(n @ lp) + d), np.concatenate([w * n, w * (-(n @ R) @ _skew(p))])
    A, B = c[:3], c[3:6]
    nu = np.cross(lp - A, lp - B)
    de = A - B
    nn, dn = float(np.linalg.norm(nu)), float(np.linalg.norm(de))
    eta = (nu / nn if nn > 0 else nu) / dn
    eD = eta @ _skew(de)
    return w * nn / dn, np.concatenate([-w * eD, w * ((eD @ R) @ _skew(p))])


def factor_rows(kind, feats, valid, coeffs, trace, pose):
    """rows of every feature (zero rows where not valid) -> r (m,), J (m x 6)"""
    w = sqrt_info_of(trace)
    r, J = np.zeros(len(feats)), np.zeros((len(feats), 6))
    for i in range(len(feats)):
        if valid[i]:
            r[i], J[i] = factor_row(kind, feats[i, :3], coeffs[i], w, pose)
    return r, J


def normal_eq(r, J, valid, delta=HUBER_DELTA, loss=True):
    """H = sum rho1 J^T J, g = sum rho1 J^T r, cost = sum 0.5 rho(r^2), count -- math.fsum; also the smallest relative distance of an |r| from the Huber gate"""
    idx = [i for i in range(len(r)) if valid[i]]
    rho1 = {i: (delta / abs(r[i]) if loss and r[i] * r[i] > delta * delta else 1.0) for i in idx}
    rho = {i: (2.0 * delta * abs(r[i]) - delta * delta if loss and r[i] * r[i] > delta * delta else r[i] * r[i]) for i in idx}
    H = np.array([[math.fsum(rho1[i] * J[i, a] * J[i, b] for i in idx) for b in range(6)] for a in range(6)])
    g = np.array([math.fsum(rho1[i] * J[i, a] * r[i] for i in idx) for a in range(6)])
    gate = min([abs(abs(r[i]) - delta) / delta for i in idx], default=np.inf)
    return dict(H=H, g=g, cost=math.fsum(0.5 * rho[i] for i in idx), count=len(idx), gate_distance=gate)


# ---------------------------------------------------------------- bars
def plane_bar(ref, c_p):
    return c_p * ref["kappa"] * EPS


def plane_err(n_hat, d, ref):
    return max(float(np.abs(np.asarray(n_hat, np.float64) - ref["n_hat"]).max()), abs(float(d) - ref["d"]) / max(ref["d"], 1.0))


def line_terms(ref):
    """the bracket of the end-point bar, of the centre's bar, and of the eigenvalue bar (all to be multiplied by c * 2^-24)"""
    cinf = float(np.abs(ref["c"]).max())
    s = ref["extent"]
    spread = (1.0 + cinf / s) if s > 0 else 1.0
    ends = cinf + 0.1 * spread / ref["gap"] if ref["gap"] >= GAP_MIN else None
    return dict(ends=ends, centre=cinf, eig=spread)


def ends_err(coef6, ref):
    a, b = np.asarray(coef6[:3], np.float64), np.asarray(coef6[3:6], np.float64)
    e = ref["ends"]
    return min(max(np.abs(a - e[0]).max(), np.abs(b - e[1]).max()), max(np.abs(a - e[1]).max(), np.abs(b - e[0]).max()))


def centre_err(coef6, ref):
    return float(np.abs((np.asarray(coef6[:3], np.float64) + np.asarray(coef6[3:6], np.float64)) / 2 - ref["c"]).max())


# ---------------------------------------------------------------- building blocks
def _patterns(k):
    """three zero-mean, mutually orthogonal unit patterns of length k (a, a^2 - mean, a^3 - alpha a): points u a_i + v b_i + w c_i have the scatter
    matrix diag(|u|^2, |v|^2, |w|^2) in the frame (u, v, w)"""
    a = np.arange(k, dtype=np.float64) - (k - 1) / 2
    b = a * a - np.mean(a * a)
    c = a ** 3 - (np.sum(a ** 4) / np.sum(a * a)) * a
    out = [v / np.linalg.norm(v) for v in (a, b, c)]
    assert all(abs(float(x @ y)) < 1e-12 for i, x in enumerate(out) for y in out[i + 1:]) and all(abs(v.sum()) < 1e-12 for v in out)
    return out


def _frame(normal, seed_vec=(0.3, -0.5, 0.8)):
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    u = np.cross(n, seed_vec)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u), n


def _scatter(centre, normal, sig, k=5):
    """k points around centre whose scatter matrix has the eigenvalues sig[0]^2 <= sig[1]^2 <= sig[2]^2 (before rounding to f32): the largest along u, the
    smallest along `normal`"""
    a, b, c = _patterns(k)
    u, v, n = _frame(normal)
    return np.asarray(centre, np.float64)[None, :] + sig[2] * a[:, None] * u + sig[1] * b[:, None] * v + sig[0] * c[:, None] * n


def _patch(centre, normal, extent, k=5):
    """k points on the plane through centre with the given normal, spread over about `extent`"""
    return _scatter(centre, normal, (0.0, 0.3 * extent, 0.4 * extent), k)


SITES = []


def _site(name, kind, family, branch, pts, query=None, cls="f64", reason="", decision=None, query_other=None, expect_valid=None):
    pts = np.ascontiguousarray(np.asarray(pts, np.float64), F32)
    k = len(pts)
    assert k in (5, 10), name
    if query is None:
        query = pts.astype(np.float64).mean(axis=0) + QOFF
    assert cls in ("f64", "bits") and (cls == "f64" or reason), name
    SITES.append(dict(name=name, kind=kind, family=family, branch=branch, pts=pts, k=k, query=np.asarray(query, np.float64), cls=cls, reason=reason,
                      decision=decision, query_other=None if query_other is None else np.asarray(query_other, np.float64), expect_valid=expect_valid))


def _tune(make, quantity, target, lo, hi):
    """bisection on the parameter of `make` (-> points) until quantity(points as f32) == target (monotone increasing on [lo, hi])"""
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if quantity(np.asarray(make(mid), np.float64).astype(F32)) < target:
            lo = mid
        else:
            hi = mid
    return make(0.5 * (lo + hi))


# ---------------------------------------------------------------- plane sites (surf map)
def _plane_sites():
    S = lambda *a, **kw: _site(a[0], "s", *a[1:], **kw)
    # each column the first pivot once: the constant coordinate's column has by far the largest norm
    S("p_x_const", "plane x = c", "QR pivot = column 0 at k = 0", _patch((-7, 0.3, 0.2), (1, 0, 0), 0.5))
    S("p_y_const", "plane y = c", "QR pivot = column 1 at k = 0", _patch((0.2, 5, 0.3), (0, 1, 0), 0.5))
    S("p_z_const", "plane z = c", "QR pivot = column 2 at k = 0", _patch((0.3, 0.2, 5), (0, 0, 1), 0.5))
    # two columns with EXACTLY equal norms: x = 10 + a / 8, y = 10 + b / 8 with sum a = sum b = 0 and sum a^2 = sum b^2; every square and every partial sum is a
    # small dyadic number, exact in f32 in any order. z = 1 + (x - 10) / 2 + (y - 10): a plane off the origin.
    a, b = np.array([-2, -1, 0, 1, 2.0]), np.array([0, -2, 2, -1, 1.0])
    tie = np.stack([10 + a / 8, 10 + b / 8, 1 + a / 16 + b / 8], axis=1)
    c32 = tie.astype(F32)
    sx = sy = F32(0)
    for i in range(5):
        sx, sy = F32(sx + c32[i, 0] * c32[i, 0]), F32(sy + c32[i, 1] * c32[i, 1])
    assert sx == sy and np.array_equal(c32.astype(np.float64), tie)
    S("p_tie", "two columns with exactly equal norms", "QR pivot tie at k = 0: the first maximum wins", tie)
    # one coordinate exactly 0, the plane off the origin: collinear points in z = 0 on a line that misses the origin; the zero column is the deficient one
    t = np.array([-0.21, -0.08, 0.02, 0.11, 0.2])
    S("p_zero_column", "one coordinate exactly 0, plane off the origin", "nonzero_pivots < 3 (= 2): the zero column never pivots",
      np.stack([5 + t, -5 + 0.5 * t, 0 * t], axis=1))
    # nearly parallel columns far out: after the first reflector the remaining column norms are ~1e-3 of the original ones
    S("p_far_patch", "patch at (20, 20, 5), 0.2 m extent", "norm down-date recompute (temp2 <= sqrt(eps)), twice", _patch((20, 20, 5), (20, 19, 7), 0.2))
    # tau == 0: the nearest neighbour (row 0) alone has x != 0, and x is the pivot column; also the patch 0.3 m from the origin (its centroid is (0.15, 0, 0.26))
    y = np.array([0.0, -0.075, -0.025, 0.025, 0.075])
    tau0 = np.stack([[0.75, 0, 0, 0, 0], y, np.full(5, 0.26)], axis=1)
    S("p_tau0_03m", "first column with a zero tail; patch 0.3 m from the origin", "tau0 == 0 (tailSq <= FLT_MIN): the first reflector is skipped", tau0,
      query=tau0[0] + np.array([-0.05, 0.012, -0.02]))
    # one point off the plane by min_plane_dis (1 -+ 0.01): the offset is tuned until the FITTED plane's largest residual (float64) is 0.2 (1 -+ 0.01)
    for tag, f, k in (("in", 0.99, 5), ("out", 1.01, 5), ("in_k10", 0.99, 10)):
        centre = {"in": (-3, 0, 0.3), "out": (0, -3, 0.3), "in_k10": (0, 0, -3)}[tag]
        base = _patch(centre, centre, 0.5, k)                   # facing the origin: a tilt does not change d to first order, the fit cannot trade it for residual
        nrm = _frame(centre)[2]

        def make(delta, base=base, nrm=nrm):
            p = base.copy()
            p[1] += delta * nrm
            return p
        pts = _tune(make, lambda p: plane_ref(p)["max_res"], MIN_PLANE_DIS * f, 0.0, 0.6)
        S(f"p_gate_{tag}", f"one point off the plane, largest residual min_plane_dis * {f}", "plane gate |n . p + d| > min_plane_dis", pts,
          decision=dict(quantity="max_res", threshold=MIN_PLANE_DIS, rel=abs(f - 1)), expect_valid=f < 1)
    S("p_3m", "patch 3 m from the origin", "generic 5 x 3 QR", _patch((3, 0, 0), (1, 0.2, -0.1), 0.5))
    S("p_50m", "patch 50 m from the origin", "generic 5 x 3 QR far out", _patch((50, 0, 0), (1, 0.1, 0.05), 0.5))
    S("p_through_origin", "plane through the origin", "A n = -1 has no finite solution", _patch((0, -10, 0), (1, 0, 1), 0.5), cls="bits",
      reason="a plane through the origin: |n| -> infinity, float64's n_hat is decided by rounding")
    t = np.array([-0.3, -0.12, 0.05, 0.17, 0.31])
    S("p_collinear", "collinear points", "nonzero_pivots < 3 on a rank-2 neighbourhood", np.array([0, 10, 1.0])[None, :] + t[:, None] * np.array([0.6, 0.3, 0.74]),
      cls="bits", reason="rank 2 without a zero column: Eigen's basic solution is not lstsq's minimum-norm one")
    S("p_identical", "identical points", "nonzero_pivots < 3 on a rank-1 neighbourhood", np.tile([1.0, 2.0, 3.0], (5, 1)), cls="bits",
      reason="rank 1: the basic solution puts everything on the pivot column (n = (0, 0, -1), d = 3, accepted)", expect_valid=True)
    S("p_k10", "K = 10 generic patch", "10 x 3 QR", _patch((-5, 5, 0), (0.3, -0.2, 1), 0.6, 10))
    S("p_k10_x_const", "K = 10 plane x = c", "10 x 3 QR, pivot = column 0", _patch((-10, 0.2, 0.3), (1, 0, 0), 0.6, 10))
    # factor sites on planes: a feature ON its plane, and |r| = delta (1 -+ 1e-3) at sqrt_info 1
    onp = _patch((10, 0, 0.5), (1, 0, 0), 0.5)
    S("p_feature_on_plane", "feature on its plane", "eval_plane with r = 0", onp, query=onp.mean(axis=0) + np.array([0.0, 0.031, -0.017]))
    for tag, f, ctr in (("below", 1 - 1e-3, (10, 5, 0.5)), ("above", 1 + 1e-3, (10, -5, 0.5))):
        hp = _patch(ctr, (1, 0, 0), 0.5)
        S(f"p_huber_{tag}", f"|r| = delta * {f:.3f}", "Huber gate r^2 > delta^2 (plane factor)", hp, query=hp.mean(axis=0) + np.array([HUBER_DELTA * f, 0.031, -0.017]))


# ---------------------------------------------------------------- line sites (corner map)
def _line_sites():
    S = lambda *a, **kw: _site(a[0], "c", *a[1:], **kw)
    t = np.array([-6, -3, 0, 2, 5.0]) / 16
    for tag, d, ctr, br in (("x", (1, 0, 0), (5, 0, 0), "a20 == 0, already diagonal: no tridiagonalisation, no rotation"),
                            ("y", (0, 1, 0), (0, 5, 0), "already diagonal, the largest eigenvalue in the middle: the selection sort swaps columns"),
                            ("z", (0, 0, 1), (0, 0, 5), "already diagonal and already sorted"),
                            ("diag", (1, 1, 1), (5, 5, 0), "a full matrix of equal entries: tridiagonalisation, then deflation")):
        S(f"l_collinear_{tag}", f"exactly collinear along {tag}", br, np.asarray(ctr, float)[None, :] + t[:, None] * np.asarray(d, float),
          query=np.asarray(ctr, float) + 0.04 * np.asarray(d, float) + np.array([0.02, 0.03, -0.025]), expect_valid=True)
    for i, ratio in enumerate((1.5, 5.0, 30.0)):
        s1 = 0.12
        S(f"l_coplanar_{ratio:g}", f"coplanar, l2 / l1 = {ratio:g}", "QL sweeps on a generic rank-2 scatter (case A, then deflation)",
          _scatter((0, 5 * (i + 1), 5), (0.3, 0.5, -0.8), (0.0, s1, s1 * np.sqrt(ratio))), expect_valid=ratio > 3)
    for tag, f, k, ctr in (("below", 0.98, 5, (5, 0, 5)), ("above", 1.02, 5, (0, -5, 0)), ("below_k10", 0.98, 10, (-5, 0, 0)), ("above_k10", 1.02, 10, (-5, -5, 0))):
        S(f"l_gate_{tag}", f"l2 / l1 = 3 * {f}", "line gate l2 > 3 l1", _scatter(ctr, (0.5, -0.3, 0.8), (0.03, 0.15, 0.15 * np.sqrt(3 * f)), k),
          decision=dict(quantity="ratio", threshold=3.0, rel=abs(f - 1)), expect_valid=f > 1)
    tet = 0.25 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [0, 0, 0.0]])
    S("l_isotropic", "isotropic: tetrahedron plus its centre", "three equal eigenvalues: a20 == 0, no sweep, the sort's first minimum wins", tet + np.array([5, 5, 5.0]), cls="bits",
      reason="an isotropic scatter has no direction; only the decision 'invalid' is float64's", expect_valid=False)
    S("l_near_isotropic", "nearly isotropic", "close eigenvalues: many QL sweeps", _scatter((5, -5, 0), (1, 2, 3), (0.2, 0.21, 0.22)), expect_valid=False)
    S("l_two_equal_large", "two equal large eigenvalues", "l2 == l1 up to rounding: deflation order decides which column is 'largest'", _scatter((0, -5, 5), (1, -1, 2), (0.02, 0.3, 0.3)),
      expect_valid=False)
    S("l_identical", "five identical points", "scale == 0", np.tile([-5.0, 5.0, 0.5], (5, 1)), expect_valid=False)
    S("l_extent_1e-4", "extent 1e-4 m", "cancellation in p - c: a few hundred ulps of extent", _scatter((0, 0, -5), (0.2, 0.9, 0.4), (1.0e-5, 2.0e-5, 7.9e-5)), expect_valid=True)
    S("l_extent_0.9", "extent 0.9 m", "K-th neighbour close to the radius", _scatter((-5, 0, 5), (0.2, 0.9, 0.4), (0.02, 0.05, 0.71)), expect_valid=True)
    e = 1.0 / 8
    S("l_a20_zero", "a20 == 0 exactly (already tridiagonal)", "v1norm2 <= FLT_MIN: the tridiagonalisation is skipped, sweeps run on the input",
      np.array([5, -5, 5.0]) + e * np.array([[1, 1, 0], [-1, -1, 0], [0, 2, 1], [0, -2, -1], [0, 0, 0.0]]))
    S("l_a10_zero", "a10 == 0 exactly", "tridiagonalisation with m01 == 0", np.array([-5, 5, 5.0]) + e * np.array([[1, 0, 1], [-1, 0, -1], [0, 2, 1], [0, -2, -1], [0, 0, 0.0]]))
    S("l_diagonal", "already diagonal", "no off-diagonal entry: end == 0 at once", np.array([-5, -5, 5.0]) + e * np.array([[3, 0, 0], [-3, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.0]]),
      expect_valid=True)
    S("l_trailing_2x2", "block diagonal, trailing 2 x 2", "s0 == 0, s1 != 0: case B only", np.array([5, 5, -5.0]) + e * np.array([[1, 0, 0], [-1, 0, 0], [0, 2, 1], [0, -2, -1], [0, 0, 0.0]]))
    S("l_leading_2x2", "block diagonal, leading 2 x 2", "s1 == 0, s0 != 0: caseC only", np.array([5, -5, -5.0]) + e * np.array([[2, 1, 0], [-2, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0.0]]))
    # l2 == 3 l1 EXACTLY, in f32 as in float64: a diagonal scatter matrix (2, 6, 18) / 64 -- 6 / 18 rounds, but (6 / 18) * (18 / 64) rounds back to 6 / 64 -- so only the
    # strictness of the gate's comparison decides, and it decides "invalid". No margin can exist here; tests/test_fit_cases.py asserts the tie itself instead.
    S("l_gate_exact_tie", "l2 == 3 l1 exactly", "the strict > of the line gate", np.array([5, 0, -5.0]) + e * np.array([[3, 0, 0], [-3, 0, 0], [0, 1, 1], [0, 1, -1], [0, -2, 0.0]]),
      expect_valid=False)
    S("l_50m", "centroid 50 m from the origin", "cancellation in p - c far out", _scatter((0, 30, 40), (0.3, 0.5, -0.8), (0.01, 0.03, 0.3)), expect_valid=True)
    t10 = np.array([-9, -7, -4, -2, -1, 1, 2, 5, 6, 8.0]) / 32
    S("l_k10_collinear_diag", "K = 10 collinear along a diagonal", "10-point centroid and scatter", np.array([-5, 5, -5.0]) + t10[:, None] * np.array([1, -1, 1.0]),
      query=np.array([-5, 5, -5.0]) + 0.02 * np.array([1, -1, 1.0]) + np.array([0.02, 0.03, -0.025]), expect_valid=True)
    S("l_k10_coplanar_5", "K = 10 coplanar, l2 / l1 = 5", "10-point scatter, QL sweeps", _scatter((-5, -5, -5), (0.3, 0.5, -0.8), (0.0, 0.12, 0.12 * np.sqrt(5)), 10), expect_valid=True)
    # factor sites on lines: a feature exactly ON its line at the identity pose (every neighbour has y = 0.5, z = -5 exactly, so the centroid and both end points do
    # too, and a feature with that y and z gives nu == 0 exactly: residual 0, an all-zero row, no NaN). At any other pose the stored feature is rounded to f32, the
    # transformed point sits ~1e-7 m off the line, and the DIRECTION of nu -- hence the whole row -- is decided by the last bits of the rotation: ill-conditioned by
    # construction, whatever the precision. There the site's query sits 5 cm off the line instead (query_other).
    on = np.array([10, 0.5, -5.0])[None, :] + t[:, None] * np.array([1.0, 0, 0])
    S("l_feature_on_line", "feature exactly on its line", "eval_edge with nu == 0", on, query=np.array([10.07, 0.5, -5.0]), query_other=np.array([10.07, 0.53, -5.04]), expect_valid=True)
    for tag, f, ctr in (("below", 1 - 1e-3, (10, 5, 0)), ("above", 1 + 1e-3, (10, -5, 0))):
        hl = np.asarray(ctr, float)[None, :] + t[:, None] * np.array([0, 0, 1.0])
        S(f"l_huber_{tag}", f"|r| = delta * {f:.3f}", "Huber gate r^2 > delta^2 (edge factor)", hl, query=np.asarray(ctr, float) + np.array([0.6, 0.8, 0]) * HUBER_DELTA * f + np.array([0, 0, 0.03]),
          expect_valid=True)


_plane_sites()
_line_sites()
NAMES = [s["name"] for s in SITES]
assert len(set(NAMES)) == len(NAMES)


def site(name):
    return SITES[NAMES.index(name)]


def sites_of(kind, k=None):
    return [s for s in SITES if s["kind"] == kind and (k is None or s["k"] == k)]


def _build_map(kind):
    rows, at = [], 0
    for s in sites_of(kind):
        s["first"] = at
        rows.append(s["pts"])
        at += s["k"]
    return np.ascontiguousarray(np.concatenate(rows), F32)


SURF_MAP, CORNER_MAP = _build_map("s"), _build_map("c")
MAPS = {"s": SURF_MAP, "c": CORNER_MAP}
assert len(SURF_MAP) > 50 and len(CORNER_MAP) > 10 and len(SURF_MAP) + len(CORNER_MAP) < 400      # the mapper's minimum; a few hundred points in all

# every site carries its float64 reference
for _s in SITES:
    _s["ref"] = plane_ref(_s["pts"]) if _s["kind"] == "s" else line_ref(_s["pts"])
    if _s["kind"] == "s" and _s["cls"] == "f64":
        assert _s["ref"]["kappa"] <= KAPPA_MAX and (_s["ref"]["rank"] == 3 or int(_s["ref"]["live"].sum()) == _s["ref"]["rank"]), (_s["name"], _s["ref"]["kappa"], _s["ref"]["rank"])
    if _s["expect_valid"] is not None and (_s["cls"] == "f64" or _s["kind"] == "c"):
        assert _s["ref"]["valid"] == _s["expect_valid"], (_s["name"], _s["ref"])
    if _s["decision"]:
        q = _s["ref"]["max_res"] if _s["kind"] == "s" else _s["ref"]["lam"][2] / _s["ref"]["lam"][1]
        _s["decision"]["value"] = float(q)
        assert abs(abs(q / _s["decision"]["threshold"] - 1) - _s["decision"]["rel"]) < 1e-4, (_s["name"], q)
assert sum(s["cls"] == "bits" for s in SITES) * 5 <= len(SITES), "at most one site in five may be held to bits only"
# the exact-zero constructions really are exact in f32
for _n, _i, _j in (("l_a20_zero", 2, 0), ("l_a10_zero", 1, 0), ("l_trailing_2x2", 1, 0), ("l_trailing_2x2", 2, 0), ("l_leading_2x2", 2, 0), ("l_leading_2x2", 2, 1),
                   ("l_diagonal", 1, 0), ("l_diagonal", 2, 0), ("l_diagonal", 2, 1), ("l_gate_exact_tie", 1, 0), ("l_gate_exact_tie", 2, 0), ("l_gate_exact_tie", 2, 1), ("l_isotropic", 1, 0), ("l_isotropic", 2, 0), ("l_isotropic", 2, 1)):
    _p = site(_n)["pts"]
    _c = _p.sum(axis=0, dtype=F32) / F32(5)
    _d = _p - _c
    assert F32(np.sum(_d[:, _i] * _d[:, _j], dtype=F32)) == 0 and np.all((_d[:, _i] * _d[:, _j]).astype(np.float64) == _d[:, _i].astype(np.float64) * _d[:, _j]), _n


def f32_scatter(nb):
    """fit_line's centroid and lower triangle in its own order and precision (f32, neighbours first to last) -> c (3,), [c00, c10, c11, c20, c21, c22]"""
    nb = np.ascontiguousarray(nb, F32)
    k = len(nb)
    c = np.zeros(3, F32)
    for j in range(k):
        c = (c + nb[j]).astype(F32)
    c = (c / F32(k)).astype(F32)
    m = np.zeros(6, F32)
    for j in range(k):
        t = (nb[j] - c).astype(F32)
        m = (m + np.array([t[0] * t[0], t[1] * t[0], t[1] * t[1], t[2] * t[0], t[2] * t[1], t[2] * t[2]], F32)).astype(F32)
    return c, m


# ---------------------------------------------------------------- features: the inverse pose applied to the site's query
def _m4(a):
    out = np.zeros((len(a), 4), F32)
    out[:, :3] = a[:, :3]
    return out


def query_of(s, pose_name):
    return s["query"] if pose_name == "identity" or s["query_other"] is None else s["query_other"]


def features(kind, k, pose_name):
    """-> (m x 4 f32 features, the sites they belong to): stored as T^-1 q, so that the kernel's own transform brings them back to the site's query"""
    ss = sites_of(kind, k)
    q = np.stack([query_of(s, pose_name) for s in ss])
    return _m4(inverse_transform(POSES[pose_name], q).astype(F32)), ss


def _check_isolation():
    for pose_name, pose in POSES.items():
        for kind in ("s", "c"):
            cloud = MAPS[kind]
            c64 = cloud.astype(np.float64)
            for k in (5, 10):
                f4, ss = features(kind, k, pose_name)
                xq = transform(pose, f4[:, :3].astype(np.float64))                     # float64: what the kernel rounds to f32 before it searches
                idx, d2 = kc.brute_knn(cloud, xq.astype(F32), k)
                for i, s in enumerate(ss):
                    own = np.arange(s["first"], s["first"] + k)
                    assert np.array_equal(np.sort(idx[i]), own), (s["name"], pose_name, idx[i])
                    assert d2[i, k - 1] <= 0.81 * SQ, (s["name"], pose_name, d2[i])                  # the K-th distance at most 0.9 of the radius
                    dist = np.linalg.norm(c64 - xq[i], axis=1)
                    foreign = np.delete(dist, own)
                    assert foreign.min() >= 2.0, (s["name"], pose_name, foreign.min())                  # nobody else within two radii
                    ds = np.sort(dist[own])
                    close = np.diff(ds) < max(1e-7, 1e-3 * (ds[-1] - ds[0]))                            # neighbours at (nearly) one distance must be one point:
                    if close.any():                                                                      # otherwise the order of the rows hangs on rounding
                        assert len(np.unique(cloud[own], axis=0)) == 1, (s["name"], pose_name, ds)
                    assert float(np.abs(xq[i] - query_of(s, pose_name)).max()) < 2e-5, (s["name"], pose_name)


_check_isolation()


def check_margins(c_p, c_l, c_e):
    """decision sites: the deciding float64 quantity is at least 20 bars from its threshold -> {site: (distance, bar)}"""
    out = {}
    for s in SITES:
        if not s["decision"]:
            continue
        ref = s["ref"]
        if s["kind"] == "s":
            bar = plane_bar(ref, c_p) * max(ref["d"], 1.0)                   # a residual moves by at most |dn| |p| + |dd|, |p| ~ d: the bar on d, un-normalised
            dist = abs(ref["max_res"] - MIN_PLANE_DIS)
        else:
            bar = c_e * EPS * line_terms(ref)["eig"] * 4.0                    # l2 - 3 l1 relative to l2 moves by at most (1 + 3) eigenvalue bars
            dist = abs(ref["lam"][2] - 3.0 * ref["lam"][1]) / ref["lam"][2]
        assert dist >= 20.0 * bar, (s["name"], dist, bar)
        out[s["name"]] = (float(dist), float(bar))
    return out


FAMILIES = sorted({s["family"] for s in SITES})
