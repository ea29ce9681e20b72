"""Pose graphs with MORE than 128 loop edges, shared by tests/test_pg_many_cases.py (CPU) and tests/test_gpu_posegraph_many.py (GPU): the graphs A, A2, B, C, D, E
built with tests/pg_cases.py's generator, the restatement's passes over them, and two transcriptions of ONE linear step in NumPy / SciPy that need no dense n x n
solve -- the band + low-rank split the device computes, and a sparse LU of the assembled system, which is the reference for E (the restatement's dense solve takes
over a minute there). Computed once per process and shared: do not modify what these functions return.

The blocked dense stage cuts m = 6 L columns into panels of PANEL = 64 (pg_host.hpp: PG_PANEL):
  A, A2  L = 129   m =  774 = 12 x 64 + 6    just over the cap, a remainder panel of 6 columns whose tile also holds the bordering row
  B      L = 150   m =  900 = 14 x 64 + 4
  C      L = 257   m = 1542 = 24 x 64 + 6    (one linear step only: the restatement's optimise takes 5.5 s)
  D      L = 175   m = 1050 = 16 x 64 + 26   35 loops end on the constant block, every 17th of the others is perturbed by decimetres (Huber active)
  E      L = 1024  m = 6144 = 96 x 64        the limit and an exact multiple: the bordering row has a row tile of its own"""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pg_cases as pc

PANEL = 64
CAP_DEFAULT, LOOPS_LIMIT = 128, 1024
FAR = ((0.3, -0.2, 0.1), (0.01, 0.0, 0.02))          # as in pg_cases.graph_linearize
MANY = ("A", "A2", "B", "C", "D", "E")
# name: (cur, L, M, first)
TABLE = {"A": (143, 129, 142, 2), "A2": (163, 129, 162, 2), "B": (213, 150, 212, 2), "C": (298, 257, 298, 1), "D": (183, 175, 181, 3), "E": (1098, 1024, 1097, 2)}
STEP_MANY = ("A", "B", "C", "D")                      # one linear step against the restatement's dense solve
OPTIMIZE_MANY = ("A", "B", "D")                       # a full optimise against the restatement (A2 too, for the launch count)
FORCED_MANY = (0b00011, 8)                            # on A: (fail_mask, max_num_iterations)


@functools.lru_cache(maxsize=None)
def graph_many(name):
    """(graph, cur)"""
    cur = TABLE[name][0]
    if name == "A":
        return pc.make_graph(145, [(k, k - 10) for k in range(12, 141)], seed=51), cur
    if name == "A2":
        return pc.make_graph(165, [(k, k - 10) for k in range(12, 141)], seed=56), cur
    if name == "B":
        return pc.make_graph(215, [(k, k - 60) for k in range(62, 212)], seed=52), cur
    if name == "C":
        return pc.make_graph(300, [(k, k - 40) for k in range(41, 298)], seed=53), cur
    if name == "D":
        return pc.make_graph(185, [(k, 3) for k in range(5, 40)] + [(k, k - 35) + (FAR if k % 17 == 0 else ()) for k in range(40, 180)], seed=54), cur
    if name == "E":
        return pc.make_graph(1100, [(k, k - 70) for k in range(72, 1096)], seed=55), cur
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def optimized_many(name):
    """the restatement's pass: (graph after, Result)"""
    g, cur = graph_many(name)
    return g.optimize(cur)


@functools.lru_cache(maxsize=None)
def forced_many():
    """the restatement's pass over A with FORCED_MANY: (graph after, Result)"""
    g, cur = graph_many("A")
    return g.optimize(cur, fail_mask=FORCED_MANY[0], max_num_iterations=FORCED_MANY[1])


@functools.lru_cache(maxsize=None)
def forced_many_radius():
    """the radius the restatement forms the LAST linear system of forced_many()'s pass with. Result.solve_radius is a read-back, clamp(A00) / (lhs00 - A00), with A00
    taken at the point the restatement believes the system was formed at; when the last step of a pass is ACCEPTED and the pass ends on the iteration limit -- as in
    forced_many(): 8 iterations, 6 successful -- that point is one evaluation ahead and the read-back is not the radius (100067.29... there; the same read-back gives
    11837.0 for the FIRST system of a plain one-iteration pass over A, which is formed at 1e4 by construction). Refusing that last solve as well leaves the
    first max_it - 1 iterations, and so the radius of the last system, as they are, and makes the read-back valid: 303750.0000029 = 1e4 / 2 / 4 x 3^5."""
    g, cur = graph_many("A")
    mask, max_it = FORCED_MANY
    _, res = g.optimize(cur, fail_mask=mask | (1 << (max_it - 1)), max_num_iterations=max_it)
    assert res.num_iterations == max_it and res.n_refused == bin(mask).count("1") + 1
    return res.solve_radius


@functools.lru_cache(maxsize=None)
def restated_step(name):
    g, cur = graph_many(name)
    return g.solve_step(cur, pc.STEP_RADIUS)


@functools.lru_cache(maxsize=None)
def edges(name):
    """the RESTATEMENT's edges (no dense H): dict(ij, r, Ji, Jj, cost) and is_loop (E,)"""
    g, cur = graph_many(name)
    lin = g.linearize(cur, dense=False)
    ij = lin["ij"]
    is_loop, pos = np.zeros(len(ij), bool), {}
    for e, (i, j) in enumerate(ij):                       # per keyframe j: its sequential edges to j - 1 .. j - 4 (those that exist), then its loop edge
        pos[int(j)] = pos.get(int(j), 0) + 1
        is_loop[e] = pos[int(j)] > min(int(j), 4)
        assert not is_loop[e] or g.loop_index[g.earliest + j] == g.earliest + i
    lin["is_loop"] = is_loop
    return lin


def _jacobian(lin, n, mask):
    """the sparse Jacobian (6 E', n) of the edges in mask over the free blocks (local keyframe k >= 1 is block k - 1) and their residuals"""
    idx = np.nonzero(mask)[0]
    rows, cols, vals = [], [], []
    a, c = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    for q, e in enumerate(idx):
        for blk, J in ((lin["ij"][e][0] - 1, lin["Ji"][e]), (lin["ij"][e][1] - 1, lin["Jj"][e])):
            if blk < 0:
                continue
            rows.append((6 * q + a).ravel())
            cols.append((6 * blk + c).ravel())
            vals.append(J.ravel())
    J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * len(idx), n))
    return J, lin["r"][idx].ravel()


@functools.lru_cache(maxsize=None)
def sparse_step(name, radius=pc.STEP_RADIUS):
    """H = J^T J, g = J^T r, S = 1 / (1 + sqrt(diag H)), A = S H S + clip(diag(S H S), 1e-6, 1e32) / radius, by a sparse LU: dict(step, delta)"""
    g, cur = graph_many(name)
    n = 6 * (cur - g.earliest)
    lin = edges(name)
    J, r = _jacobian(lin, n, np.ones(len(lin["ij"]), bool))
    H = (J.T @ J).tocsc()
    gv = J.T @ r
    S = 1.0 / (1.0 + np.sqrt(H.diagonal()))
    Sd = sp.diags(S)
    A = (Sd @ H @ Sd).tocsc()
    A = (A + sp.diags(np.clip(A.diagonal(), 1e-6, 1e32) / radius)).tocsc()
    y = spla.splu(A).solve(S * gv)
    return dict(step=-y, delta=-y * S)


@functools.lru_cache(maxsize=None)
def lowrank_step(name, radius=pc.STEP_RADIUS):
    """what the device computes, in NumPy: A = B + W^T W with B = S H_seq S + D / radius (a band of half-width 29) and W the loop edges' corrected Jacobians times S;
    B = L L^T (banded Cholesky), [Y | y_b] = L^-1 [W^T | S g], C = I + Y^T Y, C z = Y^T y_b (dense Cholesky), L^T x = y_b - Y z: dict(step, delta, cond_C)"""
    g, cur = graph_many(name)
    n = 6 * (cur - g.earliest)
    lin = edges(name)
    loop = lin["is_loop"]
    Jl, rl = _jacobian(lin, n, loop)
    Js, rs = _jacobian(lin, n, ~loop)
    Hs = (Js.T @ Js).tocsc()
    hd = Hs.diagonal() + np.asarray(Jl.multiply(Jl).sum(axis=0)).ravel()
    gv = Js.T @ rs + Jl.T @ rl
    S = 1.0 / (1.0 + np.sqrt(hd))
    D = np.clip(S * hd * S, 1e-6, 1e32)
    Sd = sp.diags(S)
    B = (Sd @ Hs @ Sd + sp.diags(D / radius)).todia()
    bw = 29
    ab = np.zeros((bw + 1, n))
    for off, data in zip(B.offsets, B.data):
        if 0 <= off <= bw:
            ab[bw - off, off:] = data[off:n]            # upper form: ab[bw + i - j, j] = B[i, j], i <= j
        else:
            assert off < 0 or np.abs(data[off:n]).max() == 0.0, off
    cb = scipy.linalg.cholesky_banded(ab, lower=False)
    # L^-1 v with L = U^T: solve_banded on the transposed (lower) band
    lb = np.zeros((bw + 1, n))
    for d in range(bw + 1):
        lb[d, :n - d] = cb[bw - d, d:]
    W = (Jl @ Sd).toarray()
    rhs = np.concatenate([W.T, (S * gv)[:, None]], axis=1)
    Yb = scipy.linalg.solve_banded((bw, 0), lb, rhs)
    Y, yb = Yb[:, :-1], Yb[:, -1]
    C = np.eye(Y.shape[1]) + Y.T @ Y
    cf = scipy.linalg.cho_factor(C, lower=True)
    z = scipy.linalg.cho_solve(cf, Y.T @ yb)
    ub = cb                                               # L^T = U, upper band
    x = scipy.linalg.solve_banded((0, bw), ub, yb - Y @ z)
    d = np.diag(cf[0])
    return dict(step=-x, delta=-x * S, cond_C_lower_bound=float((d.max() / d.min()) ** 2))


def rel(got, want):
    """the largest difference as a fraction of the largest entry of `want`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
