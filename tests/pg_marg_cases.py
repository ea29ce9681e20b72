"""Oracles for the pose graph's marginal covariances (row f18), shared by tests/test_pg_marg_cases.py (CPU) and tests/test_gpu_pg_marginals.py (GPU): the matrix H
of the undamped problem assembled from the restatement's edges (tests/host/pg_ref.cpp through pg_cases / pg_many_cases), its 6 x 6 diagonal inverse blocks by three
float64 routes that share no code with the device -- NumPy's inv, a dense Cholesky solve, a sparse LU (the only affordable one on graph E) -- and a NumPy
transcription of what the device does: band + low-rank (Woodbury), a block Takahashi recursion for the band's selected inverse, Z = L^-T Y and Q = L_c^-1 Z^T.
Block 0 (the constant keyframe `first`) is zero in every route: the gauge. Computed once per process and shared: do not modify what these functions return."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pg_cases as pc
import pg_many_cases as pm

BAR_ORACLE = 1e-10                # the float64 routes against each other, per block: 20 x the 4.6e-12 measured when the row was proposed
BAR_DEVICE = 1e-9                 # the project's bar for linear work: the device against the oracle, per block
CPU_CASES = ("L1", "L3", "L24", "M130", "A", "D", "C")
LINEARIZE = {"lin1": 1, "lin4": 4, "lin5": 5, "lin69": 69}


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """(graph, cur) by the name the tests use"""
    if name in LINEARIZE:
        return pc.graph_linearize(), LINEARIZE[name]
    if name in pc.STEP_CASES:
        return pc.graph_step(name)
    if name in pm.MANY:
        return pm.graph_many(name)
    if name == "converge":
        return pc.graph_optimize("converge")
    raise KeyError(name)


def edges_of(g, cur):
    """the restatement's edges of first..cur at g's poses: dict(ij, r, Ji, Jj, cost, is_loop)"""
    lin = g.linearize(cur, dense=False)
    ij = lin["ij"]
    is_loop, pos = np.zeros(len(ij), bool), {}
    for e, (i, j) in enumerate(ij):                       # per keyframe j: its sequential edges to j - 1 .. j - 4 (those that exist), then its loop edge
        pos[int(j)] = pos.get(int(j), 0) + 1
        is_loop[e] = pos[int(j)] > min(int(j), 4)
    lin["is_loop"] = is_loop
    return lin


def hessian(g, cur):
    """(H sparse csc (n, n), lin, n): H = J^T J over the free blocks, loop edges Huber-corrected, no damping, no scaling"""
    n = 6 * (cur - g.earliest)
    lin = edges_of(g, cur)
    if n == 0:
        return sp.csc_matrix((0, 0)), lin, 0
    J, _ = pm._jacobian(lin, n, np.ones(len(lin["ij"]), bool))
    return (J.T @ J).tocsc(), lin, n


def _with_gauge(blocks):
    return np.concatenate([np.zeros((1, 6, 6)), blocks], axis=0)


def _diag_blocks(X):
    nb = X.shape[0] // 6
    return np.array([X[6 * b:6 * b + 6, 6 * b:6 * b + 6] for b in range(nb)]).reshape(nb, 6, 6)


def blocks_inv(g, cur):
    """(M, 6, 6) by numpy.linalg.inv of the dense H"""
    H, _, n = hessian(g, cur)
    return _with_gauge(_diag_blocks(np.linalg.inv(H.toarray()))) if n else np.zeros((1, 6, 6))


def blocks_chol(g, cur):
    """(M, 6, 6) by a dense Cholesky factorisation and a solve against the identity"""
    H, _, n = hessian(g, cur)
    if not n:
        return np.zeros((1, 6, 6))
    cf = scipy.linalg.cho_factor(H.toarray(), lower=True)
    return _with_gauge(_diag_blocks(scipy.linalg.cho_solve(cf, np.eye(n))))


def blocks_sparse(g, cur, sample=None):
    """by a sparse LU of H: {local keyframe index k >= 1: (6, 6)} for k in sample (None: every free keyframe, as an (M, 6, 6) array with the gauge block)"""
    H, _, n = hessian(g, cur)
    lu = spla.splu(H)
    ks = range(1, n // 6 + 1) if sample is None else sample
    out = {}
    for k in ks:
        E = np.zeros((n, 6))
        E[6 * (k - 1):6 * k] = np.eye(6)
        out[k] = lu.solve(E)[6 * (k - 1):6 * k]
    if sample is None:
        return _with_gauge(np.array([out[k] for k in ks]).reshape(-1, 6, 6))
    return out


def _L_block(cb, bw, i, j):
    """block (i, j), i >= j, of L from scipy's cholesky_banded (upper form: cb[bw + c - r, r] = U[c][r] = L[r][c])"""
    r = 6 * i + np.arange(6)[:, None]
    c = 6 * j + np.arange(6)[None, :]
    ok = (r >= c) & (r - c <= bw)
    return np.where(ok, cb[np.clip(bw + c - r, 0, bw), r + 0 * c], 0.0)


def blocks_lowrank(g, cur, sample=None):
    """the device's route in NumPy. H = B + W^T W, B the sequential edges' band (half-width 29), W the loop edges' corrected Jacobians; B = L L^T; Y = L^-1 W^T;
    C = I + Y^T Y = L_c L_c^T; Z = L^-T Y; Q = L_c^-1 Z^T; block b of H^-1 = [B^-1]_bb - Q_b^T Q_b, with [B^-1]_bb from Takahashi's recursion over 6 x 6 blocks
    (Sigma_ij = -sum_k Sigma_ik G_kj, Sigma_jj = L_jj^-T L_jj^-1 - sum_k Sigma_jk G_kj, G_kj = L_kj L_jj^-1, k = j + 1 .. j + 4), from the last block column to the
    first. -> (M, 6, 6), or {k: block} for k in sample; also the cancellation max diag(B^-1) / max diag(H^-1) as the second value"""
    n = 6 * (cur - g.earliest)
    if n == 0:
        return np.zeros((1, 6, 6)), 1.0
    lin = edges_of(g, cur)
    loop = lin["is_loop"]
    Js, _ = pm._jacobian(lin, n, ~loop)
    B = (Js.T @ Js).todia()
    bw = 29
    ab = np.zeros((bw + 1, n))
    for off, data in zip(B.offsets, B.data):
        if 0 <= off <= bw:
            ab[bw - off, off:] = data[off:n]
        else:
            assert off < 0 or np.abs(data[off:n]).max() == 0.0, off
    cb = scipy.linalg.cholesky_banded(ab, lower=False)
    NB = n // 6
    # Takahashi over blocks; S[(i, k)] for |i - k| <= 4, both triangles
    S, diag = {}, np.zeros((NB, 6, 6))
    for j in range(NB - 1, -1, -1):
        Ljj_inv = np.linalg.inv(_L_block(cb, bw, j, j))
        ks = [k for k in range(j + 1, min(j + 5, NB))]
        G = {k: _L_block(cb, bw, k, j) @ Ljj_inv for k in ks}
        for i in ks:
            Sij = -sum(S[(i, k)] @ G[k] for k in ks)
            S[(i, j)], S[(j, i)] = Sij, Sij.T
        Sjj = Ljj_inv.T @ Ljj_inv
        for k in ks:
            Sjj = Sjj - S[(j, k)] @ G[k]
        Sjj = np.tril(Sjj) + np.tril(Sjj, -1).T
        S[(j, j)] = Sjj
        diag[j] = Sjj
        for key in [key for key in S if max(key) > j + 4]:
            del S[key]
    want = range(1, NB + 1) if sample is None else sample
    if loop.any():
        Jl, _ = pm._jacobian(lin, n, loop)
        lb = np.zeros((bw + 1, n))
        for d in range(bw + 1):
            lb[d, :n - d] = cb[bw - d, d:]
        Y = scipy.linalg.solve_banded((bw, 0), lb, Jl.T.toarray(), overwrite_b=True)
        C = Y.T @ Y
        C[np.diag_indices_from(C)] += 1.0
        Lc = scipy.linalg.cholesky(C, lower=True)
        del C
        Z = scipy.linalg.solve_banded((0, bw), cb, Y, overwrite_b=True)
        corr = {}
        for k in want:
            Qb = scipy.linalg.solve_triangular(Lc, Z[6 * (k - 1):6 * k].T, lower=True)
            corr[k] = Qb.T @ Qb
    else:
        corr = {k: np.zeros((6, 6)) for k in want}
    blocks = {k: diag[k - 1] - corr[k] for k in want}
    cancel = float(max(np.diag(diag[k - 1]).max() for k in want) / max(np.diag(blocks[k]).max() for k in want))
    if sample is None:
        return _with_gauge(np.array([blocks[k] for k in want]).reshape(-1, 6, 6)), cancel
    return blocks, cancel


def block_rel(got, want):
    """the largest difference of one block as a fraction of the reference block's largest entry"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (6, 6)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def worst_rel(got, want):
    """the worst block_rel over keyframes 1 .. M - 1 of two (M, 6, 6) arrays"""
    assert got.shape == want.shape
    return max([block_rel(a, b) for a, b in zip(got[1:], want[1:])], default=0.0)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(M, 6, 6): the reference the device is held to on the crafted graph `name` at the graph's own poses: inv of the dense H (its agreement with the Cholesky route
    and with the transcription is tests/test_pg_marg_cases.py's business)"""
    g, cur = graph_of(name)
    return blocks_inv(g, cur)


def sample_E():
    """at least 32 local keyframe indices of E: the first and last free blocks, both ends of a loop, a block next to the constant one, and a spread"""
    g, cur = pm.graph_many("E")
    M = cur - g.earliest + 1
    j = int(np.nonzero(g.loop_index >= 0)[0][1])          # the second looped keyframe and the keyframe it closes onto (the first closes onto the constant block)
    ends = [j - g.earliest, int(g.loop_index[j]) - g.earliest]
    jl = int(np.nonzero(g.loop_index >= 0)[0][-1])
    ends += [jl - g.earliest, int(g.loop_index[jl]) - g.earliest]
    spread = [int(v) for v in np.linspace(3, M - 3, 32)]
    ks = sorted(set([1, 2, M - 1] + ends + spread))
    assert len(ks) >= 32 and min(ks) >= 1 and max(ks) == M - 1
    return tuple(ks)


@functools.lru_cache(maxsize=None)
def oracle_E():
    """{k: block} for sample_E() by the sparse LU"""
    g, cur = pm.graph_many("E")
    return blocks_sparse(g, cur, sample_E())


def store_A(t):
    """A of xi = A delta: rows [rho, phi], columns [rotation, translation] (csrc/pg_marg_host.hpp has the derivation)"""
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    A = np.zeros((6, 6))
    A[:3, :3], A[:3, 3:], A[3:, :3] = 2.0 * tx, np.eye(3), 2.0 * np.eye(3)
    return A
