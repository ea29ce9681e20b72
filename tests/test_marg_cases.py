"""The NumPy restatement of the window prior (tests/marg_cases.py) held by things that do not share its structure, and the condition under which two correct
eigen-solvers cannot disagree on which eigenvalues are `> 1e-8`. CPU only; tests/test_gpu_window_prior.py compares the device against this restatement."""
import numpy as np
import pytest

import marg_cases as mc


def _svd_pinv_abs(M, eps):
    U, s, Vt = np.linalg.svd(M)
    return (Vt.T * np.where(s > eps, 1.0 / np.where(s > eps, s, 1.0), 0.0)) @ U.T


@pytest.mark.parametrize("name", list(mc.SHAPES))
def test_restatement_is_a_marginal(orc, name):
    w = mc.shape_window(name)
    m = mc.marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
    A, b = m["A"], m["b"]
    n = A.shape[0] - 6
    # (a) J0^T J0 is the thresholded Schur complement -- the complement formed through an SVD pseudo-inverse, thresholded through an SVD
    S = A[6:, 6:] - A[6:, :6] @ _svd_pinv_abs(0.5 * (A[:6, :6] + A[:6, :6].T), mc.EPS) @ A[:6, 6:]
    U, s, Vt = np.linalg.svd(0.5 * (S + S.T))
    S_thr = (U * np.where(s > mc.EPS, s, 0.0)) @ Vt
    sc = np.abs(S).max()
    assert np.abs(m["J0"].T @ m["J0"] - S_thr).max() <= 1e-9 * sc
    assert m["J0"].shape == (n, n) and m["r0"].shape == (n,)
    # (b) the definition of a marginal: over random dx on the kept blocks, min over the pivot's 6 parameters of the FULL quadratic 0.5 x^T A x + b^T x
    # equals 0.5 |r0 + J0 dx|^2 up to a constant that does not depend on dx
    rng = np.random.default_rng(5)
    diffs = []
    for _ in range(6):
        dx = rng.normal(size=n) * 0.05
        xm = np.linalg.lstsq(A[:6, :6], -(A[:6, 6:] @ dx + b[:6]), rcond=None)[0]
        x = np.concatenate([xm, dx])
        full = 0.5 * x @ A @ x + b @ x
        r = m["r0"] + m["J0"] @ dx
        diffs.append(full - 0.5 * r @ r)
    spread = max(diffs) - min(diffs)
    assert spread <= 1e-7 * max(1.0, abs(0.5 * float(m["r0"] @ m["r0"])), sc * 0.05 ** 2), (spread, diffs)


def test_thresholding_is_exercised(orc):
    w = mc.shape_window("1x1")
    m = mc.marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
    assert 0 < m["kept_rr"] < 12                                # the gauge is dropped
    w = mc.shape_window("rank_deficient")
    m = mc.marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
    assert m["kept_mm"] == 3                                    # planes with one normal: the pivot block has rank 3


def test_no_eigenvalue_near_the_threshold(orc):
    """(c) for every matrix the GPU tests decompose, no eigenvalue lies in [1e-10, 1e-6]: the `> 1e-8` decision cannot differ between two correct solvers"""
    for label, lam in mc.decomposed_spectra(orc):
        bad = lam[(lam >= 1e-10) & (lam <= 1e-6)]
        assert bad.size == 0, (label, bad)


def test_chain_prior_changes_the_solution():
    """from window 1 on the prior moves the solve: otherwise the chain test on the GPU would be vacuous"""
    for nf, ne in mc.CHAIN_SHAPES:
        with_p = mc.chain_reference(nf, ne)
        assert with_p[0][3] is not None
        # each window is solved once more from the SAME start without its prior
        import oracle as orc
        ci = mc.chain_inputs(nf, ne)
        for k in range(1, mc.CHAIN_WINDOWS):
            pivot, fr_with, ex_with, _ = with_p[k]
            frames0 = np.vstack([with_p[k - 1][1][1:], ci["windows"][k]["new_frame"][None, :]])
            fr_no, ex_no = mc.gn_solve(orc, ci["windows"][k], pivot, frames0, with_p[k - 1][2], 5, (0, 1 + nf), None)
            d = max(np.abs(fr_no - fr_with).max(), np.abs(ex_no - ex_with).max())
            assert d > 1e-5, (nf, ne, k, d)


def test_evaluate_sign_flip():
    """the relative quaternion with negative w: dx's rotation part changes sign (marginalization_factor.cpp:383-386)"""
    x0 = np.array([[0.0, 0, 0, 0, 0, 0, 1.0]])
    prior = dict(block_ids=np.array([1]), x0=x0, J0=np.eye(6), r0=np.zeros(6))
    q = mc.rotvec_quat(np.array([0.0, 0.0, 0.2]))
    pivot = np.array([0.0, 0, 0, 0, 0, 0, 1])
    a = mc.prior_evaluate(prior, pivot, np.array([[1.0, 2, 3, *q]]), np.zeros((0, 7)))["residuals"]
    b = mc.prior_evaluate(prior, pivot, np.array([[1.0, 2, 3, *(-q)]]), np.zeros((0, 7)))["residuals"]
    np.testing.assert_allclose(a, b, atol=1e-15)
    assert a[5] > 0.19
