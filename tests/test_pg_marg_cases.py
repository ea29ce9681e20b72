"""The CPU side of the pose graph's marginal covariances (row f18; no GPU): that the oracle tests/test_gpu_pg_marginals.py holds the device to stands on its own
feet -- three float64 routes to the 6 x 6 diagonal blocks of H^-1 that share only the restatement's edges agree per block within 1e-10 on the crafted graphs, and
so does the NumPy transcription of the device's band + low-rank route (Woodbury, Takahashi's selected inversion); on E, where nothing dense is affordable, the
transcription against a sparse LU on a sample of keyframes --, that the conversion matrix A to the keyframe store's convention is the first-order map it is
derived as, and the host side of the device's plan replayed by a stand-alone program under AddressSanitizer and UBSan.

Measured here (per block, relative to the block's largest entry): inv against the Cholesky route 2.3e-15 (L1), 8.1e-15 (L3), 2.5e-14 (L24), 2.2e-13 (M130),
7.2e-13 (A), 1.6e-13 (D), 1.3e-12 (C); the transcription against inv 6.7e-15, 1.2e-14, 3.2e-14, 1.8e-13, 6.9e-13, 1.9e-13, 7.3e-13; on E against the sparse LU
2.3e-12 over 37 keyframes. cond(H) runs from 2.7e4 (L1) to 4.3e7 (C). The subtraction's cancellation, max diag(B^-1) / max diag(H^-1), is 40.4 on D and 61.5 on
E's sample."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import pg_cases as pc
import pg_many_cases as pm
import pg_marg_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", mc.CPU_CASES)
def test_three_routes_agree_per_block(name):
    """(a): inv, the Cholesky solve and the band + low-rank transcription, per block within 1e-10 of the block's largest entry"""
    g, cur = mc.graph_of(name)
    a, b = mc.oracle(name), mc.blocks_chol(g, cur)
    c, cancel = mc.blocks_lowrank(g, cur)
    H, _, n = mc.hessian(g, cur)
    d_chol, d_low = mc.worst_rel(b, a), mc.worst_rel(c, a)
    print(f"PG_MARG oracle {name}: n {n} cond(H) {np.linalg.cond(H.toarray()):.2e} inv vs chol {d_chol:.3e} lowrank vs inv {d_low:.3e} cancellation {cancel:.1f}")
    assert a.shape == (cur - g.earliest + 1, 6, 6) and not a[0].any() and not c[0].any()
    assert d_chol <= mc.BAR_ORACLE and d_low <= mc.BAR_ORACLE
    for blk in a[1:]:
        assert np.linalg.eigvalsh(0.5 * (blk + blk.T)).min() > 0.0


def test_transcription_against_the_sparse_lu_at_the_limit():
    """(b): E (L = 1024, n = 6576): a sparse LU gives the blocks of at least 32 keyframes -- the first and last free blocks, both ends of a loop, a block next to the
    constant one -- and the transcription agrees within the same bar"""
    g, cur = pm.graph_many("E")
    ks = mc.sample_E()
    M = cur - g.earliest + 1
    assert len(ks) >= 32 and 1 in ks and M - 1 in ks and 6 * (M - 1) == 6576
    j = int(np.nonzero(g.loop_index >= 0)[0][1])
    assert j - g.earliest in ks and int(g.loop_index[j]) - g.earliest in ks
    want = mc.oracle_E()
    got, cancel = mc.blocks_lowrank(g, cur, ks)
    worst = max(mc.block_rel(got[k], want[k]) for k in ks)
    print(f"PG_MARG oracle E: {len(ks)} keyframes, lowrank vs sparse LU {worst:.3e} cancellation {cancel:.1f}")
    assert worst <= mc.BAR_ORACLE


def _left_perturbed(x, xi):
    """exp(xi^) T for T = x [t, q(xyzw)] and xi = [rho, phi]: the SE(3) exponential in closed form"""
    rho, phi = xi[:3], xi[3:]
    th = np.linalg.norm(phi)
    K = np.array([[0.0, -phi[2], phi[1]], [phi[2], 0.0, -phi[0]], [-phi[1], phi[0], 0.0]])
    V = np.eye(3) + (1.0 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    R = Rot.from_rotvec(phi)
    return np.concatenate([R.apply(x[:3]) + V @ rho, (R * Rot.from_quat(x[3:])).as_quat()])


def test_a_is_the_first_order_map_from_plus_to_the_left_perturbation():
    """(c): pc.plus(x, delta) against exp((A delta)^) T. The rotations agree to rounding (Plus IS the left turn exp(2 d_r)); the translations differ by the
    second-order term of the exponential, exp(phi^) t + V(phi) rho - (t + phi x t + rho) = phi x (phi x t) / 2 + phi x rho / 2 + O(3). With |phi| = 2 |d_r| <= 2 |delta|
    and |rho| <= |d_t| + |phi| |t| <= |delta| (1 + 2 |t|) that is at most |delta|^2 (2 |t| + (1 + 2 |t|)) = |delta|^2 (1 + 4 |t|); the bound below adds 1 % for the
    third-order terms (|delta| = 1e-4) and 1e-14 (1 + |t|) for rounding. Halving |delta| quarters the difference."""
    rng = np.random.default_rng(18)
    for trial in range(40):
        t = rng.normal(size=3) * rng.choice([0.5, 10.0, 80.0])
        x = np.concatenate([t, Rot.from_rotvec(rng.normal(size=3)).as_quat()])
        d = rng.normal(size=6)
        A = mc.store_A(t)
        diffs = []
        for scale in (1e-4, 0.5e-4):
            delta = d / np.linalg.norm(d) * scale
            a, b = pc.plus(x, delta), _left_perturbed(x, A @ delta)
            dq = min(np.abs(a[3:] - b[3:]).max(), np.abs(a[3:] + b[3:]).max())
            dt = float(np.linalg.norm(a[:3] - b[:3]))
            bound = 1.01 * scale ** 2 * (1.0 + 4.0 * np.linalg.norm(t)) + 1e-14 * (1.0 + np.linalg.norm(t))
            assert dq <= 1e-15 * 8 and dt <= bound, (trial, scale, dq, dt, bound)
            diffs.append(dt)
        # a first-order mistake in A (a sign, a factor 2) leaves a difference of order |delta| |t|: four orders above the bound
        if diffs[1] > 1e-11 * (1.0 + np.linalg.norm(t)):
            assert 3.9 <= diffs[0] / diffs[1] <= 4.1, (trial, diffs)
    # and the bound is no formality: A with the translation's sign flipped misses it
    t = np.array([3.0, -4.0, 1.0])
    x = np.concatenate([t, Rot.from_rotvec([0.3, -0.2, 0.5]).as_quat()])
    delta = np.array([1.0, 2.0, -1.0, 0.5, 0.5, 1.0])
    delta *= 1e-4 / np.linalg.norm(delta)
    wrong = mc.store_A(-t)
    assert np.linalg.norm(pc.plus(x, delta)[:3] - _left_perturbed(x, wrong @ delta)[:3]) > 1e-5


def test_header_binding_and_host_header_agree(mla):
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    assert int(re.search(r"MLH_PG_COV_LOCAL\s*=\s*(\d+)", hdr).group(1)) == mla.PG_COV_LOCAL
    assert int(re.search(r"MLH_PG_COV_STORE\s*=\s*(\d+)", hdr).group(1)) == mla.PG_COV_STORE
    assert int(re.search(r"MLH_KF_COV_RELATIVE\s*=\s*(\d+)", hdr).group(1)) == mla.KF_COV_RELATIVE
    assert int(re.search(r"MLH_KF_COV_ABSOLUTE\s*=\s*(\d+)", hdr).group(1)) == mla.KF_COV_ABSOLUTE
    for sym in ("mlh_pg_marginals", "mlh_pg_device_marginals", "mlh_keyframes_update_from_pose_graph_cov"):
        assert sym in mla.EXPORTED_SYMBOLS
    assert callable(mla.Context.pg_marginals) and callable(mla.Context.keyframes_update_from_pose_graph_cov)
    # the Python A and the header's are one matrix: checked through the stand-alone program's conversion test and the GPU's store form


def _marg_main(tmp_path):
    exe = tmp_path / "pg_marg_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pg_marg_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


def launches_of_marginals(M, L):
    """what mlh_pg_marginals_result::launches reports: begin (3), assemble, unit scaling, band factor, substitution, Gram, the dense stage (1, or 3 ceil(6 L / 64)
    beyond 128 loops), factor pack, selected inversion, Z, Q, tail; M == 1: begin and the tail"""
    if M <= 1:
        return 4
    return 13 + (1 if L <= pm.CAP_DEFAULT else 3 * -(-6 * L // pm.PANEL))


def test_host_plan_under_sanitizers(tmp_path):
    """(d): pg_marg_host.hpp in a stand-alone program built with -fsanitize=address,undefined and run directly (nothing is loaded into Python): the launch count for
    every L up to the limit, the buffer sizes, the selected inversion's window indexing for NB = 1 .. 12 on real numbers, the conversion"""
    exe = _marg_main(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pg_marg: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    for M, L in ((1, 0), (2, 1), (21, 1), (130, 5), (142, 129), (162, 129), (298, 257), (1097, 1024)):
        r = subprocess.run([exe, "count", str(M), str(L)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "pg_marg: ok" in r.stdout, (r.stdout, r.stderr[-3000:])
        n, out, band, factor, work = (int(v) for v in r.stdout.split("\n")[0].split()[1:])
        mp = -(-6 * L // pm.PANEL) * pm.PANEL
        assert n == launches_of_marginals(M, L)
        assert (out, band, factor) == (72 * M, 180 * (M - 1), mp * mp if L <= pm.CAP_DEFAULT else 0) and band + factor <= work <= band + factor + 32
