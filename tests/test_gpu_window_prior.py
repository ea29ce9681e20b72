"""The odometry window's marginalisation prior on the device (m-loam_amd/csrc/marg.hip; mlh_window_prior_*, mlh_window_ext_prior_set, mlh_window_marginalize and
the prior's term inside mlh_pure_odom_gn_solve) against the f64 NumPy restatement of the reference's lines in tests/marg_cases.py, which tests/test_marg_cases.py
holds on the CPU.

linearized_jacobians is unique only up to the order and sign of its rows, so priors are compared on J0^T J0 and J0^T r0: <= 1e-9 of the largest entry of the
restatement's (the bound the project uses for normal equations), and the counts of kept eigenvalues must be equal (tests/test_marg_cases.py shows that no
eigenvalue of any matrix decomposed here lies near the 1e-8 threshold)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import marg_cases as mc

pytestmark = pytest.mark.gpu

ERR_STATE, ERR_UNSUPPORTED = -3, -5


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _stage(ctx, w):
    ctx.pure_odom_set(w["types"], w["points"], w["coeffs"], w["fi"], w["ei"])


def _same_prior(got, ref, label=""):
    """the comparison rule"""
    JtJ_g, JtJ_r = got["J0"].T @ got["J0"], ref["J0"].T @ ref["J0"]
    Jtr_g, Jtr_r = got["J0"].T @ got["r0"], ref["J0"].T @ ref["r0"]
    e_h, e_g = np.abs(JtJ_g - JtJ_r).max() / np.abs(JtJ_r).max(), np.abs(Jtr_g - Jtr_r).max() / np.abs(Jtr_r).max()
    print(f"{label}: J0^T J0 {e_h:.2e}, J0^T r0 {e_g:.2e}, kept {got['info']['kept_mm']}/{got['info']['kept_rr']} (ref {ref['kept_mm']}/{ref['kept_rr']}), "
          f"sweeps {got['info']['sweeps_mm']}/{got['info']['sweeps_rr']}")
    assert e_h <= 1e-9 and e_g <= 1e-9, (label, e_h, e_g)
    assert got["info"]["kept_mm"] == ref["kept_mm"] and got["info"]["kept_rr"] == ref["kept_rr"], label
    assert np.array_equal(got["block_ids"], ref["block_ids"]), label                      # the slid map
    assert np.array_equal(got["x0"], ref["x0"]), label                                    # the call's poses


def _random_prior(rng, block_ids, poses):
    nk = len(block_ids)
    n = 6 * nk
    return dict(block_ids=np.asarray(block_ids, np.int32), x0=np.stack([mc.perturb(poses[b], rng, 0.05, 0.5) for b in block_ids]),
                J0=rng.normal(size=(n, n)) * rng.uniform(0.1, 20.0, size=(n, 1)), r0=rng.normal(size=n))


@pytest.mark.parametrize("name", ["1x1", "1x4", "3x2"])
def test_prior_set_get_evaluate(ctx, name):
    """1. mlh_window_prior_set -> _get returns the same bits; mlh_window_prior_evaluate = MarginalizationFactor::Evaluate at three states, one of them with a
    relative quaternion of negative w (the sign flip of marginalization_factor.cpp:383-386 as written)"""
    w = mc.shape_window(name)
    nf, ne = w["n_frames"], w["n_ext"]
    rng = np.random.default_rng(3)
    poses = np.vstack([w["pivot"][None, :], w["frames_gt"], w["exts_gt"]])
    ids = list(range(1, 1 + nf + ne))[::-1]                                                 # every frame and extrinsic, in an order of the caller's
    prior = _random_prior(rng, ids, poses)
    ctx.window_prior_set(prior["block_ids"], prior["x0"], prior["J0"], prior["r0"])
    back = ctx.window_prior_get()
    for k in ("block_ids", "x0", "J0", "r0"):
        assert np.array_equal(back[k], prior[k]), k
    assert back["info"]["valid"] == 1 and back["info"]["n_keep"] == len(ids) and back["info"]["n"] == 6 * len(ids)
    flipped = w["frames"].copy(); flipped[0, 3:] *= -1.0                                    # the same rotation; q0^-1 q has w < 0 for frame 0's block
    assert mc.qmul(mc.qinv(prior["x0"][ids.index(1)][3:]), flipped[0, 3:])[3] < 0 < mc.qmul(mc.qinv(prior["x0"][ids.index(1)][3:]), w["frames"][0, 3:])[3]
    states = [(w["pivot"], w["frames"], w["exts"]), (mc.perturb(w["pivot"], rng), w["frames_gt"], w["exts_gt"]), (w["pivot"], flipped, w["exts"])]
    res = []
    for i, (pv, fr, ex) in enumerate(states):
        got, ref = ctx.window_prior_evaluate(pv, fr, ex), mc.prior_evaluate(prior, pv, fr, ex)
        e_r = np.abs(got["residuals"] - ref["residuals"]).max() / np.abs(ref["residuals"]).max()
        e_h = np.abs(got["H"] - ref["H"]).max() / np.abs(ref["H"]).max()
        e_g = np.abs(got["g"] - ref["g"]).max() / np.abs(ref["g"]).max()
        print(f"{name} state {i}: residuals {e_r:.2e}, H {e_h:.2e}, g {e_g:.2e}, cost {abs(got['cost'] - ref['cost']) / ref['cost']:.2e}")
        assert e_r <= 1e-12 and e_h <= 1e-9 and e_g <= 1e-9 and abs(got["cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
        res.append(got["residuals"])
    assert np.abs(res[2] - res[0]).max() <= 1e-12 * np.abs(res[0]).max()                    # q and -q are one rotation: the flip makes the residuals agree
    ctx.window_prior_clear()
    assert ctx.window_prior_get() is None


@pytest.mark.parametrize("name", ["1x1", "1x4", "3x2"])
def test_marginalize_from_nothing(ctx, orc, name):
    """2. no prior installed: the table's factors alone"""
    w = mc.shape_window(name)
    ref = mc.marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
    _stage(ctx, w)
    info = ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    got = ctx.window_prior_get()
    assert info == got["info"] and info["valid"] == 1
    _same_prior(got, ref, name)
    nf, ne = w["n_frames"], w["n_ext"]
    assert list(got["block_ids"]) == list(range(nf)) + [1 + nf + e for e in range(ne)]
    assert np.array_equal(got["x0"], np.vstack([w["frames"], w["exts"]]))
    if name == "1x1":
        assert 0 < info["kept_rr"] < info["n"]                                             # the thresholding path is exercised (the gauge is dropped)
    assert info["min_kept_rr"] > 1e-6 and info["max_dropped_rr"] < 1e-10 and info["sweeps_rr"] > 0
    ctx.window_prior_clear()                                                                # the same call twice: identical bits
    ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    again = ctx.window_prior_get()
    for k in ("J0", "r0", "x0", "block_ids"):
        assert np.array_equal(again[k], got[k]), k


def test_marginalize_rank_deficient_pivot(ctx, orc):
    """3. plane factors with a single normal: Amm keeps 3 of its 6 eigenvalues on both sides"""
    w = mc.shape_window("rank_deficient")
    ref = mc.marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
    _stage(ctx, w)
    info = ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    assert info["kept_mm"] == 3 == ref["kept_mm"]
    _same_prior(ctx.window_prior_get(), ref, "rank_deficient")


@pytest.mark.parametrize("shape", mc.CHAIN_SHAPES)
def test_chain_of_windows(ctx, mla, orc, shape):
    """4. four windows: solve (5 iterations, pivot and extrinsic 0 constant) -> marginalise (extrinsic prior on, bit 0) -> slide -> new perturbed frame"""
    nf, ne = shape
    ci = mc.chain_inputs(nf, ne)
    ref = mc.chain_reference(nf, ne)
    ctx.window_ext_prior_set(ci["ext_rows"], in_marginalization=True, in_solve=False)
    bare = mla.Context(0)
    moved = []

    def solve(w, pivot, frames, exts):
        _stage(ctx, w)
        if ctx.window_prior_info()["valid"]:                  # the same solve without the prior, from the same start
            _stage(bare, w)
            b = bare.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=mc.HUBER)
            s = ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=mc.HUBER)
            moved.append(max(np.abs(b["frames"] - s["frames"]).max(), np.abs(b["exts"] - s["exts"]).max()))
        else:
            s = ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=mc.HUBER)
        assert s["status"] == 0
        return s["frames"], s["exts"]

    def marg(w, pivot, frames, exts):
        ctx.window_marginalize(pivot, frames, exts, mc.HUBER)
        return ctx.window_prior_get()

    try:
        got = mc.chain_run(nf, ne, solve, marg)
    finally:
        bare.close()
    for k, ((_, fr_g, ex_g, prior_g), (_, fr_r, ex_r, prior_r)) in enumerate(zip(got, ref)):
        d = max(np.abs(fr_g - fr_r).max(), np.abs(ex_g - ex_r).max())
        print(f"chain {nf}x{ne} window {k}: poses {d:.2e}")
        assert d < 1e-7, (k, d)                                                            # the project's pose bound
        # the restatement's prior was made at ITS poses (x0 differs by the pose error): compare the rest by the rule, x0 by the pose bound
        assert np.abs(prior_g["x0"] - prior_r["x0"]).max() < 1e-7
        _same_prior(dict(prior_g, x0=prior_r["x0"]), prior_r, f"chain {nf}x{ne} window {k}")
    print("with - without prior:", moved)
    assert len(moved) == mc.CHAIN_WINDOWS - 1 and min(moved) > 1e-5, moved                # not vacuous: the prior moves every solve after the first


def test_online_calibration_form(ctx, orc):
    """5. the extrinsic prior inside the solve (bit 1), 2 iterations at (1, 2) with only the pivot constant"""
    ci = mc.chain_inputs(1, 2)
    w, first = ci["windows"][0], ci["first"]
    ctx.window_ext_prior_set(ci["ext_rows"], in_marginalization=True, in_solve=True)
    _stage(ctx, w)
    got = ctx.pure_odom_gn_solve(first["pivot"], first["frames"], first["exts"], n_iters=2, huber_delta=mc.HUBER, const_blocks=[0])
    fr, ex = mc.gn_solve(orc, w, first["pivot"], first["frames"], first["exts"], 2, (0,), None, ci["ext_rows"])
    d = max(np.abs(got["frames"] - fr).max(), np.abs(got["exts"] - ex).max())
    print(f"online calibration form: {d:.2e}")
    assert got["status"] == 0 and d < 1e-9
    ctx.window_ext_prior_set(None)
    plain = ctx.pure_odom_gn_solve(first["pivot"], first["frames"], first["exts"], n_iters=2, huber_delta=mc.HUBER, const_blocks=[0])
    assert np.abs(plain["exts"] - got["exts"]).max() > 1e-6                                 # the rows were in the solve


def test_the_limit(ctx, mla, orc):
    """6. 11 frames + 10 extrinsics (22 blocks, D = 132, n = 126: the eigenvectors live in HBM); 23 blocks refused; a prior of another shape refused"""
    w = mc.shape_window("limit")
    ref = mc.marginalize_window(orc, w, w["pivot"], w["frames"], w["exts"])
    _stage(ctx, w)
    info = ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    assert info["n"] == 126
    got = ctx.window_prior_get()
    _same_prior(got, ref, "limit")
    # the new prior evaluated in the window it was slid into
    rng = np.random.default_rng(4)
    pv, fr, ex = w["frames"][0], np.stack([mc.perturb(p, rng) for p in np.vstack([w["frames"][1:], w["frames"][-1:]])]), np.stack([mc.perturb(p, rng) for p in w["exts"]])
    ev_g = ctx.window_prior_evaluate(pv, fr, ex)
    ev_r = mc.prior_evaluate(dict(ref, J0=got["J0"], r0=got["r0"]), pv, fr, ex)            # the device's own J0 (row order / signs are its own): Evaluate on it
    assert np.abs(ev_g["residuals"] - ev_r["residuals"]).max() <= 1e-12 * np.abs(ev_r["residuals"]).max()
    ev_ref = mc.prior_evaluate(ref, pv, fr, ex)                                             # ... and against the restatement's prior on H / g / cost
    assert np.abs(ev_g["H"] - ev_ref["H"]).max() <= 1e-9 * np.abs(ev_ref["H"]).max()
    assert np.abs(ev_g["g"] - ev_ref["g"]).max() <= 1e-9 * np.abs(ev_ref["g"]).max()
    assert abs(ev_g["cost"] - ev_ref["cost"]) <= 1e-9 * ev_ref["cost"]
    # 23 blocks
    lib, h = ctx.lib, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fr12 = np.ascontiguousarray(np.vstack([w["frames"], w["frames"][-1:]]))
    info_c = mla.WindowPriorInfo()
    assert lib.mlh_window_marginalize(h, p(w["pivot"]), p(fr12), 12, p(w["exts"]), 10, 1.0, C.byref(info_c)) == ERR_UNSUPPORTED
    # the installed prior is for (11, 10): a solve / marginalisation / evaluation of another shape is refused
    cost, n, st = C.c_double(0), C.c_int32(0), C.c_int32(0)
    fr10, ex10 = np.ascontiguousarray(w["frames"][:10].copy()), np.ascontiguousarray(w["exts"].copy())
    small = mc.shape_window("1x4")
    _stage(ctx, small)
    f1, e4 = np.ascontiguousarray(small["frames"].copy()), np.ascontiguousarray(small["exts"].copy())
    assert lib.mlh_pure_odom_gn_solve(h, p(small["pivot"]), p(f1), 1, p(e4), 4, 1.0, 2, 1 | (1 << 2), None, C.byref(cost), C.byref(n), C.byref(st)) == ERR_STATE
    assert b"prior" in lib.mlh_last_error(h)
    assert lib.mlh_window_marginalize(h, p(small["pivot"]), p(f1), 1, p(e4), 4, 1.0, C.byref(info_c)) == ERR_STATE
    assert lib.mlh_window_prior_evaluate(h, p(w["pivot"]), p(fr10), 10, p(ex10), 10, None, None, None, None) == ERR_STATE
    ctx.window_prior_clear()
    assert lib.mlh_pure_odom_gn_solve(h, p(small["pivot"]), p(f1), 1, p(e4), 4, 1.0, 2, 1 | (1 << 2), None, C.byref(cost), C.byref(n), C.byref(st)) == 0
    # a caller's prior that names a block the window does not have
    pr = _random_prior(rng, [0, 7], np.vstack([small["pivot"][None, :]] * 8))
    ctx.window_prior_set(pr["block_ids"], pr["x0"], pr["J0"], pr["r0"])
    assert lib.mlh_pure_odom_gn_solve(h, p(small["pivot"]), p(f1), 1, p(e4), 4, 1.0, 2, 1 | (1 << 2), None, C.byref(cost), C.byref(n), C.byref(st)) == ERR_STATE


def test_nothing_changes_without_a_prior(ctx, mla, orc):
    """7. after mlh_window_prior_clear the solve returns the bits of a fresh context; mlh_pure_odom_normal_eq never sees the prior"""
    w = mc.shape_window("3x2")
    fresh = mla.Context(0)
    try:
        _stage(fresh, w)
        want = fresh.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=4, huber_delta=mc.HUBER)
    finally:
        fresh.close()
    _stage(ctx, w)
    ne0 = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    ctx.window_ext_prior_set(np.hstack([w["exts_gt"], np.tile([5.0, 10.0], (2, 1))]), True, True)
    ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    assert ctx.window_prior_info()["valid"] == 1
    ne1 = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    for k in ("H", "g", "cost", "count"):
        assert np.array_equal(ne0[k], ne1[k]), k
    with_prior = ctx.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=4, huber_delta=mc.HUBER)
    ctx.window_prior_clear()
    ctx.window_ext_prior_set(None)
    got = ctx.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=4, huber_delta=mc.HUBER)
    for k in ("frames", "exts", "cost", "count", "status"):
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(with_prior["frames"], want["frames"])                         # (the prior had been in the solve in between)
    # an empty table and no prior: nothing touches the pivot, the prior is cleared (the reference's m == 0)
    ctx.pure_odom_begin()
    info = ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    assert info["valid"] == 0 and ctx.window_prior_get() is None


def test_marg_selftest_facade_equals_the_c_abi():
    """8. m-loam_amd/host/marg_selftest: four windows through the facade and through the plain calls end in the same poses and the same prior bits"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "marg_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/marg_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "window prior: facade equals the C-ABI" in r.stdout
