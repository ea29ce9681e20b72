"""The accumulated calibration features on the device (m-loam_amd/csrc/calib.hip; mlh_calib_* and their term inside mlh_pure_odom_normal_eq,
mlh_pure_odom_gn_solve and mlh_window_marginalize) against the reference's own LidarOnlineCalib lines and the f64 NumPy restatement of tests/calib_cases.py,
which tests/test_calib_cases.py holds on the CPU. Everything goes through the C-ABI.

Bounds: per-factor outputs as tests/test_abi.py has them for the same factors (residual 1e-12 max(1, |r|), Jacobian rtol = atol = 1e-11); normal equations
<= 1e-9 of the largest entry, the project's bound; poses of a solve < 1e-9, of a chain < 1e-7; priors by tests/test_gpu_window_prior.py's rule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import calib_cases as cc
import marg_cases as mc

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _stage(ctx, w):
    ctx.pure_odom_set(w["types"], w["points"], w["coeffs"], w["fi"], w["ei"])


def _add(ctx, cal, sqrt_info=None):
    ctx.calib_add(cal["types"], cal["points"], cal["coeffs"], cal["ei"], sqrt_info)


def _same_prior(got, ref, label=""):
    """tests/test_gpu_window_prior.py's rule"""
    JtJ_g, JtJ_r = got["J0"].T @ got["J0"], ref["J0"].T @ ref["J0"]
    Jtr_g, Jtr_r = got["J0"].T @ got["r0"], ref["J0"].T @ ref["r0"]
    e_h, e_g = np.abs(JtJ_g - JtJ_r).max() / np.abs(JtJ_r).max(), np.abs(Jtr_g - Jtr_r).max() / np.abs(Jtr_r).max()
    print(f"{label}: J0^T J0 {e_h:.2e}, J0^T r0 {e_g:.2e}, kept {got['info']['kept_mm']}/{got['info']['kept_rr']} (ref {ref['kept_mm']}/{ref['kept_rr']})")
    assert e_h <= 1e-9 and e_g <= 1e-9, (label, e_h, e_g)
    assert got["info"]["kept_mm"] == ref["kept_mm"] and got["info"]["kept_rr"] == ref["kept_rr"], label
    assert np.array_equal(got["block_ids"], ref["block_ids"]), label


def test_evaluate_is_the_references(ctx, orc):
    """1. mlh_calib_evaluate against LidarOnlineCalib{PlaneNorm,Edge}Factor::Evaluate: 300 factors on two extrinsics, both kinds mixed within a tile, and an edge
    factor whose point lies exactly on its line (nu = 0: zero residual, zero row, on both sides)"""
    if orc.ref_lib() is None:
        pytest.skip("no reference build")
    w = cc.calib_problem()["window"]
    rng = np.random.default_rng(31)
    cal = cc.make_calib(rng, w["exts_gt"], (0, 160, 140))
    on_line = dict(types=np.array([1], np.int32), points=np.array([[0.5, 0.0, 0.0]]), coeffs=np.array([[1.0, 0, 0, -1.0, 0, 0]]), ei=np.array([0], np.int32))
    cal = cc.concat([cal, on_line])
    perm = rng.permutation(len(cal["types"]))
    cal = {k: v[perm] for k, v in cal.items()}
    assert len(set(cal["types"][:100].tolist())) == 2 and np.array_equal(w["exts"][0], cc.IDENT)
    s = rng.uniform(0.5, 2.0, len(perm))
    _add(ctx, cal, s)
    r, J = ctx.calib_evaluate(w["exts"])
    assert r.shape == (301,) and J.shape == (301, 7) and np.isfinite(r).all() and np.isfinite(J).all()
    worst_r = worst_j = 0.0
    for i in range(len(r)):
        rr, Jr = orc.ref_online_calib("s" if cal["types"][i] == 0 else "c", cal["points"][i], cal["coeffs"][i], s[i], w["exts"][cal["ei"][i]])
        worst_r, worst_j = max(worst_r, abs(r[i] - rr) / max(1.0, abs(rr))), max(worst_j, float(np.abs(J[i] - Jr).max()))
        assert abs(r[i] - rr) <= 1e-12 * max(1.0, abs(rr)), i
        np.testing.assert_allclose(J[i], Jr, rtol=1e-11, atol=1e-11)
    print(f"mlh_calib_evaluate: residual {worst_r:.2e}, Jacobian {worst_j:.2e}")
    i0 = int(np.flatnonzero(cal["ei"] == 0)[0])
    assert r[i0] == 0.0 and not J[i0].any()
    assert not J[:, 6].any()


def _check_ne(got, A, b, cost, count, label):
    e_h, e_g = np.abs(got["H"] - A).max() / np.abs(A).max(), np.abs(got["g"] - b).max() / np.abs(b).max()
    e_c = abs(got["cost"] - cost) / cost
    print(f"{label}: H {e_h:.2e}, g {e_g:.2e}, cost {e_c:.2e}, count {got['count']}")
    assert e_h <= 1e-9 and e_g <= 1e-9 and e_c <= 1e-9, label
    assert got["count"] == count, label


@pytest.mark.parametrize("name", ["1x4", "3x2"])
def test_normal_equations_with_a_store_in_use(ctx, orc, name):
    """2. three interleaved appends (counts at the tile edges, an extrinsic with none, the second append outgrowing the first one's buffers), then
    mlh_pure_odom_normal_eq against the restatement; the store alone on an empty factor table; the same call twice: identical bits"""
    c = cc.store_case(name)
    w, cal = c["window"], c["all"]
    nf = w["n_frames"]
    for k, p in enumerate(c["parts"]):
        _add(ctx, p)
        info = ctx.calib_info()
        assert info["n_appends"] == k + 1 and info["n_slots"] == 256 * info["n_tiles"] and info["in_use"] == 0
    n_cal = len(cal["types"])
    tiles = sum((int((p["ei"] == e).sum()) + 255) // 256 for p in c["parts"] for e in range(w["n_ext"]))
    assert info["n_valid"] == n_cal and info["n_tiles"] == tiles and info["max_ext"] == int(cal["ei"].max())
    _stage(ctx, w)
    assert ctx.calib_info() == info                                                         # mlh_pure_odom_set does not touch the store
    plain = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    assert plain["count"] == len(w["types"])                                                # not in use yet
    ctx.calib_use(True)
    got = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    A, b, cost = cc.window_system(orc, w, cal, w["pivot"], w["frames"], w["exts"])
    _check_ne(got, A, b, cost, len(w["types"]) + n_cal, f"{name} table + store")
    again = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    for k in ("H", "g", "cost", "count"):
        assert np.array_equal(again[k], got[k]), k
    # outside the store's extrinsics the record is the table's, bit for bit
    D = 6 * (1 + nf + w["n_ext"])
    touched = np.zeros((D, D), bool)
    for e in np.unique(cal["ei"]):
        s = slice(6 * (1 + nf + e), 6 * (2 + nf + e))
        touched[s, s] = True
    assert np.array_equal(got["H"][~touched], plain["H"][~touched])
    # an empty factor table: the store's system alone
    ctx.pure_odom_begin()
    assert ctx.calib_info() == dict(info, in_use=1)                                         # mlh_pure_odom_begin does not touch the store
    alone = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
    Ac, bc, cost_c, cnt, n_outer = cc.calib_system(cal, w["exts"], nf)
    assert 0 < n_outer < cnt
    _check_ne(alone, Ac, bc, cost_c, n_cal, f"{name} store alone")
    assert np.array_equal(alone["H"], alone["H"].T)


def _fresh_results(mla, w):
    fresh = mla.Context(0)
    try:
        _stage(fresh, w)
        ne = fresh.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
        sol = fresh.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=4, huber_delta=mc.HUBER)
        fresh.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
        return ne, sol, fresh.window_prior_get()
    finally:
        fresh.close()


def test_unused_means_untouched(ctx, mla):
    """3. a store that is present but not in use, and a cleared one: normal equations, a 4-iteration solve and a marginalisation return a fresh context's bits"""
    c = cc.store_case("3x2")
    w = c["window"]
    ne0, sol0, prior0 = _fresh_results(mla, w)
    for state in ("present, not in use", "cleared"):
        if state == "cleared":
            ctx.window_prior_clear()
            ctx.calib_use(True)
            ctx.calib_clear()
            assert ctx.calib_info() == dict(n_appends=0, n_tiles=0, n_slots=0, n_valid=0, max_ext=-1, in_use=0)
        else:
            _add(ctx, c["parts"][0])
        _stage(ctx, w)
        ne = ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)
        for k in ("H", "g", "cost", "count"):
            assert np.array_equal(ne[k], ne0[k]), (state, k)
        sol = ctx.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=4, huber_delta=mc.HUBER)
        for k in ("frames", "exts", "cost", "count", "status"):
            assert np.array_equal(sol[k], sol0[k]), (state, k)
        ctx.window_marginalize(w["pivot"], w["frames"], w["exts"], mc.HUBER)
        prior = ctx.window_prior_get()
        for k in ("J0", "r0", "x0", "block_ids"):
            assert np.array_equal(prior[k], prior0[k]), (state, k)


def test_accumulate_equals_the_host_route(mla, orc, synth):
    """4. mlh_calib_accumulate on a real match pass (LiDAR 1's features against the map in the pivot frame, N_NEIGH 10, CHECK_FOV): the count rises by the valid
    correspondences mlh_match_linearize reports, and the normal equations equal those of a store filled by mlh_calib_add from the read-back valid / coeffs"""
    import conftest
    case = conftest._make_case(synth, "50k", 16, 2)
    Tinv = np.linalg.inv(synth.pose_to_mat(case["gt"]))
    maps = [np.ascontiguousarray(synth.transform_points(m[:, :3], Tinv).astype(np.float32)) for m in (case["surf_map"], case["corner_map"])]
    scn = case["scans"][1]
    ex = orc.extract(scn.points, scn.scan_start, scn.scan_end)
    feats = []
    for pts in (synth.voxel_mean(ex["less_flat_ds"][:, :3].copy(), 0.4), scn.points[ex["less_sharp"]][:, :3]):
        f = np.zeros((len(pts), 4), np.float32); f[:, :3] = pts; f[:, 3] = 1
        feats.append(np.ascontiguousarray(f))
    r = synth.HERCULES_BODY_T_LASER[1]
    ext1 = synth.perturbed_pose(np.concatenate([r[4:7], r[:4] / np.linalg.norm(r[:4])]), seed=210, dt=0.05, drot_deg=0.5)
    exts = np.stack([cc.IDENT, ext1])
    pivot, frames = cc.IDENT, cc.IDENT[None, :]
    dev, host = mla.Context(0), mla.Context(0)
    try:
        for c in (dev, host):
            c.map_set(mla.SURF, maps[0]); c.map_set(mla.CORNER, maps[1])
        dev.calib_use(True); host.calib_use(True)
        total = 0
        for kind in (mla.SURF, mla.CORNER):
            dev.features_set(kind, feats[kind])
            dev.calib_accumulate(kind, ext1, 1, k_neigh=10, flags=mla.FLAG_CHECK_FOV)
            host.features_set(kind, feats[kind])
            lin = host.match_linearize(kind, ext1, flags=mla.FLAG_CHECK_FOV, dense=False, k_neigh=10)
            m = lin["valid"].astype(bool)
            assert lin["count"] == int(m.sum()) > 30
            total += lin["count"]
            assert dev.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER)["count"] == total   # rises by exactly n_valid
            host.calib_add(np.full(int(m.sum()), kind, np.int32), feats[kind][m, :3].astype(np.float64), lin["coeffs"][m], np.full(int(m.sum()), 1, np.int32))
        a, b = dev.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER), host.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER)
        assert dev.calib_info()["n_valid"] == host.calib_info()["n_valid"] == total and a["count"] == b["count"] == total
        equal_bits = all(np.array_equal(a[k], b[k]) for k in ("H", "g", "cost"))
        e = max(np.abs(a["H"] - b["H"]).max() / np.abs(b["H"]).max(), np.abs(a["g"] - b["g"]).max() / np.abs(b["g"]).max(), abs(a["cost"] - b["cost"]) / b["cost"])
        print(f"accumulate vs add: {'equal bits' if equal_bits else 'NOT equal bits'}, worst relative difference {e:.2e}, {total} factors")
        assert e <= 1e-12
        # per-factor outputs of a device-built store (it is padded) are refused: the raw status, as in test_refusals
        ex_c = np.ascontiguousarray(exts); r_out = np.zeros(total)
        assert dev.lib.mlh_calib_evaluate(dev.h, ex_c.ctypes.data_as(C.c_void_p), len(ex_c), r_out.ctypes.data_as(C.c_void_p), None) == ERR_STATE
        assert b"device-built" in dev.lib.mlh_last_error(dev.h)
    finally:
        dev.close(); host.close()


def test_the_references_problem_solved(ctx, orc):
    """5. (1 frame, 3 extrinsics), window factors on extrinsic 0 only, pivot and extrinsic 0 constant, 5 iterations: with the store in use the restated
    Gauss-Newton loop; not in use and the other extrinsics held constant through the mask: status 0, they do not move"""
    p = cc.calib_problem()
    w, cal = p["window"], p["cal"]
    _stage(ctx, w)
    _add(ctx, cal)
    ctx.calib_use(True)
    got = ctx.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=5, huber_delta=mc.HUBER, const_blocks=[0, 2])
    fr, ex = cc.gn_solve(orc, w, cal, w["pivot"], w["frames"], w["exts"], 5, (0, 2))
    d = max(np.abs(got["frames"] - fr).max(), np.abs(got["exts"] - ex).max())
    moved = [float(np.abs(got["exts"][e] - w["exts"][e]).max()) for e in (1, 2)]
    print(f"calibration problem: {d:.2e} from the restated loop, extrinsics moved {moved}, count {got['count']}")
    assert got["status"] == 0 and d < 1e-9 and min(moved) > 1e-6
    assert got["count"] == len(w["types"]) + len(cal["types"]) and np.array_equal(got["exts"][0], w["exts"][0])
    ctx.calib_use(False)
    frozen = ctx.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=5, huber_delta=mc.HUBER, const_blocks=[0, 2, 3, 4])
    assert frozen["status"] == 0 and np.array_equal(frozen["exts"], w["exts"]) and not np.array_equal(frozen["frames"], w["frames"])
    assert frozen["count"] == len(w["types"])


def _chain_on_device(ctx, nf, ne, with_store):
    ci = cc.chain_inputs(nf, ne)
    ctx.window_ext_prior_set(ci["ext_rows"], in_marginalization=True, in_solve=False)

    def accumulate(cal):
        for e in range(1, ne):                                  # per LiDAR
            m = cal["ei"] == e
            ctx.calib_add(cal["types"][m], cal["points"][m], cal["coeffs"][m], cal["ei"][m])

    def solve(k, w, pivot, frames, exts, use):
        _stage(ctx, w)
        ctx.calib_use(use and with_store)
        s = ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=mc.HUBER, const_blocks=list(cc.chain_const_blocks(nf, ne, k)))
        assert s["status"] == 0, k
        return s["frames"], s["exts"]

    def marg(k, w, pivot, frames, exts, use):
        ctx.window_marginalize(pivot, frames, exts, mc.HUBER)
        assert ctx.calib_info()["n_valid"] > 0                  # the marginalisation does not clear the store
        return ctx.window_prior_get()

    return cc.chain_run(nf, ne, accumulate, solve, marg, ctx.calib_clear)


@pytest.mark.parametrize("shape", cc.CHAIN_SHAPES)
def test_chain_of_windows(ctx, mla, shape):
    """6. four windows, extrinsic prior rows in the marginalisation: accumulate per LiDAR -> store in use every 2nd window -> solve -> marginalise -> clear after a
    calibration window -> slide"""
    nf, ne = shape
    ref = cc.chain_reference(nf, ne)
    got = _chain_on_device(ctx, nf, ne, True)
    for k, ((_, fr_g, ex_g, prior_g), (_, fr_r, ex_r, prior_r)) in enumerate(zip(got, ref)):
        d = max(np.abs(fr_g - fr_r).max(), np.abs(ex_g - ex_r).max())
        print(f"chain {nf}x{ne} window {k}: poses {d:.2e}")
        assert d < 1e-7, (k, d)
        assert np.abs(prior_g["x0"] - prior_r["x0"]).max() < 1e-7
        _same_prior(prior_g, prior_r, f"chain {nf}x{ne} window {k}")
    bare = mla.Context(0)
    try:
        without = _chain_on_device(bare, nf, ne, False)
    finally:
        bare.close()
    diff = max(np.abs(a[2] - b[2]).max() for a, b in zip(got, without))
    print(f"chain {nf}x{ne}: with - without the store's term {diff:.2e}")
    assert diff > 1e-5                                          # not vacuous: the store's term moves an extrinsic


def test_refusals(ctx, mla):
    """7."""
    lib, h = ctx.lib, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ident = cc.IDENT.copy()
    # no staged features, no map
    assert lib.mlh_calib_accumulate(h, 0, p(ident), 10, 1, 1.0, 0.2, 1) == ERR_STATE
    assert lib.mlh_calib_accumulate(h, 0, p(ident), 10, 1, 1.0, 0.2, -1) == ERR_INVALID
    c = cc.store_case("3x2")
    w = c["window"]
    part = c["parts"][0]
    bad = part["ei"].copy(); bad[3] = -1
    assert lib.mlh_calib_add(h, len(bad), p(part["types"]), p(part["points"]), p(part["coeffs"]), None, p(np.ascontiguousarray(bad))) == ERR_INVALID
    assert ctx.calib_info()["n_valid"] == 0
    _add(ctx, part)
    ctx.calib_use(True)
    info = ctx.calib_info()
    _stage(ctx, w)
    # n_ext = 1 does not cover the store's extrinsic 1 (nor the table's); with the table's factors on extrinsic 0 only it is the store that refuses
    w0 = cc.ref_only(w)
    _stage(ctx, w0)
    D1 = 6 * (1 + w["n_frames"] + 1)
    H, g, cost, n = np.zeros((D1, D1)), np.zeros(D1), C.c_double(0), C.c_int32(0)
    fr, ex = np.ascontiguousarray(w["frames"].copy()), np.ascontiguousarray(w["exts"].copy())
    assert lib.mlh_pure_odom_normal_eq(h, p(w["pivot"]), p(fr), w["n_frames"], p(ex), 1, 1.0, p(H), p(g), C.byref(cost), C.byref(n)) == ERR_INVALID
    assert b"calibration store" in lib.mlh_last_error(h)
    st = C.c_int32(0)
    assert lib.mlh_pure_odom_gn_solve(h, p(w["pivot"]), p(fr), w["n_frames"], p(ex), 1, 1.0, 2, 1 | (1 << (1 + w["n_frames"])), None, C.byref(cost), C.byref(n), C.byref(st)) == ERR_INVALID
    r = np.zeros(info["n_valid"])
    assert lib.mlh_calib_evaluate(h, p(ex), 1, p(r), None) == ERR_INVALID
    assert ctx.calib_info() == info                                                         # the store is intact
    assert ctx.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"], mc.HUBER)["count"] == len(w0["types"]) + info["n_valid"]
    # 23 blocks at the marginalisation, store in use
    big = mc.shape_window("limit")
    fr12 = np.ascontiguousarray(np.vstack([big["frames"], big["frames"][-1:]]))
    info_c = mla.WindowPriorInfo()
    assert lib.mlh_window_marginalize(h, p(big["pivot"]), p(fr12), 12, p(big["exts"]), 10, 1.0, C.byref(info_c)) == ERR_UNSUPPORTED
    # (mlh_calib_evaluate on a device-built store -> MLH_ERR_STATE is asserted in test 4, which has the match pass it needs); an empty store has none either
    ctx.calib_clear()
    assert lib.mlh_calib_evaluate(h, p(ex), 2, p(r), None) == ERR_STATE


APPEND_M = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


@pytest.fixture(scope="module")
def append_pair(mla, case16):
    """two contexts with the 16-ring case's surf map resident: one appends on the device, the other is fed from the host"""
    dev, host = mla.Context(0), mla.Context(0)
    for c in (dev, host):
        c.map_set(mla.SURF, case16["surf_map"])
    yield dev, host
    dev.close(); host.close()


@pytest.mark.parametrize("m", APPEND_M)
def test_shared_append_at_its_edges(mla, append_pair, case16, feats16, m):
    """9. the scan-and-pack both device routes share (factor_dev.hpp: append_valid_matches) at its boundaries -- the 64-lane ballot, the 1024-feature chunk, the
    256-slot tile: the first m surf features of the 16-ring case, every third moved 100 m away (valid and invalid slots interleave), matched at the case's pose.
    One mlh_pure_odom_add_matches on a fresh table / one mlh_calib_accumulate on a fresh store must give the system of mlh_pure_odom_set / mlh_calib_add fed the
    read-back valid features and coefficients in feature order. A single append of one kind lays the factors out in the same slots and tiles as the host route
    (the device's trailing padding tiles add 0.0), and at the parent commit the two systems had equal bits for every m of APPEND_M on both routes: array_equal."""
    dev, host = append_pair
    pose = case16["gt"]
    f = np.ascontiguousarray(feats16[0][:m].copy())
    assert len(f) == m
    f[2::3, :3] += np.float32(100.0)
    host.features_set(mla.SURF, f)
    lin = host.match_linearize(mla.SURF, pose, dense=False)
    v = lin["valid"].astype(bool)
    nv = int(v.sum())
    assert lin["count"] == nv and not v[2::3].any()
    if m >= 3:
        assert 0 < nv < m
    else:
        assert nv == m == 1
    types, pts, co = np.zeros(nv, np.int32), f[v, :3].astype(np.float64), lin["coeffs"][v]
    ones = np.ones(nv, np.int32)
    pivot, frames, exts = cc.IDENT, cc.IDENT[None, :], np.stack([cc.IDENT, pose])

    def same(a, b, label):
        equal_bits = all(np.array_equal(a[k], b[k]) for k in ("H", "g", "cost"))
        e = max(np.abs(a["H"] - b["H"]).max() / np.abs(b["H"]).max(), np.abs(a["g"] - b["g"]).max() / np.abs(b["g"]).max(), abs(a["cost"] - b["cost"]) / b["cost"])
        print(f"m = {m} {label}: {'equal bits' if equal_bits else 'NOT equal bits'}, worst relative difference {e:.2e}, {nv} of {m} valid")
        assert a["count"] == b["count"] == nv, label
        for k in ("H", "g", "cost"):
            assert np.array_equal(a[k], b[k]), (label, k, e)

    # the window table (no store in the way)
    for c in (dev, host):
        c.calib_clear()
    dev.pure_odom_begin()
    dev.features_set(mla.SURF, f)
    dev.pure_odom_add_matches(mla.SURF, pose, 0, 1)
    host.pure_odom_set(types, pts, co, np.zeros(nv, np.int32), ones)
    same(dev.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER), host.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER), "window table")
    # the calibration store, alone on an empty factor table
    for c in (dev, host):
        c.pure_odom_begin()
        c.calib_use(True)
    dev.calib_accumulate(mla.SURF, pose, 1, k_neigh=5, flags=0)
    host.calib_add(types, pts, co, ones)
    same(dev.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER), host.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER), "calibration store")
    info = dev.calib_info()
    tiles = (m + 255) // 256
    assert info["n_valid"] == host.calib_info()["n_valid"] == nv and info["n_tiles"] == tiles and info["n_slots"] == 256 * tiles
    if m in (256, 1024):
        # a second append behind the first starts on the next tile
        dev.calib_accumulate(mla.SURF, pose, 1, k_neigh=5, flags=0)
        host.calib_add(types, pts, co, ones)
        info2 = dev.calib_info()
        assert info2["n_tiles"] == 2 * tiles and info2["n_slots"] == 2 * 256 * tiles and info2["n_valid"] == 2 * nv and info2["n_appends"] == 2
        a, b = dev.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER), host.pure_odom_normal_eq(pivot, frames, exts, mc.HUBER)
        assert a["count"] == b["count"] == 2 * nv
        e = max(np.abs(a["H"] - b["H"]).max() / np.abs(b["H"]).max(), np.abs(a["g"] - b["g"]).max() / np.abs(b["g"]).max(), abs(a["cost"] - b["cost"]) / b["cost"])
        print(f"m = {m} two appends: worst relative difference {e:.2e}")
        assert e <= 1e-12                                       # test_accumulate_equals_the_host_route's bound: the host's second append starts on another tile


def test_calib_selftest_facade_equals_the_c_abi():
    """8. m-loam_amd/host/calib_selftest: the chain through the facade and through the plain calls ends in the same poses and the same prior bits"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "calib_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/calib_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "calibration store: facade equals the C-ABI" in r.stdout
