"""The mapper's line and plane fits (dev_math.hpp: plane_fit_qr_f, eig3_largest_f; match.hip: fit_plane, fit_line, fit_feature) and its factor rows
(eval_plane, eval_edge, the Huber reduction) on the crafted sites of tests/fit_cases.py, held to float64 (tests/test_fit_cases.py holds the oracle and the
reference build to the same sites on the CPU, and measures the constants of the bars there).

Per site: the neighbour records are the site's own K points, bit for bit; `valid` is float64's decision and the coefficients meet the float64 bars on the
'f64' sites; validity and coefficients have the oracle's bits on every site. r, J, H, g and the cost are held to float64 rows built from the KERNEL's own
coefficients, within 1e-9 of the largest entry of the compared array (the project's bar for r, J, H and g). The same fits are then reached through
gn_solve (three schedules), scan2map (classic and consumer-side LM) and mlh_linearize at a second pose."""
import numpy as np
import pytest

import fit_cases as fc
from test_fit_cases import bits, check_fit, measured, tolerances
from test_gpu_knn_cases import LANES, SCHEDULES, _context, _stop_on_device_error

pytestmark = pytest.mark.gpu

F32 = np.float32
ROW_BAR = 1e-9


def _kind(mla, kind):
    return mla.SURF if kind == "s" else mla.CORNER


def _stage_maps(ctx):
    ctx.map_set_pair(fc._m4(fc.SURF_MAP), fc._m4(fc.CORNER_MAP), fc.SQ)


def _close(name, got, want):
    """within 1e-9 of the largest entry of the compared array"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    measured(name, err, ROW_BAR * scale)
    assert np.isfinite(got).all() and err <= ROW_BAR * scale, (name, err, scale)


def _check_rows(name, out, kind, f4, trace, pose, loss=True):
    """r, J of a dense launch and its reduced H, g, cost, count against the float64 rows of the kernel's own coefficients"""
    r, J = fc.factor_rows(kind, f4, out["valid"], out["coeffs"], trace, pose)
    ne = fc.normal_eq(r, J, out["valid"], loss=loss)
    assert not loss or ne["gate_distance"] > 1e-6, name          # no |r| so close to delta that the last bit decides the Huber branch
    if out.get("r") is not None:
        _close(f"{name} r", out["r"], r)
        _close(f"{name} J", out["J"], J)
        rest = ~out["valid"].astype(bool)
        assert not out["r"][rest].any() and not out["J"][rest].any(), name
    _close(f"{name} H", out["H"], ne["H"])
    _close(f"{name} g", out["g"], ne["g"])
    _close(f"{name} cost", [out["cost"]], [ne["cost"]])
    assert out["count"] == ne["count"] == int(out["valid"].sum()), name


def _own_points(rec, sites, where):
    """every site's neighbour records are its own K points, bit for bit (in whatever order the distances put them)"""
    for i, s in enumerate(sites):
        got = rec[i, :s["k"], :3]
        a = got[np.lexsort(got.T[::-1])]
        b = s["pts"][np.lexsort(s["pts"].T[::-1])]
        assert np.array_equal(bits(a), bits(b)), (where, s["name"])
        assert np.all(rec[i, :s["k"], 3] < F32(0.81 * fc.SQ)), (where, s["name"])


@_stop_on_device_error
def test_fits_and_rows_on_crafted_sites(mla, orc):
    tol = tolerances()
    omaps = {kind: orc.Map(fc._m4(fc.MAPS[kind])) for kind in ("s", "c")}
    want = {}
    seen = set()
    first = {}
    for lanes in LANES:
        ctx = _context(mla, lanes)
        try:
            _stage_maps(ctx)
            for pn, pose in fc.POSES.items():
                for kind in ("s", "c"):
                    for k in (5, 10):
                        f4, ss = fc.features(kind, k, pn)
                        key = (pn, kind, k)
                        where = f"{lanes} lanes {pn} {kind} K={k}"
                        if key not in want:
                            want[key] = omaps[kind].match(kind, f4, pose, n_neigh=k)
                        kd = _kind(mla, kind)
                        ctx.features_set(kd, f4)
                        out = ctx.match_linearize(kd, pose, dense=True, k_neigh=k)
                        rec = ctx.match_neighbours(kd)
                        _own_points(rec, ss, where)
                        check_fit(out["valid"], out["coeffs"], ss, tol, where)
                        ov, oc = want[key]
                        assert np.array_equal(out["valid"], ov), (where, [s["name"] for s, a, b in zip(ss, out["valid"], ov) if a != b])
                        assert np.array_equal(bits(out["coeffs"]), bits(oc)), (where, [s["name"] for s, a, b in zip(ss, out["coeffs"], oc) if not np.array_equal(a, b)])
                        _check_rows(where + " huber", out, kind, f4, 0.0075, pose)
                        nl = ctx.match_linearize(kd, pose, flags=mla.FLAG_NO_LOSS, dense=True, k_neigh=k)
                        assert np.array_equal(nl["valid"], out["valid"]) and np.array_equal(bits(nl["coeffs"]), bits(out["coeffs"])), where
                        _check_rows(where + " no loss", nl, kind, f4, 0.0075, pose, loss=False)
                        if pn == "identity" and kind == "c" and k == 5:          # the feature exactly on its line: nu == 0 -- residual 0, an all-zero row, no NaN
                            i = [s["name"] for s in ss].index("l_feature_on_line")
                            assert out["valid"][i] and out["r"][i] == 0.0 and not out["J"][i].any(), (where, out["r"][i], out["J"][i])
                        if pn == "generic":
                            for trace in fc.TRACES[1:]:
                                tr = ctx.match_linearize(kd, pose, dense=True, k_neigh=k, cov_measurement_trace=trace)
                                assert np.array_equal(bits(tr["coeffs"]), bits(out["coeffs"])), where
                                _check_rows(f"{where} trace {trace:.4g}", tr, kind, f4, trace, pose)
                        if lanes == LANES[0]:
                            first[key] = (out["valid"], out["coeffs"], out["r"], out["J"], out["H"], out["g"])
                        else:                                                      # the width of the search does not reach the fit
                            for a, b in zip(first[key], (out["valid"], out["coeffs"], out["r"], out["J"], out["H"], out["g"])):
                                assert np.array_equal(a, b), where
                        seen.update(s["name"] for s in ss)
        finally:
            ctx.close()
    assert seen == set(fc.NAMES)                                  # no site skipped


def _p0_reference(mla, ctx, sets):
    """match_linearize + Huber at p0 for both kinds on a staged context -> per kind the result, and the sums the solvers' iteration 0 must report"""
    p0 = fc.POSES["generic"]
    out = {}
    for kind, (f4, _) in sets.items():
        ctx.features_set(_kind(mla, kind), f4)
        out[kind] = ctx.match_linearize(_kind(mla, kind), p0, dense=True, k_neigh=5)
    return out, out["s"]["H"] + out["c"]["H"], out["s"]["g"] + out["c"]["g"]


def _check_iteration0(name, st, ref, H, g):
    assert (st["n_surf"], st["n_corner"]) == (ref["s"]["count"], ref["c"]["count"]), (name, st["n_surf"], st["n_corner"])
    _close(f"{name} H", st["H"], H)
    _close(f"{name} g", st["g"], g)
    print(f"FIT_MEASURED {name} H bit-equal {int(np.array_equal(st['H'], H))} g bit-equal {int(np.array_equal(st['g'], g))}")


def _check_coeffs(mla, ctx, ref, name):
    for kind in ("s", "c"):
        got = ctx.match_coeffs(_kind(mla, kind))
        assert np.array_equal(got["valid"], ref[kind]["valid"]) and got["count"] == ref[kind]["count"], (name, kind)
        assert np.array_equal(bits(got["coeffs"]), bits(ref[kind]["coeffs"])), (name, kind)


@_stop_on_device_error
def test_fits_reached_through_the_solvers(mla, monkeypatch):
    """iteration 0 of gn_solve (three schedules) and of scan2map (classic launches, consumer-side LM) fits the same sites: the same counts, H and g as
    match_linearize + Huber at p0, and the same coefficient bits read back through mlh_match_coeffs"""
    p0 = fc.POSES["generic"]
    sets = {kind: fc.features(kind, 5, "generic") for kind in ("s", "c")}
    ctx = mla.Context(0)
    try:
        _stage_maps(ctx)
        ref, H, g = _p0_reference(mla, ctx, sets)
        assert ref["s"]["count"] >= 10 and ref["c"]["count"] >= 10
        _check_coeffs(mla, ctx, ref, "match_linearize")
    finally:
        ctx.close()
    for sched in SCHEDULES:
        ctx = mla.Context(0)
        try:
            ctx.set_gn_schedule(*sched)
            _stage_maps(ctx)
            for kind, (f4, _) in sets.items():
                ctx.features_set(_kind(mla, kind), f4)
            _, st = ctx.gn_solve(p0, 1)
            _check_iteration0(f"gn_solve schedule {sched}", st[0], ref, H, g)
            _check_coeffs(mla, ctx, ref, f"gn_solve schedule {sched}")
            ctx.gn_solve(p0, 1, want_stats=False)
            _check_coeffs(mla, ctx, ref, f"gn_solve schedule {sched}, no statistics")
        finally:
            ctx.close()
    opts = mla.default_opts(max_outer=1, gf_method=mla.GF_METHODS["wo_gf"])
    ctx = mla.Context(0)
    try:
        _stage_maps(ctx)
        for kind, (f4, _) in sets.items():
            ctx.features_set(_kind(mla, kind), f4)
        pose_classic, st = ctx.scan2map(p0, opts)
        _check_iteration0("scan2map", st[0], ref, H, g)
        _check_coeffs(mla, ctx, ref, "scan2map")
        default = ctx.scan2map(p0, opts, want_stats=False)[0]
        _check_coeffs(mla, ctx, ref, "scan2map, default launches")
        monkeypatch.setenv("MLH_LM_CONSUMER", "1")
        monkeypatch.setenv("MLH_LM_LOOP", "0")
        consumer = ctx.scan2map(p0, opts, want_stats=False)[0]
        _check_coeffs(mla, ctx, ref, "scan2map, consumer-side LM")
        _, st2 = ctx.scan2map(p0, opts)
        _check_iteration0("scan2map, consumer-side LM", st2[0], ref, H, g)
        assert np.array_equal(default, pose_classic) and np.array_equal(consumer, pose_classic)
    finally:
        ctx.close()


@_stop_on_device_error
def test_linearize_at_a_second_pose(mla):
    """mlh_linearize keeps the correspondences: its rows at a second pose are the float64 factor rows of the coefficients fitted at the first"""
    ctx = mla.Context(0)
    try:
        _stage_maps(ctx)
        for kind in ("s", "c"):
            f4, _ = fc.features(kind, 5, "generic")
            kd = _kind(mla, kind)
            ctx.features_set(kd, f4)
            fit = ctx.match_linearize(kd, fc.POSES["generic"], dense=True, k_neigh=5)
            for flags, loss in ((0, True), (mla.FLAG_NO_LOSS, False)):
                lin = ctx.linearize(kd, fc.SECOND_POSE, flags=flags, dense=True)
                lin.update(valid=fit["valid"], coeffs=fit["coeffs"])
                _check_rows(f"linearize {kind} second pose loss={loss}", lin, kind, f4, 0.0075, fc.SECOND_POSE, loss=loss)
            again = ctx.match_coeffs(kd)
            assert np.array_equal(bits(again["coeffs"]), bits(fit["coeffs"])) and np.array_equal(again["valid"], fit["valid"])
    finally:
        ctx.close()
