"""The crafted fit sites of tests/fit_cases.py on the CPU: the oracle (orc.Map.match) and the reference build (orc.ref_match, the reference's own lines over
mini_eigen.hpp) agree in bits on every site, meet the float64 bars on the 'f64' sites and take float64's decision wherever the site declares one.
tests/test_gpu_fit_cases.py holds the HIP kernels to the same sites.

The constants of the bars come from here: measure() takes the worst ratio error / (2^-24 x the bar's bracket) that the REFERENCE BUILD shows over the committed
sites; tests/golden/fit_tolerances.json holds those ratios and c = 4 x ratio (room for another legitimate f32 operation order; a wrong branch moves a
coefficient by orders of magnitude more). `python tests/test_fit_cases.py --write` rewrites the file; test_tolerances_are_the_measured_ones fails when the file
and the measurement part. The eigenvalues are not part of a match's result: they are measured on the oracle's solver (orc.eig3f) fed with fit_line's own f32
scatter matrix -- the solver whose end points the reference build reproduces bit for bit in the same test."""
import json
import os
import sys

import numpy as np
import pytest

import fit_cases as fc
import knn_cases as kc

F32 = np.float32
TOL_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_tolerances.json")
KINDS = ("s", "c")
# a backward-stable 5..10 x 3 solver's forward error is a small multiple of kappa * eps; a ratio beyond this is a wrong algorithm, not rounding
RATIO_SANITY = 64.0

REQUIRED_FAMILIES = (
    "exactly collinear along x", "exactly collinear along y", "exactly collinear along z", "exactly collinear along diag", "coplanar, l2 / l1 = 1.5",
    "coplanar, l2 / l1 = 30", "l2 / l1 = 3 * 0.98", "l2 / l1 = 3 * 1.02", "isotropic: tetrahedron plus its centre", "nearly isotropic", "two equal large eigenvalues",
    "five identical points", "extent 1e-4 m", "extent 0.9 m", "a20 == 0 exactly (already tridiagonal)", "a10 == 0 exactly", "already diagonal", "l2 == 3 l1 exactly",
    "centroid 50 m from the origin", "K = 10 collinear along a diagonal", "K = 10 coplanar, l2 / l1 = 5",
    "plane x = c", "plane y = c", "plane z = c", "two columns with exactly equal norms", "one coordinate exactly 0, plane off the origin",
    "patch at (20, 20, 5), 0.2 m extent", "first column with a zero tail; patch 0.3 m from the origin", "one point off the plane, largest residual min_plane_dis * 0.99",
    "one point off the plane, largest residual min_plane_dis * 1.01", "patch 3 m from the origin", "patch 50 m from the origin", "plane through the origin",
    "collinear points", "identical points", "K = 10 generic patch", "feature exactly on its line", "feature on its plane", "|r| = delta * 0.999", "|r| = delta * 1.001")


def tolerances():
    with open(TOL_PATH) as f:
        return json.load(f)


def measured(name, value, bar):
    print(f"FIT_MEASURED {name} {value:.6g} {bar:.6g}")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------- shared by the CPU and the GPU test
def check_fit(valid, coeffs, sites, tol, where, worst=None):
    """valid (m,), coeffs (m x 6) of one match over `sites` against float64: the declared decisions everywhere, the bars on the valid 'f64' sites.
    worst: a dict that collects the largest ratio error / (2^-24 x bracket) per bar (measure() uses it without asserting)"""
    for i, s in enumerate(sites):
        ref, tag = s["ref"], f"{where} {s['name']}"
        if s["expect_valid"] is not None and worst is None:
            assert bool(valid[i]) == s["expect_valid"], tag
        if s["cls"] == "f64" and worst is None:
            assert bool(valid[i]) == ref["valid"], tag                                   # float64's decision (decision sites: 20 bars of margin)
        if not valid[i] or (s["cls"] != "f64" and s["kind"] == "s"):
            continue
        if s["kind"] == "s":
            err, br = fc.plane_err(coeffs[i, :3], coeffs[i, 3], ref), ref["kappa"] * fc.EPS
            pairs = [("plane", err, br, "c_p")]
        else:
            t = fc.line_terms(ref)
            pairs = [("centre", fc.centre_err(coeffs[i], ref), t["centre"] * fc.EPS, "c_l")]
            if t["ends"] is not None and s["cls"] == "f64":
                pairs.append(("ends", fc.ends_err(coeffs[i], ref), t["ends"] * fc.EPS, "c_l"))
        for what, err, br, c in pairs:
            if worst is not None:
                worst[c] = max(worst.get(c, 0.0), err / br if br > 0 else (0.0 if err == 0 else np.inf))
                continue
            measured(f"{tag} {what}", err, tol[c] * br)
            assert err <= tol[c] * br, (tag, what, err, tol[c] * br)


def neighbour_order(s):
    """the site's points in the order the search returns them at the identity pose (nearest first)"""
    idx, _ = kc.brute_knn(fc.MAPS[s["kind"]], s["query"].astype(F32)[None, :], s["k"])
    return fc.MAPS[s["kind"]][idx[0]]


def eigen_of_sites(orc):
    """orc.eig3f on fit_line's own f32 scatter matrix of every line site -> {name: (eigenvalues ascending f32, rc)}"""
    out = {}
    for s in fc.sites_of("c"):
        _, m = fc.f32_scatter(neighbour_order(s))
        A = np.array([[m[0], m[1], m[3]], [m[1], m[2], m[4]], [m[3], m[4], m[5]]], F32)
        val, _, rc = orc.eig3f(A)
        out[s["name"]] = (val, rc)
    return out


def all_matches(fn):
    """fn(kind, map, feats4, pose, k) -> (valid, coeffs), over every pose, kind and K"""
    out = {}
    for pn, pose in fc.POSES.items():
        for kind in KINDS:
            for k in (5, 10):
                f4, ss = fc.features(kind, k, pn)
                out[(pn, kind, k)] = fn(kind, fc.MAPS[kind], f4, pose, k) + (ss,)
    return out


def measure(orc):
    """the worst ratios of the reference build over the committed sites (eigenvalues: the oracle's solver, see the module text)"""
    worst = {}
    for (pn, kind, k), (v, co, ss) in all_matches(lambda kind, m, f4, pose, k: orc.ref_match(kind, m, f4, pose, n_neigh=k)).items():
        check_fit(v, co, ss, None, "", worst)
    for name, (val, _) in eigen_of_sites(orc).items():
        ref = fc.site(name)["ref"]
        if ref["lam"][2] > 0:
            worst["c_e"] = max(worst.get("c_e", 0.0), float(np.abs(val.astype(np.float64) - ref["lam"]).max()) / (ref["lam"][2] * fc.EPS * fc.line_terms(ref)["eig"]))
    return worst


def _need_ref(orc):
    if orc.ref_lib() is None:
        pytest.skip("no reference tree and no prebuilt oracle/_ref/libmloam_ref.so")


# ---------------------------------------------------------------- the module's own preconditions
def test_site_families_classes_and_margins():
    fams = {s["family"] for s in fc.SITES}
    missing = [f for f in REQUIRED_FAMILIES if f not in fams]
    assert not missing, missing
    assert all(s["branch"] and s["family"] for s in fc.SITES)
    n_bits = sum(s["cls"] == "bits" for s in fc.SITES)
    assert n_bits * 5 <= len(fc.SITES) and all(s["reason"] for s in fc.SITES if s["cls"] == "bits")
    assert len(fc.SURF_MAP) > 50 and len(fc.CORNER_MAP) > 10
    tol = tolerances()
    margins = fc.check_margins(tol["c_p"], tol["c_l"], tol["c_e"])
    assert sorted(margins) == sorted(s["name"] for s in fc.SITES if s["decision"]) and len(margins) >= 7
    for name, (dist, bar) in margins.items():
        measured(f"margin {name}", dist, 20 * bar)
    for pn in fc.POSES:                                        # every feature set holds every site of its kind and K, once
        for kind in KINDS:
            assert sum(len(fc.features(kind, k, pn)[1]) for k in (5, 10)) == len(fc.sites_of(kind))


def test_tolerances_are_the_measured_ones(orc):
    _need_ref(orc)
    tol, got = tolerances(), measure(orc)
    for c in ("c_p", "c_l", "c_e"):
        measured(f"worst ratio {c}", got[c], tol["worst_ratio"][c])
        assert got[c] <= RATIO_SANITY, (c, got[c])
        assert abs(got[c] - tol["worst_ratio"][c]) <= 1e-6 * tol["worst_ratio"][c], (c, got[c], tol["worst_ratio"][c])
        assert tol[c] == pytest.approx(4.0 * tol["worst_ratio"][c], rel=1e-12)


# ---------------------------------------------------------------- oracle and reference build on every site
def test_oracle_and_reference_build_on_every_site(orc):
    _need_ref(orc)
    tol = tolerances()
    maps = {kind: orc.Map(fc._m4(fc.MAPS[kind])) for kind in KINDS}
    o = all_matches(lambda kind, m, f4, pose, k: maps[kind].match(kind, f4, pose, n_neigh=k))
    r = all_matches(lambda kind, m, f4, pose, k: orc.ref_match(kind, m, f4, pose, n_neigh=k))
    seen = set()
    for key, (v, co, ss) in o.items():
        rv, rco, _ = r[key]
        assert np.array_equal(v, rv), (key, [s["name"] for s, a, b in zip(ss, v, rv) if a != b])
        assert np.array_equal(bits(co), bits(rco)), key
        check_fit(v, co, ss, tol, f"oracle {key[0]}")
        seen.update(s["name"] for s in ss)
    assert seen == set(fc.NAMES)                                # no site skipped
    # the fit does not see the pose: one site, one set of coefficients (the neighbours keep their order from pose to pose)
    for kind in KINDS:
        for k in (5, 10):
            base = o[("identity", kind, k)]
            for pn in fc.POSES:
                assert np.array_equal(bits(o[(pn, kind, k)][1]), bits(base[1])), (pn, kind, k)
    i = [s["name"] for s in o[("identity", "s", 5)][2]].index("p_identical")
    got = o[("identity", "s", 5)][1][i, :4]                     # the basic solution of the rank-1 system, as Eigen gives it: all on the pivot column
    assert np.array_equal(got[:3], [0.0, 0.0, -1.0]) and abs(got[3] - 3.0) <= 2.0 ** -21, got


def test_eigenvalues_and_line_decisions(orc):
    """the oracle's f32 eigen-solver on fit_line's own scatter matrix of every line site: eigenvalues within the bar, l2 > 3 l1 decided as float64 decides"""
    tol = tolerances()
    for name, (val, rc) in eigen_of_sites(orc).items():
        s = fc.site(name)
        ref = s["ref"]
        assert val[0] <= val[1] <= val[2], name
        if ref["lam"][2] == 0:
            assert not val.any(), name                         # identical points: scale == 0, exact zeros
            continue
        err = float(np.abs(val.astype(np.float64) - ref["lam"]).max()) / ref["lam"][2]
        bar = tol["c_e"] * fc.EPS * fc.line_terms(ref)["eig"]
        measured(f"eigenvalues {name}", err, bar)
        assert err <= bar, (name, val, ref["lam"])
        assert bool(val[2] > F32(3) * val[1]) == ref["valid"], (name, val)
        if name == "l_gate_exact_tie":
            assert val[2] == F32(3) * val[1] and ref["lam"][2] == 3.0 * ref["lam"][1], (name, val, ref["lam"])      # a tie in both precisions: the gate's > is strict


def test_plane_solver_on_every_site(orc):
    """the oracle's f32 QR on every plane site, rejected ones included (a match hands out no coefficients for those): n_hat and d within the bar on 'f64' sites"""
    tol = tolerances()
    for s in fc.sites_of("s"):
        nb = neighbour_order(s)
        n = orc.qr_solve(nb, -np.ones(s["k"], F32))
        nn = F32(np.sqrt(F32(F32(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])))
        if s["cls"] != "f64":
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            d, n_hat = F32(1) / nn, (n / nn).astype(F32)
        err, bar = fc.plane_err(n_hat, d, s["ref"]), fc.plane_bar(s["ref"], tol["c_p"])
        measured(f"qr {s['name']}", err, bar)
        assert err <= bar, (s["name"], n_hat, d, s["ref"])
        res = float(np.abs(nb.astype(np.float64) @ n_hat.astype(np.float64) + float(d)).max())
        assert (res <= fc.MIN_PLANE_DIS) == s["ref"]["valid"], s["name"]


# ---------------------------------------------------------------- the float64 factor rows test themselves
def _rows_setup(orc, pose_name="generic"):
    out = []
    maps = {kind: orc.Map(fc._m4(fc.MAPS[kind])) for kind in KINDS}
    for kind in KINDS:
        f4, ss = fc.features(kind, 5, pose_name)
        v, co = maps[kind].match(kind, f4, fc.POSES[pose_name], n_neigh=5)
        out.append((kind, f4, v, co))
    return out


def test_factor_rows_against_central_differences(orc):
    """this tests the test: the Jacobian formulas of fit_cases.factor_row against central differences through pose_plus, all in float64"""
    for x in (fc.POSES["generic"], fc.POSES["near_pi"]):
        d = np.array([0.01, -0.02, 0.015, 0.003, -0.002, 0.004])
        assert np.abs(fc.pose_plus(x, d) - orc.pose_plus(x, d)).max() < 1e-15
    h = 1e-7                                                    # 50 m from the origin a rotation by h moves the point by 5e-6 m: truncation stays below the bar
    for pn in ("generic", "near_pi"):
        pose = fc.POSES[pn]
        for kind, f4, v, co in _rows_setup(orc, pn):
            for trace in (0.0075, 0.25):
                w = fc.sqrt_info_of(trace)
                for i in np.nonzero(v)[0]:
                    r0, J = fc.factor_row(kind, f4[i, :3], co[i], w, pose)
                    if kind == "c" and r0 < 1e-3 * w:
                        continue                                # |nu| has a kink at 0: no derivative to difference
                    num = np.zeros(6)
                    for a in range(6):
                        e = np.zeros(6)
                        e[a] = h
                        num[a] = (fc.factor_row(kind, f4[i, :3], co[i], w, fc.pose_plus(pose, e))[0] - fc.factor_row(kind, f4[i, :3], co[i], w, fc.pose_plus(pose, -e))[0]) / (2 * h)
                    assert np.abs(num - J).max() <= 1e-6 * max(1.0, np.abs(J).max()), (pn, kind, i, num, J)
                    ro, Jo = orc.factor_eval(kind, f4[i, :3].astype(np.float64), co[i], trace, pose)
                    assert abs(ro - r0) <= 1e-12 * max(1.0, abs(r0)) and np.abs(Jo[:6] - J).max() <= 1e-12 * max(1.0, np.abs(J).max())


def test_huber_form_against_the_oracle(orc):
    """H = sum rho1 J^T J, g = sum rho1 J^T r, cost = sum rho / 2 is what the oracle's corrected problem sums to (the rho'' <= 0 branch of Ceres' corrector)"""
    for trace in fc.TRACES:
        for kind, f4, v, co in _rows_setup(orc):
            pose = fc.POSES["generic"]
            r, J = fc.factor_rows(kind, f4, v, co, trace, pose)
            ne = fc.normal_eq(r, J, v)
            assert ne["gate_distance"] > 1e-6                   # no row so close to the gate that the last bit of r decides
            ref = orc.linearize(kind, f4, np.full(len(f4), trace), pose, v, co, huber_delta=fc.HUBER_DELTA)
            assert ref["count"] == ne["count"] == int(v.sum())
            assert np.abs(ref["r"] - r).max() <= 1e-12 and np.abs(ref["J"] - J).max() <= 1e-12 * np.abs(J).max()
            for a, b in ((ref["H"], ne["H"]), (ref["g"], ne["g"]), (np.array([ref["cost"]]), np.array([ne["cost"]]))):
                assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
            if trace == 0.0075:                                 # at sqrt_info 1 the two Huber sites of the kind straddle the gate
                names = [s["name"] for s in fc.sites_of(kind, 5)]
                below, above = (names.index(("p" if kind == "s" else "l") + f"_huber_{t}") for t in ("below", "above"))
                assert abs(abs(r[below]) / fc.HUBER_DELTA - 0.999) < 1e-4 and abs(abs(r[above]) / fc.HUBER_DELTA - 1.001) < 1e-4, (r[below], r[above])
    # the site on its line at the identity pose: nu == 0 exactly -- residual 0, an all-zero row, no NaN
    f4, ss = fc.features("c", 5, "identity")
    i = [s["name"] for s in ss].index("l_feature_on_line")
    v, co = orc.Map(fc._m4(fc.CORNER_MAP)).match("c", f4, fc.POSES["identity"], n_neigh=5)
    assert v[i]
    r0, J0 = fc.factor_row("c", f4[i, :3], co[i], 1.0, fc.POSES["identity"])
    ro, Jo = orc.factor_eval("c", f4[i, :3].astype(np.float64), co[i], 0.0075, fc.POSES["identity"])
    assert r0 == 0.0 and not J0.any() and ro == 0.0 and not Jo.any()


if __name__ == "__main__":
    if "--write" in sys.argv:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
        import oracle as O
        O.build()
        w = measure(O)
        doc = dict(note="worst ratio error / (2^-24 x bracket) of the reference build over the sites of tests/fit_cases.py (eigenvalues: the oracle's solver); c = 4 x ratio",
                   worst_ratio={c: w[c] for c in ("c_p", "c_l", "c_e")}, **{c: 4.0 * w[c] for c in ("c_p", "c_l", "c_e")})
        with open(TOL_PATH, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(doc)
