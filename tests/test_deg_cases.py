"""The cases of tests/deg_cases.py on the CPU: every threshold stands clear of every eigenvalue of every iteration by MARGIN_ABS, every case reaches the rank it is
named for, a verdict one direction off would move the pose by at least 1000 bars, and the restatements of evalDegenracy agree on every case -- the oracle's
(cyclic Jacobi, V_f^-T V_p^T) and, where oracle/_ref is built, the reference's own lines, against deg_cases.reference_tail (numpy.linalg.eigh, Q_kept Q_kept^T).
tests/test_gpu_deg_cases.py holds the kernels to the same reference on the same cases.

The constants of the GPU test's bars come from here, measured on the ORACLE against the reference, never on the library: c_e = 4 x the worst
|lam_oracle - lam_numpy| / (2^-52 lam_max), c_t = 4 x the worst |pose_oracle - pose_reference|inf / (2^-52 (cond2 |d|inf + 1)) over every record of every case,
pose_oracle being gn_iterations' pose_after for its own H, g and x. The oracle's Jacobi and Cholesky are the algorithms the kernels restate, so the same constants
should bound the kernels; 4 is fit_tolerances.json's margin. tests/golden/deg_tolerances.json holds them (`python tests/test_deg_cases.py --write` rewrites it).
The measured quantities are a handful of float64 roundings of two eigen-solvers, one of them LAPACK's, whose kernels are picked by the CPU at hand: the file counts
as stale when the oracle no longer meets the committed bars (worst ratio > c) or the bars have become slack (worst ratio < committed worst / 4)."""
import json
import os
import sys

import numpy as np
import pytest

import deg_cases as dc

TOL_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deg_tolerances.json")
RATIO_SANITY = 64.0              # two backward-stable 6 x 6 symmetric eigen-solvers differ by a small multiple of 2^-52 lam_max; beyond this one of them is wrong
NOTE = ("worst |lam_oracle - lam_numpy| / (2^-52 lam_max) and worst |pose_oracle - pose_reference|inf / (2^-52 (cond2 |d|inf + 1)) of the oracle against "
        "deg_cases.reference_tail over the records of tests/deg_cases.py; c = 4 x ratio")


def tolerances():
    with open(TOL_PATH) as f:
        return json.load(f)


def measured(name, value, bar):
    print(f"DEG_MEASURED {name} {value:.3e} bar {bar:.1e}")


def projector_bar(ref, c_e):
    """entry-wise bar on a projector against the reference's: two solvers whose eigenvalues agree within c_e 2^-52 lam_max see matrices that far apart (backward
    stability), the invariant subspace behind a gap turns by at most 2 |dH| / gap (Davis-Kahan) and P = Q Q^T by twice that; + 8 roundings of the products"""
    k, lam = ref["k"], ref["lam"]
    gap = lam[k] - lam[k - 1]
    return (4.0 * c_e * lam[-1] / gap + 8.0) * dc.EPS


def _oracle_P(orc, H, thre, freeze):
    o = orc.eval_degeneracy(H, thre)
    if freeze and o["is_degenerate"]:
        o = dict(o, V_update=np.zeros((6, 6)))
    return o


def measure(orc):
    """the worst ratios of the oracle against the reference over every record"""
    worst = dict(c_e=0.0, c_t=0.0)
    for c in dc.CASES:
        for label, H, thre, _rank, _freeze in dc.records(c):
            lam = np.linalg.eigvalsh(H)
            if lam[-1] > 0.0:
                worst["c_e"] = max(worst["c_e"], float(np.abs(orc.eval_degeneracy(H, thre)["eigval"] - lam).max() / (dc.EPS * lam[-1])))
        if c.kind != "lm":
            for label, r, thre, freeze in dc.gn_records(c):
                ref = dc.reference_tail(r["x"], r["H"], r["g"], thre, freeze)
                worst["c_t"] = max(worst["c_t"], float(np.abs(r["pose_after"] - ref["pose"]).max()) / dc.pose_scale(ref))
    return worst


def test_required_cases_are_present():
    names = [c.name for c in dc.CASES]
    assert len(set(names)) == len(names)
    assert sorted(dc.REQUIRED_NAMES) == sorted(names)
    assert [dc.BY_NAME[f"rank_{j}"].rank for j in range(7)] == list(range(7)) and [dc.BY_NAME[f"lm_rank_{j}"].rank for j in range(7)] == list(range(7))


@pytest.mark.parametrize("name", dc.REQUIRED_NAMES)
def test_margin_condition_and_rank(orc, name):
    """no eigenvalue of the oracle's H within MARGIN_ABS of the threshold, on every iteration; the reference and the oracle both discard `rank` directions there"""
    case = dc.BY_NAME[name]
    recs = dc.records(case)
    assert len(recs) == case.iters * (1 if case.kind != "blocks" else 2 * len(case.spot))
    for label, H, thre, rank, _freeze in recs:
        dist, m = dc.clearance(H, thre)
        measured(f"{name} {label} clearance of the threshold {thre:.6g}", dist, m)
        assert dc.margin_holds(H, thre), (name, label, dist, m)
        lam = np.linalg.eigvalsh(H)
        assert int(np.sum(lam < thre)) == rank, (name, label, lam, thre)
        o = orc.eval_degeneracy(H, thre)
        assert o["is_degenerate"] == (rank > 0) and int(np.sum(o["eigval"] < thre)) == rank, (name, label)
    if case.spot[0] in ("just_below", "just_above"):
        # the closest legal placements: MARGIN_ABS from the eigenvalue, a hundred Weyl bounds, and still far outside the shortcut's own 1e-9 band
        label, H, thre, rank, _ = recs[0]
        dist, m = dc.clearance(H, thre)
        assert dist <= m * (1.0 + 1e-9) and m > 1e3 * 1e-9 * thre
        assert dc.shortcut_clear(H, thre) == (rank == 0), name


def test_nothing_matches_is_the_zero_problem(orc):
    """H and g exactly zero: every eigenvalue 0, the fallback H + 1e-6 I solves, d = 0, and the expected pose is Plus(x, 0) -- the start pose up to the normalisation"""
    case = dc.BY_NAME["nothing_matches"]
    (label, r, thre, _), = dc.gn_records(case)
    assert (r["n_surf"], r["n_corner"]) == (0, 0) and not r["H"].any() and not r["g"].any()
    ref = dc.reference_tail(r["x"], r["H"], r["g"], thre)
    assert ref["fallback"] and ref["k"] == 6 and not ref["P"].any() and not ref["d"].any()
    assert float(np.abs(ref["pose"] - r["x"]).max()) <= 2 * dc.EPS and float(np.abs(r["pose_after"] - ref["pose"]).max()) <= 2 * dc.EPS


def _agrees(name, side, verdict_of, with_freeze):
    """one restatement's verdict, eigenvalues and V_update against reference_tail on every record of a case"""
    case = dc.BY_NAME[name]
    tol = tolerances()
    for label, H, thre, _rank, freeze in dc.records(case):
        freeze = freeze and with_freeze
        ref = dc.reference_tail(np.array([0, 0, 0, 0, 0, 0, 1.0]), H, np.zeros(6), thre, freeze)
        o = verdict_of(H, thre, freeze)
        assert o["is_degenerate"] == (ref["k"] > 0), (name, label, side)
        ev = np.asarray(o["eigval"])
        assert np.all(np.diff(ev) >= 0), (name, label, side)
        de, bar = float(np.abs(ev - ref["lam"]).max()), tol["c_e"] * dc.eig_scale(ref)
        measured(f"{name} {label} {side} eigenvalues", de, bar)
        assert de <= bar, (name, label, side, de, bar)
        dP = float(np.abs(o["V_update"] - ref["P"]).max())
        if ref["k"] in (0, 6) or freeze:
            assert dP == 0.0, (name, label, side, dP)
        else:
            measured(f"{name} {label} {side} V_update", dP, projector_bar(ref, tol["c_e"]))
            assert dP <= projector_bar(ref, tol["c_e"]), (name, label, side, dP)
            assert abs(np.trace(o["V_update"]) - (6 - ref["k"])) <= 64 * dc.EPS


@pytest.mark.parametrize("name", dc.REQUIRED_NAMES)
def test_the_oracle_agrees_with_the_reference_tail(orc, name):
    """oracle.eval_degeneracy against reference_tail: the verdict, the eigenvalues (ascending) within c_e 2^-52 lam_max, V_update entry by entry -- exactly I and
    exactly 0 at ranks 0 and 6 and on a frozen block"""
    _agrees(name, "oracle", lambda H, thre, freeze: _oracle_P(orc, H, thre, freeze), True)


@pytest.mark.parametrize("name", dc.REQUIRED_NAMES)
def test_the_references_own_lines_agree_with_the_reference_tail(orc, name):
    """the same for oracle.ref_eval_degeneracy, evalDegenracy compiled from the reference's own lines (the convention of tests/test_oracle_ref_pin.py)"""
    if orc.ref_lib() is None:
        pytest.skip("no reference build")
    _agrees(name, "reference lines", lambda H, thre, freeze: orc.ref_eval_degeneracy(H, thre), False)


@pytest.mark.parametrize("name", [c.name for c in dc.CASES if c.kind != "lm"])
def test_the_cases_bite(orc, name):
    """the pose one discarded direction more or fewer would give lies at least 1000 pose bars from the expected one, on every iteration: the step has a component
    along the eigenvector at the boundary. (nothing_matches has no boundary -- six equal eigenvalues, a zero step -- and is there for the fallback.)"""
    case = dc.BY_NAME[name]
    tol = tolerances()
    for label, r, thre, freeze in dc.gn_records(case):
        ref = dc.reference_tail(r["x"], r["H"], r["g"], thre)
        if name == "nothing_matches":
            assert dc.bite(r["x"], ref) == 0.0
            continue
        b, bar = dc.bite(r["x"], ref), tol["c_t"] * dc.pose_scale(ref)
        measured(f"{name} {label} bite", b, dc.BITE * bar)
        assert b >= dc.BITE * bar, (name, label, b, bar)
        # the oracle's own pose meets the GPU test's bar
        ref = dc.reference_tail(r["x"], r["H"], r["g"], thre, freeze)
        dp = float(np.abs(r["pose_after"] - ref["pose"]).max())
        measured(f"{name} {label} oracle pose_after", dp, bar)
        assert dp <= bar, (name, label, dp, bar)


def test_blocks_freeze_is_what_it_says(orc):
    """block 1 is not degenerate in phase 0 and moves; in phase 1 it is and comes back with the bits it went in with; block 0 discards one direction both times"""
    case = dc.BY_NAME["blocks_freeze"]
    ph = dc.solved_blocks(case)
    p0 = dc.start_pose(case)
    assert not any(r["is_degenerate"] for r in ph[0][1]["iters"]) and float(np.abs(ph[0][1]["pose"] - p0).max()) > 1e-3
    assert all(r["is_degenerate"] for r in ph[1][1]["iters"]) and np.array_equal(ph[1][1]["pose"], p0)
    for p in (0, 1):
        assert all(r["is_degenerate"] for r in ph[p][0]["iters"]) and float(np.abs(ph[p][0]["pose"] - p0).max()) > 1e-3
    assert np.array_equal(ph[0][0]["pose"], ph[1][0]["pose"])


def test_lm_cases_take_the_verdict_on_both_outer_iterations(orc):
    for name in dc.LM_NAMES:
        case = dc.BY_NAME[name]
        s = dc.solved_lm(case)
        assert len(s["outer"]) == 2 and [o["is_degenerate"] for o in s["outer"]] == [case.rank > 0] * 2, name
        assert all(o["n_surf_sel"] + o["n_corner_sel"] > 1000 for o in s["outer"]), name
    # rank 6 projects every step away: the pose does not move at all
    s = dc.solved_lm(dc.BY_NAME["lm_rank_6"])
    assert float(np.abs(s["pose"] - dc.start_pose(dc.BY_NAME["lm_rank_6"])).max()) <= 2 * dc.EPS


def test_tolerances_are_the_measured_ones(orc):
    tol, got = tolerances(), measure(orc)
    for c in ("c_e", "c_t"):
        measured(f"worst ratio {c}", got[c], tol["worst_ratio"][c])
        assert got[c] <= RATIO_SANITY, (c, got[c])
        assert tol[c] == 4.0 * tol["worst_ratio"][c], c
        assert tol["worst_ratio"][c] / 4.0 <= got[c] <= tol[c], (c, got[c], tol["worst_ratio"][c])


if __name__ == "__main__":
    if "--write" in sys.argv:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
        import oracle as O
        O.build()
        w = measure(O)
        doc = dict(note=NOTE, worst_ratio={c: w[c] for c in ("c_e", "c_t")}, **{c: 4.0 * w[c] for c in ("c_e", "c_t")})
        with open(TOL_PATH, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(doc)
