"""The Levenberg-Marquardt loop on the crafted starts of tests/lm_cases.py, on the CPU: the NumPy trace (lm_cases.lm_trace) and the C++ restatement under
oracle.scan2map / oracle.track_cloud (oracle/lm.hpp) agree on every case, the tracker's hand-made clouds included -- counts, terminations and evaluations equal, costs within 1e-12 relative, poses within
1e-11, the bars of scripts/soak_ref_pin.py -- and so do the reference's own scan2MapOptimization lines where oracle/_ref is built. Every case reaches the branch
it is named for, asserted on the trace's accept / reject sequence, radii, reuse flags and decrease factors; every decision quantity of every iteration keeps
DECISION_MARGIN from its threshold; and a trace with the acceptance test or the diagonal reuse changed leaves the bars tests/test_gpu_lm_cases.py holds the device
to, so those bars do tell a loop that handles a rejected step differently from this one."""
import numpy as np
import pytest

import lm_cases as lm

COST_TOL, POSE_TOL = 1e-12, 1e-11
GPU_COST_BAR, GPU_POSE_BAR = 1e-9, 1e-7            # what tests/test_gpu_lm_cases.py holds the statistics path to
MAPPER = [c.name for c in lm.CASES]


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def outer_flags(case):
    return [lm.flags(o["trace"]) for o in lm.traced(case)["outer"]]


@pytest.mark.parametrize("name", MAPPER)
def test_the_trace_and_the_oracle_agree(name):
    case = lm.BY_NAME[name]
    tr, res = lm.traced(case), lm.oracle_solved(case)
    assert len(tr["outer"]) == len(res["outer"]) == dict(case.opts).get("max_outer", 2)
    for i, (a, b) in enumerate(zip(tr["outer"], res["outer"])):
        s = a["trace"]["summary"]
        assert (a["n_surf"], a["n_corner"], a["is_degenerate"]) == (b["n_surf_sel"], b["n_corner_sel"], b["is_degenerate"]), (name, i)
        assert (s["lm_iterations"], s["successful_steps"], s["termination"], s["evaluations"]) == \
               (b["lm_iterations"], b["successful_steps"], b["termination"], b["evaluations"]), (name, i, lm.flags(a["trace"]), s, b)
        dc = max(rel(s["initial_cost"], b["initial_cost"]), rel(s["final_cost"], b["final_cost"]))
        dp = float(np.abs(a["pose_after"] - b["pose_after"]).max())
        print(f"LM_MEASURED {name} outer {i}: {lm.flags(a['trace']) or '-'} termination {s['termination']} |dcost|/cost {dc:.2e} |dpose| {dp:.2e} margin {a['trace']['margin']:.2e}")
        assert dc <= COST_TOL and dp <= POSE_TOL, (name, i, dc, dp)
    assert np.abs(tr["pose"] - res["pose"]).max() <= POSE_TOL


@pytest.mark.parametrize("name", [c.name for c in lm.CASES if not c.opts])
def test_the_references_own_lines_agree(name, orc):
    """scan2MapOptimization compiled from the reference's lines (its own matching, block assembly, evalDegenracy and outer loop; default options only)"""
    if orc.ref_lib() is None:
        pytest.skip("oracle/_ref/libmloam_ref.so has not been built (needs the reference tree once)")
    case = lm.BY_NAME[name]
    sc = lm.SCENES[case.family](case.seed)
    ref = orc.ref_scan2map(sc["surf_map"], sc["corner_map"], sc["surf"], sc["corner"], lm.start_pose(case))
    tr = lm.traced(case)
    assert len(ref["solves"]) == len(tr["outer"])
    for i, (a, b) in enumerate(zip(tr["outer"], ref["solves"])):
        s = a["trace"]["summary"]
        assert (a["n_surf"] + a["n_corner"], s["lm_iterations"], s["successful_steps"], s["termination"]) == \
               (b["n_blocks"], b["lm_iterations"], b["successful_steps"], b["termination"]), (name, i, s, b)
        assert max(rel(s["initial_cost"], b["initial_cost"]), rel(s["final_cost"], b["final_cost"])) <= COST_TOL, (name, i)
    assert np.abs(tr["pose"] - ref["pose"]).max() <= POSE_TOL, name


@pytest.mark.parametrize("name", MAPPER)
def test_every_decision_keeps_its_margin(name):
    for i, o in enumerate(lm.traced(lm.BY_NAME[name])["outer"]):
        assert o["trace"]["margin"] >= lm.DECISION_MARGIN, (name, i, o["trace"]["margin"])


def _growth(rd):
    return 1.0 / max(1.0 / 3.0, 1.0 - (2.0 * rd - 1.0) ** 3)


def test_a_single_rejection_then_an_acceptance():
    found = 0
    for o, f in zip(lm.traced(lm.BY_NAME["a_single_rejection"])["outer"], outer_flags(lm.BY_NAME["a_single_rejection"])):
        it = o["trace"]["iters"]
        for i in range(1, len(f) - 2):
            if f[i - 1:i + 2] != "ARA":
                continue
            found += 1
            r, a, n = it[i], it[i + 1], it[i + 2]
            assert (r["reuse_diagonal"], r["decrease_factor"]) == (False, 2.0)                    # behind an accepted step: a fresh diagonal
            assert r["rd"] <= 1e-3 and r["valid"]
            assert (a["reuse_diagonal"], a["decrease_factor"], a["radius"]) == (True, 4.0, r["radius"] / 2.0)
            assert a["cost"] == r["cost"] and a["gmax"] == r["gmax"]                              # proposed again from the same record
            assert (n["reuse_diagonal"], n["decrease_factor"]) == (False, 2.0)                    # back to 2, the diagonal recomputed
            assert n["radius"] == min(lm.MAX_RADIUS, a["radius"] * _growth(a["rd"])) and n["cost"] == a["candidate_cost"]
    assert found >= 2, outer_flags(lm.BY_NAME["a_single_rejection"])


def test_b_rejections_in_a_row_radii_by_hand():
    case = lm.BY_NAME["b_rejections_in_a_row"]
    assert outer_flags(case) == ["ARRRRRRRT", "RRRRAARRRRT"]
    it = lm.traced(case)["outer"][1]["trace"]["iters"]
    # from 1e4: / 2, / 4, / 8, / 16 -- 10000, 5000, 1250, 156.25, 9.765625 (all exact in binary floating point), the fifth iteration accepted at 9.765625
    assert [r["radius"] for r in it[:5]] == [1e4, 5e3, 1250.0, 156.25, 9.765625]
    assert [r["decrease_factor"] for r in it[:5]] == [2.0, 4.0, 8.0, 16.0, 32.0]
    assert [r["reuse_diagonal"] for r in it[:5]] == [False, True, True, True, True]
    assert [r["accepted"] for r in it[:6]] == [False, False, False, False, True, True]
    assert all(r["cost"] == it[0]["cost"] and r["gmax"] == it[0]["gmax"] for r in it[:5])
    assert (it[5]["reuse_diagonal"], it[5]["decrease_factor"]) == (False, 2.0) and it[5]["radius"] == 9.765625 * _growth(it[4]["rd"])
    # ... and the second run of this outer iteration, from wherever the two accepted steps left the radius: / 2, / 4, / 8
    r6 = it[6]["radius"]
    assert [r["radius"] for r in it[6:10]] == [r6, r6 / 2.0, r6 / 8.0, r6 / 64.0]
    # outer iteration 0: seven in a row behind one accepted step at the cap (1e4 * 3)
    it0 = lm.traced(case)["outer"][0]["trace"]["iters"]
    assert [r["radius"] for r in it0[:4]] == [1e4, 3e4, 1.5e4, 3750.0] and it0[0]["radius_growth"] == 3.0


def test_c_the_first_iteration_of_an_outer_iteration_is_rejected():
    case = lm.BY_NAME["c_first_iteration_rejected"]
    f = outer_flags(case)
    assert f[1].startswith("RRRRRA") and f[0][0] == "A", f
    o = lm.traced(case)["outer"][1]
    it = o["trace"]["iters"]
    assert not it[0]["accepted"] and it[0]["valid"] and it[0]["rd"] <= 1e-3 and it[0]["radius"] == 1e4
    # the second proposal is built from the record the begin evaluated (same cost, same gradient), with the begin's diagonal and half the radius
    assert it[1]["cost"] == it[0]["cost"] == o["trace"]["summary"]["initial_cost"] and it[1]["gmax"] == it[0]["gmax"]
    assert (it[1]["reuse_diagonal"], it[1]["decrease_factor"], it[1]["radius"]) == (True, 4.0, 5e3)
    assert o["trace"]["summary"]["successful_steps"] == f[1].count("A") >= 1


def test_d_the_budget_ends_on_a_rejected_step():
    case = lm.BY_NAME["d_budget_ends_on_a_rejection"]
    assert outer_flags(case) == ["AAAARRAAAAAAR", "AAAAAAARAAARR"]
    for o in lm.traced(case)["outer"]:
        s, it = o["trace"]["summary"], o["trace"]["iters"]
        assert s["termination"] == lm.NO_CONVERGENCE and s["lm_iterations"] == 13
        last_ok = [r for r in it if r["accepted"]][-1]
        assert np.array_equal(o["pose_after"], last_ok["candidate"]) and s["final_cost"] == last_ok["candidate_cost"]
        # the rejected candidate is far enough from the accepted pose that returning it would leave the GPU bar
        assert np.abs(it[-1]["candidate"] - o["pose_after"]).max() > 100 * GPU_POSE_BAR
        assert rel(it[-1]["candidate_cost"], s["final_cost"]) > 100 * GPU_COST_BAR
        # ... and so would a covariance inverted from the rejected candidate's record instead of the accepted pose's (the 1e-9 bar on H_final)
        H = o["trace"]["last"]["H"]
        assert np.array_equal(H, last_ok["candidate_H"]) and np.abs(it[-1]["candidate_H"] - H).max() > 100 * 1e-9 * np.abs(H).max()


def test_the_other_cases_reach_their_branches():
    f = outer_flags(lm.BY_NAME["e_termination_after_rejections"])
    tr = lm.traced(lm.BY_NAME["e_termination_after_rejections"])
    assert all(x.endswith("RRRRRRRT") for x in f) and all(o["trace"]["summary"]["termination"] == lm.FUNCTION for o in tr["outer"])
    assert all(o["trace"]["iters"][-1]["reuse_diagonal"] and o["trace"]["iters"][-1]["decrease_factor"] == 256.0 for o in tr["outer"])

    tr = lm.traced(lm.BY_NAME["f_degenerate_with_rejections"])
    for o, x in zip(tr["outer"], outer_flags(lm.BY_NAME["f_degenerate_with_rejections"])):
        V = o["V_update"]
        assert o["is_degenerate"] and x.count("R") >= 3
        assert np.abs(V @ V - V).max() < 1e-9 and np.linalg.matrix_rank(V, tol=1e-6) < 6                      # a projector that removes a direction

    assert "RA" in outer_flags(lm.BY_NAME["f_degenerate_with_rejections"])[0]                                 # ... and goes on behind rejected steps

    tr = lm.traced(lm.BY_NAME["g_zero_gradient"])
    for o in tr["outer"]:
        s = o["trace"]["summary"]
        assert (o["n_surf"], o["n_corner"]) == (147, 72) and not o["trace"]["iters"]
        assert (s["termination"], s["lm_iterations"], s["successful_steps"], s["evaluations"]) == (lm.GRADIENT, 0, 0, 1)
        assert s["initial_cost"] == 0.0 and not o["trace"]["last"]["g"].any() and np.abs(o["trace"]["last"]["H"]).max() > 100.0
    assert np.array_equal(tr["pose"], lm.start_pose(lm.BY_NAME["g_zero_gradient"]))

    tr = lm.traced(lm.BY_NAME["p_parameter_tolerance"])
    o = tr["outer"][0]["trace"]
    assert o["summary"]["termination"] == lm.PARAMETER and lm.flags(o) == "AAAARRRRRRRT" and o["iters"][-1]["par_ratio"] <= 1.0 and o["iters"][-1]["fn_ratio"] is None
    assert o["iters"][-2]["par_ratio"] > 1.0 and o["iters"][-2]["fn_ratio"] > lm.FUNCTION_TOL

    o = lm.traced(lm.BY_NAME["q_radius_growth_capped"])["outer"][0]["trace"]
    assert lm.flags(o) == "A" * 27 + "RRR" and o["summary"]["termination"] == lm.NO_CONVERGENCE and o["summary"]["lm_iterations"] == 30
    capped = [i for i, r in enumerate(o["iters"]) if r.get("radius_growth") == 3.0]
    assert len(capped) >= 7 and all(o["iters"][i + 1]["radius"] == 3.0 * o["iters"][i]["radius"] for i in capped)
    assert max(r["radius"] for r in o["iters"]) < lm.MAX_RADIUS and min(r["radius"] for r in o["iters"]) > lm.MIN_RADIUS

    tr = lm.traced(lm.BY_NAME["r_radius_limit"])
    o = tr["outer"][1]["trace"]
    assert not tr["outer"][1]["is_degenerate"] and np.array_equal(tr["outer"][1]["V_update"], np.eye(6))
    assert lm.flags(o) == "A" * 27 + "T" and o["summary"]["termination"] == lm.FUNCTION
    assert all(r["radius_growth"] == 3.0 for r in o["iters"][:27])
    assert [r["radius"] for r in o["iters"][:26]] == [1e4 * 3.0 ** k for k in range(26)]                      # (products of 3 below 2^53: exact)
    assert o["iters"][25]["radius"] * 3.0 > lm.MAX_RADIUS and o["iters"][26]["radius"] == o["iters"][27]["radius"] == lm.MAX_RADIUS


@pytest.mark.parametrize("mutation", [dict(min_relative_decrease=0.5), dict(reuse_diagonal_after_rejection=False)])
def test_the_bar_bites(mutation):
    """the same cases under a loop that accepts on rd > 0.5 instead of rd > 1e-3, and under one that does not keep the diagonal behind a rejected step: the counts
    change or the poses move by more than the bars the device is held to, on each of the cases a, b and c"""
    for name in ("a_single_rejection", "b_rejections_in_a_row", "c_first_iteration_rejected"):
        case = lm.BY_NAME[name]
        good = lm.traced(case)
        bad = lm.traced(case, **mutation)
        counts = lambda t: [(o["trace"]["summary"]["lm_iterations"], o["trace"]["summary"]["successful_steps"], o["trace"]["summary"]["termination"]) for o in t["outer"]]
        dp = float(np.abs(good["pose"] - bad["pose"]).max())
        dc = max(rel(a["trace"]["summary"]["final_cost"], b["trace"]["summary"]["final_cost"]) for a, b in zip(bad["outer"], good["outer"]))
        print(f"LM_MEASURED mutation {mutation} {name}: counts {counts(bad)} vs {counts(good)} |dpose| {dp:.2e} |dcost|/cost {dc:.2e}")
        assert counts(bad) != counts(good) or dp > GPU_POSE_BAR, (name, mutation)
        assert dp > GPU_POSE_BAR or dc > GPU_COST_BAR, (name, mutation, dp, dc)


TRACK_FLAGS = {"h_rejections_in_a_round": ["AAARRRRAAAAAAAA", "AAAAAAT"], "h_first_iteration_rejected": ["RRRAAAAAAT", "AAAAT"],
               "h_default_budget_ends_on_a_rejection": ["AAAR", "AAAA"], "h_budget_ends_on_three_rejections": ["AAARRR", "AAAAAT"]}


@pytest.mark.parametrize("name", [c.name for c in lm.TRACK_CASES])
def test_h_the_tracker_rejects_steps_inside_a_round(name):
    """trackCloud on hand-made clouds (lm_cases.track_clouds): the trace and oracle.track_cloud agree -- counts, accepted steps, terminations and evaluations equal,
    costs and poses at the bars above --, every decision keeps its margin, and each case's accept / reject sequence is the one written down here"""
    case = lm.TRACK_BY_NAME[name]
    tr, res = lm.track_traced(case), lm.track_oracle_solved(case)
    assert [lm.flags(r["trace"]) for r in tr["outer"]] == TRACK_FLAGS[name]
    for i, (a, b) in enumerate(zip(tr["outer"], res["outer"])):
        s = a["trace"]["summary"]
        assert (a["n_corner"], a["n_surf"], a["solved"]) == (b["n_corner"], b["n_surf"], b["solved"]) == (1, 12, True)
        assert (s["lm_iterations"], s["successful_steps"], s["termination"], s["evaluations"]) == (b["lm_iterations"], b["successful_steps"], b["termination"], b["evaluations"])
        dc = max(rel(s["initial_cost"], b["initial_cost"]), rel(s["final_cost"], b["final_cost"]))
        dp = float(np.abs(a["pose_after"] - b["pose_after"]).max())
        print(f"LM_MEASURED {name} round {i}: {lm.flags(a['trace'])} termination {s['termination']} |dcost|/cost {dc:.2e} |dpose| {dp:.2e} margin {a['trace']['margin']:.2e}")
        assert dc <= COST_TOL and dp <= POSE_TOL and a["trace"]["margin"] >= lm.DECISION_MARGIN
    assert np.abs(tr["pose"] - res["pose"]).max() <= POSE_TOL
    it = tr["outer"][0]["trace"]["iters"]
    k = TRACK_FLAGS[name][0].index("R")                                  # the first rejection of round 0 and the run behind it
    run = len(TRACK_FLAGS[name][0][k:]) - len(TRACK_FLAGS[name][0][k:].lstrip("R"))
    assert [r["radius"] for r in it[k:k + run]] == [it[k]["radius"] / 2.0 ** (j * (j + 1) // 2) for j in range(run)]
    assert [r["decrease_factor"] for r in it[k:k + run]] == [2.0 ** (j + 1) for j in range(run)]
    assert [r["reuse_diagonal"] for r in it[k:k + run]] == [False] + [True] * (run - 1)
    assert all(r["cost"] == it[k]["cost"] and r["gmax"] == it[k]["gmax"] for r in it[k:k + run])
    if k == 0:
        assert it[0]["radius"] == 1e4 and it[0]["cost"] == tr["outer"][0]["trace"]["summary"]["initial_cost"]
    if k + run < len(it):                                                # an acceptance follows: the kept diagonal, then a fresh one and factor 2
        assert it[k + run]["accepted"] and it[k + run]["reuse_diagonal"] and it[k + run]["decrease_factor"] == 2.0 ** (run + 1)
        assert (it[k + run + 1]["reuse_diagonal"], it[k + run + 1]["decrease_factor"]) == (False, 2.0)
    else:                                                                # the budget ends on the rejection: the last accepted pose goes on to round 1
        last_ok = [r for r in it if r["accepted"]][-1]
        assert tr["outer"][0]["trace"]["summary"]["termination"] == lm.NO_CONVERGENCE and np.array_equal(tr["outer"][0]["pose_after"], last_ok["candidate"])
        assert np.abs(it[-1]["candidate"] - last_ok["candidate"]).max() > 100 * 1e-9          # (the tracker's pose bar is 1e-9)


def test_the_bar_bites_on_the_tracker():
    for name in ("h_rejections_in_a_round", "h_first_iteration_rejected"):
        case = lm.TRACK_BY_NAME[name]
        good = lm.track_traced(case)
        for mutation in (dict(min_relative_decrease=0.5), dict(reuse_diagonal_after_rejection=False)):
            bad = lm.track_traced(case, **mutation)
            dp = float(np.abs(good["pose"] - bad["pose"]).max())
            print(f"LM_MEASURED mutation {mutation} {name}: {[lm.flags(o['trace']) for o in bad['outer']]} |dpose| {dp:.2e}")
            assert dp > 100 * 1e-9, (name, mutation, dp)
