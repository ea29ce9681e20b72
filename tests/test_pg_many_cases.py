"""The CPU side of pose graphs with more than 128 loop edges (no GPU): that the graphs of tests/pg_many_cases.py have what tests/test_gpu_posegraph_many.py relies
on -- L, M, first, m against the blocked dense stage's panel width, loops onto the constant block, Huber-active loop edges, every Levenberg-Marquardt decision of
the restatement clear of its threshold --, that the two NumPy / SciPy transcriptions of one linear step (the band + low-rank split the device computes, and the sparse
LU that is E's reference) agree with the restatement's dense solve within the project's 1e-9 where that solve is affordable and with each other on E, and the
blocked stage's launch plan (m-loam_amd/csrc/pg_host.hpp) replayed by a stand-alone program under AddressSanitizer and UBSan for every L from 129 to the limit.

Measured here: band + low-rank against the dense solve 5.8e-13 (A), 5.4e-14 (B), 3.8e-13 (C), 2.8e-13 (D); the sparse route 2.1e-13, 2.5e-14, 1.4e-13, 1.9e-13; the two
against each other on E 9.4e-14. The smallest decision margin is 0.33 (relative) on the plain passes and 0.366 with two solves refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import pg_cases as pc
import pg_many_cases as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_LINEAR = 1e-9


@pytest.mark.parametrize("name", pm.MANY)
def test_graphs_have_what_the_table_claims(name):
    """L, M, first; m = 6 L against the panel width: A, A2, B, C, D end in a remainder panel, E is an exact multiple (the bordering row gets a row tile of its own),
    every graph has at least three panels, all lie above the default capacity and E exactly at the limit"""
    g, cur = pm.graph_many(name)
    _, L, M, first = pm.TABLE[name]
    assert (g.n_loops(cur), cur - g.earliest + 1, g.earliest) == (L, M, first)
    assert pm.CAP_DEFAULT < L <= pm.LOOPS_LIMIT
    m = 6 * L
    panels, rest = -(-m // pm.PANEL), m % pm.PANEL
    assert panels >= 3
    assert {"A": (13, 6), "A2": (13, 6), "B": (15, 4), "C": (25, 6), "D": (17, 26), "E": (96, 0)}[name] == (panels, rest)
    if name == "A":
        assert L == pm.CAP_DEFAULT + 1
    if name == "E":
        assert L == pm.LOOPS_LIMIT and -(-(m + 1) // pm.PANEL) == panels + 1
    if name == "A2":
        ga, _ = pm.graph_many("A")
        assert (g.loop_index[g.loop_index >= 0] == ga.loop_index[ga.loop_index >= 0]).all() and M != pm.TABLE["A"][2]


def test_header_and_binding_agree_on_the_constants(mla):
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    assert int(re.search(r"MLH_PG_LOOPS_LIMIT\s*=\s*(\d+)", hdr).group(1)) == pm.LOOPS_LIMIT == mla.PG_LOOPS_LIMIT
    host = open(os.path.join(ROOT, "m-loam_amd", "csrc", "pg_host.hpp")).read()
    assert int(re.search(r"PG_MAX_LOOPS\s*=\s*(\d+)", host).group(1)) == pm.CAP_DEFAULT
    assert int(re.search(r"PG_PANEL\s*=\s*(\d+)", host).group(1)) == pm.PANEL
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mlh_pg_reserve\s*\(\s*mlh_ctx\s*\*", hdr) and "mlh_pg_reserve" in mla.EXPORTED_SYMBOLS and callable(mla.Context.pg_reserve)


def test_d_has_loops_onto_the_constant_block_and_huber_active_edges():
    """35 of D's loop edges end on the constant block (local index 0); the loops perturbed by decimetres have |r| > 2 delta, the others |r| < delta / 2 ... as far as
    the drift over 35 steps allows: at least one edge is Huber-active and at least one inactive"""
    g, cur = pm.graph_many("D")
    lin = pm.edges("D")
    loops = lin["ij"][lin["is_loop"]]
    assert len(loops) == 175 and int((loops[:, 0] == 0).sum()) == 35
    norms = {}
    for i, j in loops:
        raw = pc.edge(g.poses[g.earliest + i], g.poses[g.earliest + j], g.loop_rel[g.earliest + j])[0]
        norms[int(j) + g.earliest] = float(np.linalg.norm(raw))
    far = [k for k in range(40, 180) if k % 17 == 0]
    assert len(far) >= 5 and all(norms[k] > 2 * pc.HUBER for k in far)
    assert sum(v > pc.HUBER for v in norms.values()) >= 1 and sum(v < pc.HUBER for v in norms.values()) >= 1


@pytest.mark.parametrize("name", pm.OPTIMIZE_MANY + ("A2", "forced"))
def test_lm_decisions_stay_clear_of_their_thresholds(name):
    """every decision quantity of the restatement's pass is at least DECISION_MARGIN (relative) from its threshold, so that rounding cannot flip a branch on the
    device; what the passes do: A, A2 5 iterations / 5 successful / iteration limit, B 5 / 4 / function tolerance, D 4 / 3 / function tolerance, no step rejected;
    A with the first two linear solves refused and 8 iterations: 8 / 6 / iteration limit, 2 refused, the restatement's read-back of the last radius 100067.2965818...
    (one evaluation late: see below)"""
    res = pm.forced_many()[1] if name == "forced" else pm.optimized_many(name)[1]
    print(f"PG_MANY {name}: {res.num_iterations} / {res.num_successful_steps} / {res.termination} cost {res.initial_cost!r} -> {res.final_cost!r} "
          f"min_margin {res.min_margin!r} rejected {res.n_rejected} refused {res.n_refused} solve_radius {res.solve_radius!r}")
    assert res.n_decisions >= 1
    for what in ("margin_relative_decrease", "margin_function", "margin_parameter", "margin_gradient", "margin_model"):
        assert getattr(res, what) >= pc.DECISION_MARGIN, (what, getattr(res, what))
    assert res.min_margin >= pc.DECISION_MARGIN and res.n_rejected == 0
    want = {"A": (5, 5, 0), "A2": (5, 5, 0), "B": (5, 4, 3), "D": (4, 3, 3), "forced": (8, 6, 0)}[name]
    assert (res.num_iterations, res.num_successful_steps, res.termination) == want
    assert res.final_cost < res.initial_cost and res.n_loops == pm.TABLE["A" if name == "forced" else name][1]
    if name == "forced":
        # the read-back 100067.29... is NOT the last system's radius here (the pass's last step is accepted: pg_many_cases.forced_many_radius says why and
        # reads it back validly): two halvings (/ 2, / 4), then five successes with a relative decrease near 1 (x 3 each) before the eighth system
        assert res.n_refused == 2 and abs(res.solve_radius / 100067.2965818 - 1) < 1e-9 and res.min_margin > 0.3
        assert abs(pm.forced_many_radius() / (1e4 / 2 / 4 * 3 ** 5) - 1) < 1e-9
        assert abs(pm.graph_many("A")[0].optimize(pm.TABLE["A"][0], max_num_iterations=1)[1].solve_radius / 1e4 - 1) > 0.1     # the same flaw, first system: 1e4
    else:
        assert res.n_refused == 0


@pytest.mark.parametrize("name", pm.STEP_MANY)
def test_transcriptions_agree_with_the_restated_dense_solve(name):
    """the band + low-rank split (what the device computes) and the sparse LU (E's reference), each against the restatement's dense Cholesky: within 1e-9 of the
    largest entry of the step"""
    want = pm.restated_step(name)
    assert want["ok"]
    for tag, got in (("lowrank", pm.lowrank_step(name)), ("sparse", pm.sparse_step(name))):
        ds, dd = pm.rel(got["step"], want["step"]), pm.rel(got["delta"], want["delta"])
        print(f"PG_MANY step {name} {tag}: step {ds:.3e} delta {dd:.3e} bar {BAR_LINEAR:.1e}")
        assert ds <= BAR_LINEAR and dd <= BAR_LINEAR


def test_transcriptions_agree_with_each_other_at_the_limit():
    """E (L = 1024): no dense n x n solve is affordable; the two routes share the restatement's edges and nothing else"""
    a, b = pm.lowrank_step("E"), pm.sparse_step("E")
    ds, dd = pm.rel(a["step"], b["step"]), pm.rel(a["delta"], b["delta"])
    print(f"PG_MANY step E lowrank vs sparse: step {ds:.3e} delta {dd:.3e} cond(C) >= {a['cond_C_lower_bound']:.1f}")
    assert ds <= BAR_LINEAR and dd <= BAR_LINEAR and np.abs(b["step"]).max() > 0


def _plan_main(tmp_path):
    exe = tmp_path / "pg_plan_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pg_plan_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


def test_launch_plan_under_sanitizers_for_every_l_above_the_cap(tmp_path):
    """pg_host.hpp's plan of the blocked dense stage, in a stand-alone program built with -fsanitize=address,undefined and run directly (nothing is loaded into
    Python): for every m = 6 L, L = 129 .. 1024, every tile of the lower triangle and the bordering row is summed once, updated once (past the first panel, after
    all it reads is final) and factored or solved once; every row tile of the backward substitution is solved once after one update per later panel; no tile is
    touched twice in one launch; the stage takes 3 ceil(m / 64) launches, so that a pass reports 3 + (9 + 3 ceil(m / 64)) max_num_iterations + 1"""
    exe = _plan_main(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"pg_plan: ok ({pm.CAP_DEFAULT + 1} .. {pm.LOOPS_LIMIT})" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    for name in pm.MANY:
        m = 6 * pm.TABLE[name][1]
        r = subprocess.run([exe, "count", str(m)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "pg_plan: ok" in r.stdout, (r.stdout, r.stderr[-3000:])
        n, T, Tb = (int(v) for v in r.stdout.split("\n")[0].split()[1:])
        assert (n, T, Tb) == (3 * -(-m // pm.PANEL), -(-m // pm.PANEL), -(-(m + 1) // pm.PANEL))
        assert launches_of_a_pass(m, pc.MAX_IT) == 3 + (9 + n) * pc.MAX_IT + 1


def launches_of_a_pass(m, max_it):
    """what mlh_pg_result::launches reports for L > 128: begin (3), per iteration assemble, band factor, substitution, Gram, the blocked stage's 3 ceil(m / 64),
    y_b - Y z, the back-substitution, candidate, linearise, decide; the write-back"""
    return 3 + (9 + 3 * -(-m // pm.PANEL)) * max_it + 1
