"""The pose-graph optimisation's CPU side (no GPU): the restatement tests/host/pg_ref.cpp (through tests/pg_cases.py) against hand-computed edges and central
differences; m-loam_amd/csrc/pg_host.hpp -- the closed-form edge arithmetic the kernels run -- in a stand-alone program under AddressSanitizer and UBSan against
that restatement; and the properties of the crafted graphs that tests/test_gpu_posegraph.py relies on: every Levenberg-Marquardt decision of the restatement at
least 1e-6 (relative) from its threshold, the 170-degree case short of one successful step per iteration, Huber active and inactive loop edges, loops onto the
constant block and inside the band."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID = np.array([0, 0, 0, 0, 0, 0, 1.0])
PG_SYMBOLS = ["mlh_pg_reset", "mlh_pg_info", "mlh_pg_add_keyframe", "mlh_pg_set_loop", "mlh_pg_optimize", "mlh_pg_poses", "mlh_pg_device_poses", "mlh_pg_linearize",
              "mlh_pg_solve_step", "mlh_pg_time_stages", "mlh_pg_optimize_forced"]


def _yaw(deg):
    h = np.deg2rad(deg) / 2
    return np.array([0, 0, np.sin(h), np.cos(h)])


def test_edge_at_identity_with_an_exact_measurement():
    """r = 0; d r_t / d t_i = -I / t_var, d r_t / d t_j = I / t_var; d r_q / d rot_j = (2 / q_var) I and its negative for i; the other blocks vanish"""
    r, Ji, Jj = pc.edge(ID, ID, ID)
    assert (r == 0).all()
    want_j = np.zeros((6, 6))
    want_j[:3, 3:] = np.eye(3) / pc.T_VAR
    want_j[3:, :3] = np.eye(3) * 2 / pc.Q_VAR
    np.testing.assert_allclose(Jj, want_j, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Ji, -want_j, rtol=0, atol=1e-12)


def test_edge_with_a_pure_translation():
    """identity rotations, t_j - t_i = (1, 2, 3), measured (0.5, 2, 3.25): r_t = (0.5, 0, -0.25) / 0.1; d r_t / d rot_i = (2 / t_var) [v]x"""
    pj = ID.copy()
    pj[:3] = (1, 2, 3)
    meas = ID.copy()
    meas[:3] = (0.5, 2, 3.25)
    r, Ji, Jj = pc.edge(ID, pj, meas)
    np.testing.assert_allclose(r, [5.0, 0.0, -2.5, 0, 0, 0], rtol=0, atol=1e-13)
    vx = np.array([[0, -3, 2], [3, 0, -1], [-2, 1, 0.0]])
    np.testing.assert_allclose(Ji[:3, :3], 2 / pc.T_VAR * vx, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Jj[:3, :3], 0, atol=0)


def test_edge_with_a_quarter_turn_of_yaw():
    """q_i = identity, q_j = 90 degrees about z, measured identity: the quaternion mismatch is q_j, so r_q = 2 (0, 0, sin 45) / q_var = (0, 0, 141.42...). With q_i = q_j = that
    yaw, t_j - t_i = (0, 1, 0) world is (1, 0, 0) in frame i; measured (0.8, 0, 0): r_t = (0.2, 0, 0) / t_var = (2, 0, 0)"""
    pj = ID.copy()
    pj[3:] = _yaw(90)
    r, _, _ = pc.edge(ID, pj, ID)
    np.testing.assert_allclose(r, [0, 0, 0, 0, 0, 2 * np.sqrt(0.5) / pc.Q_VAR], rtol=0, atol=1e-12)
    pi = ID.copy()
    pi[3:] = _yaw(90)
    pj[:3] = (0, 1, 0)
    meas = ID.copy()
    meas[:3] = (0.8, 0, 0)
    r, _, _ = pc.edge(pi, pj, meas)
    np.testing.assert_allclose(r, [2.0, 0, 0, 0, 0, 0], rtol=0, atol=1e-12)


def _random_pose(rng, unit=True):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    if not unit:
        q *= 1.0 + 1e-3 * rng.normal()
    return np.concatenate([rng.uniform(-20, 20, 3), q])


def test_dual_number_jacobians_against_central_differences():
    """the autodiff-times-parameterisation Jacobian of the restatement is the derivative of r along QuaternionParameterization::Plus: central differences with
    h = 1e-6 (truncation h^2 |r'''| ~ 1e-12 x 200 x 20, rounding 1e-16 x 4000 / h ~ 4e-7): within 1e-5 absolute on entries up to 4000"""
    rng = np.random.default_rng(3)
    h = 1e-6
    for trial in range(8):
        pi, pj, meas = _random_pose(rng, trial % 2 == 0), _random_pose(rng, trial % 2 == 0), _random_pose(rng)
        _, Ji, Jj = pc.edge(pi, pj, meas)
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            num_i = (pc.edge(pc.plus(pi, d), pj, meas)[0] - pc.edge(pc.plus(pi, -d), pj, meas)[0]) / (2 * h)
            num_j = (pc.edge(pi, pc.plus(pj, d), meas)[0] - pc.edge(pi, pc.plus(pj, -d), meas)[0]) / (2 * h)
            np.testing.assert_allclose(Ji[:, c], num_i, rtol=0, atol=1e-5)
            np.testing.assert_allclose(Jj[:, c], num_j, rtol=0, atol=1e-5)


def _host_main(tmp_path):
    exe = tmp_path / "pg_host_main"
    if not exe.exists():
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pg_host_main.cpp"), "-o", str(exe)]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pg_host: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    return {ln.split()[0]: np.array(ln.split()[1:], np.float64) for ln in r.stdout.splitlines() if ln and ln.split()[0] in "RIJPMVS"}


def test_host_arithmetic_under_sanitizers_against_the_restatement(tmp_path):
    """pg_host.hpp in a stand-alone program built with -fsanitize=address,undefined and run directly: its own checks pass; its closed-form residual and Jacobians
    agree with the restatement's dual numbers to 1e-12 of the largest entry (unit and slightly non-unit quaternions), Plus to 1e-15, pose compose / inverse to 1e-15;
    the sequential measurement makes its own edge's residual vanish in the restatement too"""
    exe = _host_main(tmp_path)
    _run(exe)
    rng = np.random.default_rng(9)
    for k in range(8):
        pi, pj, meas = _random_pose(rng, k % 2 == 0), _random_pose(rng, k % 2 == 0), _random_pose(rng)
        f = tmp_path / f"edge_{k}.f64"
        np.concatenate([pi, pj, meas]).tofile(f)
        out = _run(exe, "edge", f)
        r, Ji, Jj = pc.edge(pi, pj, meas)
        scale = max(np.abs(Ji).max(), np.abs(Jj).max())
        np.testing.assert_allclose(out["R"], r, rtol=0, atol=1e-12 * max(1.0, np.abs(r).max()))
        np.testing.assert_allclose(out["I"].reshape(6, 6), Ji, rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(out["J"].reshape(6, 6), Jj, rtol=0, atol=1e-12 * scale)
        d = rng.normal(size=6) * (0.0 if k == 7 else 0.1)
        g = tmp_path / f"plus_{k}.f64"
        np.concatenate([pi, d]).tofile(g)
        np.testing.assert_allclose(_run(exe, "plus", g)["P"], pc.plus(pi, d), rtol=0, atol=1e-15 * 20)
        a, b = _random_pose(rng), _random_pose(rng)
        c = tmp_path / f"compose_{k}.f64"
        np.concatenate([a, b]).tofile(c)
        out = _run(exe, "compose", c)
        np.testing.assert_allclose(out["M"], pc.pose_mul(a, b), rtol=0, atol=1e-15 * 60)
        np.testing.assert_allclose(out["V"], pc.pose_inverse(a), rtol=0, atol=1e-15 * 60)
        r, _, _ = pc.edge(a, b, out["S"])
        assert np.abs(r).max() < 1e-11


def test_crafted_linearisation_graph_has_every_kind_of_loop_edge():
    """what the GPU linearisation test relies on: at M = 2, 5, 6, 70 the loop edges of the graph include one onto the constant block, one with both ends inside the
    band, one with |r| < delta (Huber inactive) and one with |r| > delta (active); edge counts are 4 per keyframe less the missing ones at the start, plus L"""
    G = pc.graph_linearize()
    assert G.earliest == 0
    for cur, n_loops in zip(pc.LINEARIZE_CURS, (1, 3, 4, 7)):
        M = cur + 1
        lin = G.linearize(cur)
        n_seq = sum(min(i, 4) for i in range(M))
        assert len(lin["ij"]) == n_seq + n_loops and G.n_loops(cur) == n_loops
    lin = G.linearize(69)
    loops = {}
    for e, (i, j) in enumerate(lin["ij"]):
        if G.loop_index[j] == i and (e + 1 == len(lin["ij"]) or lin["ij"][e + 1][1] != j):
            raw = pc.edge(G.poses[i], G.poses[j], G.loop_rel[j])[0]
            loops[(int(j), int(i))] = float(np.linalg.norm(raw))
    assert set(loops) == {(1, 0), (3, 1), (4, 0), (5, 2), (40, 10), (60, 3), (69, 66)}
    assert loops[(40, 10)] > 2 * pc.HUBER and loops[(60, 3)] > 2 * pc.HUBER                 # active, clear of the corner
    assert all(loops[k] < 0.5 * pc.HUBER for k in ((1, 0), (3, 1), (4, 0), (5, 2), (69, 66)))   # inactive


@pytest.mark.parametrize("name", pc.OPTIMIZE_CASES + ("second",))
def test_lm_decisions_stay_clear_of_their_thresholds(name):
    """every decision quantity of the restatement's run -- the relative decrease against 1e-3, the function, parameter and gradient tolerances, the sign of the model
    cost change -- is at least 1e-6 (relative) from its threshold, so that rounding cannot flip a branch on the device"""
    res = pc.second_pass()[2] if name == "second" else pc.optimized(name)[1]
    assert res.n_decisions >= 1
    for what in ("margin_relative_decrease", "margin_function", "margin_parameter", "margin_gradient", "margin_model"):
        assert getattr(res, what) >= pc.DECISION_MARGIN, (what, getattr(res, what))
    assert res.min_margin >= pc.DECISION_MARGIN


def test_the_crafted_passes_do_what_they_are_for():
    """converge: two loop edges, the cost falls by more than half within the iteration limit; rejected (a loop measurement 170 degrees from the truth):
    num_successful_steps < num_iterations; L0: no loop edge in first..cur, termination by the gradient tolerance at iteration 0; the second pass starts from the
    first one's poses and has one more loop edge"""
    g, res = pc.optimized("converge")
    assert res.n_loops == 2 and res.num_successful_steps >= 2 and res.final_cost < 0.5 * res.initial_cost and res.termination in (0, 1, 2, 3)
    _, res = pc.optimized("rejected")
    assert res.n_loops == 1 and res.num_iterations >= 1 and res.num_successful_steps < res.num_iterations
    _, res = pc.optimized("L0")
    assert res.n_loops == 0 and res.num_iterations == 0 and res.termination == 1
    before, after, res = pc.second_pass()
    assert res.n_loops == 3 and (before.poses == pc.optimized("converge")[0].poses).all()


def test_forced_invalid_steps_follow_the_policy_by_hand():
    """No crafted graph makes the solver turn a step down by itself (the 170-degree pass has n_rejected == 0: its shortfall is the terminating iteration), so the
    invalid-step branch is driven by refusing chosen linear solves. By hand from the policy (radius /= decrease_factor, decrease_factor doubled, reset to 2 by a
    success, five invalid steps in a row: failure): every solve refused -> the fifth system is formed at 1e4 / (2 4 8 16) and the run fails at iteration 5 with the
    poses' values unchanged; the first two refused -> the third system at 1e4 / 2 / 4 = 1250 and, three successes later (each x 3: relative decrease near 1), the
    last at 33750; one success (x 3), then five refusals -> 3e4 / 1024"""
    assert pc.optimized("rejected")[1].n_rejected == 0 and pc.optimized("rejected")[1].n_refused == 0
    g0, cur = pc.graph_optimize("converge")
    g, res = pc.forced("all")
    assert (res.num_iterations, res.num_successful_steps, res.termination, res.n_refused) == (5, 0, 4, 5)
    assert abs(res.solve_radius / (1e4 / 1024) - 1) < 1e-9 and res.final_cost == res.initial_cost
    np.testing.assert_allclose(g.poses[g0.earliest:cur + 1], g0.poses[g0.earliest:cur + 1], rtol=0, atol=1e-15)
    _, res = pc.forced("first_two")
    assert (res.n_refused, res.num_iterations - res.num_successful_steps) == (2, 3) and res.termination == 3      # two refusals + the terminating iteration
    assert abs(res.solve_radius / 33750.0 - 1) < 1e-9
    _, res = pc.forced("five_in_a_row")
    assert (res.num_iterations, res.num_successful_steps, res.termination, res.n_refused) == (6, 1, 4, 5)
    assert abs(res.solve_radius / (3e4 / 1024) - 1) < 1e-9
    _, res = pc.forced("middle")
    assert res.n_refused == 2 and res.num_successful_steps == res.num_iterations - 3
    for name in pc.FORCED_CASES:
        r = pc.forced(name)[1]
        if r.n_decisions:
            assert r.min_margin >= pc.DECISION_MARGIN, name


def test_restated_write_back_and_drift():
    """updatePose on first..cur (last pose = the pose before), keyframes before `first` untouched, keyframes after cur left-multiplied by cur * last^-1"""
    g0, cur = pc.graph_optimize("converge")
    g1, res = pc.optimized("converge")
    first = g0.earliest
    assert first == 5 and len(g0.poses) - 1 - cur >= 3
    assert (g1.poses[:first] == g0.poses[:first]).all() and (g1.last[:first] == g0.last[:first]).all()
    assert (g1.last[first:] == g0.poses[first:]).all()
    drift = np.array(res.drift)
    np.testing.assert_allclose(drift, pc.pose_mul(g1.poses[cur], pc.pose_inverse(g0.poses[cur])), rtol=0, atol=1e-15)
    for k in range(cur + 1, len(g0.poses)):
        np.testing.assert_allclose(g1.poses[k], pc.pose_mul(drift, g0.poses[k]), rtol=0, atol=1e-14)
    assert np.abs(g1.poses[first + 1:cur + 1] - g0.poses[first + 1:cur + 1]).max() > 1e-4      # the solve moved something


def test_restated_step_is_a_solution_of_its_system():
    """the restatement's one linear solve (dense Cholesky): (S H S + D / radius) y = S g holds to 1e-10 of |S g| on the largest crafted system"""
    g, cur = pc.graph_step("M130")
    lin, s = g.linearize(cur), g.solve_step(cur, pc.STEP_RADIUS)
    assert s["ok"]
    H, gv = lin["H"], lin["g"]
    S = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    A = S[:, None] * H * S[None, :]
    A[np.diag_indices_from(A)] += np.clip(np.diag(A), 1e-6, 1e32) / pc.STEP_RADIUS
    np.testing.assert_allclose(A @ (-s["step"]), S * gv, rtol=0, atol=1e-10 * np.abs(S * gv).max())
    np.testing.assert_allclose(s["delta"], s["step"] * S, rtol=0, atol=0)


def test_library_exports_the_pose_graph(mla):
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(os.path.join(ROOT, "m-loam_amd", "lib", "libmloam_hip.so"))
    for nm in PG_SYMBOLS:
        assert re.search(r"\bint\s+" + nm + r"\s*\(\s*mlh_ctx\s*\*", hdr), nm
        assert nm in mla.EXPORTED_SYMBOLS, nm
        assert getattr(lib, nm) is not None, nm
    assert getattr(lib, "mlh_pg_opts_default") is not None and "mlh_pg_opts_default" in mla.EXPORTED_SYMBOLS
    assert C.sizeof(mla.PgOpts) == 32 and C.sizeof(mla.PgResult) == 120 and C.sizeof(mla.PgInfo) == 32
    o = mla.pg_opts()
    assert (o.max_num_iterations, o.n_sequential, o.t_var, o.q_var, o.huber_delta) == (5, 4, 0.1, 0.01, 1.0)
    for name in ("pg_reset", "pg_info", "pg_add_keyframe", "pg_set_loop", "pg_optimize", "pg_poses", "pg_device_poses", "pg_linearize", "pg_solve_step", "pg_time_stages", "pg_optimize_forced"):
        assert callable(getattr(mla.Context, name)), name
