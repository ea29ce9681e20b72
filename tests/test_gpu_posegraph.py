"""Pose-graph optimisation on the device (m-loam_amd/csrc/posegraph.hip; mlh_pg_*) against the C++ restatement (tests/host/pg_ref.cpp through tests/pg_cases.py),
which tests/test_pg_cases.py holds on the CPU: dual-number Jacobians, a dense Cholesky under the same Levenberg-Marquardt policy, the restated write-back.
Everything goes through the C-ABI.

Bars: the linearisation (residuals, Jacobians, cost, dense H and g) and one linear step within the project's 1e-9 of the largest entry of the compared array; the
poses, last poses and the drift of a full optimise within the project's 1e-7; the summary's integers equal, its costs within 1e-9 relative; keyframes before the
earliest looped one bit-equal to their input; two runs bit-equal. Every test prints what it measured (PG_MEASURED lines) before it asserts;
tests/golden/pg_tolerances.json records those figures beside the bars as measured on an MI355X.

Observed on an MI355X: linearisation at most 1.1e-14 of the largest entry; one linear step at most 1.0e-13 (M = 130); poses at most 8.9e-15, costs 3.2e-14 relative;
the device's and the restatement's summaries equal on every pass (converge 3 / 2 / function tolerance, the 170-degree case 2 / 1 / function tolerance, L = 0
iteration 0 by the gradient tolerance); with chosen linear solves refused (mlh_pg_optimize_forced) the summaries are equal too, the radius of the last
linear system within 1.3e-12 and exactly 1e4 / 1024 when every solve is refused. With L = 0 the sequential measurements come from the poses themselves, so g is rounding noise: that step is compared
with the dense Cholesky on the device's own g."""
import os
import subprocess

import numpy as np
import pytest

import pg_cases as pc

pytestmark = pytest.mark.gpu

BAR_LINEAR, BAR_POSE, BAR_COST = 1e-9, 1e-7, 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _measured(name, value, bar):
    print(f"PG_MEASURED {name} {value:.3e} bar {bar:.1e}")


def _rel(got, want):
    """the largest difference as a fraction of the largest entry of `want`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _code(excinfo):
    return int(str(excinfo.value).split("mlh error ")[1].split(":")[0])


@pytest.mark.parametrize("cur", pc.LINEARIZE_CURS)
def test_linearisation_against_the_restatement(ctx, cur):
    """M = 2 (one free block, one sequential edge and a loop onto the constant block), 5 (band not yet full), 6 (first full band), 70; loop edges onto the constant
    block, inside the band, Huber inactive and active (tests/test_pg_cases.py holds that the graph has them)"""
    G = pc.graph_linearize()
    G.upload(ctx)
    want, got = G.linearize(cur), ctx.pg_linearize(cur)
    assert (got["ij"] == want["ij"]).all()
    worst = 0.0
    for k in ("r", "Ji", "Jj", "H", "g"):
        d = _rel(got[k], want[k])
        _measured(f"linearize_M{cur + 1}_{k}", d, BAR_LINEAR)
        worst = max(worst, d)
    dc = abs(got["cost"] - want["cost"]) / want["cost"]
    _measured(f"linearize_M{cur + 1}_cost", dc, BAR_LINEAR)
    assert worst <= BAR_LINEAR and dc <= BAR_LINEAR
    assert (ctx.pg_poses() == G.poses).all()                    # a stage entry leaves the stored poses alone


@pytest.mark.parametrize("name", pc.STEP_CASES)
def test_one_linear_step_against_the_dense_cholesky(ctx, name):
    """L = 0 (the band alone), 1, 3 (nested and crossing loops), 24 (145 columns: more than two wavefronts of lanes, C beyond the dense stage's LDS image), and
    M = 130"""
    G, cur = pc.graph_step(name)
    G.upload(ctx)
    got = ctx.pg_solve_step(cur, pc.STEP_RADIUS)
    if name == "L0":
        # without a loop edge every residual is rounding noise (the sequential measurements come from the poses themselves), so g is noise and differs between
        # any two evaluations: the dense Cholesky solves the restatement's H against the DEVICE's g
        want = pc.dense_step(G.linearize(cur)["H"], ctx.pg_linearize(cur)["g"], pc.STEP_RADIUS)
    else:
        want = G.solve_step(cur, pc.STEP_RADIUS)
    assert want["ok"] and got["ok"]
    ds, dd = _rel(got["step"], want["step"]), _rel(got["delta"], want["delta"])
    _measured(f"step_{name}_step", ds, BAR_LINEAR)
    _measured(f"step_{name}_delta", dd, BAR_LINEAR)
    assert ds <= BAR_LINEAR and dd <= BAR_LINEAR


def _compare_pass(tag, ctx, before, after, res, cur):
    got = ctx.pg_optimize(cur)
    poses, last = ctx.pg_poses(last=True)
    first = before.earliest
    dp, dl, dd = float(np.abs(poses - after.poses).max()), float(np.abs(last - after.last).max()), float(np.abs(got["drift"] - np.array(res.drift)).max())
    dc0 = abs(got["initial_cost"] - res.initial_cost) / max(res.initial_cost, 1e-300)
    dc1 = abs(got["final_cost"] - res.final_cost) / max(res.final_cost, 1e-300)
    _measured(f"optimize_{tag}_poses", dp, BAR_POSE)
    _measured(f"optimize_{tag}_last_poses", dl, BAR_POSE)
    _measured(f"optimize_{tag}_drift", dd, BAR_POSE)
    _measured(f"optimize_{tag}_initial_cost", dc0, BAR_COST)
    _measured(f"optimize_{tag}_final_cost", dc1, BAR_COST)
    print(f"PG_SUMMARY {tag} device {got['num_iterations']} {got['num_successful_steps']} {got['termination']} restatement {res.num_iterations} "
          f"{res.num_successful_steps} {res.termination} launches {got['launches']} host_waits {got['host_waits']}")
    assert (got["num_iterations"], got["num_successful_steps"], got["termination"]) == (res.num_iterations, res.num_successful_steps, res.termination)
    assert (got["n_keyframes"], got["n_loops"], got["first_index"]) == (res.n_keyframes, res.n_loops, first)
    assert got["host_waits"] == 1 and got["launches"] == 3 + 10 * pc.MAX_IT + 1
    assert dp <= BAR_POSE and dl <= BAR_POSE and dd <= BAR_POSE
    if res.initial_cost > 1e-20:                               # (the L = 0 pass: both costs are rounding noise around 1e-27)
        assert dc0 <= BAR_COST and dc1 <= BAR_COST
    else:
        assert got["initial_cost"] < 1e-20 and got["final_cost"] < 1e-20
    assert (poses[:first] == before.poses[:first]).all() and (last[:first] == before.last[:first]).all()       # bits
    return got, poses, last


@pytest.mark.parametrize("name", pc.OPTIMIZE_CASES)
def test_full_optimise_against_the_restatement(ctx, name):
    """converge (first = 5: keyframes 0..4 keep their bits; five keyframes after cur moved by the drift), rejected (a loop measurement 170 degrees from the truth),
    L0 (no loop edge inside first..cur: termination by the gradient tolerance at iteration 0, whatever the write-back then does to the bits held equal to the
    restatement within the bar)"""
    G, cur = pc.graph_optimize(name)
    after, res = pc.optimized(name)
    G.upload(ctx)
    got, poses, _ = _compare_pass(name, ctx, G, after, res, cur)
    n_after = len(G.poses) - 1 - cur
    assert n_after >= 3
    for k in range(cur + 1, len(G.poses)):
        np.testing.assert_allclose(poses[k], pc.pose_mul(got["drift"], G.poses[k]), rtol=0, atol=1e-12)
    if name == "L0":
        assert got["num_iterations"] == 0 and got["termination"] == 1


def test_two_runs_give_equal_bits(ctx):
    G, cur = pc.graph_optimize("converge")
    runs = []
    for _ in range(2):
        G.upload(ctx)
        r = ctx.pg_optimize(cur)
        poses, last = ctx.pg_poses(last=True)
        runs.append((poses, last, r))
    assert (runs[0][0].view(np.uint64) == runs[1][0].view(np.uint64)).all() and (runs[0][1].view(np.uint64) == runs[1][1].view(np.uint64)).all()
    for k in ("initial_cost", "final_cost", "final_radius"):
        assert np.float64(runs[0][2][k]).view(np.uint64) == np.float64(runs[1][2][k]).view(np.uint64), k
    assert (runs[0][2]["drift"].view(np.uint64) == runs[1][2]["drift"].view(np.uint64)).all()
    G2, cur2 = pc.graph_step("L24")
    steps = []
    for _ in range(2):
        G2.upload(ctx)
        steps.append(ctx.pg_solve_step(cur2, pc.STEP_RADIUS)["step"])
    assert (steps[0].view(np.uint64) == steps[1].view(np.uint64)).all()


def test_a_second_optimise_after_another_loop(ctx):
    """the first pass, then a loop 38 -> 12 and a pass for cur = 38: last poses come from the first pass; against the restatement driven the same way"""
    G, cur = pc.graph_optimize("converge")
    G.upload(ctx)
    ctx.pg_optimize(cur)
    before, after, res = pc.second_pass()
    ctx.pg_set_loop(38, 12, before.loop_rel[38])
    _measured("second_start_poses", float(np.abs(ctx.pg_poses() - before.poses).max()), BAR_POSE)
    _compare_pass("second", ctx, before, after, res, 38)


def test_error_returns_leave_everything_as_it_was(ctx, mla):
    """MLH_ERR_STATE without a loop and for cur_index < first; MLH_ERR_INVALID for set_loop outside 0 <= loop_index < index and a cur_index that names no keyframe;
    MLH_ERR_UNSUPPORTED above the cap of loop edges; nothing is modified by a refused call"""
    truth, est = pc.trajectory(140, 41)
    ctx.pg_reset()
    for k in range(140):
        assert ctx.pg_add_keyframe(est[k]) == k
    info = ctx.pg_info()
    assert (info["n_keyframes"], info["n_loops"], info["earliest_loop_index"]) == (140, 0, -1) and info["max_loops"] >= 128 and info["bytes_hbm"] >= 140 * 176
    with pytest.raises(mla.MlhError) as e:
        ctx.pg_optimize(50)
    assert _code(e) == -3
    for index, loop_index in ((10, 10), (10, 11), (10, -1), (140, 3), (-1, 0)):
        with pytest.raises(mla.MlhError) as e:
            ctx.pg_set_loop(index, loop_index, pc.loop_measurement(truth, 10, 3))
        assert _code(e) == -1
    assert ctx.pg_info()["earliest_loop_index"] == -1
    ctx.pg_set_loop(20, 6, pc.loop_measurement(truth, 20, 6))
    ctx.pg_set_loop(20, 8, pc.loop_measurement(truth, 20, 8))          # overwrites; the earliest index stays, as in the reference
    assert ctx.pg_info()["earliest_loop_index"] == 6 and ctx.pg_info()["n_loops"] == 1
    with pytest.raises(mla.MlhError) as e:
        ctx.pg_optimize(5)
    assert _code(e) == -3
    with pytest.raises(mla.MlhError) as e:
        ctx.pg_optimize(140)
    assert _code(e) == -1
    cap = info["max_loops"]
    for k in range(9, 9 + cap + 1):
        if k != 20:
            ctx.pg_set_loop(k, k - 3, pc.loop_measurement(truth, k, k - 3))
    assert ctx.pg_info()["n_loops"] == cap + 1
    poses0, last0 = ctx.pg_poses(last=True)
    with pytest.raises(mla.MlhError) as e:
        ctx.pg_optimize(139)
    assert _code(e) == -5 and str(cap) in str(e.value)
    poses1, last1 = ctx.pg_poses(last=True)
    assert (poses0 == est).all() and (poses1 == poses0).all() and (last1 == last0).all()
    r = ctx.pg_optimize(9 + cap - 1)                                   # exactly `cap` loop edges: supported
    assert r["n_loops"] == cap and r["n_keyframes"] == 9 + cap - 1 - 6 + 1
    ptr, stride, count = ctx.pg_device_poses()
    assert ptr and stride == 176 and count == 140


@pytest.mark.parametrize("name", sorted(pc.FORCED_CASES))
def test_forced_invalid_steps_against_the_restatement(ctx, mla, name):
    """the policy's invalid-step branch on the device (pg_decide_kernel's radius halving, the decrease factor, the reused diagonal, five in a row: failure),
    driven by mlh_pg_optimize_forced and held against lm.hpp with the same linear solves refused: summaries equal, the radius of the last linear system within
    1e-9 (what the restatement's read-back of it is good for), poses and costs within the bars; every solve refused: the final radius is 1e4 / 1024 exactly"""
    G, cur = pc.graph_optimize("converge")
    mask, max_it = pc.FORCED_CASES[name]
    after, res = pc.forced(name)
    G.upload(ctx)
    got = ctx.pg_optimize_forced(cur, mask, mla.pg_opts(max_num_iterations=max_it))
    poses, last = ctx.pg_poses(last=True)
    print(f"PG_SUMMARY forced_{name} device {got['num_iterations']} {got['num_successful_steps']} {got['termination']} restatement {res.num_iterations} "
          f"{res.num_successful_steps} {res.termination} solve_radius {got['solve_radius']!r} {res.solve_radius!r} final_radius {got['final_radius']!r}")
    dp, dl = float(np.abs(poses - after.poses).max()), float(np.abs(last - after.last).max())
    dr = abs(got["solve_radius"] / res.solve_radius - 1.0)
    dc = abs(got["final_cost"] - res.final_cost) / res.final_cost
    _measured(f"forced_{name}_poses", max(dp, dl), BAR_POSE)
    _measured(f"forced_{name}_solve_radius", dr, 1e-9)
    _measured(f"forced_{name}_final_cost", dc, BAR_COST)
    assert (got["num_iterations"], got["num_successful_steps"], got["termination"]) == (res.num_iterations, res.num_successful_steps, res.termination)
    assert dr <= 1e-9 and dp <= BAR_POSE and dl <= BAR_POSE and dc <= BAR_COST
    assert got["host_waits"] == 1 and got["launches"] == 3 + 10 * max_it + 1
    if name == "all":
        assert got["final_radius"] == 1e4 / 1024 and got["solve_radius"] == 1e4 / 1024 and got["termination"] == 4


def test_stage_timing_entry_runs_the_same_pass_and_leaves_the_poses(ctx):
    """mlh_pg_time_stages: the summary of mlh_pg_optimize on the same graph, eight non-negative stage times, the stored poses untouched"""
    G, cur = pc.graph_optimize("converge")
    _, res = pc.optimized("converge")
    G.upload(ctx)
    r, ms = ctx.pg_time_stages(cur)
    assert (r["num_iterations"], r["num_successful_steps"], r["termination"]) == (res.num_iterations, res.num_successful_steps, res.termination)
    assert len(ms) == 8 and all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    poses, last = ctx.pg_poses(last=True)
    assert (poses == G.poses).all() and (last == G.last).all()


def test_pg_selftest_exits_zero():
    """m-loam_amd/host/pg_selftest: the facade's PoseGraph class against the plain C-ABI"""
    exe = os.path.join(ROOT, "m-loam_amd", "host", "pg_selftest")
    assert os.path.exists(exe), "m-loam_amd/host/pg_selftest has not been built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
