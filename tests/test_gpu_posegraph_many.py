"""Pose-graph optimisation on the device with MORE than 128 loop edges (mlh_pg_reserve; the blocked dense stage of m-loam_amd/csrc/posegraph.hip) against the C++
restatement (tests/host/pg_ref.cpp through tests/pg_cases.py) on the graphs of tests/pg_many_cases.py, which tests/test_pg_many_cases.py holds on the CPU. At
L = 1024 (graph E) the restatement's dense solve is not affordable: one linear step is held against a sparse LU of the system assembled from the restatement's
edges, and E's full optimise is NOT held against the restatement -- it must run, terminate regularly, lower the cost and repeat its bits.

Bars, the project's: the linearisation and one linear step within 1e-9 of the largest entry of the compared array; poses, last poses and drift of a full optimise
within 1e-7; the summary's integers equal, costs within 1e-9 relative; keyframes before the earliest looped one bit-equal to their input; two runs bit-equal. Every
test prints what it measured (PG_MEASURED lines) before it asserts; tests/golden/pg_many_tolerances.json records those figures beside the bars.

A pivot failure INSIDE C cannot be crafted: C = I + Y^T Y is positive definite whatever the graph. That branch of pg_cpanel_kernel (lin_ok = 0, the factorisation
continuing on 1) is covered by reading and, for what follows a failed solve, by the forced case, which shows that every launch of the blocked stage honours lin_ok.

Every test but "capacity" and "unchanged below the cap" fails on a library without mlh_pg_reserve (a missing entry), and with the entry but without the blocked stage
by error -5."""
import numpy as np
import pytest

import pg_cases as pc
import pg_many_cases as pm

pytestmark = pytest.mark.gpu

BAR_LINEAR, BAR_POSE, BAR_COST = 1e-9, 1e-7, 1e-9


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _measured(name, value, bar):
    print(f"PG_MEASURED {name} {value:.3e} bar {bar:.1e}")


def _code(excinfo):
    return int(str(excinfo.value).split("mlh error ")[1].split(":")[0])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _launches(name, max_it=pc.MAX_IT):
    m = 6 * pm.TABLE[name][1]
    return 3 + (9 + 3 * -(-m // pm.PANEL)) * max_it + 1


def test_capacity_is_per_context_and_128_by_default(ctx, mla):
    """the default is 128; mlh_pg_reserve refuses 127 and limit + 1 (-1); with 128 reserved graph A (129 loop edges) is refused with -5, the message names 128 and
    the poses keep their bits; with 129 reserved A optimises; the capacity survives mlh_pg_reset; mlh_pg_info reports it"""
    G, cur = pm.graph_many("A")
    assert ctx.pg_info()["max_loops"] == pm.CAP_DEFAULT == 128
    for bad in (127, pm.LOOPS_LIMIT + 1, 0, -1):
        with pytest.raises(mla.MlhError) as e:
            ctx.pg_reserve(bad)
        assert _code(e) == -1
    assert ctx.pg_info()["max_loops"] == 128
    ctx.pg_reserve(128)
    G.upload(ctx)
    bytes0 = ctx.pg_info()["bytes_hbm"]
    with pytest.raises(mla.MlhError) as e:
        ctx.pg_optimize(cur)
    assert _code(e) == -5 and "128" in str(e.value) and "129" in str(e.value)
    poses, last = ctx.pg_poses(last=True)
    assert (_bits(poses) == _bits(G.poses)).all() and (_bits(last) == _bits(G.last)).all()
    ctx.pg_reserve(129)
    info = ctx.pg_info()
    assert info["max_loops"] == 129 and info["bytes_hbm"] == bytes0               # bookkeeping: nothing allocated
    r = ctx.pg_optimize(cur)
    assert r["n_loops"] == 129 and r["num_iterations"] >= 1 and r["final_cost"] < r["initial_cost"]
    ctx.pg_reset()
    assert ctx.pg_info()["max_loops"] == 129 and ctx.pg_info()["n_keyframes"] == 0
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    assert ctx.pg_info()["max_loops"] == pm.LOOPS_LIMIT
    G.upload(ctx)
    assert ctx.pg_optimize(cur)["n_loops"] == 129


@pytest.mark.parametrize("name", ("A", "D"))
def test_linearisation_against_the_restatement(ctx, name):
    """A and D (loops onto the constant block, Huber active and inactive) without the dense H: the edge list equal, r, Ji, Jj and the cost within the bar"""
    G, cur = pm.graph_many(name)
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    G.upload(ctx)
    want, got = pm.edges(name), ctx.pg_linearize(cur, dense=False)
    assert (got["ij"] == want["ij"]).all()
    worst = 0.0
    for k in ("r", "Ji", "Jj"):
        d = pm.rel(got[k], want[k])
        _measured(f"many_linearize_{name}_{k}", d, BAR_LINEAR)
        worst = max(worst, d)
    dc = abs(got["cost"] - want["cost"]) / want["cost"]
    _measured(f"many_linearize_{name}_cost", dc, BAR_LINEAR)
    assert worst <= BAR_LINEAR and dc <= BAR_LINEAR
    assert (ctx.pg_poses() == G.poses).all()


@pytest.mark.parametrize("name", pm.STEP_MANY + ("E",))
def test_one_linear_step(ctx, name):
    """A (13 panels, a remainder panel of 6 columns that shares its tile with the bordering row), B, C (25 panels), D against the restatement's dense Cholesky; E
    (96 full panels, the bordering row in a row tile of its own) against the sparse LU of the system assembled from the restatement's edges"""
    G, cur = pm.graph_many(name)
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    G.upload(ctx)
    got = ctx.pg_solve_step(cur, pc.STEP_RADIUS)
    want = pm.sparse_step(name) if name == "E" else pm.restated_step(name)
    ds, dd = pm.rel(got["step"], want["step"]), pm.rel(got["delta"], want["delta"])
    _measured(f"many_step_{name}_step", ds, BAR_LINEAR)
    _measured(f"many_step_{name}_delta", dd, BAR_LINEAR)
    assert got["ok"] and want.get("ok", True)
    assert ds <= BAR_LINEAR and dd <= BAR_LINEAR


def _optimise(ctx, G, cur, **kw):
    G.upload(ctx)
    r = ctx.pg_optimize(cur, **kw)
    poses, last = ctx.pg_poses(last=True)
    return r, poses, last


@pytest.mark.parametrize("name", pm.OPTIMIZE_MANY)
def test_full_optimise_against_the_restatement(ctx, name):
    """A (5 iterations / 5 successful / iteration limit), B (5 / 4 / function tolerance), D (4 / 3 / function tolerance): the summary's integers equal, poses, last
    poses and drift within 1e-7, costs within 1e-9 relative, the keyframes before `first` keep their bits, ONE host wait, and the number of launches is
    3 + (9 + 3 ceil(6 L / 64)) max_num_iterations + 1; A2 -- A's loops among 20 more keyframes -- reports the same number: it depends on L alone"""
    G, cur = pm.graph_many(name)
    after, res = pm.optimized_many(name)
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    got, poses, last = _optimise(ctx, G, cur)
    first = G.earliest
    dp, dl, dd = float(np.abs(poses - after.poses).max()), float(np.abs(last - after.last).max()), float(np.abs(got["drift"] - np.array(res.drift)).max())
    dc0 = abs(got["initial_cost"] - res.initial_cost) / res.initial_cost
    dc1 = abs(got["final_cost"] - res.final_cost) / res.final_cost
    _measured(f"many_optimize_{name}_poses", dp, BAR_POSE)
    _measured(f"many_optimize_{name}_last_poses", dl, BAR_POSE)
    _measured(f"many_optimize_{name}_drift", dd, BAR_POSE)
    _measured(f"many_optimize_{name}_initial_cost", dc0, BAR_COST)
    _measured(f"many_optimize_{name}_final_cost", dc1, BAR_COST)
    print(f"PG_SUMMARY many_{name} device {got['num_iterations']} {got['num_successful_steps']} {got['termination']} restatement {res.num_iterations} "
          f"{res.num_successful_steps} {res.termination} launches {got['launches']} host_waits {got['host_waits']}")
    assert (got["num_iterations"], got["num_successful_steps"], got["termination"]) == (res.num_iterations, res.num_successful_steps, res.termination)
    assert (got["n_keyframes"], got["n_loops"], got["first_index"]) == (res.n_keyframes, res.n_loops, first) == (pm.TABLE[name][2], pm.TABLE[name][1], pm.TABLE[name][3])
    assert got["host_waits"] == 1 and got["launches"] == _launches(name)
    assert dp <= BAR_POSE and dl <= BAR_POSE and dd <= BAR_POSE and dc0 <= BAR_COST and dc1 <= BAR_COST
    assert (_bits(poses[:first]) == _bits(G.poses[:first])).all() and (_bits(last[:first]) == _bits(G.last[:first])).all()
    if name == "A":
        G2, cur2 = pm.graph_many("A2")
        got2, _, _ = _optimise(ctx, G2, cur2)
        assert got2["n_loops"] == got["n_loops"] and got2["n_keyframes"] != got["n_keyframes"] and got2["launches"] == got["launches"] and got2["host_waits"] == 1


def test_forced_invalid_steps_against_the_restatement(ctx, mla):
    """A with the linear solves of iterations 1 and 2 refused and 8 iterations allowed (8 / 6 / iteration limit in the restatement): the summary equal, the radius of
    the last linear system within 1e-9, poses within 1e-7 -- every launch of the blocked stage returns at once on lin_ok = 0, and the policy's invalid-step branch
    follows. The restatement's radius is pg_many_cases.forced_many_radius() (303750.0000029): Result.solve_radius of this very pass, 100067.29..., is a read-back
    taken one evaluation too late because the pass's last step is accepted, and is not the radius of any system (tests/test_pg_many_cases.py shows the same flaw on
    a first system, which is formed at 1e4). The device reports 303750.0 = 1e4 / 2 / 4 x 3^5 exactly; both figures are printed."""
    G, cur = pm.graph_many("A")
    mask, max_it = pm.FORCED_MANY
    after, res = pm.forced_many()
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    G.upload(ctx)
    got = ctx.pg_optimize_forced(cur, mask, mla.pg_opts(max_num_iterations=max_it))
    poses, last = ctx.pg_poses(last=True)
    dp, dl = float(np.abs(poses - after.poses).max()), float(np.abs(last - after.last).max())
    want_radius = pm.forced_many_radius()
    dr = abs(got["solve_radius"] / want_radius - 1.0)
    dc = abs(got["final_cost"] - res.final_cost) / res.final_cost
    print(f"PG_SUMMARY many_forced device {got['num_iterations']} {got['num_successful_steps']} {got['termination']} restatement {res.num_iterations} "
          f"{res.num_successful_steps} {res.termination} solve_radius {got['solve_radius']!r} restatement {want_radius!r} (read back one evaluation late: {res.solve_radius!r})")
    _measured("many_forced_poses", max(dp, dl), BAR_POSE)
    _measured("many_forced_solve_radius", dr, 1e-9)
    _measured("many_forced_final_cost", dc, BAR_COST)
    assert (got["num_iterations"], got["num_successful_steps"], got["termination"]) == (res.num_iterations, res.num_successful_steps, res.termination)
    assert dr <= 1e-9 and dp <= BAR_POSE and dl <= BAR_POSE and dc <= BAR_COST
    assert got["host_waits"] == 1 and got["launches"] == _launches("A", max_it)


def test_two_runs_give_equal_bits(ctx):
    """B's linear step and B's full optimise, twice each"""
    G, cur = pm.graph_many("B")
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    steps = []
    for _ in range(2):
        G.upload(ctx)
        steps.append(ctx.pg_solve_step(cur, pc.STEP_RADIUS)["step"])
    assert np.abs(steps[0]).max() > 0 and (_bits(steps[0]) == _bits(steps[1])).all()
    runs = [_optimise(ctx, G, cur) for _ in range(2)]
    assert (_bits(runs[0][1]) == _bits(runs[1][1])).all() and (_bits(runs[0][2]) == _bits(runs[1][2])).all()
    for k in ("initial_cost", "final_cost", "final_radius"):
        assert _bits(runs[0][0][k]) == _bits(runs[1][0][k]), k
    assert (_bits(runs[0][0]["drift"]) == _bits(runs[1][0]["drift"])).all()


def test_optimise_at_the_limit_and_history(ctx, mla):
    """E (L = 1024, M = 1097) is NOT held against the restatement (its dense solve takes over a minute per iteration): the pass runs, ends in a regular termination
    (0 .. 3), lowers the cost, reports the launch count of 96 panels and one host wait, and a second run repeats its bits. Then graph A on the SAME context gives the
    bits of a fresh context: nothing of the larger problem is left in the reused buffers"""
    G, cur = pm.graph_many("E")
    ctx.pg_reserve(pm.LOOPS_LIMIT)
    runs = [_optimise(ctx, G, cur) for _ in range(2)]
    r = runs[0][0]
    print(f"PG_SUMMARY many_E device {r['num_iterations']} {r['num_successful_steps']} {r['termination']} cost {r['initial_cost']!r} -> {r['final_cost']!r} "
          f"launches {r['launches']} host_waits {r['host_waits']}")
    assert (r["n_keyframes"], r["n_loops"], r["first_index"]) == (1097, 1024, 2)
    assert r["termination"] in (0, 1, 2, 3) and r["num_successful_steps"] >= 1 and r["final_cost"] < r["initial_cost"]
    assert r["host_waits"] == 1 and r["launches"] == _launches("E")
    assert (_bits(runs[0][1]) == _bits(runs[1][1])).all() and (_bits(runs[0][2]) == _bits(runs[1][2])).all()
    assert _bits(r["final_cost"]) == _bits(runs[1][0]["final_cost"])
    GA, curA = pm.graph_many("A")
    used, poses_used, last_used = _optimise(ctx, GA, curA)
    fresh_ctx = mla.Context(0)
    try:
        fresh_ctx.pg_reserve(pm.LOOPS_LIMIT)
        fresh, poses_fresh, last_fresh = _optimise(fresh_ctx, GA, curA)
    finally:
        fresh_ctx.close()
    assert (_bits(poses_used) == _bits(poses_fresh)).all() and (_bits(last_used) == _bits(last_fresh)).all()
    assert _bits(used["final_cost"]) == _bits(fresh["final_cost"]) and used["launches"] == fresh["launches"]


def test_unchanged_below_the_cap(ctx, mla):
    """on a context with the limit reserved, a problem with L <= 128 takes the launches it always took (3 + 10 x 5 + 1) and gives the bits of a context that never
    reserved: the dense stage is chosen by the problem's L, never by the capacity"""
    G1, cur1 = pc.graph_step("L24")
    G2, cur2 = pc.graph_optimize("converge")
    out = []
    for reserve in (False, True):
        c = mla.Context(0)
        try:
            if reserve:
                c.pg_reserve(pm.LOOPS_LIMIT)
            G1.upload(c)
            step = c.pg_solve_step(cur1, pc.STEP_RADIUS)["step"]
            r, poses, last = _optimise(c, G2, cur2)
            out.append((step, r, poses, last))
        finally:
            c.close()
    (s0, r0, p0, l0), (s1, r1, p1, l1) = out
    assert (_bits(s0) == _bits(s1)).all() and (_bits(p0) == _bits(p1)).all() and (_bits(l0) == _bits(l1)).all()
    assert r0["launches"] == r1["launches"] == 3 + 10 * pc.MAX_IT + 1
    for k in ("initial_cost", "final_cost", "final_radius"):
        assert _bits(r0[k]) == _bits(r1[k]), k
