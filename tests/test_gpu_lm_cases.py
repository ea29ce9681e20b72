"""The Levenberg-Marquardt loop on the crafted starts of tests/lm_cases.py, in every form its launches take on one GPU (tests/test_lm_cases.py holds the cases on the
CPU: the branch each reaches, the margins, and that the bars below tell a loop that treats a rejected step differently).

Per case the statistics path -- the classic fused launches, lm_begin_body_wave / lm_step_body_wave in the last workgroup -- is held to oracle.scan2map: counts and
terminations equal, costs within 1e-9 relative, poses within 1e-7 (the project's bars). Every other form then returns the statistics path's pose BIT FOR BIT: the
tagged one-launch loop (default), the loop behind a grid barrier (MLH_LOOP_TAGGED=0), the consumer-side launches (MLH_LM_LOOP=0), the classic launches without
statistics (MLH_LM_CONSUMER=0), mlh_scan2map_begin / _end with the automatic look-ahead and with one that is a launch short (status 2, re-solved), and the
stand-alone host-stepped kernels under a one-rank RCCL communicator; twice on one context and once on a fresh one. A `rnd` selection (linearize_launch's begin) is held
to the oracle's run of the same selection and to itself across its forms. Case d delivers its covariance from the record at the ACCEPTED pose; the tracker's
cases (hand-made clouds whose rounds reject steps) run through both forms of mlh_track_cloud."""
import numpy as np
import pytest

import lm_cases as lm
from test_gpu_knn_cases import _stop_on_device_error

pytestmark = pytest.mark.gpu

COST_BAR, POSE_BAR, H_BAR, TRACK_POSE_BAR = 1e-9, 1e-7, 1e-9, 1e-9
EPS = 2.0 ** -52
LM_ENV = ("MLH_LM_CONSUMER", "MLH_LM_LOOP", "MLH_LOOP_TAGGED")
FORMS = {"loop, tagged records (default)": {}, "loop, grid barrier": {"MLH_LOOP_TAGGED": "0"}, "consumer-side launches": {"MLH_LM_LOOP": "0"},
         "classic launches": {"MLH_LM_CONSUMER": "0"}}
RND = dict(gf_ratio=0.5, gf_seed=5)


def _measured(name, value, bar):
    print(f"LM_MEASURED {name} {value:.3e} bar {bar:.1e}")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _set_form(monkeypatch, env):
    for k in LM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _opts(mla, case, **kw):
    return mla.default_opts(**{"gf_method": mla.GF_METHODS["wo_gf"], **dict(case.opts), **kw})


def _staged(mla, case):
    sc = lm.SCENES[case.family](case.seed)
    c = mla.Context(0)
    c.map_set(mla.SURF, sc["surf_map"]); c.map_set(mla.CORNER, sc["corner_map"])
    c.features_set(mla.SURF, sc["surf"]); c.features_set(mla.CORNER, sc["corner"])
    return c


def _check_against(name, pose, st, want_pose, want_outer):
    """the statistics of one solve against the oracle's outer records"""
    assert len(st) == len(want_outer), name
    for i, (s, o) in enumerate(zip(st, want_outer)):
        got = (s["n_surf"], s["n_corner"], s["lm_iterations"], s["successful_steps"], s["termination"])
        want = (o["n_surf_sel"], o["n_corner_sel"], o["lm_iterations"], o["successful_steps"], o["termination"])
        dc, df = _rel(s["cost"], o["initial_cost"]), _rel(s["final_cost"], o["final_cost"])
        dp = float(np.abs(s["pose_after"] - o["pose_after"]).max())
        _measured(f"{name} outer {i} {got} initial cost", dc, COST_BAR)
        _measured(f"{name} outer {i} final cost", df, COST_BAR)
        _measured(f"{name} outer {i} pose_after", dp, POSE_BAR)
        assert got == want, (name, i, got, want)
        assert dc <= COST_BAR and df <= COST_BAR and dp <= POSE_BAR, (name, i, dc, df, dp)
    dp = float(np.abs(pose - want_pose).max())
    _measured(f"{name} returned pose", dp, POSE_BAR)
    assert dp <= POSE_BAR and np.array_equal(_bits(pose), _bits(st[-1]["pose_after"])), (name, dp)


@pytest.mark.parametrize("name", [c.name for c in lm.CASES])
@_stop_on_device_error
def test_every_form_of_every_case(mla, monkeypatch, name):
    case = lm.BY_NAME[name]
    want = lm.oracle_solved(case)
    p0 = lm.start_pose(case)
    _set_form(monkeypatch, {})
    c = _staged(mla, case)
    try:
        pose, st = c.scan2map(p0, _opts(mla, case))
        _check_against(name, pose, st, want["pose"], want["outer"])
        need = max(s["lm_iterations"] for s in st)
        for rep in (0, 1):                                              # twice on this context
            for form, env in FORMS.items():
                _set_form(monkeypatch, env)
                loops = c.info()["loop_launches"]
                got = c.scan2map(p0, _opts(mla, case), want_stats=False)[0]
                assert np.array_equal(_bits(got), _bits(pose)), (name, form, rep, float(np.abs(got - pose).max()))
                if form.startswith("loop"):
                    assert c.info()["loop_launches"] > loops, (name, form)          # (the one-launch loop did run)
                else:
                    assert c.info()["loop_launches"] == loops, (name, form)
            _set_form(monkeypatch, {"MLH_LM_CONSUMER": "0"})
            again, st2 = c.scan2map(p0, _opts(mla, case))
            assert np.array_equal(_bits(again), _bits(pose)) and [s["lm_iterations"] for s in st2] == [s["lm_iterations"] for s in st]
            _set_form(monkeypatch, {})
            c.scan2map_begin(p0, _opts(mla, case))
            got, status = c.scan2map_end()
            assert status == 0 and np.array_equal(_bits(got), _bits(pose)), (name, "begin / end", status)
            if need >= 2:
                c.scan2map_begin(p0, _opts(mla, case), lm_lookahead=need - 1)
                got, status = c.scan2map_end()
                assert status == 2 and np.array_equal(_bits(got), _bits(pose)), (name, "begin / end, a launch short", status)
                c.scan2map_begin(p0, _opts(mla, case), lm_lookahead=need)
                got, status = c.scan2map_end()
                assert status == 0 and np.array_equal(_bits(got), _bits(pose)), (name, "begin / end, exact look-ahead", status)
        # the rnd selection: the oracle's run of the same selection, and its own forms among themselves
        rnd = lm.oracle_solved(case, gf_method="rnd", gf_ratio=RND["gf_ratio"], seed=RND["gf_seed"])
        o_rnd = _opts(mla, case, gf_method=mla.GF_METHODS["rnd"], **RND)
        pose_r, st_r = c.scan2map(p0, o_rnd)
        _check_against(name + " rnd", pose_r, st_r, rnd["pose"], rnd["outer"])
        for form in ("loop, tagged records (default)", "classic launches"):
            _set_form(monkeypatch, FORMS[form])
            got = c.scan2map(p0, o_rnd, want_stats=False)[0]
            assert np.array_equal(_bits(got), _bits(pose_r)), (name, "rnd", form)
        _set_form(monkeypatch, {})
    finally:
        c.close()
    # a fresh context: the default form, and the stand-alone host-stepped kernels under a one-rank communicator
    c = _staged(mla, case)
    try:
        got = c.scan2map(p0, _opts(mla, case), want_stats=False)[0]
        assert np.array_equal(_bits(got), _bits(pose)), (name, "fresh context")
        # one rank of RCCL: every solve is host-stepped (lm_begin_kernel / lm_step_kernel). A machine without a usable RCCL fails here: this form is part of the check
        c.comm_init(1, 0, mla.comm_unique_id())
        got = c.scan2map(p0, _opts(mla, case), want_stats=False)[0]
        assert np.array_equal(_bits(got), _bits(pose)), (name, "host-stepped", float(np.abs(got - pose).max()))
        got, st3 = c.scan2map(p0, _opts(mla, case))
        assert np.array_equal(_bits(got), _bits(pose)), (name, "host-stepped, statistics")
        assert [(s["lm_iterations"], s["successful_steps"], s["termination"]) for s in st3] == [(s["lm_iterations"], s["successful_steps"], s["termination"]) for s in st]
    finally:
        c.close()


def _solve_cov(c, p0, opts, want_stats=False):
    pose, st = c.scan2map(p0, opts, want_stats=want_stats)
    cov, H = c.scan2map_cov()
    return pose, cov, H, st


@_stop_on_device_error
def test_d_the_covariance_is_the_accepted_poses(mla, monkeypatch):
    """the budget ends on a rejected step: H_final is the record at the ACCEPTED pose -- mlh_match_linearize at the last outer iteration's start pose, mlh_linearize +
    Huber at the returned pose -- within 1e-9 of its largest entry, in the classic, the consumer-side and the one-launch forms; the covariance is its inverse. (The
    rejected candidate's record is further than 1e-7 of the largest entry away: tests/test_lm_cases.py.)"""
    case = lm.BY_NAME["d_budget_ends_on_a_rejection"]
    p0, tr = lm.start_pose(case), lm.traced(case)
    _set_form(monkeypatch, {})
    c = _staged(mla, case)
    try:
        pose, cov, H, st = _solve_cov(c, p0, _opts(mla, case, pose_cov=True), want_stats=True)
        plain = c.scan2map(p0, _opts(mla, case), want_stats=False)[0]
        assert np.array_equal(_bits(pose), _bits(plain))
        assert [(s["lm_iterations"], s["termination"]) for s in st] == [(13, 0), (13, 0)] and [s["successful_steps"] for s in st] == [10, 10]
        outs = {"classic launches, statistics": (pose, cov, H)}
        for form, env in FORMS.items():
            _set_form(monkeypatch, env)
            outs[form] = _solve_cov(c, p0, _opts(mla, case, pose_cov=True))[:3]
        _set_form(monkeypatch, {})
        # the device's own evaluation at the returned pose, on the correspondences the last outer iteration matched at ITS start pose
        Href = np.zeros((6, 6))
        for kind in (mla.SURF, mla.CORNER):
            c.match_linearize(kind, st[-2]["pose_after"], dense=False)
            Href += c.linearize(kind, pose, dense=False)["H"]
    finally:
        c.close()
    Horc = tr["outer"][-1]["trace"]["last"]["H"]
    scale = float(np.abs(Href).max())
    for form, (p, X, A) in outs.items():
        assert np.array_equal(_bits(p), _bits(pose)), form
        e1, e2 = float(np.abs(A - Href).max()) / scale, float(np.abs(A - Horc).max()) / float(np.abs(Horc).max())
        _measured(f"d cov {form}: H against match_linearize + linearize", e1, H_BAR)
        _measured(f"d cov {form}: H against the trace", e2, H_BAR)
        assert e1 <= H_BAR and e2 <= H_BAR, (form, e1, e2)
        assert np.array_equal(_bits(A), _bits(outs["classic launches, statistics"][2])) and np.array_equal(_bits(X), _bits(outs["classic launches, statistics"][1])), form
        cond = np.linalg.cond(A, 2)
        res = float(np.abs(X @ A - np.eye(6)).max())
        _measured(f"d cov {form}: |cov H - I|max (cond2 {cond:.2e})", res, 100 * EPS * cond)
        assert res <= 100 * EPS * cond, (form, res, cond)


@pytest.mark.parametrize("name", [c.name for c in lm.TRACK_CASES])
@_stop_on_device_error
def test_h_the_tracker_rejects_steps_inside_a_round(mla, monkeypatch, name):
    """hand-made clouds on which trackCloud rejects steps (tests/test_lm_cases.py has each sequence): the statistics path against oracle.track_cloud -- counts,
    accepted steps and terminations equal, costs within 1e-9, the pose within 1e-9 (the tracker's bar) -- and the one-launch loop (track_lm_loop_kernel) and the
    launch-per-iteration form (MLH_TRACK_LOOP=0) with the statistics path's bits, twice each"""
    case = lm.TRACK_BY_NAME[name]
    tc, p0, prm = lm.track_clouds(case.seed, *case.sizes), lm.track_start(case), lm.track_params_of(case)
    ref, tr = lm.track_oracle_solved(case), lm.track_traced(case)
    opts = mla.default_track_opts(**prm)
    c = mla.Context(0)
    try:
        c.track_set_prev(mla.CORNER, tc["corner_last"], prm["distance_sq_threshold"]); c.track_set_prev(mla.SURF, tc["surf_last"], prm["distance_sq_threshold"])
        c.track_set_cur(mla.CORNER, tc["corner_sharp"]); c.track_set_cur(mla.SURF, tc["surf_flat"])
        monkeypatch.delenv("MLH_TRACK_LOOP", raising=False)
        pose, st = c.track_cloud(p0, opts)
        loop = [c.track_cloud(p0, opts, want_stats=False)[0] for _ in range(2)]
        monkeypatch.setenv("MLH_TRACK_LOOP", "0")
        launches = [c.track_cloud(p0, opts, want_stats=False)[0] for _ in range(2)]
        monkeypatch.delenv("MLH_TRACK_LOOP", raising=False)
    finally:
        c.close()
    for i, (s, o, t) in enumerate(zip(st, ref["outer"], tr["outer"])):
        got = (s["n_corner"], s["n_surf"], s["lm_iterations"], s["successful_steps"], s["termination"])
        want = (o["n_corner"], o["n_surf"], o["lm_iterations"], o["successful_steps"], o["termination"])
        assert o["successful_steps"] == t["trace"]["summary"]["successful_steps"]
        dc, df = _rel(s["cost"], o["initial_cost"]), _rel(s["final_cost"], o["final_cost"])
        dp = float(np.abs(s["pose_after"] - o["pose_after"]).max())
        _measured(f"{name} round {i} {got} initial cost", dc, COST_BAR)
        _measured(f"{name} round {i} final cost", df, COST_BAR)
        _measured(f"{name} round {i} pose_after", dp, TRACK_POSE_BAR)
        assert got == want, (name, i, got, want)
        assert dc <= COST_BAR and df <= COST_BAR and dp <= TRACK_POSE_BAR, (name, i, dc, df, dp)
    dp = float(np.abs(pose - ref["pose"]).max())
    _measured(f"{name} pose", dp, TRACK_POSE_BAR)
    assert dp <= TRACK_POSE_BAR
    for k, x in enumerate(loop + launches):
        assert np.array_equal(_bits(x), _bits(pose)), (name, k, float(np.abs(x - pose).max()))
