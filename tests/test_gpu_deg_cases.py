"""evalDegenracy's verdict and projector on the device, at every rank and in every form of the solver tail, on the cases of tests/deg_cases.py (tests/test_deg_cases.py
holds the cases, the margins and the constants of the bars on the CPU).

Per case the statistics path returns the device's own H, g, eigval, is_degenerate and pose_after for every iteration. deg_cases.reference_tail -- numpy.linalg.eigh,
Q_kept Q_kept^T, numpy.linalg.solve, Plus, in float64 NumPy -- says from that record and the pose the iteration started from what the iteration had to return:
    is_degenerate == (k > 0)
    |eigval - lam|            <= c_e 2^-52 lam_max, entry by entry, ascending
    |pose_after - pose|inf    <= c_t 2^-52 (cond2 |d|inf + 1)
with c_e and c_t from tests/golden/deg_tolerances.json (measured on the oracle against the same reference). The threshold stands MARGIN_ABS -- a hundred times what
the device's H is known to differ from the oracle's by -- clear of every eigenvalue, so the rank is the case's. The pose is also held to the oracle's run at the
project's 1e-7, counts equal: that ties the record itself to the reference.

The statistics path always runs Jacobi; a plain call tries the shortcut "H - thre (1 + 1e-9) I has a Cholesky factor" first. Every other form returns the
statistics path's pose BIT FOR BIT: want_stats=False, the six set_gn_schedule combinations (classic, deferred and final-in-successor finishes: gn_finish_wave /
eval_degeneracy_mem), gn_solve_begin / _end, twice on one context and once on a fresh one. Under a one-rank RCCL communicator the same case reaches
gn_update_kernel / gn_finish2<true> (eval_degeneracy_reg): its statistics are held to reference_tail in the same way and its pose to the fused path's within 1e-13
(test_rccl_single_rank_path's bar). A machine without a usable RCCL fails there: that form is part of the check.

blocks_freeze runs gn_solve_blocks (gn_finish_wave with freeze; gn_update_blocks_kernel under the communicator); the lm_rank_* cases run scan2map through
test_gpu_lm_cases' forms plus the host-stepped one (lm_begin_body_wave, lm_begin_wave_pp, lm_begin_body), held to oracle.scan2map by that module's own check."""
import numpy as np
import pytest

import deg_cases as dc
from test_deg_cases import tolerances
from test_gpu_knn_cases import _stop_on_device_error
from test_gpu_lm_cases import FORMS, _bits, _check_against, _set_form

pytestmark = pytest.mark.gpu

SCHEDULES = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1))          # test_gn_schedule_variants_agree_bit_for_bit's


def _measured(case, quantity, value, bar):
    print(f"DEG_MEASURED {case} {quantity} {value:.3e} bar {bar:.3e}")


def _staged(mla, case):
    """test_gpu_lm_cases._staged on the case's scene"""
    sc = dc.scene_of(case)
    c = mla.Context(0)
    c.map_set(mla.SURF, sc["surf_map"]); c.map_set(mla.CORNER, sc["corner_map"])
    c.features_set(mla.SURF, sc["surf"]); c.features_set(mla.CORNER, sc["corner"])
    return c


def _check_verdict(name, label, s, thre, rank, tol):
    """is_degenerate and eigval of one statistics record against numpy's spectrum of the record's own H"""
    lam = np.linalg.eigvalsh(s["H"])
    k = int(np.sum(lam < thre))
    de, bar = float(np.abs(s["eigval"] - lam).max()), tol["c_e"] * dc.EPS * float(lam[-1])
    _measured(name, f"{label} eigval", de, bar)
    assert k == rank, (name, label, lam, thre)
    assert s["is_degenerate"] == (k > 0), (name, label)
    assert np.all(np.diff(s["eigval"]) >= 0) and np.all(np.abs(s["eigval"] - lam) <= bar), (name, label, s["eigval"], lam)
    assert int(np.sum(s["eigval"] < thre)) == k, (name, label)


def _check_record(name, label, s, x, thre, rank, freeze, tol):
    """one iteration's statistics record against reference_tail on the record's own H and g and the pose the iteration started from"""
    _check_verdict(name, label, s, thre, rank, tol)
    ref = dc.reference_tail(x, s["H"], s["g"], thre, freeze)
    dp, bar = float(np.abs(s["pose_after"] - ref["pose"]).max()), tol["c_t"] * dc.pose_scale(ref)
    _measured(name, f"{label} pose_after", dp, bar)
    assert dp <= bar, (name, label, dp, bar)
    return ref


def _check_gn(name, pose, st, p0, want, thre, rank, freeze, tol):
    """a Gauss-Newton solve's statistics: every iteration against reference_tail, the counts and the pose against the oracle's run"""
    x = p0
    for i, (s, o) in enumerate(zip(st, want["iters"])):
        _check_record(name, f"iteration {i}", s, x, thre, rank, freeze, tol)
        assert (s["n_surf"], s["n_corner"], s["is_degenerate"]) == (o["n_surf"], o["n_corner"], o["is_degenerate"]), (name, i)
        assert s["termination"] == (1 if freeze and rank > 0 else 0), (name, i)
        x = s["pose_after"]
    dp = float(np.abs(pose - want["pose"]).max())
    _measured(name, "pose against the oracle", dp, dc.POSE_BAR_ORACLE)
    assert dp <= dc.POSE_BAR_ORACLE and np.array_equal(_bits(pose), _bits(st[-1]["pose_after"])), (name, dp)


@pytest.mark.parametrize("name", dc.GN_NAMES)
@_stop_on_device_error
def test_gn_tail_at_every_rank_in_every_form(mla, name):
    case = dc.BY_NAME[name]
    want, tol, p0 = dc.solved(case), tolerances(), dc.start_pose(case)
    thre, n = want["thre"], case.iters
    opts = mla.default_opts(map_eig_thre=thre)
    c = _staged(mla, case)
    try:
        pose, st = c.gn_solve(p0, n, opts, want_stats=True)
        _check_gn(name, pose, st, p0, want, thre, case.rank, False, tol)
        if case.spot[0] in ("just_below", "just_above"):
            # the placements next to an eigenvalue: on the device's own H the shortcut succeeds exactly where nothing is degenerate
            assert dc.shortcut_clear(st[0]["H"], thre) == (case.rank == 0), name
        if name == "nothing_matches":
            assert not st[0]["H"].any() and not st[0]["g"].any() and not st[0]["eigval"].any()
        for rep in (0, 1):                                              # twice on this context
            for sched in SCHEDULES:
                c.set_gn_schedule(*sched)
                got = c.gn_solve(p0, n, opts, want_stats=False)[0]
                assert np.array_equal(_bits(got), _bits(pose)), (name, sched, rep, "plain", float(np.abs(got - pose).max()))
                c.gn_solve_begin(p0, n, opts)
                got = c.gn_solve_end()
                assert np.array_equal(_bits(got), _bits(pose)), (name, sched, rep, "begin / end", float(np.abs(got - pose).max()))
                got, st2 = c.gn_solve(p0, n, opts, want_stats=True)
                assert np.array_equal(_bits(got), _bits(pose)) and all(np.array_equal(_bits(a["eigval"]), _bits(b["eigval"])) for a, b in zip(st, st2)), (name, sched, rep)
    finally:
        c.close()
    c = _staged(mla, case)                                              # a fresh context: the default schedule, then one rank of RCCL
    try:
        got = c.gn_solve(p0, n, opts, want_stats=False)[0]
        assert np.array_equal(_bits(got), _bits(pose)), (name, "fresh context")
        c.comm_init(1, 0, mla.comm_unique_id())
        got, st3 = c.gn_solve(p0, n, opts, want_stats=True)
        _check_gn(name + " one-rank communicator", got, st3, p0, want, thre, case.rank, False, tol)
        plain = c.gn_solve(p0, n, opts, want_stats=False)[0]            # (gn_finish2's own shortcut)
        for form, x in (("statistics", got), ("plain", plain)):
            dp = float(np.abs(x - pose).max())
            _measured(name, f"one-rank communicator, {form}: pose against the fused path", dp, dc.COMM_POSE_BAR)
            assert dp <= dc.COMM_POSE_BAR, (name, form, dp)
        assert np.array_equal(_bits(got), _bits(plain)), name
    finally:
        c.close()


def _staged_blocks(mla, case):
    sc = dc.scene_of(case)
    feats = dc.block_features(case)
    c = mla.Context(0)
    c.map_set(mla.SURF, sc["surf_map"]); c.map_set(mla.CORNER, sc["corner_map"])
    c.features_set_blocks(mla.SURF, [f[0] for f in feats])
    c.features_set_blocks(mla.CORNER, [f[1] for f in feats])
    return c


def _check_blocks(name, poses, st, p0, runs, ranks, tol):
    for b, run in enumerate(runs):
        _check_gn(f"{name} block {b}", poses[b], [it[b] for it in st], p0, run, run["thre"], ranks[b], run["freeze"], tol)


@_stop_on_device_error
def test_blocks_freeze(mla):
    """two pose blocks on the halves of the features, block 1 frozen when degenerate. Phase 0: block 1's threshold below its spectrum -- it moves, and the move is
    reference_tail's. Phase 1: between its second and third eigenvalue -- its pose comes back with the bits it went in with, termination 1. Block 0 discards one
    direction both times."""
    name = "blocks_freeze"
    case = dc.BY_NAME[name]
    tol, p0, phases = tolerances(), dc.start_pose(case), dc.solved_blocks(case)
    poses0 = np.stack([p0, p0])
    opts = mla.default_opts()
    plain, comm = _staged_blocks(mla, case), _staged_blocks(mla, case)
    try:
        comm.comm_init(1, 0, mla.comm_unique_id())
        for p, runs in enumerate(phases):
            arg = (poses0, case.iters, list(dc.BLOCK_K_NEIGH), [r["thre"] for r in runs], list(dc.BLOCK_FREEZE), opts)
            plain.set_gn_schedule(1, 1, 1)
            poses, st = plain.gn_solve_blocks(*arg)
            _check_blocks(f"{name} phase {p}", poses, st, p0, runs, case.rank[p], tol)
            if case.rank[p][1] > 0:
                assert np.array_equal(_bits(poses[1]), _bits(p0)) and all(it[1]["termination"] == 1 for it in st)
            else:
                assert float(np.abs(poses[1] - p0).max()) > 1e-3 and all(it[1]["termination"] == 0 for it in st)
            for rep in (0, 1):
                for sched in ((1, 1, 1), (0, 0, 0), (1, 0, 0)):
                    plain.set_gn_schedule(*sched)
                    got = plain.gn_solve_blocks(*arg, want_stats=False)[0]
                    assert np.array_equal(_bits(got), _bits(poses)), (p, sched, rep, float(np.abs(got - poses).max()))
            got, st2 = comm.gn_solve_blocks(*arg)
            _check_blocks(f"{name} phase {p} one-rank communicator", got, st2, p0, runs, case.rank[p], tol)
            lean = comm.gn_solve_blocks(*arg, want_stats=False)[0]
            for form, x in (("statistics", got), ("plain", lean)):
                dp = float(np.abs(x - poses).max())
                _measured(f"{name} phase {p}", f"one-rank communicator, {form}: poses against the fused path", dp, dc.COMM_POSE_BAR)
                assert dp <= dc.COMM_POSE_BAR, (p, form, dp)
            if case.rank[p][1] > 0:
                assert np.array_equal(_bits(got[1]), _bits(p0)) and np.array_equal(_bits(lean[1]), _bits(p0)) and all(it[1]["termination"] == 1 for it in st2)
    finally:
        plain.close()
        comm.close()


@pytest.mark.parametrize("name", dc.LM_NAMES)
@_stop_on_device_error
def test_lm_begin_at_every_rank_in_every_form(mla, monkeypatch, name):
    case = dc.BY_NAME[name]
    want, tol, p0 = dc.solved_lm(case), tolerances(), dc.start_pose(case)
    thre = want["thre"]
    opts = lambda: mla.default_opts(gf_method=mla.GF_METHODS["wo_gf"], map_eig_thre=thre, max_outer=case.iters)
    _set_form(monkeypatch, {})
    c = _staged(mla, case)
    try:
        pose, st = c.scan2map(p0, opts())
        _check_against(name, pose, st, want["pose"], want["outer"])
        for i, (s, o) in enumerate(zip(st, want["outer"])):
            _check_verdict(name, f"outer {i}", s, thre, case.rank, tol)
            assert s["is_degenerate"] == o["is_degenerate"], (name, i)
        for rep in (0, 1):
            for form, env in FORMS.items():
                _set_form(monkeypatch, env)
                got = c.scan2map(p0, opts(), want_stats=False)[0]
                assert np.array_equal(_bits(got), _bits(pose)), (name, form, rep, float(np.abs(got - pose).max()))
            _set_form(monkeypatch, {})
            c.scan2map_begin(p0, opts())
            got, status = c.scan2map_end()
            assert status == 0 and np.array_equal(_bits(got), _bits(pose)), (name, "begin / end", status)
    finally:
        c.close()
    c = _staged(mla, case)
    try:
        got = c.scan2map(p0, opts(), want_stats=False)[0]
        assert np.array_equal(_bits(got), _bits(pose)), (name, "fresh context")
        c.comm_init(1, 0, mla.comm_unique_id())                        # host-stepped: lm_begin_kernel / lm_step_kernel
        got = c.scan2map(p0, opts(), want_stats=False)[0]
        assert np.array_equal(_bits(got), _bits(pose)), (name, "host-stepped", float(np.abs(got - pose).max()))
        got, st3 = c.scan2map(p0, opts())
        assert np.array_equal(_bits(got), _bits(pose)), (name, "host-stepped, statistics")
        for i, s in enumerate(st3):
            _check_verdict(name + " host-stepped", f"outer {i}", s, thre, case.rank, tol)
        assert [(s["lm_iterations"], s["successful_steps"], s["termination"]) for s in st3] == [(s["lm_iterations"], s["successful_steps"], s["termination"]) for s in st]
    finally:
        c.close()
