"""The odometry window's crafted cases (tests/odom_cases.py) on the CPU: the windows are what the cases say they are, the reference's three sides agree --
window_system with oracle.pure_odom_normal_eq inside the bars the device is held to, window_gn with a host loop over oracle.pure_odom_normal_eq within 1e-12 in the
poses --, the conditions the GPU file's pose bar rests on hold at every iterate of the reference (cond(H_free) <= 1e6, steps <= 0.2, a falling cost), the Huber
case's planted rows take the branch they are named for, and every mutant of the reference leaves the bars of tests/test_gpu_odom_cases.py on the case named for
it: those bars do tell a wrong implementation."""
import numpy as np
import pytest

import marg_cases as mc
import odom_cases as oc

HOST_LOOP_TOL = 1e-12


def _oracle_system(orc, w, pivot, frames, exts, hd):
    return orc.pure_odom_normal_eq(w["types"], w["points"], w["coeffs"], w["sqrt_info"], w["fi"], w["ei"], pivot, frames, exts, hd)


def _show(name, measured):
    for k, (v, bar) in measured.items():
        print(f"ODOM_MEASURED {name}: {k} {v:.3e} bar {bar:.1e}")


def _group_sizes(w):
    return {(int(f), int(e)): int(((w["fi"] == f) & (w["ei"] == e)).sum()) for f in range(w["n_frames"]) for e in range(w["n_ext"])}


def test_the_windows_are_what_the_cases_say():
    assert _group_sizes(oc.ragged()) == {(0, 0): 1, (0, 1): 255, (1, 0): 256, (1, 1): 257}
    assert _group_sizes(oc.ragged(True))[(1, 1)] == 513
    w = oc.ragged()
    key = w["fi"] * 2 + w["ei"]
    assert (np.diff(key) < 0).any() and (np.diff(key) > 0).any()                                  # the table arrives shuffled
    assert (np.diff(oc.reordered(w, "sorted")["fi"] * 2 + oc.reordered(w, "sorted")["ei"]) >= 0).all()
    assert np.array_equal(oc.reordered(w, "reversed")["points"], w["points"][::-1])
    assert 0.2 < (w["types"] == 1).mean() < 0.3                                                   # about a quarter are edge factors
    assert np.array_equal(w["exts"][0], oc.IDENT) and np.abs(w["pivot"][:3]).max() <= 5.0
    s = _group_sizes(oc.sparse_ext())
    assert all((n == 0) == (e in (1, 3)) for (f, e), n in s.items()) and oc.sparse_ext()["n_ext"] == 4
    s = _group_sizes(oc.empty_frame())
    assert s[(1, 0)] == s[(1, 1)] == 0 and min(s[(0, 0)], s[(0, 1)], s[(2, 0)], s[(2, 1)]) > 0
    w = oc.max_window()
    assert (w["n_frames"], w["n_ext"], len(w["types"])) == (10, 11, 2640) and set(_group_sizes(w).values()) == {24}      # 22 blocks, D = 132, 110 tiles
    w = oc.poses("half_turn")
    assert w["frames"][0][6] == 0.0 and np.array_equal(w["pivot"], oc.IDENT)                      # q.w = 0 exactly, 180 degrees from the pivot
    w = oc.poses("frame_is_pivot")
    assert np.array_equal(w["frames"][0], w["pivot"]) and np.array_equal(w["exts"][0], oc.IDENT)
    assert np.isnan(oc.non_finite()["points"]).sum() == 1 and not np.isnan(oc.ragged()["points"]).any()
    V = oc.masks_and_V()["V"]
    assert V.shape == (7, 6, 6) and np.abs(V).max() <= 1.0 and np.abs(V - V.transpose(0, 2, 1)).max(axis=(1, 2)).min() > 0.5       # dense, and no block symmetric


@pytest.mark.parametrize("name", list(oc.SYSTEMS))
def test_window_system_and_the_oracle_agree(orc, name):
    fn, hd = oc.SYSTEMS[name]
    w = fn()
    ref = oc.system_reference(name)
    at = oc.negated(w) if name == "poses negated" else w
    m = oc.measure_system(_oracle_system(orc, w, at["pivot"], at["frames"], at["exts"], hd), ref)
    _show(name, m)
    assert oc.within(m), (name, m)
    assert ref["count"] == len(w["types"]) and np.array_equal(ref["H"], ref["H"].T)


def _host_loop(orc, mla, a):
    """window_gn's loop driven by oracle.pure_odom_normal_eq"""
    w = a["w"]
    pv, fr, ex = w["pivot"].copy(), w["frames"].copy(), w["exts"].copy()
    nb = 1 + len(fr) + len(ex)
    const = (0, 1 + len(fr)) if a["const_blocks"] is None else a["const_blocks"]
    fb = [b for b in range(nb) if b not in const]
    free = np.concatenate([np.arange(6 * b, 6 * b + 6) for b in fb])
    for _ in range(a["n_iters"]):
        ne = _oracle_system(orc, w, pv, fr, ex, 1.0)
        H, g = ne["H"], ne["g"]
        if a["prior"] is not None:
            p = mc.prior_evaluate(a["prior"], pv, fr, ex)
            H, g = H + p["H"], g + p["g"]
        Hf = H[np.ix_(free, free)]
        if (np.diag(Hf) == 0.0).any():
            Hf = Hf + 1e-6 * np.eye(len(free))
        d = np.linalg.solve(Hf, -g[free])
        poses = [pv] + list(fr) + list(ex)
        for k, b in enumerate(fb):
            poses[b] = mla.pose_plus(poses[b], d[6 * k:6 * k + 6], None if a["V"] is None else a["V"][b])
        pv, fr, ex = poses[0], np.stack(poses[1:1 + len(fr)]), np.stack(poses[1 + len(fr):])
    return dict(frames=fr, exts=ex)


@pytest.mark.parametrize("name", list(oc.SOLVES))
def test_window_gn_and_its_conditions(orc, mla, name):
    """window_gn against the host loop, and at every iterate the conditions the 1e-9 pose bar rests on"""
    a = oc.solve_args(name)
    ref = oc.solve_reference(name)
    host = _host_loop(orc, mla, a)
    dp = oc.measure_poses(host, ref)["poses"][0]
    print(f"ODOM_MEASURED {name}: host loop {dp:.3e} bar {HOST_LOOP_TOL:.1e}; " + " ".join(f"[cond {i['cond']:.2e} step {i['step']:.3f} cost {i['cost']:.4f}]" for i in ref["iters"]))
    assert dp <= HOST_LOOP_TOL, (name, dp)
    assert ref["status"] == a["status"] and ref["count"] == len(a["w"]["types"])
    assert len(ref["iters"]) == a["n_iters"]
    for i in ref["iters"]:
        assert i["cond"] <= oc.MAX_COND and i["step"] <= oc.MAX_STEP, (name, i)
        assert i["regularised"] == (a["status"] == 1)
    if a["V"] is None:
        costs = [i["cost"] for i in ref["iters"]]
        assert all(b < c for b, c in zip(costs[1:], costs[:-1])), (name, costs)
    # held blocks stay, free ones move
    w = a["w"]
    const = (0, 1 + w["n_frames"]) if a["const_blocks"] is None else a["const_blocks"]
    start = [w["pivot"]] + list(w["frames"]) + list(w["exts"])
    end = [ref["pivot"]] + list(ref["frames"]) + list(ref["exts"])
    for b, (x0, x1) in enumerate(zip(start, end)):
        if b in const:
            assert np.array_equal(x0, x1), (name, b)
        elif name != "empty_frame" or b != 2:
            assert np.abs(x0 - x1).max() > 1e-4, (name, b)


def test_empty_frame_is_decoupled_and_regularised():
    ref = oc.solve_reference("empty_frame")
    w = oc.empty_frame()
    s = oc.system_reference("empty_frame")
    assert not s["H"][12:18, :].any() and not s["H"][:, 12:18].any() and not s["g"][12:18].any()
    assert ref["status"] == 1 and np.abs(ref["frames"][1] - w["frames"][1]).max() <= 1e-15


def test_huber_rows_take_their_branches(orc):
    """more than 40 % of the residuals are outliers at delta = 0.05, and the planted rows: a point exactly on its plane and one exactly on its line (zero residual;
    the line's row is zero, Eigen's normalized() of a zero vector), a residual of 1e6 delta, and the weights 0, 1e-3 and 1e3"""
    w = oc.huber()
    s = oc.system_reference("huber")
    p = w["planted"]
    r, J = orc.pure_odom_eval_batch(w["types"], w["points"], w["coeffs"], w["sqrt_info"], w["fi"], w["ei"], w["pivot"], w["frames"], w["exts"])
    share = float(s["outlier"].mean())
    share_ragged = float(oc.system_reference("huber on ragged")["outlier"].mean())
    print(f"ODOM_MEASURED huber: outlier share {share:.3f}, on the ragged window {share_ragged:.3f} (above 0.4)")
    assert share > 0.4 and share_ragged > 0.4
    assert r[p["on_plane"]] == 0.0 and not s["outlier"][p["on_plane"]] and np.abs(J[p["on_plane"]]).max() > 0.5
    assert r[p["on_line"]] == 0.0 and not s["outlier"][p["on_line"]] and not J[p["on_line"]].any()
    assert s["outlier"][p["far"]] and 0.99e6 < abs(r[p["far"]]) / oc.HUBER_DELTA < 1.01e6
    assert r[p["w0"]] == 0.0 and not J[p["w0"]].any() and not s["outlier"][p["w0"]]
    assert 0.0 < abs(r[p["w_small"]]) < oc.HUBER_DELTA and not s["outlier"][p["w_small"]]
    assert abs(r[p["w_large"]]) > 10 * oc.HUBER_DELTA and s["outlier"][p["w_large"]]
    assert _group_sizes(w) == {(0, 0): 3, (0, 1): 255, (1, 0): 256, (1, 1): 257}
    # no loss: delta = 0 and delta = 1e9 never take the outlier branch -- the same bits
    a, b = (oc.window_system(w, w["pivot"], w["frames"], w["exts"], hd) for hd in (0.0, 1e9))
    assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"]) and a["cost"] == b["cost"] and not a["outlier"].any() and not b["outlier"].any()
    # the iterate's free system is well conditioned with the planted rows in it
    free = np.r_[6:18, 24:30]
    assert np.linalg.cond(s["H"][np.ix_(free, free)]) <= oc.MAX_COND


def test_huber_is_continuous_at_the_threshold():
    """rho0 and rho1 are continuous at sq = delta^2, so a residual whose branch flips in the last bit moves H, g and the cost by rounding only: no case needs a
    margin from the threshold"""
    d = oc.HUBER_DELTA
    for sq in (np.nextafter(d * d, 0.0), d * d, np.nextafter(d * d, 1.0)):
        rho0, rho1, _ = oc.huber_rho(np.array([sq]), d)
        assert abs(rho0[0] - d * d) <= 4e-16 * d * d and abs(rho1[0] - 1.0) <= 4e-16


SYSTEM_MUTANT_CASES = {"rows_by_rho1": "huber", "outlier_cost_sq": "huber", "offsets_swapped": "ragged", "tile_dropped": "ragged"}
GN_MUTANT_CASES = {"V_transposed": "masks dense V", "plus_offset_6b": "masks", "no_regularisation": "empty_frame"}


@pytest.mark.parametrize("mutant", list(SYSTEM_MUTANT_CASES))
def test_the_bars_tell_a_wrong_assembly(mutant):
    name = SYSTEM_MUTANT_CASES[mutant]
    fn, hd = oc.SYSTEMS[name]
    w = fn()
    bad = oc.window_system(w, w["pivot"], w["frames"], w["exts"], hd, mutant)
    m = oc.measure_system(bad, oc.system_reference(name))
    _show(f"mutant {mutant} on {name}", m)
    assert not oc.within(m), (mutant, m)
    if mutant == "rows_by_rho1":
        assert m["H per block"][0] > 100 * oc.H_BAR and m["cost"][0] == 0.0                       # (the cost does not see the row scaling: H and g have to)
    if mutant == "outlier_cost_sq":
        assert m["cost"][0] > 100 * oc.COST_BAR and m["H per block"][0] == 0.0
    if mutant in ("offsets_swapped", "tile_dropped"):
        assert m["H per block"][0] > 100 * oc.H_BAR or m["H zero blocks"][0] > 0.0


@pytest.mark.parametrize("mutant", list(GN_MUTANT_CASES))
def test_the_bars_tell_a_wrong_solve(mutant):
    name = GN_MUTANT_CASES[mutant]
    good, bad = oc.solve_reference(name), oc.solve_reference(name, mutant)
    m = oc.measure_poses(bad, good)
    _show(f"mutant {mutant} on {name}", m)
    assert m["poses"][0] > 100 * oc.POSE_BAR, (mutant, m)
    if mutant == "no_regularisation":
        assert bad["status"] == 2 and good["status"] == 1
    if mutant == "plus_offset_6b":
        # the dense-V case alone would not do: with the identity V and no constant block before a free one the two offsets coincide
        a = oc.solve_args(name)
        assert a["const_blocks"] == oc.MASK_CONST and 2 in a["const_blocks"] and 5 in a["const_blocks"]


def test_the_recorded_figures_belong_to_these_cases():
    """tests/golden/odom_tolerances.json: the bars are the ones above, every system and solve of odom_cases has its measured figures, each inside its bar"""
    import json
    import os
    rec = json.load(open(os.path.join(oc.ROOT, "tests", "golden", "odom_tolerances.json")))
    assert rec["bars"] == {"H": oc.H_BAR, "g": oc.G_BAR, "cost": oc.COST_BAR, "poses": oc.POSE_BAR}
    for name in list(oc.SYSTEMS) + ["ragged sorted", "ragged reversed", "huber no loss", "device_built_order interleaved", "device_built_order grouped"]:
        assert {"H per block", "H zero blocks", "g per block", "g zero blocks", "cost", "count difference", "H asymmetry"} <= set(rec["cases"][name]), name
    for name in oc.SOLVES:
        assert "poses" in rec["cases"][name], name
    for name, case in rec["cases"].items():
        for q, d in case.items():
            assert d["measured"] <= d["bar"], (name, q, d)


def test_pose_plus_is_linear_in_V(orc, mla):
    """the reference's Plus with a dense V: the package's host function and the oracle's agree, and V d is what is applied (V read row-major)"""
    w = oc.masks_and_V()
    d = np.array([0.01, -0.02, 0.03, 0.004, -0.005, 0.006])
    for b in range(7):
        x = ([w["pivot"]] + list(w["frames"]) + list(w["exts"]))[b]
        got = mla.pose_plus(x, d, w["V"][b])
        assert np.abs(got - orc.pose_plus(x, d, w["V"][b])).max() <= 1e-15
        assert np.abs(got - mla.pose_plus(x, w["V"][b] @ d, None)).max() <= 1e-15
        assert np.abs(got - mla.pose_plus(x, w["V"][b].T @ d, None)).max() > 1e-4
