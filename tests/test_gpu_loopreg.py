"""Loop-closure local registration on the device (m-loam_amd/csrc/loopreg.hip; mlh_loop_*) against the C++ restatement of the reference's lines
(tests/host/loopreg_ref.cpp through tests/loopreg_cases.py), which tests/test_loopreg_cases.py holds on the CPU. Everything goes through the C-ABI.

Bounds: transformed and filtered clouds bit-equal; match validity and counts equal and the f32-born coefficients bit-equal (zero decision flips: the crafted decisions
keep 1e-3 from their thresholds, asserted on the restatement before the GPU is asked); normal equations within 1e-9 of the largest entry (the kernel sums a block's
scalar form in tiles, the restatement its three rows in order); poses within 1e-7."""
import os
import subprocess

import numpy as np
import pytest

import loopreg_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NE_TOL, POSE_TOL = 1e-9, 1e-7


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_cloud(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _poses3():
    s = lc.scene()
    return {"T_ini": s["T_ini"], "truth": s["truth"], "far": lc.yaw_T(-40.0, (3.0, 2.5, -0.6))}


def _check_matches(ctx, clouds4, T, label):
    ctx.loop_set_clouds(*clouds4)
    ws, wc = lc.match_surf(clouds4[0], clouds4[2], T), lc.match_corner(clouds4[1], clouds4[3], T)
    for kind, want in ((0, ws), (1, wc)):
        valid, coeffs, n = ctx.loop_match(kind, T)
        flips = int((valid != want["valid"]).sum())
        assert flips == 0, (label, kind, flips)
        assert n == want["n"], (label, kind, n, want["n"])
        assert np.array_equal(_bits64(coeffs), _bits64(want["coeffs"])), (label, kind, int((_bits64(coeffs) != _bits64(want["coeffs"])).sum()))
    return ws, wc


def _save_scene(mla, ctx, s):
    from scipy.spatial.transform import Rotation as Rot
    keys = []
    for T, (surf, corner) in zip(s["poses"], s["clouds"]):
        pose = np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
        keys.append(ctx.keyframe_save(pose, np.eye(6) * 1e-4, surf, corner))
    return keys


def test_build_clouds_is_transform_concatenation_and_voxel_grid(mla, ctx, orc):
    """the scene's two lists, plus a keyframe whose surf cloud is empty and whose corner cloud has one point and one the other way round: the pre-filter clouds are
    the restatement's f32 transform + concatenation bit for bit, the filtered clouds the voxel-grid restatement of those bit for bit, the counts equal; the totals
    are no multiple of the 256-point transform tile; a second build allocates nothing"""
    s = lc.scene()
    keys = _save_scene(mla, ctx, s)
    assert keys == list(range(10))
    one = np.array([[1.5, -2.0, 0.7, 1.0]], np.float32)
    eye7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
    k_a = ctx.keyframe_save(eye7, np.eye(6), lc.EMPTY, one)
    k_b = ctx.keyframe_save(eye7, np.eye(6), one * 2.0, lc.EMPTY)
    odd = lc.yaw_T(-70.0, (4.0, 1.0, 0.5)).astype(np.float32)
    data, model = list(s["lists"][0]), list(s["lists"][1])
    data = data[:2] + [(k_a, odd)] + data[2:] + [(k_b, odd)]
    model = [(k_b, odd)] + model
    extra = {k_a: (lc.EMPTY, one), k_b: (one * 2.0, lc.EMPTY)}
    cloud_of = lambda k, kind: extra[k][kind] if k in extra else s["clouds"][k][kind]
    want_pre = []
    for lst in (model, data):
        for kind in (0, 1):
            parts = [lc.transform(cloud_of(k, kind), Tf) for k, Tf in lst if len(cloud_of(k, kind))]
            want_pre.append(np.concatenate(parts))
    assert all(len(p) % 256 for p in want_pre)
    n_pre, n_ds = ctx.loop_build_clouds(data, model)
    for which in range(4):
        pre, flt = ctx.loop_cloud(which, filtered=False), ctx.loop_cloud(which, filtered=True)
        want_flt = orc.voxel_grid(want_pre[which], lc.LEAF)
        assert n_pre[which] == len(want_pre[which]) and n_ds[which] == len(want_flt), (which, n_pre, n_ds)
        assert _same_cloud(pre, want_pre[which]), which
        assert _same_cloud(flt, want_flt), which
    a0 = ctx.loop_info()["allocations"]
    ctx.loop_build_clouds(data, model)
    assert ctx.loop_info()["allocations"] == a0
    # the scene's own lists give the clouds every other test sets directly
    ctx.loop_build_clouds(*s["lists"])
    for which in range(4):
        assert _same_cloud(ctx.loop_cloud(which), s["clouds4"][which]), which
    # registration straight from the built clouds = registration from the same clouds given directly
    got = ctx.loop_register(s["T_ini"])
    ctx.loop_set_clouds(*s["clouds4"])
    again = ctx.loop_register(s["T_ini"])
    assert np.array_equal(_bits64(got["T_relative"]), _bits64(again["T_relative"]))


def test_build_clouds_at_tile_edges(mla, ctx, orc):
    """keyframes whose (surf, corner) sizes sit on the edges of the 256-point transform tile -- (0, 257), (1, 0), (513, 256), (255, 1), (256, 513), (7, 7): points
    uniform in +-20 m, intensity 0..16 -- in both lists under twelve distinct transforms, then a build without a model list, one without a data list and one whose
    keyframes are all empty: n_pre, the pre-filter clouds (the restatement's f32 transform + concatenation) and the filtered clouds (the voxel-grid restatement of
    those at the loop's own leaf, 0.4) bit for bit; zeros and empty clouds where a list is empty; a repeat of the largest build allocates nothing"""
    rng = np.random.default_rng(1207)

    def crafted(n):
        a = np.empty((n, 4), np.float32)
        a[:, :3] = rng.uniform(-20, 20, (n, 3))
        a[:, 3] = rng.uniform(0, 16, n)
        return a

    sizes = [(0, 257), (1, 0), (513, 256), (255, 1), (256, 513), (7, 7)]
    clouds = [(crafted(ns), crafted(nc)) for ns, nc in sizes]
    eye7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
    keys = [ctx.keyframe_save(eye7, np.eye(6), surf, corner) for surf, corner in clouds]
    k_none = ctx.keyframe_save(eye7, np.eye(6), lc.EMPTY, lc.EMPTY)
    T = lambda i: lc.yaw_T(17.0 * i - 40.0, (0.5 * i - 2.0, 1.5 - 0.3 * i, 0.1 * i)).astype(np.float32)
    model_all = [(k, T(i)) for i, k in enumerate(keys)]
    data_all = [(k, T(6 + i)) for i, k in reversed(list(enumerate(keys)))]

    def check(data, model, label):
        n_pre, n_ds = ctx.loop_build_clouds(data, model)
        for which in range(4):
            lst, kind = (model, data)[which >> 1], which & 1
            parts = [lc.transform(clouds[keys.index(k)][kind], Tf) for k, Tf in lst if k != k_none and len(clouds[keys.index(k)][kind])]
            want_pre = np.concatenate(parts) if parts else lc.EMPTY
            want_flt = orc.voxel_grid(want_pre, lc.LEAF) if len(want_pre) else lc.EMPTY
            pre, flt = ctx.loop_cloud(which, filtered=False), ctx.loop_cloud(which, filtered=True)
            print(label, which, "n_pre", n_pre[which], len(want_pre), "n_ds", n_ds[which], len(want_flt))
            assert n_pre[which] == len(want_pre) and n_ds[which] == len(want_flt), (label, which, n_pre, n_ds)
            assert _same_cloud(pre, want_pre), (label, which)
            assert _same_cloud(flt, want_flt), (label, which)
        info = ctx.loop_info()
        assert info["n_pre"] == list(n_pre) and info["n_ds"] == list(n_ds), label

    check(data_all, model_all, "both")
    assert ctx.loop_info()["n_pre"] == [1032, 1034, 1032, 1034]
    a0 = ctx.loop_info()["allocations"]
    check(data_all, model_all, "both again")
    assert ctx.loop_info()["allocations"] == a0
    check(data_all, [], "no model")
    assert ctx.loop_info()["n_pre"][:2] == [0, 0] and ctx.loop_info()["n_ds"][:2] == [0, 0]
    check([], model_all, "no data")
    assert ctx.loop_info()["n_pre"][2:] == [0, 0] and ctx.loop_info()["n_ds"][2:] == [0, 0]
    check([(k_none, T(3))], [(k_none, T(4)), (k_none, T(5))], "all empty")
    assert ctx.loop_info()["n_pre"] == [0, 0, 0, 0] and ctx.loop_info()["n_ds"] == [0, 0, 0, 0]
    assert all(len(ctx.loop_cloud(w, filtered=f)) == 0 for w in range(4) for f in (False, True))
    check(data_all, model_all, "both after the empty ones")
    assert ctx.loop_info()["allocations"] == a0


@pytest.mark.parametrize("pose", ["T_ini", "truth", "far"])
def test_match_on_the_scene(mla, ctx, pose):
    """both kinds at the hand-over pose, the truth and a pose far off: validity, features.size() and every coefficient's bits"""
    s = lc.scene()
    ws, wc = _check_matches(ctx, s["clouds4"], _poses3()[pose], pose)
    if pose != "far":
        assert ws["n"] > 0.5 * len(s["clouds4"][2]) and wc["n"] > len(s["clouds4"][3])       # (the corner count is in features: two per point)
    else:
        assert ws["n"] < 0.7 * len(s["clouds4"][2])


def test_match_crafted_decisions(mla, ctx):
    """fifth neighbour just inside / outside 2.0 and 5.0, a neighbour 0.25 m / 0.15 m off the fitted plane, a blob, a line, fewer than five map points in reach:
    the decisions the case generator asserted on the restatement (with their 1e-3 margins), on the device"""
    c = lc.crafted()
    ws, wc = _check_matches(ctx, c["clouds4"], np.eye(4), "crafted")
    assert ws["valid"].tolist() == c["surf_want"] and wc["valid"].tolist() == c["corner_want"]


def _half_outside_delta(clouds4, T, pose):
    lo, hi = 1e-4, 1.0
    for _ in range(40):
        mid = np.sqrt(lo * hi)
        r = lc.evaluate(clouds4, T, pose, lc.opts(huber_delta=mid))
        frac = r["outside"] / max(1, int(r["counts"].sum()))
        if 0.4 <= frac <= 0.6:
            return mid, frac
        lo, hi = (mid, hi) if frac > 0.6 else (lo, mid)
    raise AssertionError("no delta puts about half the blocks outside the inlier band")


def test_one_evaluation_at_a_fixed_pose(mla, ctx):
    """J^T J, J^T r, cost and counts at a pose that is not the matching pose, with delta = 1 and with a delta that leaves about half the blocks outside the inlier
    band (asserted on the restatement). Observed on an MI355X: H 2.3e-15, g 4.3e-15, cost 1.4e-16 of the largest entry, against the 1e-9 bar"""
    s = lc.scene()
    T = s["T_ini"]
    pose = lc.pose_of(lc.yaw_T(24.6, (0.2, -0.1, 0.05)))
    ctx.loop_set_clouds(*s["clouds4"])
    delta_half, frac = _half_outside_delta(s["clouds4"], T, pose)
    assert 0.4 <= frac <= 0.6
    for delta in (1.0, delta_half):
        want = lc.evaluate(s["clouds4"], T, pose, lc.opts(huber_delta=delta))
        got = ctx.loop_evaluate(T, pose, mla.loop_opts(huber_delta=delta))
        assert np.array_equal(got["counts"], want["counts"]) and want["counts"].min() > 0
        eH = np.abs(got["H"] - want["H"]).max() / np.abs(want["H"]).max()
        eg = np.abs(got["g"] - want["g"]).max() / np.abs(want["g"]).max()
        ec = abs(got["cost"] - want["cost"]) / want["cost"]
        print(f"delta {delta:.4g}: H {eH:.2e} g {eg:.2e} cost {ec:.2e}")
        assert eH <= NE_TOL and eg <= NE_TOL and ec <= NE_TOL, (delta, eH, eg, ec)
        again = ctx.loop_evaluate(T, pose, mla.loop_opts(huber_delta=delta))
        assert np.array_equal(_bits64(got["H"]), _bits64(again["H"])) and np.array_equal(_bits64(got["g"]), _bits64(again["g"])) and got["cost"] == again["cost"]


def _same_outer(got, want):
    assert got["n_outer"] == want["n_outer"]
    for a, b in zip(got["outer"], want["outer"]):
        for k in ("entered", "ran", "surf_num", "corner_num", "lm_iterations", "termination"):
            assert a[k] == b[k], (k, a, b)


def test_register_on_the_scene(mla, ctx):
    """from the Scan Context hand-over (the truth's yaw on the 6-degree grid, zero translation): T_relative and para_pose within 1e-7 of the restatement (observed
    on an MI355X: 8.9e-16 for both), the per-outer counts, LM iteration counts and terminations equal, accepted equal at thresholds on both sides of opti_cost"""
    s = lc.scene()
    ctx.loop_set_clouds(*s["clouds4"])
    want = lc.register(s["clouds4"], s["T_ini"])
    got = ctx.loop_register(s["T_ini"])
    eT, ep = np.abs(got["T_relative"] - want["T_relative"]).max(), np.abs(got["para_pose"] - want["para_pose"]).max()
    print(f"|dT| {eT:.2e} |dpose| {ep:.2e} cost {got['opti_cost']:.6f} / {want['opti_cost']:.6f}")
    assert eT <= POSE_TOL and ep <= POSE_TOL
    _same_outer(got, want)
    assert want["n_outer"] == 2 and all(o["ran"] for o in want["outer"])
    assert abs(got["opti_cost"] - want["opti_cost"]) <= 1e-9 * want["opti_cost"] and got["accepted"] and want["accepted"]
    assert np.abs(got["T_relative"] - s["truth"]).max() < 0.05
    for thr, acc in ((want["opti_cost"] * 1.01, True), (want["opti_cost"] * 0.99, False)):
        assert ctx.loop_register(s["T_ini"], mla.loop_opts(local_registration_threshold=thr))["accepted"] is acc
        assert lc.register(s["clouds4"], s["T_ini"], lc.opts(threshold=thr))["accepted"] is acc


def _mostly_displaced(cloud, keep_every=8):
    """the cloud with all but every keep_every-th point moved 200 m away: its match ratio stays under 0.2"""
    out = cloud.copy()
    far = np.ones(len(out), bool)
    far[::keep_every] = False
    out[far, :3] += np.float32(200.0)
    return out


def test_the_rules_of_the_outer_loop(mla, ctx):
    s = lc.scene()
    ms, mc, ds, dc = s["clouds4"]
    # data 30 m above the model: nothing matches, break in iteration 0, T_ini back bit for bit with cost 1e7, not accepted
    T_far = lc.yaw_T(24.0, (0.0, 0.0, 30.0))
    ctx.loop_set_clouds(ms, mc, ds, dc)
    got, want = ctx.loop_register(T_far), lc.register(s["clouds4"], T_far)
    assert want["n_outer"] == 1 and not want["outer"][0]["ran"] and want["opti_cost"] == 1e7 and not want["accepted"]
    _same_outer(got, want)
    assert np.array_equal(_bits64(got["T_relative"]), _bits64(T_far)) and got["opti_cost"] == 1e7 and not got["accepted"]
    # surf under 0.2 and NO corner data: 0 / 0 is NaN, NaN <= 0.2 is false, the loop does not break and the solve runs on surf alone
    thin = _mostly_displaced(ds)
    c4 = [ms, mc, thin, lc.EMPTY]
    want = lc.register(c4, s["T_ini"])
    assert want["n_outer"] == 2 and all(o["ran"] and o["corner_num"] == 0 and 0 < o["surf_num"] <= 0.2 * len(thin) for o in want["outer"])
    ctx.loop_set_clouds(*c4)
    got = ctx.loop_register(s["T_ini"])
    _same_outer(got, want)
    assert np.abs(got["T_relative"] - want["T_relative"]).max() <= POSE_TOL
    # ... with corner data that matches nothing the same surf cloud breaks
    c4 = [ms, mc, thin, dc + np.array([0.0, 0.0, 200.0, 0.0], np.float32)]
    want = lc.register(c4, s["T_ini"])
    assert want["n_outer"] == 1 and not want["outer"][0]["ran"]
    ctx.loop_set_clouds(*c4)
    got = ctx.loop_register(s["T_ini"])
    _same_outer(got, want)
    assert np.array_equal(_bits64(got["T_relative"]), _bits64(s["T_ini"])) and got["opti_cost"] == 1e7
    # a corner ratio above 1.0 (two features per matched point) alone keeps the loop going while surf is under 0.2
    c4 = [ms, mc, thin, dc]
    want = lc.register(c4, s["T_ini"])
    assert want["n_outer"] == 2 and all(o["ran"] and o["corner_num"] > len(dc) and o["surf_num"] <= 0.2 * len(thin) for o in want["outer"])
    ctx.loop_set_clouds(*c4)
    got = ctx.loop_register(s["T_ini"])
    _same_outer(got, want)
    assert np.abs(got["T_relative"] - want["T_relative"]).max() <= POSE_TOL
    # both data clouds empty: what the restatement does -- no break, a solve without residual blocks, cost 0, accepted
    c4 = [ms, mc, lc.EMPTY, lc.EMPTY]
    want = lc.register(c4, s["T_ini"])
    assert want["n_outer"] == 2 and want["opti_cost"] == 0.0 and want["accepted"]
    ctx.loop_set_clouds(*c4)
    got = ctx.loop_register(s["T_ini"])
    _same_outer(got, want)
    assert got["opti_cost"] == 0.0 and got["accepted"] and np.abs(got["T_relative"] - want["T_relative"]).max() <= 1e-15


def test_state_errors_and_repeatability(mla, ctx, synth, case16, feats16):
    s = lc.scene()
    ctx.loop_set_clouds(*s["clouds4"])
    a, b = ctx.loop_register(s["T_ini"]), ctx.loop_register(s["T_ini"])
    assert np.array_equal(_bits64(a["T_relative"]), _bits64(b["T_relative"])) and a["opti_cost"] == b["opti_cost"] and a["outer"] == b["outer"]
    # a call after other work on the same context = a call on a fresh context
    other = mla.Context(0)
    try:
        surf, corner = feats16
        other.map_set(mla.SURF, case16["surf_map"])
        other.map_set(mla.CORNER, case16["corner_map"])
        other.features_set(mla.SURF, surf)
        other.features_set(mla.CORNER, corner)
        other.scan2map(case16["p0"], want_stats=False)
        other.loop_set_clouds(*s["clouds4"])
        c = other.loop_register(s["T_ini"])
        assert np.array_equal(_bits64(a["T_relative"]), _bits64(c["T_relative"])) and a["opti_cost"] == c["opti_cost"] and a["outer"] == c["outer"]
        # MLH_ERR_STATE while a submitted solve is uncollected: the loop registration, and the other stages of the loop process -- FGR and the pose graph, each in
        # a state in which nothing but the open solve stands in its entries' way, and with the counters of a call that ran
        for which in (mla.LOOP_MODEL_SURF, mla.LOOP_DATA_SURF):
            other.fgr_features(which)
        pairs = other.fgr_match()
        other.pg_reset()
        for p in ([0, 0, 0, 0, 0, 0, 1.0], [1.0, 0.05, 0, 0, 0, 0, 1.0], [2.0, 0.2, 0.05, 0, 0, 0, 1.0]):
            other.pg_add_keyframe(p)
        other.pg_set_loop(2, 0, [2.1, 0.1, 0.0, 0, 0, 0, 1.0])
        lin = other.pg_linearize(2)
        other.map_set(mla.SURF, case16["surf_map"])
        other.map_set(mla.CORNER, case16["corner_map"])
        other.scan2map_begin(case16["p0"])
        with pytest.raises(mla.MlhError, match="mlh error -3"):
            other.loop_register(s["T_ini"])
        fgr_info, pg_info = other.fgr_info(), other.pg_info()
        assert fgr_info["launches"] > 0 and pg_info["n_keyframes"] == 3 and pg_info["n_loops"] == 1
        refused = [lambda: other.fgr_features(mla.LOOP_MODEL_SURF), other.fgr_match, other.fgr_register,
                   lambda: other.pg_optimize(2), lambda: other.pg_linearize(2), lambda: other.pg_solve_step(2, 1e4)]
        for call in refused:
            with pytest.raises(mla.MlhError, match="mlh error -3.*has not been collected"):
                call()
        assert other.fgr_info() == fgr_info and other.pg_info() == pg_info
        other.scan2map_end()
        d = other.loop_register(s["T_ini"])
        assert np.array_equal(_bits64(a["T_relative"]), _bits64(d["T_relative"]))
        other.fgr_features(mla.LOOP_MODEL_SURF)
        assert np.array_equal(other.fgr_match(), pairs)
        assert other.fgr_register()["n_corres"] >= 0
        again = other.pg_linearize(2)
        assert np.array_equal(_bits64(again["r"]), _bits64(lin["r"])) and again["cost"] == lin["cost"]
        assert other.pg_solve_step(2, 1e4)["step"].shape == (12,)
        assert other.pg_optimize(2)["n_keyframes"] == 3
    finally:
        other.close()
    # MLH_ERR_INVALID on bad options
    for bad in (dict(max_outer=0), dict(max_outer=9), dict(huber_delta=float("nan")), dict(match_sq_dis_surf=0.0), dict(max_lm_iterations=-1), dict(leaf_surf=0.0)):
        with pytest.raises(mla.MlhError, match="mlh error -1"):
            ctx.loop_register(s["T_ini"], mla.loop_opts(**bad))
    with pytest.raises(mla.MlhError, match="mlh error -1"):
        ctx.loop_register(np.full((4, 4), np.nan))
    # keys that are not in the store: an error, not a fault
    eye = np.eye(4, dtype=np.float32)
    for data, model in (([(0, eye)], []), ([], [(-1, eye)])):
        with pytest.raises(mla.MlhError, match="mlh error -1"):
            ctx.loop_build_clouds(data, model)
    _save_scene(mla, ctx, s)
    with pytest.raises(mla.MlhError, match="mlh error -1"):
        ctx.loop_build_clouds([(10, eye)], [(0, eye)])
    with pytest.raises(mla.MlhError, match="mlh error -1"):
        ctx.loop_build_clouds([(0, eye * np.float32("nan"))], [(0, eye)])


def test_loopreg_selftest_exits_zero():
    exe = os.path.join(ROOT, "m-loam_amd", "host", "loopreg_selftest")
    assert os.path.exists(exe), "m-loam_amd/host/loopreg_selftest has not been built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
