"""MLH_FLAG_POSE_COV / mlh_scan2map_cov: scan2MapOptimization's pose covariance (lidar_mapper_keyframe.cpp:600-622, 632) delivered with the pose.

The LM state's record at the pose the loop ends on IS evalHessian at that pose, so the wavefront that publishes the pose inverts it (solver_dev.hpp: inv6_wave) and
stores H and H^-1 in front of the pose; no launch and no host wait are added. Held here against the CPU checker (H), against a bound derived for an LU inverse
(H^-1), against the reference's own lines (cov_mapping), across every form the solve's launches can take (same 72 doubles, bit for bit), on the edges, and for the
getter's state rules. Scenes: conftest's case16 / feats16 (a 16-ring scan against the "50k" map: 3 838 + 1 613 features) or cuts of it.

Where the tolerances come from:
  H        1e-9 of the largest entry: the project's bar for f64 normal equations.
  H^-1     eps = 2^-52; || X A - I ||_max <= 100 eps cond2(A): the residual bound of an inverse from LU with partial pivoting, a modest multiple of n^2 eps ||X|| ||A||
           with n = 6; the same against numpy.linalg.inv(A), relative to ||X||_max.
  cov      against the reference: || X - X_ref ||_2 / || X_ref ||_2 <= 6e-9 cond2(H_ref) -- the first-order perturbation of an inverse under a relative change of H of
           1e-9 per entry (|| dH ||_2 <= 6 x 1e-9 ||H||_max <= 6e-9 ||H||_2); the rounding of the inverse itself (1e-14 cond2) is negligible beside it. Only on
           scenes with cond2(H_ref) <= 1e6, asserted: case16 has cond2 = 345 (seed 42, preset "50k", checked on the CPU with the checker when this was written).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LM_ENV = ("MLH_LM_CONSUMER", "MLH_LM_LOOP", "MLH_LOOP_TAGGED", "MLH_TRACK_LOOP")
KERNELS = ("KNN", "FIT", "LINEARIZE", "SOLVE", "KNN_PRE", "KNN_FIRST")
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
ERR_STATE, ERR_UNSUPPORTED = "mlh error -3", "mlh error -5"


def _lm_env(mode):
    return {"MLH_LM_CONSUMER": mode[0], "MLH_LM_LOOP": mode[1], "MLH_LOOP_TAGGED": "0" if mode.endswith("b") else "1"}


def _with_env(env, call):
    """`env` holds for this call only (the library reads the schedule switches per call)"""
    saved = {k: os.environ.pop(k, None) for k in LM_ENV}
    try:
        os.environ.update(env or {})
        return call()
    finally:
        for k in LM_ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _features11(feats, cov_scale, rng):
    """(m, 4) features -> (m, 11) PointXYZIWithCov records with a small per-point covariance (so that with_ua weighs them differently)"""
    out = np.zeros((len(feats), 11), np.float32)
    out[:, :4] = feats[:, :4]
    d = rng.uniform(0.2, 1.0, (len(feats), 3)) * cov_scale
    out[:, 4] = d[:, 0]; out[:, 7] = d[:, 1]; out[:, 9] = d[:, 2]
    out[:, 10] = out[:, 4] + out[:, 7] + out[:, 9]
    return out


def _stage(c, mla, case, surf, corner):
    c.map_set(mla.SURF, case["surf_map"])
    c.map_set(mla.CORNER, case["corner_map"])
    c.features_set(mla.SURF, surf)
    c.features_set(mla.CORNER, corner)


def _flagged(mla, **kw):
    return mla.default_opts(pose_cov=True, **kw)


def _solve(c, p0, opts, want_stats=False):
    """mlh_scan2map + the getter -> pose, the 72 doubles (cov then H_final), stats"""
    pose, st = c.scan2map(p0, opts, want_stats=want_stats)
    cov, H = c.scan2map_cov()
    return pose, np.concatenate([cov.ravel(), H.ravel()]), st


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _oracle_H(orc, case, surf, corner, traces, res):
    """evalHessian at the pose the checker's scan2map returned, over the last outer iteration's blocks: its correspondences (matched at the pose that iteration
    began from), linearised at the final pose with the Huber correction. With with_ua this is the checker's own H_final (6.8e-16 of it on case16, checked when this
    was written); the checker fills H_final only with with_ua, so the with_ua-off case is put together here from the same two checker calls."""
    start = res["outer"][-2]["pose_after"] if len(res["outer"]) > 1 else case["p0"]
    H = np.zeros((6, 6))
    for kind, m, f, tr in (("s", case["surf_map"], surf, traces[0]), ("c", case["corner_map"], corner, traces[1])):
        v, co = orc.Map(m).match(kind, f, start)
        H += orc.linearize(kind, f, tr, res["pose"], v, co, huber_delta=0.1)["H"]
    return H


def _assert_inverse_bound(X, A, what):
    """the residual bound of an LU inverse, and the same against numpy's inverse (module docstring)"""
    cond = np.linalg.cond(A, 2)
    res = float(np.abs(X @ A - np.eye(6)).max())
    ref = np.linalg.inv(A)
    dif = float(np.abs(X - ref).max() / np.abs(X).max())
    print(f"{what}: cond2 {cond:.4e}  |XA - I|max {res:.3e} = {res / (EPS * cond):.2f} eps cond2  |X - inv|max/|X|max {dif:.3e} = {dif / (EPS * cond):.2f} eps cond2")
    assert res <= 100 * EPS * cond, (what, res, cond)
    assert dif <= 100 * EPS * cond, (what, dif, cond)


@pytest.fixture(scope="module")
def feats11(feats16):
    rng = np.random.default_rng(5)
    return _features11(feats16[0], 0.01, rng), _features11(feats16[1], 0.01, rng)


@pytest.fixture(scope="module")
def ctx16(mla, case16, feats16):
    """one context with case16's maps and the plain features staged, the profiler counting every launch"""
    c = mla.Context(0)
    c.profile_enable()
    c.profile_sample(1)
    _stage(c, mla, case16, feats16[0], feats16[1])
    yield c
    c.close()


@pytest.fixture(scope="module")
def default72(ctx16, mla, case16):
    """the flagged default call's pose and 72 doubles, computed once"""
    pose, d72, _ = _solve(ctx16, case16["p0"], _flagged(mla))
    return pose, d72


# ---------------------------------------------------------------- 1. H against the checker, 2. the inverse at its bound
@pytest.mark.parametrize("with_ua", [False, True])
def test_H_final_equals_the_checkers_and_the_inverse_holds_its_bound(mla, orc, case16, feats16, feats11, with_ua):
    surf, corner = feats11 if with_ua else feats16
    flags = mla.FLAG_WITH_UA if with_ua else 0
    c = mla.Context(0)
    try:
        _stage(c, mla, case16, surf, corner)
        plain, _ = c.scan2map(case16["p0"], mla.default_opts(flags=flags), want_stats=False)
        pose, d72, _ = _solve(c, case16["p0"], _flagged(mla, flags=flags))
    finally:
        c.close()
    assert np.array_equal(_bits(pose), _bits(plain))                      # the flag does not touch the pose
    cov, H = d72[:36].reshape(6, 6), d72[36:].reshape(6, 6)
    res = orc.scan2map(orc.Map(case16["surf_map"]), orc.Map(case16["corner_map"]), surf, corner, case16["p0"], orc.mapper_params(with_ua=with_ua))
    traces = (surf[:, 10].astype(np.float64), corner[:, 10].astype(np.float64)) if with_ua else (np.full(len(surf), 0.0075), np.full(len(corner), 0.0075))
    Href = res["H_final"] if with_ua else _oracle_H(orc, case16, surf, corner, traces, res)
    assert np.abs(Href).max() > 1e3
    if with_ua:                                                           # (the construction used for with_ua off reproduces the checker's own matrix)
        assert np.abs(_oracle_H(orc, case16, surf, corner, traces, res) - Href).max() <= 1e-12 * np.abs(Href).max()
    err = float(np.abs(H - Href).max() / np.abs(Href).max())
    print(f"with_ua={with_ua}: |H - H_checker|max / |H|max = {err:.3e}")
    assert err <= 1e-9, err
    assert np.array_equal(H, H.T)
    _assert_inverse_bound(cov, H, f"case16 with_ua={with_ua}")


# ---------------------------------------------------------------- 3. the covariance against the reference's own lines
def test_cov_equals_the_references_cov_mapping(mla, orc, case16, feats11):
    if orc.ref_lib() is None:
        pytest.skip("oracle/_ref/libmloam_ref.so has not been built (needs the reference tree once)")
    surf, corner = feats11
    ref = orc.ref_scan2map(case16["surf_map"], case16["corner_map"], surf, corner, case16["p0"], with_ua=True)
    cond = np.linalg.cond(np.linalg.inv(ref["cov"]), 2)
    assert cond <= 1e6, cond                                              # the condition under which the bound below is claimed
    c = mla.Context(0)
    try:
        _stage(c, mla, case16, surf, corner)
        pose, d72, _ = _solve(c, case16["p0"], _flagged(mla, flags=mla.FLAG_WITH_UA))
    finally:
        c.close()
    cov = d72[:36].reshape(6, 6)
    rel = float(np.linalg.norm(cov - ref["cov"], 2) / np.linalg.norm(ref["cov"], 2))
    print(f"cond2(H_ref) {cond:.4e}  ||cov - cov_ref||_2 / ||cov_ref||_2 = {rel:.3e}  (bound {6e-9 * cond:.3e})  |pose - pose_ref| {np.linalg.norm(pose - ref['pose']):.3e}")
    assert rel <= 6e-9 * cond, (rel, cond)


# ---------------------------------------------------------------- 4. the same bits from every form
def test_every_form_delivers_the_same_72_doubles(ctx16, mla, case16, default72):
    c, p0 = ctx16, case16["p0"]
    pose0, want = default72
    assert np.isfinite(want).all() and np.abs(want[:36]).max() > 0
    for mode in ("00", "10", "11", "11b"):
        pose, got, _ = _with_env(_lm_env(mode), lambda: _solve(c, p0, _flagged(mla)))
        assert np.array_equal(_bits(pose), _bits(pose0)), mode
        assert np.array_equal(_bits(got), _bits(want)), mode
    pose, got, st = _solve(c, p0, _flagged(mla), want_stats=True)
    assert np.array_equal(_bits(pose), _bits(pose0)) and np.array_equal(_bits(got), _bits(want))
    need = max(int(x["lm_iterations"]) for x in st)
    for kw in ({}, {"lm_lookahead": need}):
        c.scan2map_begin(p0, _flagged(mla), **kw)
        pose, status = c.scan2map_end()
        cov, H = c.scan2map_cov()
        assert status == 0 and np.array_equal(_bits(pose), _bits(pose0)), kw
        assert np.array_equal(_bits(np.concatenate([cov.ravel(), H.ravel()])), _bits(want)), kw


def test_two_solves_in_flight_keep_their_own_matrices(ctx16, mla, case16, default72):
    c, p0 = ctx16, case16["p0"]
    c.scan2map_begin(p0, _flagged(mla))
    c.scan2map_begin_chained(IDENT, IDENT, _flagged(mla))
    pose_a, st_a = c.scan2map_end()
    a = np.concatenate([x.ravel() for x in c.scan2map_cov()])
    pose_b, st_b = c.scan2map_end()
    b = np.concatenate([x.ravel() for x in c.scan2map_cov()])
    assert st_a == 0 and st_b == 0
    assert np.array_equal(_bits(a), _bits(default72[1]))                 # the first frame is the synchronous call's
    assert not np.array_equal(_bits(a), _bits(b))                        # the second began from the first one's result: another pose, another Hessian
    assert np.array_equal(_bits(pose_a), _bits(default72[0])) and not np.array_equal(_bits(pose_a), _bits(pose_b))
    _assert_inverse_bound(b[:36].reshape(6, 6), b[36:].reshape(6, 6), "chained frame")


@pytest.mark.parametrize("kw", [dict(max_outer=1), dict(max_outer=3), dict(max_lm_iterations=1)])
def test_forms_agree_over_loop_counts(ctx16, mla, case16, kw):
    """one and three outer iterations; one LM iteration (the loop ends on its budget, termination 0, right behind an accepted step)"""
    c, p0 = ctx16, case16["p0"]
    pose0, want, _ = _solve(c, p0, _flagged(mla, **kw))
    plain, _ = c.scan2map(p0, mla.default_opts(**kw), want_stats=False)
    assert np.array_equal(_bits(pose0), _bits(plain))
    for mode in ("00", "10", "11b"):
        pose, got, _ = _with_env(_lm_env(mode), lambda: _solve(c, p0, _flagged(mla, **kw)))
        assert np.array_equal(_bits(pose), _bits(pose0)) and np.array_equal(_bits(got), _bits(want)), (kw, mode)
    pose, got, st = _solve(c, p0, _flagged(mla, **kw), want_stats=True)
    assert np.array_equal(_bits(got), _bits(want)), kw
    if "max_lm_iterations" in kw:
        assert st[-1]["termination"] == 0 and st[-1]["lm_iterations"] == 1
    _assert_inverse_bound(want[:36].reshape(6, 6), want[36:].reshape(6, 6), str(kw))


def test_downsample_scan2map_delivers_the_two_calls_matrices(mla, orc, synth, case16):
    """staged as the launch census stages it: the one-call form on the device-resident fused clouds against the two calls on host copies of them"""
    scans = case16["scans"] * 2
    ext = np.array([np.concatenate([r[4:7], r[:4]]) for r in synth.HERCULES_BODY_T_LASER])[:2]
    for e in ext:
        e[3:] /= np.linalg.norm(e[3:])
    covs = np.stack([np.zeros((6, 6)), np.diag([0.0025] * 3 + [0.00030461] * 3)])
    meas = np.diag([0.0025] * 3)
    p0 = case16["p0"]
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"]); c.map_set(mla.CORNER, case16["corner_map"])
        c.fuse_reset()
        ref_surf, ref_corner = [], []
        for i, s in enumerate(scans):
            c.scan_upload(s.points, s.scan_start, s.scan_end); c.extract_run()
            ex = c.extract_fetch(); lf = c.extract_voxel(0.2)
            c.fuse_add_scan(i, ext[i])
            ref_surf.append(orc.transform_cloud_feature(lf, ext[i], i))
            ref_corner.append(orc.transform_cloud_feature(s.points[ex["less_sharp"]], ext[i], i))
        host = (np.concatenate(ref_surf), np.concatenate(ref_corner))
        o = _flagged(mla, flags=mla.FLAG_WITH_UA)
        loops = c.info()["loop_launches"]
        pose_d, _ = c.downsample_scan2map(c.fused_cloud(mla.SURF), c.fused_cloud(mla.CORNER), 0.4, 0.2, ext, covs, meas, p0, o)
        assert c.info()["loop_launches"] == loops + 1                     # (the one-call form did run)
        d = np.concatenate([x.ravel() for x in c.scan2map_cov()])
        pose_h, _ = c.downsample_scan2map(host[0], host[1], 0.4, 0.2, ext, covs, meas, p0, o)
        h = np.concatenate([x.ravel() for x in c.scan2map_cov()])
    finally:
        c.close()
    assert np.array_equal(_bits(pose_d), _bits(pose_h)) and np.array_equal(_bits(d), _bits(h))
    _assert_inverse_bound(d[:36].reshape(6, 6), d[36:].reshape(6, 6), "downsample_scan2map")


# ---------------------------------------------------------------- 5. selections
@pytest.mark.parametrize("method", ["rnd", "fps"])
def test_selections(ctx16, mla, orc, case16, feats11, method):
    c, p0 = ctx16, case16["p0"]
    kw = dict(gf_method=mla.GF_METHODS[method], gf_ratio=0.3, gf_seed=5)
    pose0, want, _ = _solve(c, p0, _flagged(mla, **kw))
    plain, _ = c.scan2map(p0, mla.default_opts(**kw), want_stats=False)
    assert np.array_equal(_bits(pose0), _bits(plain))
    for mode in ("00", "10"):
        pose, got, _ = _with_env(_lm_env(mode), lambda: _solve(c, p0, _flagged(mla, **kw)))
        assert np.array_equal(_bits(pose), _bits(pose0)) and np.array_equal(_bits(got), _bits(want)), mode
    _, got, _ = _solve(c, p0, _flagged(mla, **kw), want_stats=True)
    assert np.array_equal(_bits(got), _bits(want))
    # the checker with the same selection fills H_final with with_ua only: the features with their covariances, in a context of their own
    cov, H = want[:36].reshape(6, 6), want[36:].reshape(6, 6)
    c2 = mla.Context(0)
    try:
        _stage(c2, mla, case16, feats11[0], feats11[1])
        pose_ua, got_ua, _ = _solve(c2, p0, _flagged(mla, flags=mla.FLAG_WITH_UA, **kw))
    finally:
        c2.close()
    res = orc.scan2map(orc.Map(case16["surf_map"]), orc.Map(case16["corner_map"]), feats11[0], feats11[1], p0,
                       orc.mapper_params(with_ua=True, gf_method=method, gf_ratio=0.3, seed=5))
    H_ua = got_ua[36:].reshape(6, 6)
    err = float(np.abs(H_ua - res["H_final"]).max() / np.abs(res["H_final"]).max())
    print(f"{method}: |H - H_checker|max / |H|max = {err:.3e}  |pose - pose_checker| = {np.linalg.norm(pose_ua - res['pose']):.3e}")
    assert err <= 1e-9, err
    _assert_inverse_bound(cov, H, method)
    _assert_inverse_bound(got_ua[:36].reshape(6, 6), H_ua, method + " with_ua")


# ---------------------------------------------------------------- 6. edges
@pytest.mark.parametrize("n_surf,n_corner", [(256, 256), (256, 1), (257, 256), (1, 257), (257, 0), (0, 256)])
def test_tile_edges(mla, case16, feats16, n_surf, n_corner):
    """one tile, exactly 256 and 257 features of one kind (one tile and one more), the other kind at one tile, at one feature and at none"""
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"]); c.map_set(mla.CORNER, case16["corner_map"])
        empty = n_surf == 0 or n_corner == 0
        if n_surf:
            c.features_set(mla.SURF, feats16[0][:n_surf])
        if n_corner:
            c.features_set(mla.CORNER, feats16[1][:n_corner])
        if empty:                                                         # scan2map wants both kinds: refused, and the getter has nothing
            with pytest.raises(mla.MlhError, match=ERR_STATE):
                c.scan2map(case16["p0"], _flagged(mla), want_stats=False)
            with pytest.raises(mla.MlhError, match=ERR_STATE):
                c.scan2map_cov()
            return
        pose0, want, _ = _solve(c, case16["p0"], _flagged(mla))
        plain, _ = c.scan2map(case16["p0"], want_stats=False)
        assert np.array_equal(_bits(pose0), _bits(plain))
        for mode in ("00", "10"):
            pose, got, _ = _with_env(_lm_env(mode), lambda: _solve(c, case16["p0"], _flagged(mla)))
            assert np.array_equal(_bits(pose), _bits(pose0)) and np.array_equal(_bits(got), _bits(want)), mode
        H = want[36:].reshape(6, 6)
        assert np.isfinite(want).all() and H[0, 0] > 0                    # every one of these cuts constrains all six directions: finite H, finite inverse
        assert np.linalg.cond(H, 2) < 1e6
        _assert_inverse_bound(want[:36].reshape(6, 6), H, f"{n_surf}+{n_corner} features")
    finally:
        c.close()


def test_a_loop_that_ends_in_its_begin_publishes_the_begin_record(mla, case16, feats16):
    """no feature finds a plane or a line (the frame is 500 m off the map): the loop terminates in its begin on a zero gradient (termination 1), and H is the begin
    record -- the last statistics record's H of the same call with statistics, here all zeros. Its inverse is what IEEE division makes of a zero pivot; the call
    succeeds. (The issue's "too few blocks", termination 4, cannot be reached through scan2map: its launches pass lm_min_blocks = 0.) So that zeros can only come
    from THIS frame's begin record, every form first solves the ordinary frame on the same context: the records that solve leaves in the solver state, in the
    consumer-side state pair and wherever else a form could pick one up from are non-zero, and a publication that inverted one of them would show it."""
    far_s, far_c = feats16[0][:300].copy(), feats16[1][:300].copy()
    far_s[:, :3] += 500.0; far_c[:, :3] += 500.0
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"]); c.map_set(mla.CORNER, case16["corner_map"])

        def after_an_ordinary_frame(call):
            c.features_set(mla.SURF, feats16[0]); c.features_set(mla.CORNER, feats16[1])
            _, d72, _ = call()
            assert np.isfinite(d72).all() and d72[36] > 1.0                # (a non-zero record is what the forms leave behind)
            c.features_set(mla.SURF, far_s); c.features_set(mla.CORNER, far_c)
            return call()
        outs = [after_an_ordinary_frame(lambda: _solve(c, case16["p0"], _flagged(mla), want_stats=True))]
        for mode in (None, "00", "10", "11b"):
            outs.append(_with_env(_lm_env(mode) if mode else None, lambda: after_an_ordinary_frame(lambda: _solve(c, case16["p0"], _flagged(mla)))))
    finally:
        c.close()
    st = outs[0][2]
    assert st[-1]["n_surf"] + st[-1]["n_corner"] == 0 and st[-1]["lm_iterations"] == 0 and st[-1]["termination"] == 1
    for pose, d72, _ in outs:
        assert np.array_equal(pose, case16["p0"])
        assert np.array_equal(d72[36:].reshape(6, 6), np.asarray(st[-1]["H"]).reshape(6, 6))
        assert not np.isfinite(d72[:36]).any()
        assert np.array_equal(np.isnan(d72[:36]), np.isnan(outs[0][1][:36]))


def test_a_map_below_the_minimum_gives_zero_matrices(mla, case16, feats16):
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"][:40]); c.map_set(mla.CORNER, case16["corner_map"])
        c.features_set(mla.SURF, feats16[0]); c.features_set(mla.CORNER, feats16[1])
        pose, d72, _ = _solve(c, case16["p0"], _flagged(mla))
        assert np.array_equal(pose, case16["p0"]) and not d72.any()
        c.scan2map_begin(case16["p0"], _flagged(mla))
        pose, status = c.scan2map_end()
        cov, H = c.scan2map_cov()
        assert status == 0 and np.array_equal(pose, case16["p0"]) and not cov.any() and not H.any()
    finally:
        c.close()


def test_a_degenerate_single_plane_scene(mla, orc):
    """a map that is ONE plane (and one short line): evalDegenracy flags the frame; H_final and the pose are the checker's, the covariance only has to come back"""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(-12, 12, 0.4), np.arange(-12, 12, 0.4)), -1).reshape(-1, 2)
    plane = np.concatenate([g + rng.uniform(-0.05, 0.05, g.shape), rng.normal(0, 0.005, (len(g), 1))], 1).astype(np.float32)
    line = np.stack([np.full(200, 3.0), np.full(200, 2.0), np.linspace(0, 4, 200)], 1).astype(np.float32) + rng.normal(0, 0.003, (200, 3)).astype(np.float32)
    feats_s = np.concatenate([rng.uniform(-8, 8, (3000, 2)), np.zeros((3000, 2))], 1).astype(np.float32)
    feats_c = np.concatenate([line[::4] + np.float32(0.01), np.zeros((50, 1), np.float32)], 1)
    p0 = np.array([0.0, 0.0, 0.08, 0.004, -0.003, 0.0, 1.0]); p0[3:] /= np.linalg.norm(p0[3:])
    case = dict(surf_map=plane, corner_map=line, p0=p0)
    c = mla.Context(0)
    try:
        _stage(c, mla, case, feats_s, feats_c)
        pose, d72, st = _solve(c, p0, _flagged(mla), want_stats=True)
        pose_l, d72_l, _ = _solve(c, p0, _flagged(mla))
    finally:
        c.close()
    assert any(s["is_degenerate"] for s in st)
    assert np.array_equal(_bits(pose), _bits(pose_l)) and np.array_equal(_bits(d72[36:]), _bits(d72_l[36:]))
    res = orc.scan2map(orc.Map(plane), orc.Map(line), feats_s, feats_c, p0, orc.mapper_params())
    assert any(o["is_degenerate"] for o in res["outer"])
    Href = _oracle_H(orc, case, feats_s, feats_c, (np.full(len(feats_s), 0.0075), np.full(len(feats_c), 0.0075)), res)
    H = d72[36:].reshape(6, 6)
    err = float(np.abs(H - Href).max() / np.abs(Href).max())
    print(f"degenerate scene: |H - H_checker|max / |H|max = {err:.3e}, cond2(H) = {np.linalg.cond(H, 2):.3e}")
    assert err <= 1e-9, err
    assert np.linalg.norm(pose[:3] - res["pose"][:3]) < 1e-7 and np.linalg.norm(pose[3:] - res["pose"][3:]) < 1e-7


# ---------------------------------------------------------------- 7. the getter's state, refusals
def test_getter_state_rules(mla, case16, feats16):
    c = mla.Context(0)
    try:
        with pytest.raises(mla.MlhError, match=ERR_STATE):                # nothing collected yet
            c.scan2map_cov()
        _stage(c, mla, case16, feats16[0], feats16[1])
        with pytest.raises(mla.MlhError, match=ERR_STATE):
            c.scan2map_cov()
        c.scan2map(case16["p0"], want_stats=False)                        # an unflagged solve
        with pytest.raises(mla.MlhError, match=ERR_STATE + ".*MLH_FLAG_POSE_COV"):
            c.scan2map_cov()
        _, d72, _ = _solve(c, case16["p0"], _flagged(mla))                # a flagged one
        assert np.isfinite(d72).all()
        # the flag means nothing to the Gauss-Newton solves: same pose, and the scan2map solve's matrices stay the collected ones
        a, _ = c.gn_solve(case16["p0"], 3, want_stats=False)
        b, _ = c.gn_solve(case16["p0"], 3, _flagged(mla), want_stats=False)
        assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(np.concatenate([x.ravel() for x in c.scan2map_cov()])), _bits(d72))
        c.scan2map_begin(case16["p0"])                                    # a further unflagged solve, split this time
        assert c.scan2map_end()[1] == 0
        with pytest.raises(mla.MlhError, match=ERR_STATE):
            c.scan2map_cov()
    finally:
        c.close()


def test_refused_under_a_mailbox_communicator(mla, case16, feats16):
    c = mla.Context(0)
    try:
        c.profile_enable(); c.profile_sample(1)
        _stage(c, mla, case16, feats16[0], feats16[1])
        c.p2p_comm_init(1, 0, [c.p2p_mailbox()])
        c.profile_reset()
        with pytest.raises(mla.MlhError, match=ERR_UNSUPPORTED):
            c.scan2map(case16["p0"], _flagged(mla), want_stats=False)
        with pytest.raises(mla.MlhError, match=ERR_UNSUPPORTED):
            c.scan2map_begin(case16["p0"], _flagged(mla))
        assert [int(c.profile_get(getattr(mla, "K_" + k))[1]) for k in KERNELS] == [0] * len(KERNELS)      # nothing was enqueued
    finally:
        c.close()


# ---------------------------------------------------------------- 8. no launch is added
def test_the_flag_adds_no_launch(mla, orc, synth, case16, feats16):
    ids = [getattr(mla, "K_" + k) for k in KERNELS]

    def counted(c, call):
        c.profile_reset()
        loops = c.info()["loop_launches"]
        call()
        return [int(c.profile_get(k)[1]) for k in ids], c.info()["loop_launches"] - loops

    def split(c, o):
        c.scan2map_begin(case16["p0"], o)
        assert c.scan2map_end()[1] == 0

    c = mla.Context(0)
    try:
        c.profile_enable(); c.profile_sample(1)
        _stage(c, mla, case16, feats16[0], feats16[1])
        for o_plain, o_flag in ((mla.default_opts(), _flagged(mla)),):
            assert counted(c, lambda: c.scan2map(case16["p0"], o_plain, want_stats=False)) == counted(c, lambda: c.scan2map(case16["p0"], o_flag, want_stats=False))
            assert counted(c, lambda: split(c, o_plain)) == counted(c, lambda: split(c, o_flag))
        # the fused thinning + solve call, on the device-resident fused clouds
        scans = case16["scans"] * 2
        ext = np.array([np.concatenate([r[4:7], r[:4]]) for r in synth.HERCULES_BODY_T_LASER])[:2]
        for e in ext:
            e[3:] /= np.linalg.norm(e[3:])
        covs = np.stack([np.zeros((6, 6)), np.diag([0.0025] * 3 + [0.00030461] * 3)])
        meas = np.diag([0.0025] * 3)
        c.fuse_reset()
        for i, s in enumerate(scans):
            c.scan_upload(s.points, s.scan_start, s.scan_end); c.extract_run()
            c.extract_fetch(); c.extract_voxel(0.2)
            c.fuse_add_scan(i, ext[i])
        run = lambda o: c.downsample_scan2map(c.fused_cloud(mla.SURF), c.fused_cloud(mla.CORNER), 0.4, 0.2, ext, covs, meas, case16["p0"], o)
        plain = counted(c, lambda: run(mla.default_opts(flags=mla.FLAG_WITH_UA)))
        flag = counted(c, lambda: run(_flagged(mla, flags=mla.FLAG_WITH_UA)))
        assert plain == flag and plain[1] == 1
    finally:
        c.close()


# ---------------------------------------------------------------- the façade: the covariance reaches the keyframe store
def test_pipelined_mapper_stores_the_covariance_with_its_keyframes():
    """m-loam_amd/host/posecov_selftest: 12 frames through PipelinedMapper over a KeyframeMap, with_ua on, every frame a keyframe -- the covariance stored with a
    keyframe is zero while the mapper holds at most 10 keyframes (cpp:607-608), then mlh_scan2map_cov's bits for that frame; with_ua off: zero throughout"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "posecov_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/posecov_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "with_ua 1: 12 keyframes, 11 stored with a zero covariance, 1 with mlh_scan2map_cov's bits" in r.stdout
    assert "with_ua 0: 12 keyframes, 12 stored with a zero covariance, 0 with" in r.stdout
    assert "posecov selftest: pass" in r.stdout
