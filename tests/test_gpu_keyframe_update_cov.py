"""(f18) the pose graph's marginal covariances into the mapper's keyframe store: mlh_keyframes_update_from_pose_graph_cov. A dozen tiny keyframes: the 12 poses
of a crafted pose graph (tests/pg_cases.py) with one loop 10 -> 2, each saved in the store with a random covariance and two clouds of 40 points; the pose graph is
optimised for cur = 10 (first = 2), its marginals computed, and the store updated from it.

Held: both cov_modes against NumPy (the oracle of tests/pg_marg_cases.py at the device's poses, converted with A) within 1e-9 per block, and to the bit against the
store form mlh_pg_marginals hands out; the keys before `first`, the anchor and the drift tail keep their covariance bits; n_changed counts keys whose only change
is the covariance; the next mlh_local_map_assemble rebuilds, and its clouds (point covariances included) equal, bit for bit, those of a store that was given the same
poses and covariances through mlh_keyframes_update_poses; without the opt-in mlh_keyframes_update_from_pose_graph leaves every covariance alone. Every test fails
without the feature: the entry points do not exist."""
import numpy as np
import pytest

import pg_cases as pc
import pg_marg_cases as mc

pytestmark = pytest.mark.gpu

N_KF, CUR, FIRST = 12, 10, 2
BAR = mc.BAR_DEVICE
EXT, EXT_COV = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]]), np.zeros((1, 6, 6))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _code(excinfo):
    return int(str(excinfo.value).split("mlh error ")[1].split(":")[0])


@pytest.fixture(scope="module")
def case():
    g = pc.make_graph(N_KF, [(CUR, FIRST)], seed=71, drift_t=2e-2, drift_r=2e-3)
    rng = np.random.default_rng(72)
    covs = []
    for _ in range(N_KF):
        A = rng.normal(size=(6, 6))
        covs.append(A @ A.T * 2e-5)
    clouds = []
    for _ in range(N_KF):
        s = np.concatenate([rng.uniform(-3, 3, size=(40, 3)), np.zeros((40, 1))], axis=1).astype(np.float32)
        c = np.concatenate([rng.uniform(-3, 3, size=(40, 3)), np.zeros((40, 1))], axis=1).astype(np.float32)
        clouds.append((s, c))
    return dict(g=g, covs=np.array(covs), clouds=clouds)


def _opts(mla):
    return mla.local_map_opts(surrounding_kf_radius=50.0, map_sur_kf_res=0.2, leaf_surf=0.4, leaf_corner=0.2, trace_threshold=1e6, with_ua=True)


def _setup(mla, case):
    """a context with the store (original poses and covariances, the cache filled by one assemble) and the optimised pose graph with valid marginals"""
    ctx = mla.Context(0)
    g = case["g"]
    for k in range(N_KF):
        assert ctx.keyframe_save(g.poses[k], case["covs"][k], *case["clouds"][k]) == k
    assert ctx.local_map_assemble(g.poses[CUR], EXT, EXT_COV, _opts(mla))["rebuilt"]
    g.upload(ctx)
    res = ctx.pg_optimize(CUR)
    assert res["first_index"] == FIRST and res["num_successful_steps"] >= 1
    sto = ctx.pg_marginals(CUR, form=mla.PG_COV_STORE)
    assert sto["ok"] == 1 and sto["n_keyframes"] == CUR - FIRST + 1
    return ctx, sto["cov"]


def _expected_covs(case, blocks, mode_absolute):
    want = case["covs"].copy()
    for k in range(FIRST + 1, CUR + 1):
        want[k] = blocks[k - FIRST] + case["covs"][FIRST] if mode_absolute else blocks[k - FIRST]
    return want


def _maps(ctx):
    return [ctx.local_map_fetch(k, f) for k in range(2) for f in (False, True)]


@pytest.mark.parametrize("mode", ["relative", "absolute"])
def test_both_modes_against_numpy_and_the_host_route(mla, case, mode):
    g = case["g"]
    cov_mode = mla.KF_COV_ABSOLUTE if mode == "absolute" else mla.KF_COV_RELATIVE
    ctx, blocks = _setup(mla, case)
    side = mla.Context(0)
    try:
        pg_poses = ctx.pg_poses()
        assert not (_bits(pg_poses[FIRST + 1:]) == _bits(g.poses[FIRST + 1:])).all(axis=1).any()
        up = ctx.keyframes_update_from_pose_graph_cov(first_index=0, first_key=0, n=CUR + 1, drift_tail=True, cov_mode=cov_mode)
        st = ctx.keyframe_poses()
        # poses: the pose graph's bits on 0 .. cur, the drift on the tail (the pose graph applied it itself: within the pose bar of f15)
        assert (_bits(st["poses"][:CUR + 1]) == _bits(pg_poses[:CUR + 1])).all()
        assert np.abs(st["poses"][CUR + 1:] - pg_poses[CUR + 1:]).max() <= 1e-7
        # keys 3 .. 10 and the tail; `first` itself only if the write-back's normalisation moved a bit of its quaternion; the keys before it never
        moved = (_bits(pg_poses) != _bits(g.poses)).any(axis=1)
        assert not moved[:FIRST].any() and moved[FIRST + 1:].all()
        assert up["n_changed"] == N_KF - FIRST - 1 + int(moved[FIRST])
        # covariances: to the bit what the store form and the rule give; before first, the anchor and the tail keep theirs
        want = _expected_covs(case, blocks, mode == "absolute")
        assert (_bits(st["covs"]) == _bits(want)).all()
        for k in (0, 1, FIRST, N_KF - 1):
            assert (_bits(st["covs"][k]) == _bits(case["covs"][k])).all()
        # against NumPy: the oracle at the device's poses, converted with A
        d = g.copy()
        d.poses = pg_poses
        local = mc.blocks_inv(d, CUR)
        worst = 0.0
        for k in range(FIRST + 1, CUR + 1):
            A = mc.store_A(pg_poses[k][:3])
            ref = A @ local[k - FIRST] @ A.T + (case["covs"][FIRST] if mode == "absolute" else 0.0)
            worst = max(worst, mc.block_rel(st["covs"][k], ref))
        print(f"PG_MEASURED keyframe covariances {mode} {worst:.3e} bar {BAR:.1e}")
        assert worst <= BAR
        # the next assemble rebuilds, and builds what the host route builds
        r = ctx.local_map_assemble(pg_poses[CUR], EXT, EXT_COV, _opts(mla))
        assert r["rebuilt"]
        for k in range(N_KF):
            assert side.keyframe_save(g.poses[k], case["covs"][k], *case["clouds"][k]) == k
        assert side.local_map_assemble(g.poses[CUR], EXT, EXT_COV, _opts(mla))["rebuilt"]
        hu = side.keyframes_update_poses(0, st["poses"], st["covs"])
        assert hu["n_changed"] == up["n_changed"]
        r2 = side.local_map_assemble(pg_poses[CUR], EXT, EXT_COV, _opts(mla))
        assert r2["rebuilt"] and list(r2["kf_ids"]) == list(r["kf_ids"])
        got, ref_maps = _maps(ctx), _maps(side)
        for a, b in zip(got, ref_maps):
            assert a.shape == b.shape and len(a) > 0 and a.tobytes() == b.tobytes()
        assert np.abs(got[0][:, 4:10]).max() > 0
    finally:
        ctx.close()
        side.close()


def test_n_changed_counts_keys_whose_only_change_is_the_covariance(mla, case):
    ctx, blocks = _setup(mla, case)
    try:
        a = ctx.keyframes_update_from_pose_graph_cov(n=CUR + 1, drift_tail=True, cov_mode=mla.KF_COV_RELATIVE)
        assert a["n_changed"] in (N_KF - FIRST - 1, N_KF - FIRST)
        ctx.local_map_assemble(ctx.pg_poses()[CUR], EXT, EXT_COV, _opts(mla))
        same = ctx.keyframes_update_from_pose_graph_cov(n=CUR + 1, drift_tail=True, cov_mode=mla.KF_COV_RELATIVE)
        assert same["n_changed"] == 0 and not ctx.local_map_assemble(ctx.pg_poses()[CUR], EXT, EXT_COV, _opts(mla))["rebuilt"]
        poses0 = ctx.keyframe_poses()["poses"]
        # (without the drift tail: a last key that changed by its covariance alone would, by the rule of (f15), re-apply a drift of new * old^-1 to the tail)
        b = ctx.keyframes_update_from_pose_graph_cov(n=CUR + 1, drift_tail=False, cov_mode=mla.KF_COV_ABSOLUTE)
        st = ctx.keyframe_poses()
        assert b["n_changed"] == CUR - FIRST and (_bits(st["poses"]) == _bits(poses0)).all()       # keys 3 .. 10: only their covariance moved
        assert (_bits(st["covs"]) == _bits(_expected_covs(case, blocks, True))).all()
        assert ctx.local_map_assemble(st["poses"][CUR], EXT, EXT_COV, _opts(mla))["rebuilt"]
    finally:
        ctx.close()


def test_without_the_opt_in_the_covariances_stay(mla, case):
    ctx, _ = _setup(mla, case)
    try:
        up = ctx.keyframes_update_from_pose_graph(first_index=0, first_key=0, n=-1, drift_tail=False)
        st = ctx.keyframe_poses()
        assert up["n_changed"] == int((_bits(ctx.pg_poses()) != _bits(case["g"].poses)).any(axis=1).sum())
        assert (_bits(st["covs"]) == _bits(case["covs"])).all() and (_bits(st["poses"]) == _bits(ctx.pg_poses())).all()
    finally:
        ctx.close()


def test_refused_calls_change_nothing(mla, case):
    """MLH_ERR_STATE without valid marginals (stale after an optimise, a new loop, a reset) and for a range beyond their cur; MLH_ERR_INVALID for an unknown
    cov_mode, for a range outside the store, and in the absolute mode when `first` maps to no key"""
    ctx, _ = _setup(mla, case)
    try:
        before = ctx.keyframe_poses()

        def refused(code, **kw):
            with pytest.raises(mla.MlhError) as e:
                ctx.keyframes_update_from_pose_graph_cov(**kw)
            assert _code(e) == code, str(e.value)
            st = ctx.keyframe_poses()
            assert (_bits(st["poses"]) == _bits(before["poses"])).all() and (_bits(st["covs"]) == _bits(before["covs"])).all()

        refused(-3, n=-1)                                            # reaches keyframe 11, beyond cur = 10
        refused(-1, n=CUR + 1, cov_mode=5)
        refused(-1, first_index=0, first_key=5, n=CUR + 1)           # outside the store
        refused(-1, first_index=4, first_key=0, n=3, cov_mode=mla.KF_COV_ABSOLUTE)       # first = 2 would be key -2
        assert ctx.keyframes_update_from_pose_graph_cov(first_index=4, first_key=4, n=3, cov_mode=mla.KF_COV_RELATIVE)["n_changed"] == 3
        before = ctx.keyframe_poses()
        ctx.pg_optimize(CUR)
        refused(-3, n=CUR + 1)
        assert ctx.pg_marginals(CUR)["ok"] == 1
        ctx.pg_set_loop(9, 3, case["g"].loop_rel[CUR])
        refused(-3, n=CUR + 1)
        assert ctx.pg_marginals(CUR)["ok"] == 1
        ctx.pg_reset()
        refused(-1, n=CUR + 1)                                       # an empty pose graph is refused as (f15) refuses it
    finally:
        ctx.close()


def test_pgcov_selftest():
    """m-loam_amd/host/pgcov_selftest: PoseGraph::computeMarginals / marginalCov, staleness, the default route of KeyframeMap::updateKeyframe unchanged and the
    covariance route through PipelinedMapper::applyLoopInfo (the program's head lists what it checks)"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "pgcov_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/pgcov_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pgcov_selftest: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
