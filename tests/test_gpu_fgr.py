"""FPFH + Fast Global Registration on the device (m-loam_amd/csrc/fgr.hip; mlh_fgr_*) against the C++ restatement of performGlobalRegistration
(tests/host/fgr_ref.cpp through tests/fgr_cases.py), which tests/test_fgr_cases.py holds on the CPU. Everything goes through the C-ABI; every stage is compared
on the device's own output of the stage before it (mlh_fgr_fetch), so that one stage's rounding does not leak into the next one's comparison.

Bounds: normals within 8 x the measured f32-against-f64 angle of the restatement (tests/golden/fgr_tolerances.json), NaN patterns equal; SPFH counts bit-equal at
every unflagged point and within 2 x the point's fragile pair features elsewhere, neighbour counts equal; FPFH within 2 k 2^-24 100 per bin (the reordering bound
of a k-term f32 sum after the scale to 100); pairs identical; the registration within 1e-6 of the restatement's tail on the device's pairs, and within 2 x the
restatement's own end-to-end error of the transform that made the scene.

Observed on an MI355X: normals at most 6.3e-5 rad from the restatement (bound 4.8e-4); no SPFH count differs on any cloud, flagged points included; FPFH at most
0.12 of its bound; the registration 2.4e-7 from the restatement's tail on the device's 500 pairs and 4.65e-7 from the truth (bound 9.06e-7)."""
import numpy as np
import pytest

import fgr_cases as fc

pytestmark = pytest.mark.gpu

MODEL, DATA = 0, 2                      # MLH_LOOP_MODEL_SURF, MLH_LOOP_DATA_SURF
EMPTY = np.zeros((0, 4), np.float32)
CLOUDS = ["room_a", "room_b", "one_cell", "tiny_0", "tiny_1", "tiny_2", "tiny_3"]
U24 = 2.0 ** -24


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stage(ctx, cloud, which=MODEL):
    clouds4 = [EMPTY, EMPTY, EMPTY, EMPTY]
    clouds4[which] = cloud
    ctx.loop_set_clouds(*clouds4)


@pytest.mark.parametrize("name", CLOUDS)
def test_normals_spfh_fpfh_stage_by_stage(mla, ctx, name):
    """mlh_fgr_features on one cloud, as the model and (room_b) as the data cloud; each stage against the restatement run on the device's output of the stage before"""
    cloud = fc.clouds()[name]
    which = DATA if name == "room_b" else MODEL
    n = len(cloud)
    _stage(ctx, cloud, which)
    ctx.fgr_features(which)
    info = ctx.fgr_info()
    assert info["n"][which >> 1] == n and info["have_features"][which >> 1]
    got_n = ctx.fgr_fetch(which, mla.FGR_NORMALS)
    got_c, got_k = ctx.fgr_fetch(which, mla.FGR_SPFH)
    got_f = ctx.fgr_fetch(which, mla.FGR_FPFH)
    assert got_n.shape == (n, 4) and got_c.shape == (n, 33) and got_f.shape == (n, 33)
    if n == 0:
        return
    tol = fc.tolerances()
    # 1. normals
    want = fc.normals(cloud)
    flagged = want["flagged"]
    if n >= 90:
        assert flagged.sum() <= 0.10 * n, (name, int(flagged.sum()))
    ok = ~flagged
    nan_w, nan_g = np.isnan(want["normals"][:, 0]), np.isnan(got_n[:, 0])
    assert np.array_equal(nan_w[ok], nan_g[ok]), name
    assert np.array_equal(np.isnan(got_n).all(1), np.isnan(got_n).any(1))
    fin = ok & ~nan_w
    if fin.any():
        ang = fc.angle_between(got_n[fin, :3], want["normals"][fin, :3])
        sign = np.sum(got_n[fin, :3].astype(np.float64) * want["normals"][fin, :3], 1)
        dcurv = float(np.abs(got_n[fin, 3].astype(np.float64) - want["normals"][fin, 3]).max())
        print(f"{name}: normals max angle {ang.max():.3e} rad (bound {tol['normal_angle_bound_rad']:.3e}), curvature max diff {dcurv:.3e}")
        assert ang.max() <= tol["normal_angle_bound_rad"], (name, float(ang.max()))
        assert (sign > 0).all(), name                                   # flipped towards the origin the same way
        assert (np.abs(np.linalg.norm(got_n[fin, :3].astype(np.float64), axis=1) - 1.0) < 1e-5).all()
    # 2. SPFH on the device's normals
    ws = fc.spfh(cloud, got_n)
    frag = ws["fragile"]
    if n >= 90:
        assert (frag > 0).sum() <= 0.10 * n, (name, int((frag > 0).sum()))
    assert np.array_equal(got_k, ws["k"]), name
    l1 = np.abs(got_c.astype(np.int64) - ws["counts"]).sum(1)
    print(f"{name}: SPFH points differing {int((l1 > 0).sum())} of {n} (fragile points {int((frag > 0).sum())}), largest L1 {int(l1.max())}")
    assert (l1[frag == 0] == 0).all(), (name, np.nonzero((l1 > 0) & (frag == 0))[0][:8].tolist())
    assert (l1 <= 2 * frag).all(), name
    # 3. FPFH on the device's counts
    wf = fc.fpfh(cloud, got_c, got_k)
    bound = 2.0 * got_k.astype(np.float64) * U24 * 100.0
    diff = np.abs(got_f.astype(np.float64) - wf)
    print(f"{name}: FPFH largest |diff| / bound {float((diff / bound[:, None]).max()):.3f}")
    assert np.isfinite(got_f).all() and (diff <= bound[:, None]).all(), name
    for blk in range(3):
        s = got_f[:, 11 * blk:11 * blk + 11].astype(np.float64).sum(1)
        nz = s != 0.0
        assert (np.abs(s[nz] - 100.0) <= bound[nz] + 11 * 100.0 * U24).all(), (name, blk)      # (+ the 11 roundings of this check's own f64 sum of f32 values)


def test_stage_overrides_run_the_next_stage_on_known_inputs(mla, ctx):
    """mlh_fgr_set_normals -> mlh_fgr_spfh and mlh_fgr_set_spfh -> mlh_fgr_fpfh on the restatement's own outputs: the counts (normals with a NaN row included: a
    NaN feature counts in bin 0) and the features of exactly those inputs"""
    cloud = fc.clouds()["room_a"]
    nm = fc.normals(cloud)["normals"].copy()
    nm[5] = np.nan
    _stage(ctx, cloud)
    ctx.fgr_set_normals(MODEL, nm)
    ctx.fgr_features(MODEL, first=mla.FGR_SPFH)
    got_c, got_k = ctx.fgr_fetch(MODEL, mla.FGR_SPFH)
    ws = fc.spfh(cloud, nm)
    l1 = np.abs(got_c.astype(np.int64) - ws["counts"]).sum(1)
    assert np.array_equal(got_k, ws["k"]) and (l1[ws["fragile"] == 0] == 0).all() and (l1 <= 2 * ws["fragile"]).all()
    assert got_c[5, 0] == got_c[5, 11] == got_c[5, 22] == got_k[5] - 1             # every pair of the NaN point lands in bin 0
    assert np.isfinite(ctx.fgr_fetch(MODEL, mla.FGR_FPFH)).all()
    ctx.fgr_set_spfh(MODEL, ws["counts"], ws["k"])
    ctx.fgr_features(MODEL, first=mla.FGR_FPFH)
    got_f = ctx.fgr_fetch(MODEL, mla.FGR_FPFH)
    wf = fc.fpfh(cloud, ws["counts"], ws["k"])
    assert (np.abs(got_f.astype(np.float64) - wf) <= 2.0 * ws["k"][:, None] * U24 * 100.0).all()


def _match_case(ctx, f0, f1):
    ctx.loop_set_clouds(EMPTY, EMPTY, EMPTY, EMPTY)
    ctx.fgr_set_features(MODEL, f0)
    ctx.fgr_set_features(DATA, f1)
    got = ctx.fgr_match()
    want, _ = fc.match(f0, f1)
    assert np.array_equal(got, want), (got.shape, want.shape)
    return got


def test_match_is_the_restatements_pairs_in_its_order(mla, ctx):
    """random 33-vectors at 257 x 130 (the dataset split over several workgroups, no multiple of the tile), duplicated rows (the tie goes to the lower index), NaN and
    infinite rows (match nothing), the swapped case (the second cloud larger) and one empty side"""
    rng = np.random.default_rng(9)
    f0 = rng.uniform(0, 30, (257, 33)).astype(np.float32)
    f1 = (f0[rng.permutation(257)[:130]] + rng.normal(0, 2.0, (130, 33))).astype(np.float32)
    got = _match_case(ctx, f0, f1)
    assert 20 < len(got) <= 130 and (np.diff(got[:, 0]) > 0).all()
    # duplicated rows on both sides, NaN / inf rows
    g0, g1 = f0.copy(), f1.copy()
    g0[200] = g0[17]; g0[201] = g0[17]
    g1[100] = g1[3]
    g1[50] = g0[17]                                                     # three equal candidates in cloud 0 for row 50: the lowest, 17, takes it
    g0[30, 7] = np.nan; g1[60, 32] = np.inf; g0[31] = np.nan
    got = _match_case(ctx, g0, g1)
    assert [17, 50] in got.tolist() and not {30, 31} & set(got[:, 0].tolist()) and 60 not in got[:, 1].tolist()
    assert 200 not in got[:, 0].tolist() and 201 not in got[:, 0].tolist()
    # swapped: pairs stay (model, data), ascending in the LARGER cloud's index -- the data cloud's
    got = _match_case(ctx, f1, f0)
    assert (np.diff(got[:, 1]) > 0).all() and not (np.diff(got[:, 0]) > 0).all()
    # one empty side, both empty
    assert len(_match_case(ctx, f0, np.zeros((0, 33), np.float32))) == 0
    assert len(_match_case(ctx, np.zeros((0, 33), np.float32), f1)) == 0
    assert len(_match_case(ctx, np.zeros((0, 33), np.float32), np.zeros((0, 33), np.float32))) == 0


def test_register_end_to_end(mla, ctx):
    """the 500-point model and its copy moved by yaw 0.3 rad and 1.5 m"""
    s = fc.scene()
    tol = fc.tolerances()
    ctx.loop_set_clouds(s["model"], EMPTY, s["data"], EMPTY)
    got = ctx.fgr_register()
    a0 = ctx.fgr_info()["allocations"]
    pairs = ctx.fgr_match()
    assert got["n_mutual"] == len(pairs) and not got["swapped"]
    # the device's pairs through the restatement's tail (its own NormalizePoints, the shared tuple test / OptimizePairwise / GetOutputTrans)
    want = fc.tail(s["model"], s["data"], pairs, False)
    dT = float(np.abs(got["T_relative"] - want["T_relative"]).max())
    dc = abs(got["final_cost_normalize"] - want["final_cost_normalize"])
    err = float(np.abs(got["T_relative"] - s["truth"]).max())
    print(f"register: {len(pairs)} mutual pairs, |T - tail(T)| {dT:.2e}, |cost - tail(cost)| {dc:.2e}, |T - truth| {err:.2e} (bound {tol['register_T_bound']:.2e}), "
          f"cost {got['final_cost_normalize']:.3e}, host waits {got['host_waits']}")
    assert (got["n_tuples"], got["n_corres"], got["n_trials"]) == (want["n_tuples"], want["n_corres"], want["n_trials"])
    assert dT <= 1e-6 and dc <= 1e-6
    assert err <= tol["register_T_bound"], err
    ref = fc.scene_reference()
    assert got["accepted"] == want["accepted"] == ref["accepted"] == True
    # a second run: the same bits, the features reused (one wait), nothing allocated
    again = ctx.fgr_register()
    assert np.array_equal(again["T_relative"].view(np.uint64), got["T_relative"].view(np.uint64)) and again["final_cost_normalize"] == got["final_cost_normalize"]
    assert again["host_waits"] == 1
    assert ctx.fgr_info()["allocations"] == a0
    # ... and from scratch in a new context: the same bits again (every sum has one order)
    c2 = mla.Context(0)
    try:
        c2.loop_set_clouds(s["model"], EMPTY, s["data"], EMPTY)
        fresh = c2.fgr_register()
        assert np.array_equal(fresh["T_relative"].view(np.uint64), got["T_relative"].view(np.uint64))
        assert np.array_equal(_bits(c2.fgr_fetch(DATA, mla.FGR_FPFH)), _bits(ctx.fgr_fetch(DATA, mla.FGR_FPFH)))
    finally:
        c2.close()
    # fewer than 10 correspondences: T = GetOutputTrans of the identity, the cost NaN, not accepted
    few = ctx.fgr_register(mla.fgr_opts(tuple_scale=1.0))                # li < lj < li: no tuple passes
    assert few["n_corres"] == 0 and not few["accepted"] and np.isnan(few["final_cost_normalize"])
    assert np.array_equal(few["T_relative"][:3, :3], np.eye(3))
    np.testing.assert_allclose(few["T_relative"][:3, 3], few["means"][0] - few["means"][1], rtol=0, atol=1e-6)


def test_errors(mla, ctx):
    """options out of range (every call validates them), a stage fetched before it is computed, a wrong cloud, a call under a communicator"""
    cloud = fc.clouds()["one_cell"]
    _stage(ctx, cloud)
    bad = [dict(normal_radius=0.0), dict(fpfh_radius=float("nan")), dict(div_factor=1.0), dict(use_absolute_scale=2), dict(max_corr_dist=-1.0), dict(iteration_number=-1),
           dict(tuple_scale=0.0), dict(tuple_scale=1.5), dict(tuple_max_cnt=0), dict(global_registration_threshold=float("nan")), dict(normal_radius=float("inf"))]
    for kw in bad:
        for call in (lambda o: ctx.fgr_features(MODEL, o), lambda o: ctx.fgr_match(o), lambda o: ctx.fgr_register(o)):
            with pytest.raises(mla.MlhError, match="bad"):
                call(mla.fgr_opts(**kw))
    for what in (mla.FGR_NORMALS, mla.FGR_SPFH, mla.FGR_FPFH):
        with pytest.raises(mla.MlhError, match="not been computed"):
            ctx.fgr_fetch(MODEL, what)
    with pytest.raises(mla.MlhError, match="no normals"):
        ctx.fgr_features(MODEL, first=mla.FGR_SPFH)
    with pytest.raises(mla.MlhError, match="no features"):
        ctx.fgr_match()
    with pytest.raises(mla.MlhError, match="which"):
        ctx.fgr_features(1)
    with pytest.raises(mla.MlhError, match="size"):
        ctx.fgr_set_normals(MODEL, np.zeros((5, 4), np.float32))
    ctx.fgr_features(MODEL)
    ctx.fgr_fetch(MODEL, mla.FGR_FPFH)
    _stage(ctx, fc.clouds()["room_a"])                                  # new clouds: what was computed is stale
    with pytest.raises(mla.MlhError, match="not been computed"):
        ctx.fgr_fetch(MODEL, mla.FGR_FPFH)
    # under a communicator (one rank is enough to make the context a distributed one)
    c2 = mla.Context(0)
    try:
        c2.p2p_comm_init(1, 0, [c2.p2p_mailbox()])
        for call in (lambda: c2.fgr_features(MODEL), lambda: c2.fgr_match(), lambda: c2.fgr_register()):
            with pytest.raises(mla.MlhError, match="communicator"):
                call()
    finally:
        c2.close()
