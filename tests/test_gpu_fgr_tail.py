"""The tail of Fast Global Registration on the device (m-loam_amd/csrc/fgr.hip: fgr_tuple_count_kernel / _scan_kernel / _emit_kernel, fgr_optimize_kernel;
mlh_fgr_register_device, mlh_fgr_tail_tuple_test, mlh_fgr_tail_optimize) against the CPU restatement's sequential tuple test and OptimizePairwise
(tests/fgr_cases.py: fr_tuple_test, fr_optimize) on the cases of tests/fgr_tail_cases.py, and against mlh_fgr_register on the registration scene.

Bounds. The tuple test is integer decisions on correctly rounded f32 sqrt and division without contraction: n_tuples, n_trials and every index EQUAL, no tolerance.
OptimizePairwise: trans within 1e-6 of the restatement (the bar tests/test_gpu_fgr.py holds the registration to), the two costs within 1e-9 relative (the project's
f64 bar); the device adds the 28 f64 sums of an iteration in another order and has its own sin / cos / sqrt, and every iteration rounds delta to f32.

Observed on an MI355X (tests/golden/fgr_tail_tolerances.json; `python tests/test_gpu_fgr_tail.py` measures and rewrites it; test_optimize_against_the_restatement
prints the figures): all 77 tuple-test cases equal; over the 56 OptimizePairwise cases trans is BIT-EQUAL to the restatement's in 56 (largest difference 0), the
costs differ by at most 7.5e-15 relative (n = 6150, 5 iterations, absolute scale) -- the reordering of the f64 sums is absorbed by delta's rounding to f32, as on
the CPU under other summation orders; end to end on the 500-point scene T_relative and both costs come out bit-equal to mlh_fgr_register's."""
import json

import numpy as np
import pytest

import fgr_cases as fc
import fgr_tail_cases as tc

pytestmark = pytest.mark.gpu

MODEL, DATA = 0, 2
EMPTY = np.zeros((0, 4), np.float32)
TRANS_BOUND, COST_RTOL = 1e-6, 1e-9


@pytest.fixture(scope="module")
def mctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- the tuple test
@pytest.mark.parametrize("name", sorted(tc.sets()))
def test_tuple_test_equals_the_sequential_loop(mla, mctx, name):
    """every set, both values of `swapped`, the seeds 1, 7 and 2^63 + 5 (and for n = 325 the caps around its total): n_tuples, n_trials and the whole corres list"""
    ref = tc.tuple_reference()
    ran = 0
    for cid, set_name, sw, cap, seed in tc.tuple_cases():
        if set_name != name:
            continue
        got, trials = mctx.fgr_tail_tuple_test(tc.pq_of(name), sw, mla.fgr_opts(tuple_scale=tc.TUPLE_SCALE, tuple_max_cnt=cap, seed=seed))
        want, want_trials = ref[cid]
        assert len(got) == len(want) and trials == want_trials, (cid, len(got), len(want), trials, want_trials)
        assert np.array_equal(got, want), (cid, int(np.argmax((got != want).any(1))))
        info = mctx.fgr_info()
        assert info["host_waits"] == 1 and info["launches"] == (3 if len(tc.pq_of(name)) else 1), (cid, info)
        ran += 1
    assert ran >= 6
    print(f"{name}: {ran} cases equal")


# ---------------------------------------------------------------- OptimizePairwise
def _optimize_measure(mla, c):
    """id -> (max |trans diff|, cost relative diff, trans bit-equal)"""
    ref = tc.optimize_reference()
    out = {}
    for cid, n, it, ab, ss in tc.optimize_cases():
        trans, cost, ran = c.fgr_tail_optimize(tc.optimize_records(n, ab), ss, mla.fgr_opts(iteration_number=it, use_absolute_scale=ab))
        w_trans, w_cost, w_ran = ref[cid]
        assert ran == w_ran == (n >= 10), cid
        dt = float(np.abs(trans.reshape(16).astype(np.float64) - w_trans).max())
        if ran and it > 0:
            assert np.isfinite(cost).all() and np.isfinite(w_cost).all(), cid
            dc = float(np.max(np.abs(np.array(cost) - w_cost) / np.abs(w_cost)))
        else:
            assert np.isnan(cost).all() and np.isnan(w_cost).all(), cid
            dc = 0.0
        if not ran or it == 0:
            assert np.array_equal(trans, np.eye(4, dtype=np.float32)), cid
        out[cid] = (dt, dc, bool(np.array_equal(trans.reshape(16).view(np.uint32), w_trans.view(np.uint32))))
    return out


def test_optimize_against_the_restatement(mla, mctx):
    """n_corres 9 (not run), 10, 12, the register-resident limit - 1, + 0, + 1 and twice the limit + 6; iteration_number 0, 1, 5, 64; use_absolute_scale 0 / 1
    through start_scale: trans within 1e-6, costs within 1e-9 relative"""
    m = _optimize_measure(mla, mctx)
    assert len(m) == 56
    worst_t, worst_c = max(m.items(), key=lambda kv: kv[1][0]), max(m.items(), key=lambda kv: kv[1][1])
    equal = sum(1 for v in m.values() if v[2])
    print(f"optimize: max |trans - restatement| {worst_t[1][0]:.3e} ({worst_t[0]}), max relative cost difference {worst_c[1][1]:.3e} ({worst_c[0]}), "
          f"trans bit-equal in {equal} of {len(m)} cases")
    for cid, (dt, dc, _) in m.items():
        assert dt <= TRANS_BOUND, (cid, dt)
        assert dc <= COST_RTOL, (cid, dc)
    rec = json.load(open(tc.TOL_PATH))
    assert rec["trans_bound"] == TRANS_BOUND and rec["cost_rtol"] == COST_RTOL


# ---------------------------------------------------------------- end to end
def _same_counts(a, b):
    return all(a[k] == b[k] for k in ("n_mutual", "n_tuples", "n_corres", "n_trials", "swapped", "accepted"))


def test_register_device_end_to_end(mla, ctx):
    """mlh_fgr_register_device against mlh_fgr_register on the same context, the 500-point scene"""
    s = fc.scene()
    tol = fc.tolerances()
    ctx.loop_set_clouds(s["model"], EMPTY, s["data"], EMPTY)
    host = ctx.fgr_register()
    dev = ctx.fgr_register_device()
    a0 = ctx.fgr_info()["allocations"]
    assert _same_counts(dev, host), ({k: dev[k] for k in ("n_mutual", "n_tuples", "n_corres", "n_trials")}, {k: host[k] for k in ("n_mutual", "n_tuples", "n_corres", "n_trials")})
    assert dev["accepted"] and dev["n_tuples"] > 0
    assert np.array_equal(dev["means"], host["means"]) and dev["global_scale"] == host["global_scale"] and dev["start_scale"] == host["start_scale"]
    dT = float(np.abs(dev["T_relative"] - host["T_relative"]).max())
    err = float(np.abs(dev["T_relative"] - s["truth"]).max())
    dc = abs(dev["final_cost_normalize"] - host["final_cost_normalize"]) / abs(host["final_cost_normalize"])
    print(f"register_device: {dev['n_mutual']} pairs, {dev['n_tuples']} tuples of {dev['n_trials']} trials, |T - host tail's T| {dT:.2e}, relative cost difference {dc:.2e}, "
          f"|T - truth| {err:.2e} (bound {tol['register_T_bound']:.2e}), host waits {dev['host_waits']}")
    assert dT <= 1e-6 and dc <= COST_RTOL
    assert err <= tol["register_T_bound"], err
    assert dev["host_waits"] == 1                                        # the features were computed by the first call
    info = ctx.fgr_info()
    assert info["host_waits"] == 1 and info["launches"] >= 2 + 3 + 4
    # a second run: the same bits, nothing allocated
    again = ctx.fgr_register_device()
    assert np.array_equal(_bits64(again["T_relative"]), _bits64(dev["T_relative"])) and again["final_cost"] == dev["final_cost"] and again["host_waits"] == 1
    assert ctx.fgr_info()["allocations"] == a0
    # the host tail afterwards: the bits it had before
    host2 = ctx.fgr_register()
    assert np.array_equal(_bits64(host2["T_relative"]), _bits64(host["T_relative"])) and host2["final_cost"] == host["final_cost"] and _same_counts(host2, host)
    # a fresh context, the device tail alone
    c2 = mla.Context(0)
    try:
        c2.loop_set_clouds(s["model"], EMPTY, s["data"], EMPTY)
        fresh = c2.fgr_register_device()
        assert np.array_equal(_bits64(fresh["T_relative"]), _bits64(dev["T_relative"])) and fresh["final_cost"] == dev["final_cost"] and _same_counts(fresh, dev)
        assert fresh["host_waits"] == 3                                  # two index builds and the record
    finally:
        c2.close()
    # no tuple passes: T = GetOutputTrans of the identity, NaN cost, not accepted
    few = ctx.fgr_register_device(mla.fgr_opts(tuple_scale=1.0))
    few_host = ctx.fgr_register(mla.fgr_opts(tuple_scale=1.0))
    assert few["n_corres"] == 0 and few["n_tuples"] == 0 and not few["accepted"] and np.isnan(few["final_cost_normalize"]) and np.isnan(few["final_cost"])
    assert few["n_trials"] == few_host["n_trials"] == 100 * few["n_mutual"]
    assert np.array_equal(_bits64(few["T_relative"]), _bits64(few_host["T_relative"]))
    assert np.array_equal(few["T_relative"][:3, :3], np.eye(3))
    # an empty data cloud: no pairs, no trial, the identity
    ctx.loop_set_clouds(s["model"], EMPTY, EMPTY, EMPTY)
    none, none_host = ctx.fgr_register_device(), ctx.fgr_register()
    assert none["n_mutual"] == none["n_trials"] == none["n_corres"] == 0 and not none["accepted"]
    assert np.array_equal(_bits64(none["T_relative"]), _bits64(none_host["T_relative"]))


def test_interleaving_keeps_the_host_tails_bits(mla, ctx):
    """after any device-tail call -- the two test entries overwrite the pair buffer -- mlh_fgr_register returns the bits it returned before"""
    s = fc.scene()
    ctx.loop_set_clouds(s["model"], EMPTY, s["data"], EMPTY)
    host = ctx.fgr_register()
    ctx.fgr_tail_tuple_test(tc.pq_of("n325_w80"))
    ctx.fgr_tail_optimize(tc.optimize_records(12, 0))
    dev = ctx.fgr_register_device()
    ctx.fgr_tail_optimize(tc.optimize_records(tc.plan_constants()["opt_reg_max"] + 1, 0))
    host2 = ctx.fgr_register()
    assert np.array_equal(_bits64(host2["T_relative"]), _bits64(host["T_relative"])) and host2["final_cost"] == host["final_cost"] and _same_counts(host2, host)
    assert np.array_equal(_bits64(ctx.fgr_register_device()["T_relative"]), _bits64(dev["T_relative"]))


def test_errors(mla, ctx, case16, feats16):
    """bad options on all three entries, NULL outputs, a capacity that cannot hold the call's tuples, the communicator, an uncollected solve; a refused call changes nothing"""
    import ctypes as C
    pq = tc.pq_of("n12")
    ctx.loop_set_clouds(fc.clouds()["one_cell"], EMPTY, EMPTY, EMPTY)
    got, trials = ctx.fgr_tail_tuple_test(pq)
    info = ctx.fgr_info()
    bad = [dict(normal_radius=0.0), dict(fpfh_radius=float("nan")), dict(div_factor=1.0), dict(use_absolute_scale=2), dict(max_corr_dist=-1.0), dict(iteration_number=-1),
           dict(tuple_scale=0.0), dict(tuple_scale=1.5), dict(tuple_max_cnt=0), dict(global_registration_threshold=float("nan"))]
    for kw in bad:
        for call in (lambda o: ctx.fgr_register_device(o), lambda o: ctx.fgr_tail_tuple_test(pq, 0, o, capacity_tuples=1200), lambda o: ctx.fgr_tail_optimize(pq, 1.0, o)):
            with pytest.raises(mla.MlhError, match="mlh error -1.*bad"):
                call(mla.fgr_opts(**kw))
    lib, h = ctx.lib, ctx.h
    a = np.ascontiguousarray(pq)
    p = a.ctypes.data_as(C.c_void_p)
    out, k, t = np.zeros((1200, 3), np.int32), C.c_int32(0), C.c_int32(0)
    o = mla.fgr_opts()
    trans, cost, ran = np.zeros(16, np.float32), np.zeros(2), C.c_int32(0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    invalid = [lib.mlh_fgr_register_device(h, None, None),
               lib.mlh_fgr_tail_tuple_test(h, p, -1, 0, C.byref(o), vp(out), 1200, C.byref(k), C.byref(t)),
               lib.mlh_fgr_tail_tuple_test(h, None, 12, 0, C.byref(o), vp(out), 1200, C.byref(k), C.byref(t)),
               lib.mlh_fgr_tail_tuple_test(h, p, 12, 2, C.byref(o), vp(out), 1200, C.byref(k), C.byref(t)),
               lib.mlh_fgr_tail_tuple_test(h, p, 12, 0, C.byref(o), None, 1200, C.byref(k), C.byref(t)),
               lib.mlh_fgr_tail_tuple_test(h, p, 12, 0, C.byref(o), vp(out), 1200, None, C.byref(t)),
               lib.mlh_fgr_tail_tuple_test(h, p, 12, 0, C.byref(o), vp(out), 1200, C.byref(k), None),
               lib.mlh_fgr_tail_tuple_test(h, p, 12, 0, C.byref(o), vp(out), 999, C.byref(k), C.byref(t)),      # min(1000, 1200) = 1000 tuples may come
               lib.mlh_fgr_tail_optimize(h, p, -1, 1.0, C.byref(o), vp(trans), vp(cost), C.byref(ran)),
               lib.mlh_fgr_tail_optimize(h, None, 12, 1.0, C.byref(o), vp(trans), vp(cost), C.byref(ran)),
               lib.mlh_fgr_tail_optimize(h, p, 12, 0.0, C.byref(o), vp(trans), vp(cost), C.byref(ran)),
               lib.mlh_fgr_tail_optimize(h, p, 12, float("nan"), C.byref(o), vp(trans), vp(cost), C.byref(ran)),
               lib.mlh_fgr_tail_optimize(h, p, 12, 1.0, C.byref(o), None, vp(cost), C.byref(ran)),
               lib.mlh_fgr_tail_optimize(h, p, 12, 1.0, C.byref(o), vp(trans), None, C.byref(ran)),
               lib.mlh_fgr_tail_optimize(h, p, 12, 1.0, C.byref(o), vp(trans), vp(cost), None)]
    assert invalid == [-1] * len(invalid), invalid
    assert not out.any() and ctx.fgr_info() == info
    # exactly enough room is enough; NULL options are the defaults
    assert lib.mlh_fgr_tail_tuple_test(h, p, 12, 0, None, vp(out), 1000, C.byref(k), C.byref(t)) == 0
    assert k.value == len(got) and t.value == trials and np.array_equal(out[:k.value], got)
    # under a communicator
    c2 = mla.Context(0)
    try:
        c2.p2p_comm_init(1, 0, [c2.p2p_mailbox()])
        for call in (c2.fgr_register_device, lambda: c2.fgr_tail_tuple_test(pq), lambda: c2.fgr_tail_optimize(pq)):
            with pytest.raises(mla.MlhError, match="communicator"):
                call()
    finally:
        c2.close()
    # while a submitted solve is uncollected
    surf, corner = feats16
    ctx.map_set(mla.SURF, case16["surf_map"])
    ctx.map_set(mla.CORNER, case16["corner_map"])
    ctx.features_set(mla.SURF, surf)
    ctx.features_set(mla.CORNER, corner)
    info = ctx.fgr_info()
    ctx.scan2map_begin(case16["p0"])
    for call in (ctx.fgr_register_device, lambda: ctx.fgr_tail_tuple_test(pq), lambda: ctx.fgr_tail_optimize(pq)):
        with pytest.raises(mla.MlhError, match="mlh error -3.*has not been collected"):
            call()
    assert ctx.fgr_info() == info
    ctx.scan2map_end()
    again, trials2 = ctx.fgr_tail_tuple_test(pq)
    assert np.array_equal(again, got) and trials2 == trials


if __name__ == "__main__":
    import importlib
    import sys
    sys.path.insert(0, tc.ROOT)
    mla_ = importlib.import_module("m-loam_amd")
    c_ = mla_.Context(0)
    m_ = _optimize_measure(mla_, c_)
    c_.close()
    rec_ = {"trans_bound": TRANS_BOUND, "cost_rtol": COST_RTOL, "cases": len(m_), "trans_max_abs_diff_measured": max(v[0] for v in m_.values()),
            "cost_max_rel_diff_measured": max(v[1] for v in m_.values()), "trans_bit_equal_cases": sum(1 for v in m_.values() if v[2])}
    with open(tc.TOL_PATH, "w") as f_:
        json.dump(rec_, f_, indent=1, sort_keys=True)
        f_.write("\n")
    print(rec_)
