"""Pose-graph marginal covariances on the device (row f18: mlh_pg_marginals, mlh_pg_device_marginals; m-loam_amd/csrc/pgcov.inc) against the float64 oracles of
tests/pg_marg_cases.py, which tests/test_pg_marg_cases.py holds on the CPU: the 6 x 6 diagonal blocks of H^-1 of the undamped problem at the DEVICE's stored poses.

Bars: per block, within 1e-9 of that block's largest entry (the project's bar for linear work; the float64 routes agree among themselves to 1.3e-12 on these
graphs); the store form within 1e-9 of A Sigma A^T of the fetched local form; block `first` exactly zero, every block symmetric to the bit and positive definite;
poses and last poses untouched to the bit; two runs bit-equal. Every test prints what it measured (PG_MEASURED lines) before it asserts;
tests/golden/pg_marginals_tolerances.json records those figures beside the bars.

Every test fails on a library without the entry points (a missing symbol)."""
import json
import os

import numpy as np
import pytest

import pg_cases as pc
import pg_many_cases as pm
import pg_marg_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = mc.BAR_DEVICE
LOCAL_CASES = ("lin1", "lin4", "lin5", "lin69", "L0", "L1", "L3", "L24", "M130", "A", "C", "D")


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    c.pg_reserve(pm.LOOPS_LIMIT)
    yield c
    c.close()


def _measured(name, value, bar):
    print(f"PG_MEASURED {name} {value:.3e} bar {bar:.1e}")


def _code(excinfo):
    return int(str(excinfo.value).split("mlh error ")[1].split(":")[0])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _loops(name):
    g, cur = mc.graph_of(name)
    return g.n_loops(cur)


def _launches(M, L):
    if M <= 1:
        return 4
    return 13 + (1 if L <= pm.CAP_DEFAULT else 3 * -(-6 * L // pm.PANEL))


def _device_graph(ctx, g):
    """g with the device's stored poses in the place of its own"""
    d = g.copy()
    d.poses = ctx.pg_poses()
    return d


def _block_properties(cov):
    assert not cov[0].any()                                                   # the gauge: block `first` is exactly zero
    assert (_bits(cov) == _bits(np.transpose(cov, (0, 2, 1)))).all()          # symmetric to the bit
    for blk in cov[1:]:
        assert np.linalg.eigvalsh(blk).min() > 0.0


@pytest.mark.parametrize("name", LOCAL_CASES)
def test_local_form_against_the_oracle(ctx, mla, name):
    """the oracle is built from the device's own stored poses (bit-equal to the uploaded graph's here, so the shared oracle of that graph is the one)"""
    g, cur = mc.graph_of(name)
    g.upload(ctx)
    assert (_bits(ctx.pg_poses()) == _bits(g.poses)).all()
    r = ctx.pg_marginals(cur, form=mla.PG_COV_LOCAL)
    M, L = cur - g.earliest + 1, g.n_loops(cur)
    want = mc.oracle(name)
    worst = mc.worst_rel(r["cov"], want) if r["ok"] else float("inf")
    _measured(f"marginals local {name} M {M} L {L}", worst, BAR)
    assert r["ok"] == 1 and (r["n_keyframes"], r["n_loops"], r["first_index"]) == (M, L, g.earliest)
    assert r["host_waits"] == 1 and r["launches"] == _launches(M, L)
    assert worst <= BAR
    _block_properties(r["cov"])


def test_local_form_at_the_limit_against_the_sparse_lu(ctx, mla):
    """E (L = 1024, n = 6576, 96 panels): the sample of tests/pg_marg_cases.py -- the first and last free blocks, both ends of a loop, a block next to the constant one"""
    g, cur = pm.graph_many("E")
    g.upload(ctx)
    r = ctx.pg_marginals(cur)
    want = mc.oracle_E()
    worst = max(mc.block_rel(r["cov"][k], want[k]) for k in want) if r["ok"] else float("inf")
    _measured(f"marginals local E sample of {len(want)}", worst, BAR)
    assert r["ok"] == 1 and r["host_waits"] == 1 and r["launches"] == _launches(pm.TABLE["E"][2], 1024) == 13 + 3 * 96
    assert worst <= BAR
    _block_properties(r["cov"])


@pytest.mark.parametrize("name", ("converge", "A"))
def test_after_a_full_optimise(ctx, mla, name):
    """the oracle is rebuilt from the device's poses read back with mlh_pg_poses: the device's and the restatement's optimised poses differ by up to 1e-7"""
    g, cur = mc.graph_of(name)
    g.upload(ctx)
    ctx.pg_optimize(cur)
    d = _device_graph(ctx, g)
    assert not (_bits(d.poses) == _bits(g.poses)).all()
    r = ctx.pg_marginals(cur)
    want = mc.blocks_inv(d, cur)
    worst = mc.worst_rel(r["cov"], want) if r["ok"] else float("inf")
    _measured(f"marginals after optimise {name}", worst, BAR)
    assert r["ok"] == 1 and worst <= BAR
    _block_properties(r["cov"])


@pytest.mark.parametrize("name", ("L3", "D"))
def test_store_form_is_the_converted_local_form(ctx, mla, name):
    g, cur = mc.graph_of(name)
    g.upload(ctx)
    loc = ctx.pg_marginals(cur, form=mla.PG_COV_LOCAL)
    sto = ctx.pg_marginals(cur, form=mla.PG_COV_STORE)
    assert loc["ok"] == 1 and sto["ok"] == 1
    poses = ctx.pg_poses()[g.earliest:cur + 1]
    want = np.array([mc.store_A(p[:3]) @ S @ mc.store_A(p[:3]).T for p, S in zip(poses, loc["cov"])])
    worst = max(mc.block_rel(a, b) for a, b in zip(sto["cov"][1:], want[1:]))
    _measured(f"marginals store form {name}", worst, BAR)
    assert worst <= BAR
    _block_properties(sto["cov"])


def test_no_side_effects_on_the_graph(ctx, mla):
    """poses and last poses keep their bits; an optimise after a marginals call gives the bits of one without it"""
    g, cur = mc.graph_of("converge")
    g.upload(ctx)
    ref = ctx.pg_optimize(cur)
    want, want_last = ctx.pg_poses(last=True)
    g.upload(ctx)
    before, before_last = ctx.pg_poses(last=True)
    assert ctx.pg_marginals(cur)["ok"] == 1
    after, after_last = ctx.pg_poses(last=True)
    assert (_bits(before) == _bits(after)).all() and (_bits(before_last) == _bits(after_last)).all()
    got = ctx.pg_optimize(cur)
    poses, last = ctx.pg_poses(last=True)
    assert (_bits(poses) == _bits(want)).all() and (_bits(last) == _bits(want_last)).all()
    for k in ("num_iterations", "num_successful_steps", "termination", "launches", "host_waits"):
        assert got[k] == ref[k]
    assert got["final_cost"] == ref["final_cost"] and got["launches"] == 3 + 10 * pc.MAX_IT + 1


def test_determinism_and_reuse(ctx, mla):
    """two runs are bit-equal; E then A on one context gives the bits of a fresh context; launches is the documented function of L, the same for A and A2"""
    gE, curE = pm.graph_many("E")
    gA, curA = pm.graph_many("A")
    gE.upload(ctx)
    assert ctx.pg_marginals(curE)["ok"] == 1
    gA.upload(ctx)
    a1 = ctx.pg_marginals(curA)
    a2 = ctx.pg_marginals(curA)
    assert a1["ok"] == 1 and (_bits(a1["cov"]) == _bits(a2["cov"])).all()
    fresh = mla.Context(0)
    try:
        fresh.pg_reserve(pm.LOOPS_LIMIT)
        gA.upload(fresh)
        f = fresh.pg_marginals(curA)
        assert (_bits(f["cov"]) == _bits(a1["cov"])).all()
        g2, cur2 = pm.graph_many("A2")
        g2.upload(fresh)
        b = fresh.pg_marginals(cur2)
    finally:
        fresh.close()
    assert a1["host_waits"] == 1 and b["host_waits"] == 1
    assert a1["launches"] == b["launches"] == _launches(2, 129) == 13 + 3 * 13 and a1["n_keyframes"] != b["n_keyframes"]


def test_buffers_are_allocated_by_the_first_call_only(ctx, mla):
    g, cur = mc.graph_of("L3")
    g.upload(ctx)
    ctx.pg_optimize(cur)
    g.upload(ctx)
    i0 = ctx.pg_info()
    assert ctx.pg_marginals(cur)["ok"] == 1
    i1 = ctx.pg_info()
    assert ctx.pg_marginals(cur, form=mla.PG_COV_STORE)["ok"] == 1
    i2 = ctx.pg_info()
    M = cur - g.earliest + 1
    assert i1["bytes_hbm"] > i0["bytes_hbm"] and i1["bytes_hbm"] - i0["bytes_hbm"] >= 8 * (72 * M + 180 * (M - 1) + 64 * 64)
    assert i1["allocations"] == i0["allocations"] + 1 and (i2["bytes_hbm"], i2["allocations"]) == (i1["bytes_hbm"], i1["allocations"])


def test_staleness(ctx, mla):
    """mlh_pg_device_marginals reports the problem after a call, and none after mlh_pg_set_loop / mlh_pg_optimize / mlh_pg_reset; mlh_pg_add_keyframe keeps it; the
    store update with covariances returns MLH_ERR_STATE without valid marginals"""
    g, cur = mc.graph_of("L3")
    M = cur - g.earliest + 1

    def fresh():
        g.upload(ctx)
        assert ctx.pg_device_marginals() == (None, None, -1, 0)
        assert ctx.pg_marginals(cur)["ok"] == 1
        a, b, first, n = ctx.pg_device_marginals()
        assert a and b and b - a == 8 * 36 * M and (first, n) == (g.earliest, M)

    fresh()
    ctx.pg_add_keyframe(g.poses[-1])
    assert ctx.pg_device_marginals()[3] == M
    ctx.pg_set_loop(cur, int(g.earliest) + 2, g.loop_rel[30])
    assert ctx.pg_device_marginals() == (None, None, -1, 0)
    fresh()
    ctx.pg_optimize(cur)
    assert ctx.pg_device_marginals() == (None, None, -1, 0)
    with pytest.raises(mla.MlhError) as e:
        ctx.keyframes_update_from_pose_graph_cov(first_index=g.earliest, first_key=0, n=2)
    assert _code(e) in (-1, -3)                                               # (an empty store is refused as f15 refuses it; with keys: test_gpu_keyframe_update_cov.py)
    fresh()
    ctx.pg_reset()
    assert ctx.pg_device_marginals() == (None, None, -1, 0)


def test_error_paths_leave_everything_untouched(mla):
    """MLH_ERR_UNSUPPORTED above the context's capacity, MLH_ERR_STATE without a loop or below the earliest index, MLH_ERR_INVALID for a cur_index that names no
    keyframe or an unknown form: the poses keep their bits and a valid earlier result stays valid. cur == first (M = 1): the one zero block, ok = 1"""
    c = mla.Context(0)
    try:
        gA, curA = pm.graph_many("A")
        g, cur = mc.graph_of("L3")
        # no loop yet
        for k in range(3):
            c.pg_add_keyframe(g.poses[k])
        with pytest.raises(mla.MlhError) as e:
            c.pg_marginals(2)
        assert _code(e) == -3
        g.upload(c)
        ok = c.pg_marginals(cur)
        assert ok["ok"] == 1
        valid = c.pg_device_marginals()
        for bad_cur, code in ((g.earliest - 1, -3), (len(g.poses), -1), (-1, -1)):
            with pytest.raises(mla.MlhError) as e:
                c.pg_marginals(bad_cur)
            assert _code(e) == code
        with pytest.raises(mla.MlhError) as e:
            c.pg_marginals(cur, form=7)
        assert _code(e) == -1
        assert c.pg_device_marginals() == valid and (_bits(c.pg_poses()) == _bits(g.poses)).all()
        one = c.pg_marginals(g.earliest)
        assert one["ok"] == 1 and one["n_keyframes"] == 1 and one["launches"] == 4 and one["host_waits"] == 1
        assert one["cov"].shape == (1, 6, 6) and not one["cov"].any()
        # capacity: 129 loop edges against the default 128
        gA.upload(c)
        bytes0 = c.pg_info()["bytes_hbm"]
        with pytest.raises(mla.MlhError) as e:
            c.pg_marginals(curA)
        assert _code(e) == -5 and "128" in str(e.value)
        poses, last = c.pg_poses(last=True)
        assert (_bits(poses) == _bits(gA.poses)).all() and (_bits(last) == _bits(gA.last)).all() and c.pg_info()["bytes_hbm"] == bytes0
    finally:
        c.close()


def test_recorded_tolerances():
    """the figures of this file's PG_MEASURED lines are recorded beside their bars"""
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "pg_marginals_tolerances.json")))
    assert t["local_form_bar"] == t["store_form_bar"] == t["after_optimise_bar"] == BAR
    assert 0 < t["local_form_measured"] <= BAR and 0 < t["local_form_at_the_limit_measured"] <= BAR
    assert 0 < t["after_optimise_measured"] <= BAR and 0 <= t["store_form_measured"] <= BAR
