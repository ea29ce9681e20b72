"""The initial extrinsic calibration on the device (m-loam_amd/csrc/initext.hip; mlh_initext_*) against the NumPy transcription of InitialExtrinsics
(tests/initext_cases.py), which tests/test_initext_cases.py holds on the CPU: every case runs through add_pose / calibrate exactly as its mode says (stage by stage
or fused) and, for the call-site cases, through the facade's names via m-loam_amd/host/initext_selftest.

Bars: singular values within 1e-9 of the largest (the f64 linear-algebra bar of DESIGN section 2); q and t within 1e-7 (the pose bar of the f12-f14 tests), compared
only where the rotation has converged -- where sigma_3 is near zero the null vector is not unique, and only singular values and flags are held; accepted flags, slot
indices, convergence flags, ranks and the cov states equal; the stored sets and Q_ bit-equal to what the host header gives (the sets are the caller's doubles; each
block is recomputed by tests/host/initext_host_main.cpp from the calib_ext_ the device held at that moment); two runs bit-equal; one launch and one host wait per
calibration, one launch and no wait per accepted set, no allocation after reset. Every test prints what it measured (IE_MEASURED name value bar) before it asserts;
tests/golden/initext_tolerances.json records those figures beside the bars as measured on an MI355X.

Observed on an MI355X: singular values at most 9.2e-15 of the largest (callsite_4, whose late LiDAR is fed outliers), q and t at most 5.1e-15 (sweep, 320 accepted
sets); Q_ within 1.0e-15 of the transcription's (the weights of down-weighted blocks read estimates that differ by rounding) and bit-equal to the host header's."""
import os
import subprocess

import numpy as np
import pytest

import initext_cases as ic

pytestmark = pytest.mark.gpu

BAR_SV, BAR_POSE = 1e-9, 1e-7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_KEYS = ("n_sets", "heap_size", "last_slot", "cov_rot_mask", "cov_pos_mask", "full_cov_rot", "full_cov_pos")


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _measured(name, value, bar):
    print(f"IE_MEASURED {name} {value:.3e} {bar:.1e}")


def _code(excinfo):
    return int(str(excinfo.value).split("mlh error ")[1].split(":")[0])


class DevApi:
    """the device behind the interface of ic.RefInitExt; holds the launch / wait / allocation counts of every call and logs what each written block was made of"""

    def __init__(self, mla, ctx, opts):
        self.mla, self.ctx, self.opts = mla, ctx, opts
        ctx.initext_reset(mla.initext_opts(**opts))
        self.allocations = ctx.initext_info()["allocations"]
        self.blocks = {}             # (lidar, slot) -> (pose_ref, pose_data, calib_ext before the call): the last write wins
        self.last = None

    def add_pose(self, poses):
        acc = self.ctx.initext_add_pose(poses)
        i = self.ctx.initext_info()
        assert (i["launches"], i["host_waits"]) == ((1, 0) if acc else (0, 0)) and i["allocations"] == self.allocations
        if acc:
            self.last = np.array(poses, np.float64).reshape(-1, 7)
        return acc

    def calibrate(self, lidars, stages=ic.ROT | ic.TRANS):
        ext = self.ctx.initext_read_state()["calib_ext"]
        out = self.ctx.initext_calibrate(lidars, stages)
        i = self.ctx.initext_info()
        ran = any(r["rot_ran"] or r["trans_solved"] for r in out) or stages == ic.TRANS
        assert (i["launches"], i["host_waits"]) == ((1, 1) if ran else (0, 0)) and i["allocations"] == self.allocations
        for r in out:
            if r["rot_ran"]:
                self.blocks[(r["lidar"], r["slot"])] = (self.last[self.opts["idx_ref"]], self.last[r["lidar"]], ext[r["lidar"]].copy())
        return out

    def info(self):
        return self.ctx.initext_info()


def _compare(name, dev, ref):
    """the records of a run on the device against the transcription's -> the largest distances seen"""
    worst = dict(rot_sv=0.0, trans_sv=0.0, q=0.0, t=0.0)
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d["accepted"] == r["accepted"], (name, k)
        assert {x: d["info"][x] for x in INFO_KEYS} == {x: r["info"][x] for x in INFO_KEYS}, (name, k)
        assert len(d["results"]) == len(r["results"]), (name, k)
        for dres, rres in zip(d["results"], r["results"]):
            for a, b in zip(dres, rres):
                for key in ("lidar", "rot_ran", "slot", "rot_converged", "trans_solved", "trans_rank"):
                    assert a[key] == b[key], (name, k, key, a, b)
                if b["rot_ran"]:
                    worst["rot_sv"] = max(worst["rot_sv"], np.abs(a["rot_sv"] - b["rot_sv"]).max() / max(b["rot_sv"][0], 1e-300))
                    assert a["rot_sweeps"] < 30
                has_rotation = bool((r["info"]["cov_rot_mask"] >> b["lidar"]) & 1)
                if b["trans_solved"] and has_rotation:
                    worst["trans_sv"] = max(worst["trans_sv"], np.abs(a["trans_sv"] - b["trans_sv"]).max() / b["trans_sv"][0])
                    worst["t"] = max(worst["t"], np.abs(a["t"] - b["t"]).max())
                if has_rotation and (b["rot_ran"] or b["trans_solved"]):
                    worst["q"] = max(worst["q"], np.abs(a["q"] - b["q"]).max())
    return worst


def _host_main(tmp_path):
    exe = tmp_path / "initext_host_main"
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "initext_host_main.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


@pytest.mark.parametrize("name", sorted(ic.cases()))
def test_case_against_the_transcription(mla, ctx, name, tmp_path):
    """sweep: N = 5 .. 300 accepted sets and 20 replacements, rotation after every frame (five of them without a new set, one rewriting a down-weighted block), translation alone at the checkpoints;
    callsite_2 / callsite_staged_2: estimator.cpp:437-467 fused and stage by stage; callsite_4: four LiDARs, idx_ref = 2, one converging a dozen frames late;
    planar_z_0 / planar_wobble_1: planar motion under both settings (the planar system and its rank); pure_translation: the zero matrix gives the identity"""
    case = ic.cases()[name]
    api = DevApi(mla, ctx, case["opts"])
    dev = ic.run(api, case)
    ref, ref_api = ic.expected(name)
    worst = _compare(name, dev, ref)
    for key, bar in (("rot_sv", BAR_SV), ("trans_sv", BAR_SV), ("q", BAR_POSE), ("t", BAR_POSE)):
        _measured(f"{name}_{key}", worst[key], bar)
    assert worst["rot_sv"] <= BAR_SV and worst["trans_sv"] <= BAR_SV and worst["q"] <= BAR_POSE and worst["t"] <= BAR_POSE
    st = ctx.initext_read_state()
    # the stored sets: the caller's doubles, bit for bit, in the transcription's slots; the rest zero
    want = np.zeros_like(st["sets"])
    want[:len(ref_api.v_pose)] = np.array(ref_api.v_pose)
    assert np.array_equal(st["sets"].view(np.uint64), want.view(np.uint64))
    # Q_: every written block bit-equal to the host header's for the calib_ext_ of that moment; every other row zero
    exe = _host_main(tmp_path)
    want_q = np.zeros_like(st["Q"])
    if api.blocks:
        f = tmp_path / "block.bin"
        np.concatenate([np.concatenate(v) for v in api.blocks.values()]).tofile(f)
        r = subprocess.run([exe, "block", str(f)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-500:]
        rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("B ")]
        assert len(rows) == len(api.blocks)
        for (lidar, slot), row in zip(api.blocks, rows):
            want_q[lidar, 4 * slot:4 * slot + 4] = np.array(row, np.float64).reshape(4, 4)
    assert np.array_equal(st["Q"].view(np.uint64), want_q.view(np.uint64))
    # ... and within rounding of the transcription's (whose weights come from LAPACK's estimates)
    d_q = np.abs(st["Q"] - ref_api.Q).max()
    _measured(f"{name}_Q", d_q, BAR_SV)
    assert d_q <= BAR_SV
    if name == "pure_translation":
        assert not st["Q"].any() and np.array_equal(st["calib_ext"][1], [0, 0, 0, 0, 0, 0, 1.0])
        assert all(np.array_equal(r["rot_sv"], np.zeros(4)) and r["rot_sweeps"] == 1 for rec in dev for res in rec["results"] for r in res if r["rot_ran"])
    if name == "planar_wobble_1":
        assert any(r["trans_solved"] and r["trans_rank"] == 4 for rec in dev for res in rec["results"] for r in res)


def test_two_runs_give_the_same_bits(mla, ctx):
    case = ic.cases()["callsite_4"]
    runs = []
    for _ in range(2):
        api = DevApi(mla, ctx, case["opts"])
        rec = ic.run(api, case)
        flat = [np.concatenate([r[k] for k in ("q", "t", "rot_sv", "trans_sv")]) for x in rec for res in x["results"] for r in res]
        runs.append((np.array(flat), ctx.initext_read_state()))
    assert len(runs[0][0]) > 20
    assert np.array_equal(runs[0][0].view(np.uint64), runs[1][0].view(np.uint64))
    for key in ("Q", "sets", "calib_ext"):
        assert np.array_equal(runs[0][1][key].view(np.uint64), runs[1][1][key].view(np.uint64))


@pytest.mark.parametrize("name,mode", [("callsite_2", "callsite"), ("callsite_2", "step"), ("callsite_4", "step"), ("planar_wobble_1", "callsite")])
def test_facade_names_through_the_selftest(name, mode, tmp_path):
    """InitialExtrinsics<Pose> of mloam_facade.hpp: the call site of estimator.cpp:437-467 written with the reference's names (callsite) and as one fused step() per
    frame (step): accepted flags, convergence flags and frames equal to the transcription's, rot_cov within 1e-9 of the largest singular value, the extrinsics handed to
    the call site within 1e-7"""
    exe = os.path.join(ROOT, "m-loam_amd", "host", "initext_selftest")
    assert os.path.exists(exe), "m-loam_amd/host/initext_selftest is built by build()"
    case = ic.cases()[name]
    o = case["opts"]
    f = tmp_path / "seq.bin"
    np.concatenate([[o["n_lidar"], o["idx_ref"], o["planar_movement"], len(case["frames"])], np.array(case["frames"]).ravel()]).tofile(f)
    r = subprocess.run([exe, mode, str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "initext_selftest: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
    ref, ref_api = ic.expected(name)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(x[2]) for x in lines if x[0] == "A"] == [int(rec["accepted"]) for rec in ref]
    want_r, want_t = {}, {}
    for k, rec in enumerate(ref):
        for res in rec["results"]:
            for x in res:
                if x["rot_ran"]:
                    want_r[(k, x["lidar"])] = (x["rot_converged"], x["rot_sv"][2], x["rot_sv"][0])
                if x["trans_solved"]:
                    want_t[(k, x["lidar"])] = np.concatenate([x["q"], x["t"]])
    got_r = {(int(x[1]), int(x[2])): (int(x[3]), float(x[4])) for x in lines if x[0] == "R"}
    got_t = {(int(x[1]), int(x[2])): np.array(x[3:], np.float64) for x in lines if x[0] == "T"}
    assert set(got_r) == set(want_r) and set(got_t) == set(want_t) and len(got_t) == o["n_lidar"] - 1
    d_cov = max(abs(got_r[k][1] - want_r[k][1]) / want_r[k][2] for k in want_r)
    d_ext = max(np.abs(got_t[k] - want_t[k]).max() for k in want_t)
    _measured(f"facade_{name}_{mode}_rot_cov", d_cov, BAR_SV)
    _measured(f"facade_{name}_{mode}_extrinsic", d_ext, BAR_POSE)
    assert all(got_r[k][0] == want_r[k][0] for k in want_r) and d_cov <= BAR_SV and d_ext <= BAR_POSE
    assert [ln for ln in lines if ln[0] == "E"][0][1:] == [str(ref_api.info()["full_cov_rot"]), str(ref_api.info()["full_cov_pos"])]


def test_error_returns_leave_state_and_results_untouched(mla, ctx):
    """before reset: MLH_ERR_STATE (-3); bad options, a bad LiDAR list, bad stages, a non-finite pose: MLH_ERR_INVALID (-1) with the state, the counts and the cov
    states as they were"""
    with pytest.raises(mla.MlhError) as e:
        ctx.initext_calibrate([1], ic.ROT)
    assert _code(e) == -3
    assert ctx.initext_info()["configured"] == 0 and ctx.initext_info()["allocations"] == 0
    for bad in (dict(n_lidar=9), dict(n_lidar=2, idx_ref=2), dict(window_size=0), dict(n_pose=301), dict(eps_r=float("nan")), dict(rot_cov_thre=-1.0),
                dict(qbl=np.zeros((2, 4)))):
        with pytest.raises(mla.MlhError) as e:
            ctx.initext_reset(mla.initext_opts(**bad))
        assert "bad option" in str(e.value)
    assert ctx.initext_info()["configured"] == 0
    case = ic.cases()["callsite_2"]
    api = DevApi(mla, ctx, case["opts"])
    for k in range(8):
        api.add_pose(case["frames"][k])
        api.calibrate([1], ic.ROT)
    before, info = ctx.initext_read_state(), ctx.initext_info()
    bad_pose = np.array(case["frames"][8])
    bad_pose[1, 4] = np.inf
    for call in (lambda: ctx.initext_calibrate([0], ic.ROT),            # the reference LiDAR
                 lambda: ctx.initext_calibrate([2], ic.ROT),            # out of range
                 lambda: ctx.initext_calibrate([1, 1], ic.ROT),         # listed twice
                 lambda: ctx.initext_calibrate([], ic.ROT),
                 lambda: ctx.initext_calibrate([1], 0),
                 lambda: ctx.initext_calibrate([1], 4),
                 lambda: ctx.initext_add_pose(bad_pose),
                 lambda: ctx.initext_reset(mla.initext_opts(n_lidar=0))):
        with pytest.raises(mla.MlhError) as e:
            call()
        assert _code(e) == -1, str(e.value)
        after = ctx.initext_read_state()
        assert all(np.array_equal(before[key].view(np.uint64), after[key].view(np.uint64)) for key in before)
        assert ctx.initext_info() == info
    # and the run goes on as if nothing had happened
    assert api.add_pose(case["frames"][8]) and api.calibrate([1], ic.ROT)[0]["rot_ran"]


def test_track_cloud_is_untouched_by_the_calibration(mla, ctx, track_case):
    """a context that ran the calibration gives mlh_track_cloud's result bit for bit as a context that never did"""
    tc = track_case
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])

    def track(c):
        c.track_set_prev(mla.CORNER, tc["corner_last"]); c.track_set_prev(mla.SURF, tc["surf_last"])
        c.track_set_cur(mla.CORNER, tc["corner_sharp"]); c.track_set_cur(mla.SURF, tc["surf_flat"])
        return c.track_cloud(ident)

    fresh = mla.Context(0)
    try:
        want_pose, want_stats = track(fresh)
    finally:
        fresh.close()
    case = ic.cases()["callsite_2"]
    ic.run(DevApi(mla, ctx, case["opts"]), case)
    got_pose, got_stats = track(ctx)
    assert np.linalg.norm(want_pose[:3]) > 0.1          # (the tracker moved: the comparison is not between two untouched identities)
    assert np.array_equal(got_pose.view(np.uint64), want_pose.view(np.uint64))
    assert [s["cost"] for s in got_stats] == [s["cost"] for s in want_stats] and len(got_stats) >= 1
