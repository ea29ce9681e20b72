"""The launch census: how many launches of each solver kernel every entry point enqueues, against a recording (tests/golden/solver_launch_census.json).

The parity tests compare the schedules' pose bits; two schedules can give the same bits from different launches -- one launch too many, an LM step taken in the
classic form where the consumer-side form is meant -- and that costs time without failing anything. The library's own profiler counts launches per kernel id
(mlh_profile_sample(1): every launch); the counts are integers, so the comparison is exact. The census does not see a lost warm-start flag: a cold search runs
under the same kernel id.

The tracker's kernels carry no profiler id, so it has no rows in the recording: its census is the one-launch loops that mlh_get_info counts (loop_launches),
one per round by default and none with MLH_TRACK_LOOP=0.

MLOAM_CENSUS_RECORD=1 writes the recording instead of comparing against it (run on the commit whose schedule is the reference)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_launch_census.json")
KERNELS = ("KNN", "FIT", "LINEARIZE", "SOLVE", "KNN_PRE", "KNN_FIRST")
LM_ENV = ("MLH_LM_CONSUMER", "MLH_LM_LOOP", "MLH_LOOP_TAGGED", "MLH_TRACK_LOOP")
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _stage(c, mla, case, feats):
    c.map_set(mla.SURF, case["surf_map"])
    c.map_set(mla.CORNER, case["corner_map"])
    c.features_set(mla.SURF, feats[0])
    c.features_set(mla.CORNER, feats[1])


def _profiled(mla):
    c = mla.Context(0)
    c.profile_enable()
    c.profile_sample(1)
    return c


class _Census:
    def __init__(self, mla):
        self.mla = mla
        self.ids = [getattr(mla, "K_" + k) for k in KERNELS]
        self.counts = {}
        self.loops = {}

    def take(self, name, c, call, env=None):
        """profile_reset, the call, the six counters (and the loop launches it added). `env` holds for this call only."""
        assert name not in self.counts, name
        saved = {k: os.environ.pop(k, None) for k in LM_ENV}
        try:
            os.environ.update(env or {})
            c.profile_reset()
            loops = c.info()["loop_launches"]
            out = call()
            self.counts[name] = [int(c.profile_get(k)[1]) for k in self.ids]
            self.loops[name] = c.info()["loop_launches"] - loops
        finally:
            for k in LM_ENV:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
        return out


def _lm_env(mode):
    return {"MLH_LM_CONSUMER": mode[0], "MLH_LM_LOOP": mode[1], "MLH_LOOP_TAGGED": "0" if mode.endswith("b") else "1"}


def _census_scan2map(cs, mla, case16, feats16):
    p0 = case16["p0"]
    c = _profiled(mla)
    try:
        _stage(c, mla, case16, feats16)
        cs.take("scan2map/lean/default", c, lambda: c.scan2map(p0, want_stats=False))
        for mode in ("00", "10", "11", "11b"):
            cs.take(f"scan2map/lean/{mode}", c, lambda: c.scan2map(p0, want_stats=False), _lm_env(mode))
        _, st = cs.take("scan2map/stats", c, lambda: c.scan2map(p0))
        need = max(int(x["lm_iterations"]) for x in st)
        for m in ("rnd", "fps"):
            opts = mla.default_opts(gf_method=mla.GF_METHODS[m], gf_ratio=0.3, gf_seed=5)
            cs.take(f"scan2map/{m}/lean", c, lambda: c.scan2map(p0, opts, want_stats=False))
            cs.take(f"scan2map/{m}/stats", c, lambda: c.scan2map(p0, opts))

        def split(**kw):
            c.scan2map_begin(p0, **kw)
            pose, status = c.scan2map_end()
            assert status == 0
        cs.take("scan2map_begin/default", c, split)
        cs.take("scan2map_begin/lookahead=need", c, lambda: split(lm_lookahead=need))

        def chained():
            c.scan2map_begin(p0)
            c.scan2map_begin_chained(IDENT, IDENT)
            assert c.scan2map_end()[1] == 0 and c.scan2map_end()[1] == 0
        cs.take("scan2map_begin+chained", c, chained)
    finally:
        c.close()


def _census_gn(cs, mla, case16, feats16):
    p0 = case16["p0"]
    c = _profiled(mla)
    try:
        _stage(c, mla, case16, feats16)
        cs.take("gn_solve5/lean", c, lambda: c.gn_solve(p0, 5, want_stats=False))
        cs.take("gn_solve5/stats", c, lambda: c.gn_solve(p0, 5))

        def chained():
            c.gn_solve_begin(p0, 5)
            c.gn_solve_begin_chained(IDENT, IDENT, 5)
            c.gn_solve_end()
            c.gn_solve_end()
        for name, sched in (("all_on", (1, 1, 1)), ("all_off", (0, 0, 0))):
            c.set_gn_schedule(*sched)
            cs.take(f"gn_solve_begin+chained/{name}", c, chained)
        c.set_gn_schedule(1, 1, 1)
        half_s, half_c = len(feats16[0]) // 2, len(feats16[1]) // 2
        c.features_set_blocks(mla.SURF, [feats16[0][:half_s], feats16[0][half_s:]])
        c.features_set_blocks(mla.CORNER, [feats16[1][:half_c], feats16[1][half_c:]])
        poses0 = np.stack([p0, p0])
        cs.take("gn_solve_blocks/2", c, lambda: c.gn_solve_blocks(poses0, 3, [5, 10], [100.0, 100.0], [0, 1]))
    finally:
        c.close()


def _census_track(cs, mla, tc):
    """the tracker's rows: its loop launches only, kept apart from the recording (see the module's docstring)"""
    c = _profiled(mla)
    try:
        c.track_set_prev(mla.CORNER, tc["corner_last"]); c.track_set_prev(mla.SURF, tc["surf_last"])
        c.track_set_cur(mla.CORNER, tc["corner_sharp"]); c.track_set_cur(mla.SURF, tc["surf_flat"])
        cs.take("track_cloud/lean/default", c, lambda: c.track_cloud(IDENT, want_stats=False))
        cs.take("track_cloud/lean/launches", c, lambda: c.track_cloud(IDENT, want_stats=False), {"MLH_TRACK_LOOP": "0"})
    finally:
        c.close()
    for k in ("track_cloud/lean/default", "track_cloud/lean/launches"):
        assert cs.counts.pop(k) == [0] * len(KERNELS)      # (no profiler id: were that to change, the rows belong in the recording)


def _census_downsample_scan2map(cs, mla, orc, synth, case16):
    """staged as test_mapper_inputs_stay_on_device stages it: the one-call form on the device-resident fused clouds, the two calls inside on host buffers"""
    scans = case16["scans"] * 2
    ext = np.array([np.concatenate([r[4:7], r[:4]]) for r in synth.HERCULES_BODY_T_LASER])[:2]
    for e in ext:
        e[3:] /= np.linalg.norm(e[3:])
    covs = np.stack([np.zeros((6, 6)), np.diag([0.0025] * 3 + [0.00030461] * 3)])
    meas = np.diag([0.0025] * 3)
    p0 = case16["p0"]
    c = _profiled(mla)
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
        for name, o in (("default", mla.default_opts(flags=mla.FLAG_WITH_UA)), ("max_outer=3", mla.default_opts(flags=mla.FLAG_WITH_UA, max_outer=3))):
            cs.take(f"downsample_scan2map/device/{name}", c,
                    lambda: c.downsample_scan2map(c.fused_cloud(mla.SURF), c.fused_cloud(mla.CORNER), 0.4, 0.2, ext, covs, meas, p0, o))
        o = mla.default_opts(flags=mla.FLAG_WITH_UA)
        cs.take("downsample_scan2map/host", c, lambda: c.downsample_scan2map(host[0], host[1], 0.4, 0.2, ext, covs, meas, p0, o))
    finally:
        c.close()


@pytest.fixture(scope="module")
def census(mla, orc, synth, case16, feats16, track_case):
    cs = _Census(mla)
    _census_scan2map(cs, mla, case16, feats16)
    _census_gn(cs, mla, case16, feats16)
    _census_track(cs, mla, track_case)
    _census_downsample_scan2map(cs, mla, orc, synth, case16)
    if os.environ.get("MLOAM_CENSUS_RECORD") == "1":
        with open(GOLDEN, "w") as f:
            json.dump({"kernels": list(KERNELS), "launches": cs.counts}, f, indent=1, sort_keys=True)
            f.write("\n")
    return cs


def test_solver_launch_census_equals_the_recording(census):
    """Every censused call enqueues exactly the recorded number of launches of each solver kernel (no tolerance: they are counts)."""
    with open(GOLDEN) as f:
        rec = json.load(f)
    assert rec["kernels"] == list(KERNELS)
    got = census.counts
    for name, n in got.items():
        print(name, dict(zip(KERNELS, n)))
    assert sorted(got) == sorted(rec["launches"])
    differ = {k: (dict(zip(KERNELS, got[k])), dict(zip(KERNELS, rec["launches"][k]))) for k in got if got[k] != rec["launches"][k]}
    assert not differ, differ


def test_solver_launch_census_anchors(census):
    """Two counts that follow from reading the schedule: the default scan2map (two outer iterations) is two correspondence launches, each with one launch behind it
    that runs the fit and the whole LM loop (counted under the linearise id): no stand-alone fit, no solve kernel. Five lean Gauss-Newton iterations are one cold
    search, four bounded ones that begin with the previous iteration's finish, and five fits, the last of which publishes. The tracker's two rounds are a loop
    launch each by default and none with MLH_TRACK_LOOP=0."""
    s = dict(zip(KERNELS, census.counts["scan2map/lean/default"]))
    assert (s["KNN"], s["FIT"], s["LINEARIZE"], s["SOLVE"]) == (2, 0, 2, 0), s
    g = dict(zip(KERNELS, census.counts["gn_solve5/lean"]))
    assert (g["KNN"], g["KNN_PRE"], g["FIT"], g["SOLVE"]) == (1, 4, 5, 0), g
    assert (census.loops["track_cloud/lean/default"], census.loops["track_cloud/lean/launches"]) == (2, 0), census.loops
