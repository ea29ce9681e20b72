"""The fused Gauss-Newton iteration (match.hip: knn_features_wide_kernel<.., FIT>: the fit runs in the tail of its search launch) against the two-launch form.

Fusing moves the fit from a launch of its own, one lane per feature in 256-feature workgroups, into the wide search workgroup that just found the feature's
neighbours; the wavefront rows it leaves are added by the next launch's prologue in the order the fit kernel's workgroup adds them. It changes no arithmetic. So
every solve has to come out of a context created under MLH_GN_FIT_IN_SEARCH=1 with the BITS it has under =0 and under MLH_KNN_WG_THREADS=256: poses, and with
statistics (the classic solve, never fused) the per-iteration H, g, cost and counts.

Map, features and the walk through the solve forms are test_gpu_knn_wg_width.py's. Feature counts straddle the edges of a wavefront row (64 features), of a wide
tile (64 or 128 queries) and of a 256-feature tile -- 191/192/193 and 255/256/257 included --, once per kind, against a partner of 141 features (two full rows and a
part of one: the fourth row of its 256-feature tile is one no workgroup produces and the kind's last wide workgroup has to write as zeros).

Which launches fuse, read from the schedule (match.hip: fit_in_search; solve_host.hip): a launch fuses when it is wide, has a prologue in front and its fit would only
leave records, and every kind of the frame puts 64 queries or more into a workgroup (width / lanes >= 64: at 1 024 threads 8 and 16 lanes, at 512 threads 8 lanes
only). Five iterations then enqueue, as mlh_debug_gn_fused_launches counts them (the number of the last submitted solve):
  gn_solve with statistics            0  (the classic finish: every fit launch solves)
  gn_solve                            3  (iteration 0 has no prologue, iteration 4's fit publishes; iterations 1-3 fuse)
  gn_solve_begin                      4  (iteration 0 has no prologue; the last iteration leaves its records to the successor: iterations 1-4)
  gn_solve_begin_chained              5  (iteration 0 completes the predecessor first: PRE 2)
and 0 where the launches do not fuse or under MLH_GN_FIT_IN_SEARCH=0. Without the switch the rule adds one condition, a chip-filling frame (more than 8 192
queries): test_rule_fuses_the_chip_filling_frame_only."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
WIDE = (1024, 512)
LANES = (None, "8", "816")
COUNTS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300)
PARTNER = 141
SHAPES = [(m, PARTNER) for m in COUNTS] + [(PARTNER, m) for m in COUNTS] + [(300, 300), (129, 0), (0, 129), (0, 64), (65, 0)]
FUSED_IF_FUSABLE = (0, 3, 4, 5, 5, 4, 5)         # per solve of _solves, in its order
P_TRUE = np.array([0.30, -0.20, 0.10, 0.010, -0.015, 0.020, 0.0])
P_TRUE[6] = np.sqrt(1.0 - (P_TRUE[3:6] ** 2).sum())
P_START = np.array([0.34, -0.17, 0.07, 0.016, -0.011, 0.026, 0.0])
P_START[6] = np.sqrt(1.0 - (P_START[3:6] ** 2).sum())
EDGES_XY = ((6.0, -7.5), (6.0, 7.5), (-4.0, 3.0))


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _maps():
    rng = np.random.default_rng(5)
    g = np.arange(-20, 21) * 0.4
    xx, yy = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([xx.ravel(), yy.ravel(), np.zeros(xx.size)], 1)
    floor[:, :2] += rng.uniform(-0.05, 0.05, (len(floor), 2))
    yy, zz = np.meshgrid(g, np.arange(1, 17) * 0.4, indexing="ij")
    wall = np.stack([np.full(yy.size, 6.0), yy.ravel(), zz.ravel()], 1)
    wall[:, 1:] += rng.uniform(-0.05, 0.05, (len(wall), 2))
    z = np.arange(61) * 0.1 + 0.2
    edges = np.concatenate([np.stack([np.full(61, x), np.full(61, y), z + 0.013 * i], 1) for i, (x, y) in enumerate(EDGES_XY)])
    return np.ascontiguousarray(np.concatenate([floor, wall]), F32), np.ascontiguousarray(edges, F32)


def _features(ms, mc, seed):
    """(ms, 4), (mc, 4): points of the planes / the edges, in the body frame of P_TRUE"""
    rng = np.random.default_rng(seed)
    R, t = _rot(P_TRUE[3:]), P_TRUE[:3]
    on_floor = rng.random(ms) < 0.6
    ws = np.where(on_floor[:, None],
                  np.stack([rng.uniform(-7, 5.5, ms), rng.uniform(-7, 7, ms), np.zeros(ms)], 1),
                  np.stack([np.full(ms, 6.0), rng.uniform(-7, 7, ms), rng.uniform(0.8, 6.0, ms)], 1))
    e = rng.integers(0, 3, mc)
    wc = np.stack([np.array([EDGES_XY[i][0] for i in e]), np.array([EDGES_XY[i][1] for i in e]), rng.uniform(0.6, 5.8, mc)], 1).reshape(mc, 3)
    out = []
    for w in (ws, wc):
        f = np.zeros((len(w), 4), F32)
        f[:, :3] = (w - t) @ R          # R^T (w - t)
        out.append(f)
    return out


class _Contexts:
    def __init__(self, mla):
        self.mla, self.ctx, self.lib = mla, {}, mla.load_library()
        for fn in (self.lib.mlh_debug_knn_wg_threads, self.lib.mlh_debug_gn_fused_launches):
            fn.argtypes = [C.c_void_p]
            fn.restype = C.c_int
        self.maps = _maps()

    def get(self, wg=None, fis=None, lanes=None, tag=None):
        """tag: a context of its own for frames that must not inherit what another test staged (a kind left without features, pose blocks)"""
        key = (wg, fis, lanes, tag)
        if key not in self.ctx:
            env = {"MLH_KNN_WG_THREADS": wg and str(wg), "MLH_GN_FIT_IN_SEARCH": None if fis is None else str(fis), "MLH_KNN_LANES": lanes}
            old = {k: os.environ.get(k) for k in env}
            for k, v in env.items():
                os.environ.pop(k, None)
                if v:
                    os.environ[k] = v
            try:
                c = self.mla.Context(0)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            c.map_set(self.mla.SURF, self.maps[0])
            c.map_set(self.mla.CORNER, self.maps[1])
            self.ctx[key] = c
        return self.ctx[key]

    def fused(self, c):
        return int(self.lib.mlh_debug_gn_fused_launches(c.h))

    def width_taken(self, c):
        return int(self.lib.mlh_debug_knn_wg_threads(c.h))

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def ctxs(mla):
    cs = _Contexts(mla)
    yield cs
    cs.close()


def _stage(mla, c, fs, fc):
    if len(fs):
        c.features_set(mla.SURF, fs)
    if len(fc):
        c.features_set(mla.CORNER, fc)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def _same_stats(a, b, where):
    assert len(a) == len(b)
    for it, (x, y) in enumerate(zip(a, b)):
        for k in ("n_surf", "n_corner", "is_degenerate"):
            assert x[k] == y[k], (where, it, k, x[k], y[k])
        for k in ("H", "g", "cost", "pose_after"):
            assert _bits(x[k]) == _bits(y[k]), (where, it, k, x[k], y[k])


def _solves(cs, mla, c, fs, fc):
    """every form of the solve on one staged frame (test_gpu_knn_wg_width.py: _solves) -> (poses, stats, fused launches of every submitted solve)"""
    poses, fused = [], []
    _stage(mla, c, fs, fc)
    p, stats = c.gn_solve(P_START, 5, want_stats=True)          # classic finish
    fused.append(cs.fused(c))
    p, _ = c.gn_solve(P_START, 5, want_stats=False)             # deferred finish: PRE 1 warm
    fused.append(cs.fused(c))
    poses.append(p)
    conv = p
    c.gn_solve_begin(P_START, 5)                                # three frames in flight one behind the other: PRE 2 twice
    fused.append(cs.fused(c))
    c.gn_solve_begin_chained(conv, P_START, 5)
    fused.append(cs.fused(c))
    poses.append(c.gn_solve_end())
    c.gn_solve_begin_chained(conv, P_START, 5)
    fused.append(cs.fused(c))
    poses.append(c.gn_solve_end())
    poses.append(c.gn_solve_end())                              # the drain: the pending rows go through the one-workgroup launch ...
    _stage(mla, c, fs, fc)                                      # ... and a fresh begin on a restaged frame
    c.gn_solve_begin(P_START, 5)
    fused.append(cs.fused(c))
    c.gn_solve_begin_chained(conv, P_START, 5)
    fused.append(cs.fused(c))
    poses.append(c.gn_solve_end())
    poses.append(c.gn_solve_end())
    return poses, stats, tuple(fused)


@pytest.mark.parametrize("lanes", LANES, ids=lambda l: f"lanes-{l or 'rule'}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_bits_fused_and_not(mla, ctxs, shape, lanes):
    ms, mc = shape
    fs, fc = _features(ms, mc, seed=100 + ms + 7 * mc)
    tag = None if ms and mc else ("only-surf" if ms else "only-corner")
    ref_poses, ref_stats, ref_fused = _solves(ctxs, mla, ctxs.get(256, None, lanes, tag), fs, fc)
    assert ref_fused == (0,) * 7, ref_fused
    for p in ref_poses:
        assert np.isfinite(p).all(), ref_poses
    for wg in WIDE:
        for fis in (1, 0):
            c = ctxs.get(wg, fis, lanes, tag)
            poses, stats, fused = _solves(ctxs, mla, c, fs, fc)
            assert ctxs.width_taken(c) == wg, (wg, ctxs.width_taken(c))
            kinds = [k for k, m in ((mla.SURF, ms), (mla.CORNER, mc)) if m]
            fusable = fis == 1 and all(wg // c.map_info(k)["knn_lanes"] >= 64 for k in kinds)
            assert fused == (FUSED_IF_FUSABLE if fusable else (0,) * 7), (shape, lanes, wg, fis, fused)
            for i, (a, b) in enumerate(zip(ref_poses, poses)):
                assert _bits(a) == _bits(b), (shape, lanes, wg, fis, "solve form", i, a, b)
            _same_stats(ref_stats, stats, (shape, lanes, wg, fis))


def test_fused_launches_are_taken_at_both_widths(mla, ctxs):
    """the comparison above must not pass because nothing ever fused: 8 lanes fuse at 1 024 and at 512 threads, 16 lanes at 1 024 only"""
    fs, fc = _features(129, 141, seed=9)
    for wg, lanes, expect in ((1024, "8", FUSED_IF_FUSABLE), (512, "8", FUSED_IF_FUSABLE), (1024, None, FUSED_IF_FUSABLE), (512, None, (0,) * 7)):
        c = ctxs.get(wg, 1, lanes)
        _, _, fused = _solves(ctxs, mla, c, fs, fc)
        assert fused == expect, (wg, lanes, fused)


def test_narrow_stays_narrow(mla, ctxs):
    """20 features: two 256-thread workgroups, far fewer than compute units: the launches stay on the 256-thread kernels and none of them fuses"""
    c = ctxs.get()
    fs, fc = _features(12, 8, seed=3)
    _stage(mla, c, fs, fc)
    c.gn_solve(P_START, 5, want_stats=False)
    assert ctxs.width_taken(c) == 256
    assert ctxs.fused(c) == 0
    c.gn_solve_begin(P_START, 5)
    c.gn_solve_begin_chained(P_START, P_START, 5)
    assert ctxs.fused(c) == 0
    c.gn_solve_end()
    c.gn_solve_end()


def test_rule_fuses_the_chip_filling_frame_only(mla, ctxs):
    """Without the switch, a launch that can fuse does when it is chip-filling: more than 8 192 queries (knn_dev.hpp: KNN_LATENCY_LIMIT, the throughput regime of the
    lanes rule). 6 000 features at 16 lanes are 375 workgroups of 256 threads -- more than compute units, so the launches go wide where the device has fewer than
    375 -- and stay at two launches per iteration, as tests/golden/solver_launch_census.json records the 16-ring frame; 10 240 + 300 features fuse. Same bits
    as with the switch off."""
    rule, off = ctxs.get(), ctxs.get(None, 0)
    for ms, mc, fuses in ((4500, 1500, False), (40 * 256, 300, True)):
        fs, fc = _features(ms, mc, seed=21 + ms)
        poses = []
        for c in (rule, off):
            _stage(mla, c, fs, fc)
            poses.append(c.gn_solve(P_START, 5, want_stats=False)[0])
        wide = ctxs.width_taken(rule) != 256
        assert wide or not fuses, (ms, mc, ctxs.width_taken(rule), rule.info()["cu_solver"])
        assert ctxs.fused(rule) == (3 if fuses else 0), (ms, mc, ctxs.fused(rule))
        assert ctxs.fused(off) == 0
        assert _bits(poses[0]) == _bits(poses[1])


def test_blocks_stay_unfused(mla, ctxs):
    """a solve over two pose blocks keeps its two launches per iteration under MLH_GN_FIT_IN_SEARCH=1, and its bits"""
    fs, fc = _features(300, 129, seed=6)
    out = []
    for wg, fis in ((256, None), (1024, 1)):
        c = ctxs.get(wg, fis, tag="blocks")
        c.features_set_blocks(mla.SURF, [fs[:170], fs[170:]])
        c.features_set_blocks(mla.CORNER, [fc[:70], fc[70:]])
        poses, _ = c.gn_solve_blocks(np.stack([P_START, np.array([0, 0, 0, 0, 0, 0, 1.0])]), 3, [5, 5], [100.0, 100.0], [0, 0], want_stats=False)
        assert ctxs.fused(c) == 0
        out.append(poses)
    assert _bits(out[0]) == _bits(out[1])


def test_switch_from_the_environment_is_checked(mla):
    os.environ["MLH_GN_FIT_IN_SEARCH"] = "2"
    try:
        with pytest.raises(mla.MlhError):
            mla.Context(0)
    finally:
        os.environ.pop("MLH_GN_FIT_IN_SEARCH", None)
