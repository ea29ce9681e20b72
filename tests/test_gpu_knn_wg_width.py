"""The wide forms of the correspondence kernel (match.hip: knn_features_wide_kernel, 512 / 1024 threads per workgroup) against the 256-thread kernels.

A workgroup's width changes which queries share a workgroup and how many workgroups run the Gauss-Newton prologue; it changes no arithmetic. So every
solve has to come out of a context created under MLH_KNN_WG_THREADS=512 or =1024 with the BITS it has under =256: poses, and with statistics the
per-iteration H, g, cost and counts.

Map: two planes (a floor and a wall, jittered lattices) and three vertical edges, 2 520 points. Features: points of those planes and edges seen from a pose a
few centimetres off. Feature counts straddle the wide tiles' edges (a 1 024-thread workgroup holds 64 queries at 16 lanes, 128 at 8; a 512-thread one 32 / 64),
for both kinds independently, with one kind absent, and -- every count that is no multiple of the tile -- with the kind boundary inside what would have been one
wide workgroup. Lanes: the small launch's 16, 8, and 8 for surf with 16 for corner (the per-kind kernel of the full-size frame).

Padding slots (w < 0) exist only between the pose blocks of a solve over blocks, which keeps the 256-thread kernels whatever the width asked for
(test_blocks_solve_stays_narrow).

The width a launch took is read through mlh_debug_knn_wg_threads (exported by the library for this file; not part of the C-ABI header)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
WIDTHS = (256, 512, 1024)
WIDE_DEFAULT = 1024          # match.hip: KNN_WG_WIDE
LANES = (None, "8", "816")
COUNTS = (1, 63, 64, 65, 127, 128, 129, 300)
# (surf, corner): every count once per kind, against a partner that is no multiple of any tile; one kind absent
SHAPES = [(m, COUNTS[-1 - i]) for i, m in enumerate(COUNTS)] + [(300, 300), (129, 0), (0, 129), (0, 64), (65, 0)]
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
        self.lib.mlh_debug_knn_wg_threads.argtypes = [C.c_void_p]
        self.lib.mlh_debug_knn_wg_threads.restype = C.c_int
        self.maps = _maps()

    def get(self, wg=None, lanes=None, cu_mask=None, tag=None):
        """tag: a context of its own for frames that must not inherit what another test staged (a kind left without features, pose blocks)"""
        key = (wg, lanes, cu_mask, tag)
        if key not in self.ctx:
            env = {"MLH_KNN_WG_THREADS": wg and str(wg), "MLH_KNN_LANES": lanes, "MLH_SOLVER_CU_MASK": cu_mask}
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
    """a context holds a kind's features until they are replaced: a frame without one kind gets a context that never saw that kind (_ctx_for)"""
    if len(fs):
        c.features_set(mla.SURF, fs)
    if len(fc):
        c.features_set(mla.CORNER, fc)


def _ctx_for(ctxs, wg, lanes, ms, mc):
    return ctxs.get(wg, lanes, tag=None if ms and mc else ("only-surf" if ms else "only-corner"))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def _same_stats(a, b, where):
    assert len(a) == len(b)
    for it, (x, y) in enumerate(zip(a, b)):
        for k in ("n_surf", "n_corner", "is_degenerate"):
            assert x[k] == y[k], (where, it, k, x[k], y[k])
        for k in ("H", "g", "cost", "pose_after"):
            assert _bits(x[k]) == _bits(y[k]), (where, it, k, x[k], y[k])


def _solves(mla, c, fs, fc):
    """every form of the solve on one staged frame -> (poses, stats)"""
    poses = []
    _stage(mla, c, fs, fc)
    p, stats = c.gn_solve(P_START, 5, want_stats=True)          # classic finish, bounded search from iteration 1: PRE 0 warm
    poses.append(p)
    p, _ = c.gn_solve(P_START, 5, want_stats=False)             # deferred finish: PRE 1 warm
    poses.append(p)
    conv = p
    c.gn_solve_begin(P_START, 5)                                # three frames in flight one behind the other: PRE 2 twice
    c.gn_solve_begin_chained(conv, P_START, 5)
    poses.append(c.gn_solve_end())
    c.gn_solve_begin_chained(conv, P_START, 5)
    poses.append(c.gn_solve_end())
    poses.append(c.gn_solve_end())                              # the drain ...
    _stage(mla, c, fs, fc)                                      # ... and a fresh begin on a restaged frame (bench.py --restage-every)
    c.gn_solve_begin(P_START, 5)
    c.gn_solve_begin_chained(conv, P_START, 5)
    poses.append(c.gn_solve_end())
    poses.append(c.gn_solve_end())
    return poses, stats


@pytest.mark.parametrize("lanes", LANES, ids=lambda l: f"lanes-{l or 'rule'}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_bits_at_every_width(mla, ctxs, shape, lanes):
    ms, mc = shape
    fs, fc = _features(ms, mc, seed=100 + ms + 7 * mc)
    ref_poses, ref_stats = None, None
    for wg in WIDTHS:
        c = _ctx_for(ctxs, wg, lanes, ms, mc)
        poses, stats = _solves(mla, c, fs, fc)
        assert ctxs.width_taken(c) == wg, (wg, ctxs.width_taken(c))
        for p in poses:
            assert np.isfinite(p).all(), (wg, poses)
        if wg == 256:
            ref_poses, ref_stats = poses, stats
            continue
        for i, (a, b) in enumerate(zip(ref_poses, poses)):
            assert _bits(a) == _bits(b), (shape, lanes, wg, "solve form", i, a, b)
        _same_stats(ref_stats, stats, (shape, lanes, wg))


@pytest.mark.parametrize("schedule", [dict(knn_warm_start=False), dict(final_in_successor=False), dict(deferred_finish=False)], ids=lambda d: next(iter(d)))
def test_same_bits_in_the_other_schedules(mla, ctxs, schedule):
    """without the bounded search the prologue launch is the cold form (PRE 1, WARM off); without final_in_successor a chained solve starts behind a chain launch
    (no PRE 2); without the deferred finish only the bounded search is left (PRE 0 warm)"""
    fs, fc = _features(65, 127, seed=11)
    ref = None
    for wg in WIDTHS:
        c = ctxs.get(wg, tag="schedule-" + next(iter(schedule)))
        c.set_gn_schedule(**schedule)
        poses, stats = _solves(mla, c, fs, fc)
        if wg == 256:
            ref = poses, stats
            continue
        for i, (a, b) in enumerate(zip(ref[0], poses)):
            assert _bits(a) == _bits(b), (schedule, wg, "solve form", i, a, b)
        _same_stats(ref[1], stats, (schedule, wg))


def _tiles256(mla, c, ms, mc):
    return sum((m + 256 // c.map_info(k)["knn_lanes"] - 1) // (256 // c.map_info(k)["knn_lanes"]) for k, m in ((mla.SURF, ms), (mla.CORNER, mc)) if m)


def test_rule_keeps_a_small_launch_narrow(mla, ctxs):
    """20 features: two 256-thread workgroups -- far fewer than compute units, so the rule leaves the launch on the 256-thread kernel"""
    c = ctxs.get()
    fs, fc = _features(12, 8, seed=3)
    _stage(mla, c, fs, fc)
    c.gn_solve(P_START, 5, want_stats=False)
    assert _tiles256(mla, c, 12, 8) <= c.info()["cu_solver"]
    assert ctxs.width_taken(c) == 256


def test_rule_counts_the_solver_streams_compute_units(mla, ctxs):
    """900 features are 57 workgroups of 256 threads: at most one per compute unit on the whole device, more than one on a solver stream masked to 32. The masked
    context goes wide, the unmasked one does not, and the pose has the same bits. A frame with more 256-thread workgroups than the device has compute units
    goes wide on the unmasked context too."""
    full, masked, narrow = ctxs.get(), ctxs.get(cu_mask="ffffffff"), ctxs.get(256)
    assert masked.info()["cu_solver"] == 32 and full.info()["cu_solver"] == full.info()["cu_count"]
    fs, fc = _features(600, 300, seed=4)
    poses = []
    for c in (full, masked):
        _stage(mla, c, fs, fc)
        poses.append(c.gn_solve(P_START, 5, want_stats=False)[0])
        t = _tiles256(mla, c, 600, 300)
        assert ctxs.width_taken(c) == (WIDE_DEFAULT if t > c.info()["cu_solver"] else 256)
    assert 32 < _tiles256(mla, masked, 600, 300) <= full.info()["cu_count"] or full.info()["cu_count"] < 57
    assert ctxs.width_taken(masked) == WIDE_DEFAULT
    assert _bits(poses[0]) == _bits(poses[1])
    # a frame-sized launch
    m_big = 40 * full.info()["cu_count"]
    fs, fc = _features(m_big, 300, seed=5)
    poses = []
    for c in (full, narrow):
        _stage(mla, c, fs, fc)
        poses.append(c.gn_solve(P_START, 5, want_stats=False)[0])
    assert _tiles256(mla, full, m_big, 300) > full.info()["cu_solver"]
    assert ctxs.width_taken(full) == WIDE_DEFAULT and ctxs.width_taken(narrow) == 256
    assert _bits(poses[0]) == _bits(poses[1])


def test_blocks_solve_stays_narrow(mla, ctxs):
    """a solve over two pose blocks (padding slots between the blocks) has no wide form: under MLH_KNN_WG_THREADS=1024 it runs the kernels it runs under =256"""
    fs, fc = _features(300, 129, seed=6)
    out = []
    for wg in (256, 1024):
        c = ctxs.get(wg, tag="blocks")
        before = ctxs.width_taken(c)
        c.features_set_blocks(mla.SURF, [fs[:170], fs[170:]])
        c.features_set_blocks(mla.CORNER, [fc[:70], fc[70:]])
        poses, _ = c.gn_solve_blocks(np.stack([P_START, np.array([0, 0, 0, 0, 0, 0, 1.0])]), 3, [5, 5], [100.0, 100.0], [0, 0], want_stats=False)
        assert ctxs.width_taken(c) == before
        out.append(poses)
    assert _bits(out[0]) == _bits(out[1])


def test_width_from_the_environment_is_checked(mla):
    os.environ["MLH_KNN_WG_THREADS"] = "768"
    try:
        with pytest.raises(mla.MlhError):
            mla.Context(0)
    finally:
        os.environ.pop("MLH_KNN_WG_THREADS", None)
