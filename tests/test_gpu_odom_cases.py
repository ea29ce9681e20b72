"""The odometry window's coupled solve (odom.hip: odom_ne_kernel, odom_ne_finish_kernel, odom_window_solve_kernel behind mlh_pure_odom_set / _normal_eq /
_gn_solve) on the crafted windows of tests/odom_cases.py, held to the float64 reference there (window_system / window_gn; tests/test_odom_cases.py holds the cases,
the reference's agreement with the oracle, the conditions the pose bar rests on and the mutants on the CPU).

Bars, each against the reference and never against the device: H per 6 x 6 block within 1e-9 of the block's largest |reference| entry, a block that is exactly
zero in the reference exactly zero here, H bit-symmetric; g per entry within 1e-9 of the largest sum of absolute terms in its block (g cancels); cost 1e-9
relative; count equal; poses after mlh_pure_odom_gn_solve within 1e-9 absolute (cond <= 1e6 and steps <= 0.2, asserted on the CPU, leave a backward-stable
Cholesky about cond * eps * |step| = 4e-11 per iteration). Every result is bit-equal on a second call and on a fresh context. Every test prints
`ODOM_MEASURED name: quantity value bar` before it asserts; tests/golden/odom_tolerances.json records the values measured on an MI355X beside the bars."""
import re

import numpy as np
import pytest

import odom_cases as oc
from test_gpu_knn_cases import _stop_on_device_error

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED = 0, -1, -2, -5


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_system(a, b):
    return np.array_equal(_bits(a["H"]), _bits(b["H"])) and np.array_equal(_bits(a["g"]), _bits(b["g"])) and _bits(a["cost"]) == _bits(b["cost"]) and a["count"] == b["count"]


def _same_solve(a, b):
    return (np.array_equal(_bits(a["frames"]), _bits(b["frames"])) and np.array_equal(_bits(a["exts"]), _bits(b["exts"])) and _bits(a["cost"]) == _bits(b["cost"])
            and (a["count"], a["status"]) == (b["count"], b["status"]))


def _held(name, measured):
    for k, (v, bar) in measured.items():
        print(f"ODOM_MEASURED {name}: {k} {v:.3e} bar {bar:.1e}")
    assert oc.within(measured), (name, measured)


def _rc(mla, fn, *a, **kw):
    """the return code of a call made through the Context"""
    try:
        fn(*a, **kw)
        return OK
    except mla.MlhError as e:
        code = int(re.match(r"mlh error (-?\d+):", str(e)).group(1))
        if code == ERR_HIP:
            raise
        return code


def _normal_eq(c, w, hd, n_ext=None):
    return c.pure_odom_normal_eq(w["pivot"], w["frames"], w["exts"][:n_ext], huber_delta=hd)


def _fresh_normal_eq(mla, w, hd, n_ext=None):
    c = mla.Context(0)
    try:
        c.pure_odom_set(*oc.table(w))
        return _normal_eq(c, w, hd, n_ext)
    finally:
        c.close()


def _solve(c, a, w=None):
    w = a["w"] if w is None else w
    return c.pure_odom_gn_solve(w["pivot"], w["frames"], w["exts"], n_iters=a["n_iters"], huber_delta=1.0, const_blocks=a["const_blocks"], V_update=a["V"])


def _staged(mla, a):
    c = mla.Context(0)
    c.pure_odom_set(*oc.table(a["w"]))
    if a["prior"] is not None:
        c.window_prior_set(a["prior"]["block_ids"], a["prior"]["x0"], a["prior"]["J0"], a["prior"]["r0"])
    return c


@pytest.mark.parametrize("name", list(oc.SYSTEMS))
@_stop_on_device_error
def test_normal_equations(mla, name):
    """mlh_pure_odom_normal_eq at every window's linearisation point: tile groups of 1, 255, 256, 257 and 513 factors, empty extrinsic and frame blocks, the Huber
    outlier branch on more than 40 % of the rows with the planted ones, negated quaternions, a half turn, frame = pivot, and 22 blocks (D = 132, 110 tiles)"""
    fn, hd = oc.SYSTEMS[name]
    w, ref = fn(), oc.system_reference(name)
    at = oc.negated(w) if name == "poses negated" else w
    c = mla.Context(0)
    try:
        c.pure_odom_set(*oc.table(at))
        got = _normal_eq(c, at, hd)
        _held(name, oc.measure_system(got, ref))
        assert _same_system(_normal_eq(c, at, hd), got), name
        assert _same_system(_fresh_normal_eq(mla, at, hd), got), name
        if name.startswith("ragged"):
            # the same factors sorted by group and reversed: inside the bars again (another summation order), the same order twice the same bits
            for order in ("sorted", "reversed"):
                wo = oc.reordered(w, order)
                c.pure_odom_set(*oc.table(wo))
                other = _normal_eq(c, wo, hd)
                _held(f"{name} {order}", oc.measure_system(other, ref))
                assert _same_system(_normal_eq(c, wo, hd), other) and _same_system(_fresh_normal_eq(mla, wo, hd), other), (name, order)
            c.pure_odom_set(*oc.table(w))
            assert _same_system(_normal_eq(c, w, hd), got), name                               # ... and back
        if name == "sparse_ext":
            for b in (4, 6):                                                                      # extrinsics 1 and 3 have no factor: exactly zero rows, columns and gradient
                assert not got["H"][6 * b:6 * b + 6, :].any() and not got["H"][:, 6 * b:6 * b + 6].any() and not got["g"][6 * b:6 * b + 6].any()
        if name == "empty_frame":
            assert not got["H"][12:18, :].any() and not got["H"][:, 12:18].any() and not got["g"][12:18].any()
        if name == "huber":
            p = w["planted"]
            r, J = c.pure_odom_evaluate(w["pivot"], w["frames"], w["exts"])
            assert r[p["on_plane"]] == 0.0 and r[p["on_line"]] == 0.0 and not J[p["on_line"]].any() and r[p["w0"]] == 0.0 and not J[p["w0"]].any()
            assert abs(r[p["far"]]) > 0.99e6 * oc.HUBER_DELTA
            # no loss: delta = 0 and delta = 1e9 never take the outlier branch -- the same bits, inside the bars of the reference without a loss
            a, b = _normal_eq(c, w, 0.0), _normal_eq(c, w, 1e9)
            assert _same_system(a, b)
            _held("huber no loss", oc.measure_system(a, oc.window_system(w, w["pivot"], w["frames"], w["exts"], 0.0)))
    finally:
        c.close()


@_stop_on_device_error
def test_sparse_ext_rekeys_the_tile_groups_both_ways(mla):
    """the table names extrinsics 0 and 2; one context is called with n_ext = 3, 4, 3: every call re-keys the tile groups for its extrinsic count
    (odom_ne_prepare) and has the bits of a fresh context's call of that shape"""
    w = oc.sparse_ext()
    fresh = {n: _fresh_normal_eq(mla, w, 1.0, n) for n in (3, 4)}
    assert fresh[3]["H"].shape == (36, 36) and fresh[4]["H"].shape == (42, 42)
    assert np.array_equal(_bits(fresh[3]["H"]), _bits(fresh[4]["H"][:36, :36])) and fresh[3]["count"] == fresh[4]["count"] == len(w["types"])
    c = mla.Context(0)
    try:
        c.pure_odom_set(*oc.table(w))
        for k, n in enumerate((3, 4, 3)):
            assert _same_system(_normal_eq(c, w, 1.0, n), fresh[n]), (k, n)
        # two extrinsics do not cover extrinsic 2: refused, and the context goes on
        assert _rc(mla, c.pure_odom_normal_eq, w["pivot"], w["frames"], w["exts"][:2]) == ERR_INVALID
        assert _same_system(_normal_eq(c, w, 1.0, 4), fresh[4])
    finally:
        c.close()


@pytest.mark.parametrize("name", list(oc.SOLVES))
@_stop_on_device_error
def test_gn_solve(mla, name):
    """mlh_pure_odom_gn_solve against window_gn: the default constant blocks, constant blocks in the middle of the free set, a dense V_update per block, empty
    extrinsics held constant, a frame without factors (status 1: the + 1e-6 I second attempt), and the largest window with nf = 120 and -- under a window prior
    on blocks 0 and 1 + n_frames, nothing held constant -- nf = 132"""
    a, ref = oc.solve_args(name), oc.solve_reference(name)
    w = a["w"]
    c = _staged(mla, a)
    try:
        got = _solve(c, a)
        print(f"ODOM_MEASURED {name}: status {got['status']} expected {a['status']}")
        _held(name, dict(oc.measure_poses(got, ref), **{"cost of the last linearisation": (abs(got["cost"] - ref["cost"]) / ref["cost"], oc.COST_BAR)}))
        assert got["status"] == ref["status"] == a["status"] and got["count"] == ref["count"]
        const = (0, 1 + w["n_frames"]) if a["const_blocks"] is None else a["const_blocks"]
        for b in range(1, 1 + w["n_frames"] + w["n_ext"]):
            x0 = w["frames"][b - 1] if b <= w["n_frames"] else w["exts"][b - 1 - w["n_frames"]]
            x1 = got["frames"][b - 1] if b <= w["n_frames"] else got["exts"][b - 1 - w["n_frames"]]
            if b in const:
                assert np.array_equal(_bits(x0), _bits(x1)), (name, b)                            # a constant block comes back bit-equal to its input
            elif name == "empty_frame" and b == 2:
                d = float(np.abs(x1 - x0).max())
                print(f"ODOM_MEASURED {name}: the frame without factors {d:.3e} bar 1.0e-15")
                assert d <= 1e-15                                                                 # (Plus renormalises the quaternion)
            else:
                assert np.abs(x1 - x0).max() > 1e-4, (name, b)
        assert _same_solve(_solve(c, a), got), name
        if name == "empty_frame":
            # status is per call: the ragged window on the same context afterwards is positive definite at the first attempt
            r = oc.solve_args("ragged")
            c.pure_odom_set(*oc.table(r["w"]))
            again = _solve(c, r)
            assert again["status"] == 0
            _held("ragged behind empty_frame", oc.measure_poses(again, oc.solve_reference("ragged")))
        if name == "max_window nf 120":
            # 23 blocks: refused by both entry points, and the 22-block call behind the refusals has the bits of the one before
            fr23 = np.vstack([w["frames"], w["frames"][:1]])
            assert len(fr23) + len(w["exts"]) + 1 == 23
            ne = _normal_eq(c, w, 1.0)
            assert _rc(mla, c.pure_odom_normal_eq, w["pivot"], fr23, w["exts"]) == ERR_UNSUPPORTED
            assert _rc(mla, c.pure_odom_gn_solve, w["pivot"], fr23, w["exts"], n_iters=1) == ERR_UNSUPPORTED
            assert _same_system(_normal_eq(c, w, 1.0), ne) and _same_solve(_solve(c, a), got)
    finally:
        c.close()
    c = _staged(mla, a)
    try:
        assert _same_solve(_solve(c, a), got), (name, "fresh context")
    finally:
        c.close()


@_stop_on_device_error
def test_non_finite_point_skips_every_update(mla):
    """one point's x is NaN: ordinary NaN arithmetic through bounded loops (no index depends on it). The factor's three blocks are NaN in the system, the
    Cholesky's pivot test `!(d > 0)` fails at both attempts of each of the three iterations: MLH_OK with status 2, frames and extrinsics bit-equal to their
    input. The clean table on the same context afterwards solves with a fresh context's bits."""
    a = oc.solve_args("ragged")
    bad = oc.non_finite()
    c = mla.Context(0)
    try:
        c.pure_odom_set(*oc.table(bad))
        ne = _normal_eq(c, bad, 1.0)
        assert np.isnan(ne["H"][6:12, 6:12]).any() or np.isnan(ne["H"][12:18, 12:18]).any()
        got = c.pure_odom_gn_solve(bad["pivot"], bad["frames"], bad["exts"], n_iters=3, huber_delta=1.0)
        print(f"ODOM_MEASURED non_finite: status {got['status']} expected 2")
        assert got["status"] == 2 and got["count"] == len(bad["types"])
        assert np.array_equal(_bits(got["frames"]), _bits(bad["frames"])) and np.array_equal(_bits(got["exts"]), _bits(bad["exts"]))
        c.pure_odom_set(*oc.table(a["w"]))
        clean = _solve(c, a)
    finally:
        c.close()
    c = _staged(mla, a)
    try:
        fresh = _solve(c, a)
    finally:
        c.close()
    assert clean["status"] == 0 and _same_solve(clean, fresh)
    _held("clean table behind non_finite", oc.measure_poses(clean, oc.solve_reference("ragged")))


@_stop_on_device_error
def test_rejected_set_leaves_the_staged_table(mla):
    """mlh_pure_odom_set validates types and block indices before it touches the context or the device: a call rejected for a negative frame or extrinsic index, a
    type that is neither 0 nor 1, or an index no supported window covers (at most 22 blocks: indices beyond 19) returns MLH_ERR_INVALID and
    mlh_pure_odom_normal_eq / mlh_pure_odom_gn_solve go on returning the staged table's results bit for bit"""
    a = oc.solve_args("ragged")
    w, other = a["w"], oc.ragged(True)                                                            # the rejected table is another, larger one
    c = mla.Context(0)
    try:
        c.pure_odom_set(*oc.table(w))
        ne, sol = _normal_eq(c, w, 1.0), _solve(c, a)
        _held("rejected_set before", oc.measure_system(ne, oc.system_reference("ragged")))
        for what, key, value in (("frame_idx = -1", "fi", -1), ("ext_idx = -1", "ei", -1), ("type = 2", "types", 2), ("frame_idx = 20", "fi", 20), ("ext_idx = 21", "ei", 21),
                                 ("frame_idx = 1000", "fi", 1000), ("ext_idx = 1000", "ei", 1000)):
            t = {k: other[k].copy() for k in oc.TABLE_KEYS}
            t[key][-1] = value
            assert _rc(mla, c.pure_odom_set, *oc.table(t)) == ERR_INVALID, what
            assert _same_system(_normal_eq(c, w, 1.0), ne), what
        assert _same_solve(_solve(c, a), sol)
        # the largest indices a window can cover are accepted
        t = {k: w[k].copy() for k in oc.TABLE_KEYS}
        t["fi"][-1] = 19
        assert _rc(mla, c.pure_odom_set, *oc.table(t)) == OK
        c.pure_odom_set(*oc.table(w))
        assert _same_system(_normal_eq(c, w, 1.0), ne)
    finally:
        c.close()


@_stop_on_device_error
def test_device_built_order(mla, orc, synth, case16, feats16):
    """a device-built table whose groups' tiles are NOT contiguous -- (surf, ext 0), (surf, ext 1), (corner, ext 0), (corner, ext 1) at one frame: the run loop of
    odom_ne_finish_kernel -- against the grouped call order, the same correspondences staged through mlh_pure_odom_set, and the reference on them"""
    from scipy.spatial.transform import Rotation as Rot
    to_pose = lambda T: np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
    exts = np.array([oc.IDENT, np.concatenate([[0.3, -0.2, 0.1], oc.mc.rotvec_quat(np.array([0.02, -0.01, 0.4]))])])
    frame, pivot = case16["p0"], oc.IDENT.copy()
    maps = {mla.SURF: orc.Map(case16["surf_map"]), mla.CORNER: orc.Map(case16["corner_map"])}
    feats, rel = {}, [to_pose(synth.pose_to_mat(frame) @ synth.pose_to_mat(e)) for e in exts]
    for kind, f in ((mla.SURF, feats16[0]), (mla.CORNER, feats16[1])):
        half = len(f) // 2
        for n, part in enumerate((f[:half], f[half:])):
            q = part.copy()
            q[:, :3] = synth.transform_points(part[:, :3], np.linalg.inv(synth.pose_to_mat(exts[n])))
            feats[(kind, n)] = np.ascontiguousarray(q)
    interleaved = [(mla.SURF, 0), (mla.SURF, 1), (mla.CORNER, 0), (mla.CORNER, 1)]
    grouped = [(mla.SURF, 0), (mla.CORNER, 0), (mla.SURF, 1), (mla.CORNER, 1)]
    tab = [[], [], [], [], []]
    for kind, n in interleaved:                                                                  # what the device passes must find (oracle-checked elsewhere)
        f = feats[(kind, n)]
        v, co = maps[kind].match("s" if kind == mla.SURF else "c", f, rel[n], n_neigh=5, check_fov=True)
        m = v.astype(bool)
        assert m.sum() > 30
        tab[0].append(np.full(m.sum(), kind, np.int32)); tab[1].append(f[m, :3].astype(np.float64)); tab[2].append(co[m])
        tab[3].append(np.zeros(m.sum(), np.int32)); tab[4].append(np.full(m.sum(), n, np.int32))
    tab = [np.concatenate(x) for x in tab]
    w = dict(types=tab[0], points=tab[1], coeffs=tab[2], fi=tab[3], ei=tab[4], sqrt_info=np.ones(len(tab[0])))
    ref = oc.window_system(w, pivot, frame[None, :], exts, 1.0)
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"]); c.map_set(mla.CORNER, case16["corner_map"])
        out = {}
        for label, order in (("interleaved", interleaved), ("grouped", grouped), ("interleaved again", interleaved)):
            c.pure_odom_begin()
            for kind, n in order:
                c.features_set(kind, feats[(kind, n)])
                c.pure_odom_add_matches(kind, rel[n], 0, n, k_neigh=5, flags=mla.FLAG_CHECK_FOV)
            out[label] = c.pure_odom_normal_eq(pivot, frame[None, :], exts, huber_delta=1.0)
        c.pure_odom_set(*oc.table(w))
        out["host-staged"] = c.pure_odom_normal_eq(pivot, frame[None, :], exts, huber_delta=1.0)
    finally:
        c.close()
    for label in ("interleaved", "grouped", "host-staged"):
        _held(f"device_built_order {label}", oc.measure_system(out[label], ref))
    assert _same_system(out["interleaved again"], out["interleaved"])
    assert all(len(f) > 0 for f in feats.values())                                                # (every add reserves whole tiles: each group's tiles lie apart)

