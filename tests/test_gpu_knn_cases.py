"""The mapper's index build (grid.hip) and its 5-NN / 10-NN searches (knn_dev.hpp) on the crafted maps of tests/knn_cases.py, held to the brute-force
reference knn_cases.brute_knn (tests/test_knn_cases.py holds the same cases to the oracle on the CPU).

The bar, for every query and every rank t: where the reference's squared distance is below min_match_sq_dis, the kernel's index (through mlh_knn) or point
(through the neighbour records, mlh_match_neighbours) is the reference's and the distance has the reference's bits; everywhere else the kernel reports a
distance of at least min_match_sq_dis, or none (+inf / index -1). The matching kernels answer a feature with fewer than K points in its 27 cells with no
record at all. Before the kernel is looked at, the reference has to agree with what the case declares per query."""
import functools
import os

import numpy as np
import pytest

import knn_cases as kc
from test_knn_cases import bounded_reference

pytestmark = pytest.mark.gpu

F32 = np.float32
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
LANES = ("8", "16", "32")
BUILD, SEARCH = kc.build_case_names(), kc.search_case_names()
ERR_HIP = -2


def _stop_on_device_error(fn):
    """a HIP error ends the session: nothing more is started on a device that has just reported one"""
    @functools.wraps(fn)
    def run(*args, **kw):
        try:
            return fn(*args, **kw)
        except Exception as e:
            if type(e).__name__ == "MlhError" and f"mlh error {ERR_HIP}:" in str(e):
                pytest.exit(f"{fn.__name__}: {e}", returncode=3)
            raise
    return run


def _m4(a):
    out = np.zeros((len(a), 4), F32)
    out[:, :3] = a[:, :3]
    return out


def _context(mla, lanes=None):
    if lanes is None:
        return mla.Context(0)
    os.environ["MLH_KNN_LANES"] = lanes
    try:
        return mla.Context(0)
    finally:
        os.environ.pop("MLH_KNN_LANES", None)


_bits = kc.bits


def _check_knn(ctx, kind, cloud, queries, n_inside, sq, where):
    idx, d2 = ctx.knn(kind, queries)
    kc.check_knn(idx, d2, cloud, queries, n_inside, sq, where)


_check_records = kc.check_records


def _refused(mla, code, text, fn, *args, **kw):
    with pytest.raises(mla.MlhError) as e:
        fn(*args, **kw)
    assert f"mlh error {code}:" in str(e.value) and text in str(e.value), str(e.value)


# ---------------------------------------------------------------- the index build, answered through mlh_knn
@pytest.mark.parametrize("name", BUILD)
@_stop_on_device_error
def test_index_build(mla, name):
    case = kc.case_by_name(name)
    ctx = _context(mla)
    last = {}
    try:
        for i, st in enumerate(case["steps"]):
            where = f"{name} step {i} ({st['op']}: {st['note']})"
            op, kind, sq = st["op"], st["kind"], st["sq"]
            if op == "map_set":
                if st["error"]:
                    _refused(mla, *st["error"], ctx.map_set, kind, _m4(st["cloud"]), sq)
                    assert ctx.map_info(kind)["n"] == 0, where                    # a refusal leaves the kind without an index
                    continue
                ctx.map_set(kind, _m4(st["cloud"]), sq)
                last[kind] = st["cloud"]
                assert ctx.map_info(kind)["n"] == len(st["cloud"])
            elif op == "map_set_pair":
                if st["error"]:
                    _refused(mla, *st["error"], ctx.map_set_pair, _m4(st["surf"]), _m4(st["corner"]), sq)
                    continue
                ctx.map_set_pair(_m4(st["surf"]), _m4(st["corner"]), sq)
                _check_knn(ctx, mla.CORNER, st["corner"], st["q_corner"], st["n_inside_corner"], sq, where + " corner")
                _check_knn(ctx, mla.SURF, st["surf"], st["queries"], st["n_inside"], sq, where + " surf")
                continue
            elif op == "rebuild":
                if st["error"]:
                    _refused(mla, *st["error"], ctx.map_rebuild, kind)
                    continue
                ctx.map_rebuild(kind)
            elif op == "knn_refused":
                _refused(mla, *st["error"], ctx.knn, kind, np.zeros((1, 3), F32))
                continue
            elif op == "match_exceeds":
                ctx.features_set(kind, _m4(last[kind][:8]))
                _refused(mla, *st["error"], ctx.match_linearize, kind, IDENT, dense=False, min_match_sq_dis=sq)
                continue
            else:
                raise AssertionError(op)
            _check_knn(ctx, kind, st["cloud"], st["queries"], st["n_inside"], sq, where)
    finally:
        ctx.close()


# ---------------------------------------------------------------- the search regimes: the records of the matching kernels, and mlh_knn
@pytest.mark.parametrize("name", SEARCH)
@_stop_on_device_error
def test_search_regime(mla, orc, name):
    case = kc.case_by_name(name)
    cloud, feats, k, sq = case["cloud"], case["feats"], case["k"], case["sq"]
    f4 = _m4(feats)
    rv, rco = orc.Map(_m4(cloud)).match("s", f4, IDENT, n_neigh=k, min_match_sq_dis=sq)
    fixed = case["expect"] >= 0
    records = {}
    for lanes in LANES:
        where = f"{name}, {lanes} lanes"
        ctx = _context(mla, lanes)
        try:
            ctx.map_set(mla.SURF, _m4(cloud), sq)
            ctx.features_set(mla.SURF, f4)
            _refused(mla, kc.ERR_STATE, "match first", ctx.match_neighbours, mla.SURF)      # nothing matched since the features were staged
            got = ctx.match_linearize(mla.SURF, IDENT, dense=False, k_neigh=k, min_match_sq_dis=sq)
            rec = ctx.match_neighbours(mla.SURF)
            assert rec.shape == (len(feats), k, 4), rec.shape
            _check_records(rec, k, cloud, feats, case["n27"], case["n_inside"], sq, where)
            full = (case["n_inside"] == k)[:, None] & fixed                         # ... and the indices written down with the construction
            assert np.array_equal(_bits(rec[..., :3][full]), _bits(cloud[case["expect"][full], :3])), where
            assert np.array_equal(got["valid"], rv), where
            mm = rv.astype(bool)
            assert np.array_equal(_bits(got["coeffs"][mm]), _bits(rco[mm])), where
            if k == 5:
                _check_knn(ctx, mla.SURF, cloud, feats, case["n_inside"], sq, where)
            records[lanes] = rec
        finally:
            ctx.close()
    for lanes in LANES[1:]:
        assert np.array_equal(_bits(records[lanes]), _bits(records[LANES[0]])), f"{name}: {lanes} lanes differ from {LANES[0]}"


# ---------------------------------------------------------------- the bounded search of iterations >= 1
SCHEDULES = ((0, 0, 0), (0, 1, 0), (1, 1, 0))


@_stop_on_device_error
def test_bounded_search_records(mla, orc):
    """the records a solve of n = 2 and 3 iterations leaves are those of a search from the pose n - 1 iterations gave: bit-equal with and without the bound
    (and with the finish in the consumer), at 8, 16 and 32 lanes, and brute_knn's wherever its distance is inside the radius"""
    case = kc.bounded_case()
    _, _, behaves = bounded_reference(orc, case)
    assert all(any(v) for v in behaves.values()) and sorted(behaves) == ["a", "b", "c", "d"], behaves
    maps = {mla.SURF: case["surf_map"], mla.CORNER: case["corner_map"]}
    feats = {mla.SURF: case["f4s"], mla.CORNER: case["f4c"]}
    grids = {kd: kc.grid_rule(m, case["sq"]) for kd, m in maps.items()}
    first = None
    for lanes in LANES:
        for sched in SCHEDULES:
            where = f"{lanes} lanes, schedule {sched}"
            ctx = _context(mla, lanes)
            try:
                ctx.set_gn_schedule(*sched)
                ctx.map_set_pair(_m4(maps[mla.SURF]), _m4(maps[mla.CORNER]), case["sq"])
                for kd in maps:
                    ctx.features_set(kd, feats[kd])
                run = {"pose": {}, "rec": {}}
                for n in (1, 2, 3):
                    run["pose"][n] = ctx.gn_solve(case["p0"], n, want_stats=False)[0]
                    run["rec"][n] = {kd: ctx.match_neighbours(kd) for kd in maps}
            finally:
                ctx.close()
            if first is None:
                first = run
                for n in (2, 3):
                    for kd in maps:
                        xq = orc.associate_to_map(feats[kd], run["pose"][n - 1])
                        n27 = grids[kd].counts27(maps[kd], xq)
                        _, rd2 = kc.brute_knn(maps[kd], xq, 5)
                        _check_records(run["rec"][n][kd], 5, maps[kd], xq, n27, (rd2 < F32(case["sq"])).sum(axis=1), case["sq"], f"{where}, n = {n}, kind {kd}")
            for n in (1, 2, 3):
                assert np.array_equal(run["pose"][n], first["pose"][n]), (where, n)
                for kd in maps:
                    assert np.array_equal(_bits(run["rec"][n][kd][:, :5]), _bits(first["rec"][n][kd][:, :5])), (where, n, kd)
