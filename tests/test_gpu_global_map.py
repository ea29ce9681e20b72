"""(f7) the global map built on the device from the keyframe store: mlh_keyframe_attach_outlier + mlh_global_map_assemble against a short restatement of
pubGlobalMap / saveGlobalMap (lidar_mapper_keyframe.cpp:796-849, 853-901) written in this file over the reference-built calls (oracle/_ref:
cloudUCTAssociateToMap, VoxelGridCovarianceMLOAM), and against the per-keyframe C-ABI loop it replaces (mlh_cloud_uct_associate_to_map per keyframe and kind,
concatenation on the caller's side, mlh_voxel_filter). Inputs: the generator of tests/test_gpu_local_map.py (scene "50k", the 40-frame circle, 16 rings x 900
columns, two LiDARs); a frame's outlier cloud is a strided subset of its surf cloud thinned at 0.8 m. Every test here fails without the feature: the entry
points do not exist."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_local_map as lm
from global_map_cases import select_restated

pytestmark = pytest.mark.gpu

MEAS = lm.MEAS
EMPTY = np.zeros((0, 11), np.float32)
PUBLISH = dict(split=0, radius=1000.0, kf_res=10.0, leaf=0.4)          # pubGlobalMap's values (cpp:805, 839, 1293)
SAVE = dict(split=1, radius=-1.0, kf_res=10.0, leaf=0.8)               # saveGlobalMap's (cpp:865-866, 896)


class GlobalMapRestated:
    """pubGlobalMap (cpp:796-849) and saveGlobalMap (cpp:853-901, without the leftover of cpp:865-866), line by line, over `uct` (cloudUCTAssociateToMap) and
    `vfilter` (VoxelGridCovarianceMLOAM, covariance branch); the keyframe filter is the reference-built plain branch (global_map_cases.select_restated)."""

    def __init__(self, orc, uct, vfilter):
        self.orc, self.uct, self.vfilter = orc, uct, vfilter
        self.keys = []

    def save(self, pose, cov, surf, corner, outlier):
        pos = np.array([pose[0], pose[1], pose[2]], np.float32)
        self.keys.append((np.asarray(pose, np.float64), np.asarray(cov, np.float64), pos, lm._rec11(surf), lm._rec11(corner), lm._rec11(outlier)))

    def assemble(self, pose_cur, ext, ext_cov, o):
        if not self.keys:
            return [], [EMPTY, EMPTY], [EMPTY, EMPTY]
        ids = select_restated(self.orc, np.array([k[2] for k in self.keys]), None if pose_cur is None else pose_cur[:3], o["radius"], o["kf_res"])
        groups = [[3, 4, 5]] if o["split"] == 0 else [[3, 5], [4]]           # cpp:818-827; cpp:872-882
        pre, flt = [], []
        for g in groups:
            parts = []
            for kid in ids:
                kp, kc = self.keys[kid][0], self.keys[kid][1]
                for f in g:
                    if len(self.keys[kid][f]):
                        parts.append(self.uct(self.keys[kid][f], kp, kc, ext, ext_cov, MEAS, o["with_ua"], o["thr"]))
            p = np.concatenate(parts) if parts else EMPTY
            pre.append(p)
            flt.append(self.vfilter(p, o["leaf"], o["thr"]) if len(p) else EMPTY)
        while len(pre) < 2:
            pre.append(EMPTY)
            flt.append(EMPTY)
        return ids, pre, flt


def _opts(mla, o):
    return mla.global_map_opts(kf_radius=o["radius"], kf_res=o["kf_res"], leaf=o["leaf"], split=o["split"], trace_threshold=o["thr"], with_ua=o["with_ua"],
                               cov_measurement=MEAS)


def _ref_restated(orc):
    return GlobalMapRestated(orc, orc.ref_cloud_uct_associate_to_map, lambda x, leaf, t: orc.ref_voxel_filter(x, leaf, t))


def _abi_restated(orc, side):
    return GlobalMapRestated(orc, lambda x, p, c, e, ec, m, w, t: side.cloud_uct_associate_to_map(x, p, c, e, ec, m, w, t),
                             lambda x, leaf, t: side.voxel_filter(x, leaf, t))


def _outlier(orc, surf, k):
    return orc.ref_voxel_filter(np.ascontiguousarray(surf[k % 5::5]), 0.8)


@pytest.fixture(scope="module")
def scene(synth):
    return synth.make_scene(seed=42, **synth.SCENE_PRESETS["50k"])


@pytest.fixture(scope="module")
def world(mla, orc, synth, scene):
    """the circle's keyframes (saveKeyframe's own decisions) with outlier clouds, stored once in a context; a side context for the per-keyframe loop"""
    poses, clouds, covs = lm._sequence(synth, orc, scene, 1.05)
    ext, ext_cov = lm._ext(synth)
    saved = orc.ref_save_keyframes(poses, 1.0, 1.0)
    frames = [t for t in range(len(poses)) if saved[t]]
    assert len(frames) > 20
    keys = [(poses[t], covs[t], clouds[t][0], clouds[t][1], _outlier(orc, clouds[t][0], t)) for t in frames]
    assert all(len(k[4]) > 50 for k in keys)
    ctx, side = mla.Context(0), mla.Context(0)
    for j, k in enumerate(keys):
        assert ctx.keyframe_save(k[0], k[1], k[2], k[3]) == j
        ctx.keyframe_attach_outlier(j, k[4])
    w = dict(ctx=ctx, side=side, keys=keys, ext=ext, ext_cov=ext_cov, cur=poses[frames[-1]])
    yield w
    ctx.close()
    side.close()


def _filled(ref, keys):
    for k in keys:
        ref.save(*k)
    return ref


def _compare(ctx, r, ids, pre, flt, o, exact):
    assert list(r["kf_ids"]) == ids
    for k in range(2):
        for filtered, want in ((False, pre[k]), (True, flt[k])):
            g = ctx.global_map_fetch(k, filtered)
            assert (r["n_ds"] if filtered else r["n_pre"])[k] == len(g)
            assert g.shape == want.shape, (k, filtered, g.shape, want.shape)
            if exact or not o["with_ua"]:
                assert np.array_equal(lm._bits(g), lm._bits(want)), (k, filtered)
            elif not filtered:
                # the tolerances of tests/test_gpu_local_map.py::_run_sequence for the same comparison
                assert np.array_equal(lm._bits(g[:, :4]), lm._bits(want[:, :4])), k
                np.testing.assert_allclose(g[:, 4:], want[:, 4:], rtol=2e-5, atol=1e-9)
            else:
                np.testing.assert_allclose(g[:, :3], want[:, :3], rtol=0, atol=2e-5)
                np.testing.assert_allclose(g[:, 4:], want[:, 4:], rtol=1e-4, atol=1e-9)
                assert len(g) == 0 or np.mean(g[:, 3] == want[:, 3]) > 0.99


MODES = [("publish", PUBLISH), ("publish_1m", dict(PUBLISH, kf_res=1.0)), ("save", SAVE)]


@pytest.mark.parametrize("with_ua", [False, True])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_parity_with_the_reference(mla, orc, world, mode, with_ua):
    """both modes against the restatement over the reference's own lines: the keyframes the map is made of, both pre-filter clouds and both filtered clouds.
    Without uncertainty every field is bit-exact; with it, xyz / intensity of the transformed clouds are bit-exact and the rest agrees to the tolerances
    tests/test_gpu_local_map.py::_run_sequence uses for the same comparison (covariances rtol 2e-5 / atol 1e-9; filtered xyz atol 2e-5, covariances rtol 1e-4,
    intensity equal on more than 99 % of the points)."""
    o = dict(mode[1], with_ua=with_ua, thr=10.0)
    ref = _filled(_ref_restated(orc), world["keys"])
    ids, pre, flt = ref.assemble(world["cur"], world["ext"], world["ext_cov"], o)
    r = world["ctx"].global_map_assemble(world["cur"] if o["radius"] >= 0 else None, world["ext"], world["ext_cov"], _opts(mla, o))
    _compare(world["ctx"], r, ids, pre, flt, o, exact=False)
    assert len(pre[0]) > 10000 and (o["split"] == 0) == (len(pre[1]) == 0)
    if o["kf_res"] == 10.0:
        assert 0 < len(ids) < len(world["keys"])            # keyframes 1 m apart share 10 m position voxels: only each voxel's last member reaches the map
    else:
        assert len(ids) > len(world["keys"]) // 2


@pytest.mark.parametrize("with_ua,thr", [(True, 0.02), (True, 10.0), (False, 0.6)])
@pytest.mark.parametrize("mode", [MODES[1], MODES[2]], ids=["publish_1m", "save"])
def test_equal_to_the_per_keyframe_abi_loop(mla, orc, world, mode, with_ua, thr):
    """the same bits, all 11 fields, as mlh_cloud_uct_associate_to_map per keyframe and kind + mlh_voxel_filter -- a trace threshold that drops points among the cases"""
    o = dict(mode[1], with_ua=with_ua, thr=thr)
    ref = _filled(_abi_restated(orc, world["side"]), world["keys"])
    ids, pre, flt = ref.assemble(world["cur"], world["ext"], world["ext_cov"], o)
    r = world["ctx"].global_map_assemble(world["cur"] if o["radius"] >= 0 else None, world["ext"], world["ext_cov"], _opts(mla, o))
    _compare(world["ctx"], r, ids, pre, flt, o, exact=True)
    stored = sum(len(world["keys"][i][f]) for i in ids for f in (2, 3, 4))
    if with_ua and thr < 1:
        assert 0 < sum(r["n_pre"]) < stored                  # the gate really cut
    else:
        assert sum(r["n_pre"]) == stored


def test_a_radius_that_cuts(mla, orc, world):
    """radius 5 on the circle: the selection is mlh_global_map_select's and the restatement's, and keyframes outside the radius contribute nothing"""
    o = dict(PUBLISH, radius=5.0, kf_res=1.0, with_ua=False, thr=0.6)
    keys = world["keys"]
    centre = keys[len(keys) // 2][0]
    pos = np.array([k[0][:3] for k in keys]).astype(np.float32)
    ref = _filled(_abi_restated(orc, world["side"]), keys)
    ids, pre, flt = ref.assemble(centre, world["ext"], world["ext_cov"], o)
    r = world["ctx"].global_map_assemble(centre, world["ext"], world["ext_cov"], _opts(mla, o))
    assert list(r["kf_ids"]) == ids == list(mla.global_map_select(pos, centre[:3], 5.0, 1.0))
    assert 1 < len(ids) < len(keys)
    assert all(np.linalg.norm(pos[i] - centre[:3].astype(np.float32)) <= 5.0 for i in ids)
    _compare(world["ctx"], r, ids, pre, flt, o, exact=True)
    assert r["n_pre"] == [sum(len(keys[i][f]) for i in ids for f in (2, 3, 4)), 0]


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513]


def _crafted(rng):
    """keyframes whose three clouds run through the sizes where tiling and ranking can go wrong; keyframe 9 gets no outlier cloud; keyframe 0's surf cloud is
    empty; keyframe 4's covariance puts every one of its points over the trace threshold"""
    def cloud(n):
        p = np.zeros((n, 4), np.float32)
        p[:, :3] = rng.uniform(-20, 20, (n, 3))
        p[:, 3] = rng.integers(0, 2, n)
        return p
    keys = []
    for j in range(10):
        yaw = 0.1 * j
        pose = np.array([3.0 * j, 0.5 * np.sin(j), 0.2, 0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])
        cov = np.eye(6) if j == 4 else lm._cov(rng)
        n = (300, 100, 0) if j == 9 else (SIZES[j], SIZES[(j + 3) % 9], SIZES[(j + 6) % 9])
        keys.append((pose, cov, cloud(n[0]), cloud(n[1]), cloud(n[2])))
    return keys


@pytest.mark.parametrize("with_ua,thr", [(True, 0.6), (True, 1e-9), (False, 0.6)])
@pytest.mark.parametrize("mode", [dict(PUBLISH, kf_res=1.0), dict(SAVE, kf_res=1.0), SAVE], ids=["publish", "save", "save_10m"])
def test_crafted_segment_sizes(mla, orc, synth, mode, with_ua, thr):
    """segments of 0, 1, 63, 64, 65, 255, 256, 257 and 513 points mixed over the three kinds, a keyframe without an outlier cloud, one with an empty surf
    cloud, a threshold that drops a whole keyframe's segments and one that drops everything (counts 0, MLH_OK): bit-equal to the per-keyframe C-ABI loop"""
    keys = _crafted(np.random.default_rng(3))
    ext, ext_cov = lm._ext(synth)
    o = dict(mode, with_ua=with_ua, thr=thr)
    ctx, side = mla.Context(0), mla.Context(0)
    try:
        ref = _filled(_abi_restated(orc, side), keys)
        for j, k in enumerate(keys):
            assert ctx.keyframe_save(k[0], k[1], k[2], k[3]) == j
            if j != 9:
                ctx.keyframe_attach_outlier(j, k[4])
        cur = keys[5][0]
        ids, pre, flt = ref.assemble(cur, ext, ext_cov, o)
        r = ctx.global_map_assemble(cur if o["radius"] >= 0 else None, ext, ext_cov, _opts(mla, o))
        _compare(ctx, r, ids, pre, flt, o, exact=True)
        if o["kf_res"] == 1.0:
            assert sorted(ids) == list(range(10))
        if with_ua and thr < 1e-6:
            assert r["n_pre"] == [0, 0] and r["n_ds"] == [0, 0] and len(r["kf_ids"]) == len(ids) > 0
        elif with_ua:
            # keyframe 4 contributes nothing: the map is the map of the store without it
            other = _filled(_abi_restated(orc, side), [k if j != 4 else (k[0], k[1], k[2][:0], k[3][:0], k[4][:0]) for j, k in enumerate(keys)])
            _, pre4, _ = other.assemble(cur, ext, ext_cov, o)
            assert all(np.array_equal(lm._bits(a), lm._bits(b)) for a, b in zip(pre, pre4)) and sum(r["n_pre"]) > 0
            assert 4 in ids or o["kf_res"] != 1.0
        else:
            assert sum(r["n_pre"]) == sum(len(keys[i][f]) for i in ids for f in (2, 3, 4))
    finally:
        ctx.close()
        side.close()


def test_edges(mla, orc, synth, world):
    keys, ext, ext_cov = world["keys"], world["ext"], world["ext_cov"]
    o = dict(PUBLISH, kf_res=1.0, with_ua=True, thr=0.6)
    ctx = mla.Context(0)
    try:
        lib = ctx.lib
        # no keyframes: zeros
        r = ctx.global_map_assemble(keys[0][0], ext, ext_cov, _opts(mla, o))
        assert r["n_pre"] == [0, 0] and r["n_ds"] == [0, 0] and len(r["kf_ids"]) == 0 and ctx.global_map_cloud(0, True).n == 0
        # one keyframe; radius 0 finds it only from its own position
        ctx.keyframe_save(*keys[0][:4])
        ctx.keyframe_attach_outlier(0, keys[0][4])
        one = ctx.global_map_assemble(keys[0][0], ext, ext_cov, _opts(mla, o))
        assert list(one["kf_ids"]) == [0] and 0 < one["n_ds"][0] <= one["n_pre"][0] <= sum(len(keys[0][f]) for f in (2, 3, 4))
        r0 = ctx.global_map_assemble(keys[0][0], ext, ext_cov, _opts(mla, dict(o, radius=0.0)))
        assert list(r0["kf_ids"]) == [0] and r0["n_pre"] == one["n_pre"]
        r0 = ctx.global_map_assemble(keys[1][0], ext, ext_cov, _opts(mla, dict(o, radius=0.0)))
        assert len(r0["kf_ids"]) == 0 and r0["n_pre"] == [0, 0] and r0["n_ds"] == [0, 0]
        # the outlier cloud is attached once; a bad key and bad records are refused
        out4 = np.ascontiguousarray(keys[0][4])
        vp = out4.ctypes.data_as(C.c_void_p)
        assert lib.mlh_keyframe_attach_outlier(ctx.h, 0, vp, len(out4), 16, 12, 0) == -3                  # MLH_ERR_STATE
        assert lib.mlh_keyframe_attach_outlier(ctx.h, 1, vp, len(out4), 16, 12, 0) == -1                  # no such keyframe
        assert lib.mlh_keyframe_attach_outlier(ctx.h, -1, vp, len(out4), 16, 12, 0) == -1
        ctx.keyframe_save(*keys[1][:4])
        assert lib.mlh_keyframe_attach_outlier(ctx.h, 1, None, 5, 16, 12, 0) == -1                        # bad records
        assert lib.mlh_keyframe_attach_outlier(ctx.h, 1, vp, len(out4), 6, 12, 0) == -1
        assert lib.mlh_keyframe_attach_outlier(ctx.h, 1, vp, 0, 16, 12, 0) == 0                           # n == 0 attaches nothing ...
        ctx.keyframe_attach_outlier(1, keys[1][4])                                                        # ... so the cloud can still be attached
        # bad options, with_ua without covariances, n_lidar
        p = np.ascontiguousarray(keys[0][0])
        e, c = np.ascontiguousarray(ext), np.ascontiguousarray(ext_cov)
        n2a, n2b, n = (C.c_int32 * 2)(), (C.c_int32 * 2)(), C.c_int32(0)

        def call(opts, n_lidar=2, cov=c, pose=p):
            return lib.mlh_global_map_assemble(ctx.h, None if pose is None else pose.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                               None if cov is None else cov.ctypes.data_as(C.c_void_p), n_lidar, C.byref(opts), n2a, n2b, None, C.byref(n))
        assert call(_opts(mla, o)) == 0
        for bad in (dict(radius=float("nan")), dict(radius=float("inf")), dict(kf_res=0.0), dict(kf_res=float("nan")), dict(leaf=0.0), dict(leaf=-0.4),
                    dict(leaf=float("nan")), dict(thr=float("nan")), dict(split=2)):
            assert call(_opts(mla, dict(o, **bad))) == -1, bad
        assert call(_opts(mla, o), cov=None) == -1
        assert call(_opts(mla, dict(o, with_ua=False)), cov=None) == 0
        assert call(_opts(mla, o), n_lidar=0) == -1 and call(_opts(mla, o), n_lidar=17) == -1
        assert call(_opts(mla, o), pose=None) == -1 and call(_opts(mla, dict(o, radius=-1.0)), pose=None) == 0
        ptr = C.c_void_p()
        assert lib.mlh_global_map_cloud(ctx.h, 2, 1, C.byref(ptr), C.byref(n)) == -1 and lib.mlh_global_map_cloud(ctx.h, 0, 2, C.byref(ptr), C.byref(n)) == -1
        # two identical calls give identical bits; two more keyframes and the map grows; release and a rebuild gives the same bits
        def snapshot(opts):
            r = ctx.global_map_assemble(keys[0][0], ext, ext_cov, opts)
            return r, [ctx.global_map_fetch(k, f) for k in range(2) for f in (False, True)]
        for mode in (dict(SAVE, kf_res=1.0, with_ua=True, thr=0.6), dict(o)):
            ra, a = snapshot(_opts(mla, mode))
            rb, b = snapshot(_opts(mla, mode))
            assert ra["n_pre"] == rb["n_pre"] and all(np.array_equal(lm._bits(x), lm._bits(y)) for x, y in zip(a, b)) and len(a[1]) > 0
        for j in (2, 3):
            ctx.keyframe_save(*keys[j][:4])
            ctx.keyframe_attach_outlier(j, keys[j][4])
        rc_, grown = snapshot(_opts(mla, o))
        assert sorted(rc_["kf_ids"]) == [0, 1, 2, 3] and rc_["n_pre"][0] > ra["n_pre"][0] and rc_["n_ds"][0] > 0
        ctx.global_map_release()
        assert ctx.global_map_cloud(0, True).n == 0 and ctx.global_map_cloud(0, False).n == 0
        rd, again = snapshot(_opts(mla, o))
        assert rd["n_pre"] == rc_["n_pre"] and all(np.array_equal(lm._bits(x), lm._bits(y)) for x, y in zip(grown, again))
        # mlh_keyframes_reset empties it
        ctx.keyframes_reset()
        assert all(ctx.global_map_cloud(k, f).n == 0 for k in range(2) for f in (False, True))
        r = ctx.global_map_assemble(keys[0][0], ext, ext_cov, _opts(mla, o))
        assert r["n_pre"] == [0, 0] and len(r["kf_ids"]) == 0
    finally:
        ctx.close()


def test_the_local_map_does_not_notice(mla, orc, synth, scene):
    """the first frames of the local-map sequence on two contexts, one of which builds the global map (both modes) between every pair of mlh_local_map_assemble
    calls -- also while one kind filters to empty and the `+=` of the reference keeps appending: every local-map cloud, flag and id list is bit-identical"""
    poses, clouds, covs = lm._sequence(synth, orc, scene, 1.05)
    ext, ext_cov = lm._ext(synth)
    saved = orc.ref_save_keyframes(poses, 1.0, 1.0)
    lo = lm._opts(mla, dict(lm.BASE, with_ua=True, thr=0.6))
    g_pub = _opts(mla, dict(PUBLISH, kf_res=1.0, with_ua=True, thr=0.6))
    g_save = _opts(mla, dict(SAVE, with_ua=True, thr=0.6))
    a, b = mla.Context(0), mla.Context(0)

    def same(t):
        for k in range(2):
            for f in (False, True):
                x, y = a.local_map_fetch(k, f), b.local_map_fetch(k, f)
                assert x.shape == y.shape and np.array_equal(lm._bits(x), lm._bits(y)), (t, k, f)

    def both_global(pose):
        r = a.global_map_assemble(pose, ext, ext_cov, g_pub)
        s = a.global_map_assemble(None, ext, ext_cov, g_save)
        return r, s
    try:
        n_rebuilt = 0
        for t in range(14):
            ra, rb = a.local_map_assemble(poses[t], ext, ext_cov, lo), b.local_map_assemble(poses[t], ext, ext_cov, lo)
            assert ra["rebuilt"] == rb["rebuilt"] and list(ra["kf_ids"]) == list(rb["kf_ids"]) and (ra["n_surf_ds"], ra["n_corner_ds"]) == (rb["n_surf_ds"], rb["n_corner_ds"])
            n_rebuilt += ra["rebuilt"]
            same(t)
            g, s = both_global(poses[t])
            same(t)                                         # ... and the global call left the local clouds alone
            if saved[t]:
                for c in (a, b):
                    c.keyframe_save(poses[t], covs[t], clouds[t][0], clouds[t][1])
                    c.local_map_clear()
                a.keyframe_attach_outlier(a.local_map_info()["n_keyframes"] - 1, _outlier(orc, clouds[t][0], t))
        assert n_rebuilt > 5 and sum(g["n_pre"]) > 0 and s["n_pre"][1] > 0
        # keyframes without corners: the corner map filters to empty, every call rebuilds and appends again (`+=`)
        for c in (a, b):
            c.keyframes_reset()
            for t in (0, 1):
                c.keyframe_save(poses[t], covs[t], clouds[t][0], np.zeros((0, 4), np.float32))
        lens = []
        for rep in range(3):
            ra, rb = a.local_map_assemble(poses[0], ext, ext_cov, lo), b.local_map_assemble(poses[0], ext, ext_cov, lo)
            assert ra["rebuilt"] and rb["rebuilt"] and ra["n_corner_ds"] == 0 and list(ra["kf_ids"]) == list(rb["kf_ids"])
            same(("+=", rep))
            g, s = both_global(poses[0])
            assert g["n_pre"][0] > 0 and s["n_pre"][1] == 0
            same(("+=", rep))
            lens.append(a.local_map_cloud(mla.SURF, False).n)
        assert lens == [lens[0], 2 * lens[0], 3 * lens[0]] and lens[0] > 0
    finally:
        a.close()
        b.close()


def test_globalmap_selftest_equals_the_per_keyframe_loop():
    """m-loam_amd/host/globalmap_selftest: keyframes with outlier clouds saved through the facade's KeyframeMap, pubGlobalMap and saveGlobalMap built on the
    device and compared bit for bit with the per-keyframe C-ABI loop on a second context"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "globalmap_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/globalmap_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "the device maps equal the per-keyframe loop's" in r.stdout
