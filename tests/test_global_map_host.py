"""(f7) the host side of the global map, without a GPU: mlh_global_map_opts_default gives pubGlobalMap's / saveGlobalMap's values
(lidar_mapper_keyframe.cpp:805, 839, 896, 1293; lidar_mapper.h:81), mlh_global_map_select restates the keyframe selection of cpp:804-810 / 865-868 -- held
against the radius rule + the reference-built VoxelGridCovarianceMLOAM<PointI> with intensity = the keyframe's index --, and the new entry points refuse a
null context."""
import ctypes as C

import numpy as np
import pytest

from global_map_cases import circle_positions, select_restated

MAP_SURF_RES = 0.4


def test_opts_default_are_the_references_values(mla):
    pub, save = mla.global_map_opts(False), mla.global_map_opts(True)
    assert (pub.kf_radius, pub.kf_res, pub.leaf, pub.split) == (1000.0, 10.0, np.float32(MAP_SURF_RES), 0)
    assert save.kf_radius < 0 and (save.kf_res, save.leaf, save.split) == (10.0, np.float32(2 * MAP_SURF_RES), 1)
    for o in (pub, save):
        assert o.trace_threshold == 0.6 and o.with_ua == 1
        assert np.array_equal(np.array(o.cov_measurement).reshape(3, 3), np.diag([0.0025] * 3))
    assert mla.global_map_opts(True, leaf=1.5, with_ua=False).leaf == 1.5 and mla.global_map_opts(with_ua=False).with_ua == 0


def _cases():
    circle = circle_positions()
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = np.arange(40) - 3.5          # 1 m apart, crossing 10 m voxel borders (and zero)
    line[:, 1] = 0.25
    c = np.array([5.0, 5.0, 5.0], np.float32)
    ring = np.array([c + d for d in ([1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1], [2, 0, 0], [0, -2, 0])], np.float32)
    return circle, line, c, ring


def test_select_equals_the_restatement(mla, orc):
    if orc.ref_lib() is None:
        pytest.skip("no reference build")
    circle, line, c, ring = _cases()
    n_cut = 0
    for center in (circle[0], circle[17], np.array([-6.0, 0.0, 0.3], np.float32)):
        for radius, res in ((1000.0, 10.0), (1000.0, 1.0), (5.0, 1.0), (5.0, 0.01), (2.0, 10.0)):
            got = list(mla.global_map_select(circle, center, radius, res))
            want = select_restated(orc, circle, center, radius, res)
            assert got == want, (center, radius, res)
            n_cut += len(got) < len(circle)
    assert n_cut > 0
    # keyframes 1 m apart share 10 m voxels: only each voxel's last member (std::sort order) is selected
    got = list(mla.global_map_select(line, line[20], 1000.0, 10.0))
    assert got == select_restated(orc, line, line[20], 1000.0, 10.0)
    assert len(got) == len({int(np.floor(x / 10.0)) for x in line[:, 0]}) < len(line)
    # equal distances: by index
    for radius in (1.0, 2.0, 1.5):
        for res in (10.0, 0.5):
            assert list(mla.global_map_select(ring, c, radius, res)) == select_restated(orc, ring, c, radius, res), (radius, res)
    assert sorted(mla.global_map_select(ring, c, 1.0, 0.5)) == [0, 1, 2, 3, 4, 5]
    # radius 0: only a keyframe exactly at the centre; radius < 0: every keyframe in index order, no centre needed
    assert list(mla.global_map_select(circle, circle[7], 0.0, 10.0)) == select_restated(orc, circle, circle[7], 0.0, 10.0) == [7]
    assert list(mla.global_map_select(circle, circle[7] + np.float32(0.5), 0.0, 10.0)) == []
    for res in (10.0, 1.0, 0.01):
        assert list(mla.global_map_select(circle, None, -1.0, res)) == select_restated(orc, circle, None, -1.0, res), res
        assert list(mla.global_map_select(line, None, -1.0, res)) == select_restated(orc, line, None, -1.0, res), res
    assert sorted(mla.global_map_select(circle, None, -1.0, 0.01)) == list(range(len(circle)))


def test_select_edges(mla):
    assert list(mla.global_map_select(np.zeros((0, 3), np.float32), np.zeros(3, np.float32), 1000.0, 10.0)) == []
    assert list(mla.global_map_select(np.zeros((0, 3), np.float32), None, -1.0, 10.0)) == []
    pos = circle_positions()
    for bad in (dict(kf_res=0.0), dict(kf_res=-1.0), dict(kf_res=float("nan")), dict(kf_radius=float("nan")), dict(kf_radius=float("inf"))):
        args = dict(kf_radius=1000.0, kf_res=10.0)
        args.update(bad)
        with pytest.raises(mla.MlhError):
            mla.global_map_select(pos, pos[0], args["kf_radius"], args["kf_res"])
    with pytest.raises(mla.MlhError):
        mla.global_map_select(pos, None, 5.0, 10.0)          # a radius search needs the centre


def test_new_entry_points_refuse_a_null_context(mla):
    lib = mla.load_library()
    o = mla.global_map_opts()
    n2a, n2b, n = (C.c_int32 * 2)(), (C.c_int32 * 2)(), C.c_int32(0)
    ext = np.array([0, 0, 0, 0, 0, 0, 1.0])
    assert lib.mlh_global_map_assemble(None, None, ext.ctypes.data_as(C.c_void_p), None, 1, C.byref(o), n2a, n2b, None, C.byref(n)) != 0
    ptr = C.c_void_p()
    assert lib.mlh_global_map_cloud(None, 0, 1, C.byref(ptr), C.byref(n)) != 0
    pts = np.zeros((4, 4), np.float32)
    assert lib.mlh_keyframe_attach_outlier(None, 0, pts.ctypes.data_as(C.c_void_p), 4, 16, 12, 0) != 0
    assert lib.mlh_global_map_release(None) != 0
