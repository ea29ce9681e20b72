"""The odometry's sliding window in HBM (mlh_window_*): the store, slideWindow as CircularBuffer::push, and buildLocalMap / buildCalibMap in one call, against the
per-call loop over the existing ABI (mlh_transform_point_cloud + mlh_voxel_grid) and against the oracle, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -3
W3 = 3


def _fill(ctx, clouds, window):
    """clouds[n][slot] = (surf, corner) -> a fresh store with every slot set"""
    ctx.window_reset(len(clouds), window)
    for n, per_slot in enumerate(clouds):
        for slot, (s, c) in enumerate(per_slot):
            ctx.window_set(n, slot, s, c)


def _check_maps(mla, ctx, orc, clouds, poses, window, source_lidar, leaf_surf, leaf_corner, n_scans=16, need_thinning=True):
    n_lidar = len(clouds)
    o = mla.window_map_opts(n_scans, n_lidar, window, source_lidar=source_lidar, leaf_surf=leaf_surf, leaf_corner=leaf_corner)
    ls, lc = list(o.leaf_surf)[:n_lidar], list(o.leaf_corner)[:n_lidar]
    r = ctx.window_build_local_map(poses, o)
    got = [[(ctx.window_map_fetch(n, k, False), ctx.window_map_fetch(n, k, True)) for k in range(2)] for n in range(n_lidar)]
    abi = wc.loop_maps(ctx.transform_point_cloud, ctx.voxel_grid, clouds, poses, window, source_lidar, ls, lc)
    ref = wc.loop_maps(orc.transform_point_cloud, orc.voxel_grid, clouds, poses, window, source_lidar, ls, lc)
    for n in range(n_lidar):
        for k in range(2):
            for f in range(2):
                assert wc.same_bits(got[n][k][f], abi[n][k][f]), ("per-call loop", n, k, f, got[n][k][f].shape, abi[n][k][f].shape)
                assert wc.same_bits(got[n][k][f], ref[n][k][f]), ("oracle", n, k, f)
            assert (r["n_pre"][n, k], r["n_ds"][n, k]) == (len(abi[n][k][0]), len(abi[n][k][1]))
            if need_thinning:
                assert 0 < r["n_ds"][n, k] < r["n_pre"][n, k], (n, k, r)
    return r


@pytest.fixture(scope="module")
def drive():
    return wc.drive(4, 2)


def _drive_clouds(d, n_lidar=2, frames=range(4)):
    return [[d["stack"][f][n] for f in frames] for n in range(n_lidar)]


@pytest.mark.parametrize("mode", ["local", "calib"])
def test_build_equals_the_per_call_loop_and_the_oracle(mla, orc, drive, mode):
    """window 3, two LiDARs, every (n, i) its own pose_local: the pre-filter and the filtered clouds of both modes -- buildLocalMap's one ratio from the stacks of
    each LiDAR; buildCalibMap's stacks of LiDAR 0 for every map at 0.4 (reference LiDAR) / 0.2 -- equal the loop over the existing ABI and the oracle's"""
    clouds = _drive_clouds(drive)
    poses = wc.pose_local(drive, 1, range(4), 2)
    ctx = mla.Context(0)
    try:
        _fill(ctx, clouds, W3)
        if mode == "local":
            r = _check_maps(mla, ctx, orc, clouds, poses, W3, -1, None, None)
            assert len({tuple(x) for x in r["n_pre"]}) == 2               # the two LiDARs' maps are made of different stacks
        else:
            r = _check_maps(mla, ctx, orc, clouds, poses, W3, 0, [0.4, 0.2], [0.4, 0.2])
            assert tuple(r["n_pre"][0]) == tuple(r["n_pre"][1]) and tuple(r["n_ds"][0]) != tuple(r["n_ds"][1])
        # the stacks are left untouched
        for n in range(2):
            for slot in range(4):
                for k in range(2):
                    assert wc.same_bits(ctx.window_fetch(n, slot, k), clouds[n][slot][k])
    finally:
        ctx.close()


def _crafted(rng, n):
    a = np.empty((n, 4), np.float32)
    a[:, :3] = rng.uniform(-20, 20, (n, 3))
    a[:, 3] = rng.uniform(0, 16, n)
    return a


def _random_poses(rng, n_lidar, n_slots):
    p = np.zeros((n_lidar, n_slots, 7))
    for x in p.reshape(-1, 7):
        q = np.array([0.02, -0.03, 0.05, 1.0]) * [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]
        x[:] = np.concatenate([rng.uniform(-1, 1, 3), q / np.linalg.norm(q)])
    return p


def test_tile_and_segment_edges(mla, orc):
    """segments of 0, 1, 255, 256, 257 and 513 points spread over the slots of three LiDARs (tiles of 256: none, a short one, one point short of full, full,
    full + one point, two full + one point), one LiDAR with every slot empty; window 1 with one LiDAR"""
    rng = np.random.default_rng(8)
    lens = {0: [(0, 257), (1, 0), (513, 256), (255, 1)],         # LiDAR 0: (surf, corner) per slot 0..3 (slot 3 is not part of a map)
            1: [(0, 0), (0, 0), (0, 0), (0, 0)],
            2: [(256, 513), (255, 0), (0, 1), (7, 7)]}
    clouds = [[(_crafted(rng, a), _crafted(rng, b)) for a, b in lens[n]] for n in range(3)]
    poses = _random_poses(rng, 3, 4)
    ctx = mla.Context(0)
    try:
        _fill(ctx, clouds, W3)
        for source, leaf in ((-1, 1.5), (2, [1.5, 0.7, 3.0])):
            r = _check_maps(mla, ctx, orc, clouds, poses, W3, source, leaf, leaf, need_thinning=False)
            if source < 0:
                assert r["n_pre"].tolist() == [[0 + 1 + 513, 257 + 0 + 256], [0, 0], [256 + 255 + 0, 513 + 0 + 1]]
                assert r["n_ds"][1].tolist() == [0, 0]
                for k in range(2):
                    for f in (False, True):
                        assert ctx.window_map_cloud(1, k, f).n == 0
            else:
                assert r["n_pre"].tolist() == [[511, 514]] * 3
        # every slot empty: a build is all zeros
        _fill(ctx, [[(wc.EMPTY, wc.EMPTY)] * 4] * 3, W3)
        r = ctx.window_build_local_map(poses, mla.window_map_opts(16, 3, W3))
        assert not r["n_pre"].any() and not r["n_ds"].any() and ctx.window_map_cloud(0, 0, True).n == 0
        # window 1, one LiDAR: the map is slot 0 alone
        one = [[(_crafted(rng, 300), _crafted(rng, 256)), (_crafted(rng, 50), _crafted(rng, 50))]]
        _fill(ctx, one, 1)
        r = _check_maps(mla, ctx, orc, one, _random_poses(rng, 1, 2), 1, -1, 2.0, 2.0, need_thinning=False)
        assert r["n_pre"].tolist() == [[300, 256]]
    finally:
        ctx.close()


def test_slide_window_is_circular_buffer_push(mla):
    """the store and the restated CircularBuffer driven through Estimator::process's own sequence for window 3 (estimator.cpp:485-527): INITIAL with its double
    slide at cir_buf_cnt_ == WINDOW_SIZE (the second pushes a still-empty slot), then 2 (W + 1) + 3 NON_LINEAR frames (the start index wraps twice); after every
    step every slot of every LiDAR and kind is the restatement's, bit for bit"""
    rng = np.random.default_rng(5)
    n_lidar, cap = 2, W3 + 1
    ref = [[wc.CircularBuffer(cap) for _ in range(2)] for _ in range(n_lidar)]          # [lidar][kind]
    ctx = mla.Context(0)

    def check(what):
        for n in range(n_lidar):
            for k in range(2):
                for slot in range(cap):
                    assert wc.same_bits(ctx.window_fetch(n, slot, k), ref[n][k][slot]), (what, n, k, slot)

    def slide(cnt):
        ctx.window_slide(cnt)
        for n in range(n_lidar):
            for k in range(2):
                ref[n][k].push(ref[n][k][cnt])
        check(("slide", cnt))

    try:
        ctx.window_reset(n_lidar, W3)
        check("reset")
        cnt, initial, starts, saw_empty_push, saw_twins = 0, True, [], False, False
        for frame in range(3 + 2 * cap + 3):
            for n in range(n_lidar):
                s, c = _crafted(rng, int(rng.integers(40, 300))), _crafted(rng, int(rng.integers(1, 120)))
                if frame == 5 and n == 1:
                    c = wc.EMPTY                                   # a scan without corners
                ctx.window_set(n, cnt, s, c)
                ref[n][0][cnt], ref[n][1][cnt] = s, c
            check(("set", frame))
            if initial:
                slide(cnt)
                if cnt < W3:
                    cnt += 1
                    if cnt == W3:
                        saw_empty_push = len(ref[0][0][cnt]) == 0
                        slide(cnt)
                if cnt == W3:
                    initial = False
            else:
                slide(cnt)
                saw_twins = saw_twins or ref[0][0][W3] is ref[0][0][W3 - 1]
            starts.append(ref[0][0].start)
        assert saw_empty_push and saw_twins
        assert sum(1 for a, b in zip(starts, starts[1:]) if b < a) >= 2          # the start index wrapped twice
        assert ctx.window_info()["pushes"] == 3 + 1 + (2 * cap + 3)
    finally:
        ctx.close()


def test_steady_state_allocates_nothing(mla, drive):
    """twenty frames of set + slide + build with clouds no larger than the largest seen: no device allocation, and the bytes in use come back to the same value"""
    clouds = [drive["stack"][f][n] for f in range(4) for n in range(2)]
    cycle = clouds[:4] + [(clouds[4][0][:200], wc.EMPTY)]               # period 5: four real clouds, a small one without corners
    poses = wc.pose_local(drive, 1, range(4), 2)
    o = mla.window_map_opts(16, 2, W3)
    ctx = mla.Context(0)
    try:
        ctx.window_reset(2, W3)
        t = [0]

        def frame():
            for n in range(2):
                s, c = cycle[(t[0] + 2 * n) % 5]
                ctx.window_set(n, W3, s, c)
            ctx.window_slide(W3)
            r = ctx.window_build_local_map(poses, o)
            t[0] += 1
            return r

        for _ in range(10):                                              # two periods: every state of the cycle has been seen
            frame()
        before = ctx.window_info()
        assert before["allocations"] > 0 and before["bytes_used"] > 0 and before["bytes_reserved"] >= before["bytes_used"]
        for _ in range(20):
            r = frame()
            assert ctx.window_info()["allocations"] == before["allocations"]
        assert r["n_ds"].all()
        after = ctx.window_info()
        assert after["bytes_used"] == before["bytes_used"] and after["bytes_reserved"] == before["bytes_reserved"]
        assert after["pushes"] == 30
    finally:
        ctx.close()


def test_set_from_scan(mla, drive):
    """after scan_upload + extract_run + extract_voxel(0.2) the slot's clouds are pcl::VoxelGrid of the less-sharp points at 0.2 and of the thinned less-flat cloud
    at 0.4; the same with the scan held by a second context, which re-uploads another scan at once without disturbing the slot"""
    rng = np.random.default_rng(2)
    scans = []
    for n in range(2):
        s = drive["scans"][0][n]
        pts = s.points.copy()
        pts[:, 3] = rng.uniform(0, 16, len(pts)).astype(np.float32)     # an intensity to average
        scans.append((pts, s.scan_start, s.scan_end))
    ctx, other = mla.Context(0), mla.Context(0)
    try:
        ctx.window_reset(2, W3)
        want = []
        for pts, ss, se in scans:
            lists = ctx.extract(pts, ss, se, voxel_leaf=0.2)
            want.append((ctx.voxel_grid(lists["less_flat_ds"], 0.4), ctx.voxel_grid(pts[lists["less_sharp"]], 0.2)))
        assert all(len(w[0]) > 100 and len(w[1]) > 20 for w in want)
        # the plain case: the context's own scan (scan 1 is the one it holds)
        ctx.window_set_from_scan(1, 2)
        for k in range(2):
            assert wc.same_bits(ctx.window_fetch(1, 2, k), want[1][k]), k
        # the scan of another context
        other.scan_upload(*scans[0]); other.extract_run(); other.extract_voxel_run(0.2)
        ctx.window_set_from_scan(0, 3, src=other)
        other.scan_upload(*scans[1]); other.extract_run(); other.extract_voxel_run(0.2)       # at once: ordered behind the reads by the hand-over's event
        other.synchronize()
        for k in range(2):
            assert wc.same_bits(ctx.window_fetch(0, 3, k), want[0][k]), k
            assert wc.same_bits(ctx.window_fetch(1, 2, k), want[1][k]), k
        ctx.window_set_from_scan(0, 0, src=other)
        for k in range(2):
            assert wc.same_bits(ctx.window_fetch(0, 0, k), want[1][k]), k
    finally:
        ctx.close(); other.close()


def test_window_problem_from_device_clouds(mla, synth, drive):
    """one window (pivot = slot 1, frames = slots 2 and 3, two LiDARs): maps staged from mlh_window_map_cloud and features from mlh_window_cloud, device to device,
    against the same calls fed the same clouds as host arrays: H, g, the cost and the residual count are bit-equal, and at least half the features matched"""
    clouds = _drive_clouds(drive)
    poses = wc.pose_local(drive, 1, range(4), 2)
    to_pose = drive["to_pose"]
    pert = lambda T, k: synth.perturbed_pose(to_pose(T), seed=300 + k, dt=0.03, drot_deg=0.3)
    pivot = to_pose(drive["T"][1])
    frames = np.stack([pert(drive["T"][2 + k], k) for k in range(2)])
    exts = np.stack([to_pose(drive["exts_T"][0]), pert(drive["exts_T"][1], 10)])
    ctx, host = mla.Context(0), mla.Context(0)
    try:
        _fill(ctx, clouds, W3)
        r = ctx.window_build_local_map(poses, mla.window_map_opts(16, 2, W3))
        assert r["n_ds"].all()
        maps = [[ctx.window_map_fetch(n, k, True) for k in range(2)] for n in range(2)]
        ctx.pure_odom_begin(); host.pure_odom_begin()
        staged = 0
        for n in range(2):
            ctx.map_set_pair(ctx.window_map_cloud(n, mla.SURF), ctx.window_map_cloud(n, mla.CORNER))
            host.map_set_pair(maps[n][0], maps[n][1])
            for i in (2, 3):
                for k in (mla.SURF, mla.CORNER):
                    ctx.features_set(k, ctx.window_cloud(n, i, k))
                    host.features_set(k, clouds[n][i][k])
                    for c in (ctx, host):
                        c.pure_odom_add_matches(k, poses[n][i], i - 2, n)
                    staged += len(clouds[n][i][k])
        a, b = ctx.pure_odom_normal_eq(pivot, frames, exts), host.pure_odom_normal_eq(pivot, frames, exts)
        print(f"staged features {staged}, residuals {a['count']}, cost {a['cost']:.6g}")
        assert a["count"] == b["count"] and a["cost"] == b["cost"]
        assert np.array_equal(a["H"].view(np.uint64), b["H"].view(np.uint64)) and np.array_equal(a["g"].view(np.uint64), b["g"].view(np.uint64))
        assert 2 * a["count"] >= staged, (a["count"], staged)
        assert np.isfinite(a["H"]).all() and a["H"].any()
    finally:
        ctx.close(); host.close()


def test_errors_leave_the_store_usable(mla, orc, drive):
    clouds = _drive_clouds(drive)
    poses = wc.pose_local(drive, 1, range(4), 2)
    s, c = clouds[0][0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    i32 = lambda n: (C.c_int32 * n)()
    ctx = mla.Context(0)
    try:
        lib, h = ctx.lib, ctx.h
        o = mla.window_map_opts(16, 2, W3)
        ptr, n, n_pre, n_ds = C.c_void_p(), C.c_int32(0), i32(4), i32(4)
        # before mlh_window_reset
        assert lib.mlh_window_set(h, 0, 0, p(s), len(s), p(c), len(c), 16, 12, 0) == STATE
        assert lib.mlh_window_set_from_scan(h, h, 0, 0, 0.4, 0.2) == STATE
        assert lib.mlh_window_slide(h, 0) == STATE
        assert lib.mlh_window_cloud(h, 0, 0, 0, C.byref(ptr), C.byref(n)) == STATE
        assert lib.mlh_window_info(h, None, None, None, None, None, None) == STATE
        assert lib.mlh_window_build_local_map(h, p(poses), C.byref(o), n_pre, n_ds) == STATE
        assert lib.mlh_window_map_cloud(h, 0, 0, 1, C.byref(ptr), C.byref(n)) == STATE
        for bad in ((0, 3), (17, 3), (2, 0), (2, 17)):
            assert lib.mlh_window_reset(h, *bad) == INVALID
        _fill(ctx, clouds, W3)
        # a LiDAR or slot out of range
        for lidar, slot in ((-1, 0), (2, 0), (0, -1), (0, 4)):
            assert lib.mlh_window_set(h, lidar, slot, p(s), len(s), p(c), len(c), 16, 12, 0) == INVALID
            assert lib.mlh_window_cloud(h, lidar, slot, 0, C.byref(ptr), C.byref(n)) == INVALID
            assert lib.mlh_window_set_from_scan(h, h, lidar, slot, 0.4, 0.2) == INVALID
        assert lib.mlh_window_slide(h, 4) == INVALID and lib.mlh_window_slide(h, -1) == INVALID
        assert lib.mlh_window_map_cloud(h, 2, 0, 1, C.byref(ptr), C.byref(n)) == INVALID
        assert lib.mlh_window_cloud(h, 0, 0, 2, C.byref(ptr), C.byref(n)) == INVALID
        # bad records: stride, a null cloud with points, an intensity outside the record, an unknown memory kind
        assert lib.mlh_window_set(h, 0, 0, p(s), len(s), p(c), len(c), 10, 12, 0) == INVALID
        assert b"stride_bytes" in lib.mlh_last_error(h)
        assert lib.mlh_window_set(h, 0, 0, None, len(s), p(c), len(c), 16, 12, 0) == INVALID
        assert lib.mlh_window_set(h, 0, 0, p(s), len(s), p(c), len(c), 16, 16, 0) == INVALID
        assert lib.mlh_window_set(h, 0, 0, p(s), len(s), p(c), len(c), 16, 12, 7) == INVALID
        # the scan calls: no scan yet, bad leaves
        assert lib.mlh_window_set_from_scan(h, h, 0, 0, 0.4, 0.2) == STATE
        for ls, lc in ((0.0, 0.2), (0.4, -1.0), (float("nan"), 0.2), (0.4, float("inf"))):
            assert lib.mlh_window_set_from_scan(h, h, 0, 0, ls, lc) == INVALID
        # the build: leaves, source_lidar, poses
        for field, v in (("leaf_surf", 0.0), ("leaf_corner", float("nan")), ("leaf_surf", float("inf")), ("leaf_corner", -0.4)):
            bad = mla.window_map_opts(16, 2, W3)
            getattr(bad, field)[1] = v
            assert lib.mlh_window_build_local_map(h, p(poses), C.byref(bad), n_pre, n_ds) == INVALID
        bad = mla.window_map_opts(16, 2, W3, source_lidar=2)
        assert lib.mlh_window_build_local_map(h, p(poses), C.byref(bad), n_pre, n_ds) == INVALID
        assert b"source_lidar" in lib.mlh_last_error(h)
        assert lib.mlh_window_build_local_map(h, None, C.byref(o), n_pre, n_ds) == INVALID
        assert lib.mlh_window_build_local_map(h, p(poses), None, n_pre, n_ds) == INVALID
        nan_poses = poses.copy(); nan_poses[1, 2, 4] = np.nan
        assert lib.mlh_window_build_local_map(h, p(nan_poses), C.byref(o), n_pre, n_ds) == INVALID
        # ... and the store is what it was: a valid build still equals the loop and the oracle
        _check_maps(mla, ctx, orc, clouds, poses, W3, -1, None, None)
    finally:
        ctx.close()


def test_window_selftest_device_window_equals_the_host_cloud_path():
    """m-loam_amd/host/window_selftest: ten odometry frames of two LiDARs through SlidingWindowMap and through the host-cloud loop end in the same normal equations"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "window_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/window_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "device window equals the host-cloud path" in r.stdout
