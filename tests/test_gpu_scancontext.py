"""Scan Context place recognition on the device (m-loam_amd/csrc/scancontext.hip; mlh_sc_*) against the NumPy restatement of tests/sc_cases.py, which
tests/test_sc_cases.py holds on the CPU. Everything goes through the C-ABI.

Bounds: descriptors and ring keys bit-equal (a maximum of floats, a left-to-right f64 sum cast to f32); key distances bit-equal (f32, no contraction); sector keys
and scores within 1e-12 -- about 150 f64 roundings of quantities <= 1 are 2e-14, with a 60x margin for another summation order; indices, shifts and yaw equal."""
import numpy as np
import pytest

import sc_cases as sc

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -3
GRIDS = {"20x60": dict(num_ring=20, num_sector=60), "5x7": dict(num_ring=5, num_sector=7, max_radius=30.0, lidar_height=0.0),
         "64x128": dict(num_ring=64, num_sector=128, lidar_height=1.5)}


@pytest.fixture
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _reset(mla, ctx, o):
    ctx.sc_reset(mla.sc_opts(**o))


def _records(p, stride):
    """xyz as records of `stride` bytes (the rest is filler the library must not read as coordinates)"""
    a = np.full((len(p), stride // 4), 7.5e8, np.float32)
    a[:, :3] = p
    return a


def _same_desc(ctx, index, cloud, o, label=""):
    want = sc.descriptor(cloud, o)
    desc, rk, sk = ctx.sc_fetch(index)
    assert np.array_equal(desc, want), (label, int((desc != want).sum()))
    assert np.array_equal(rk.view(np.uint32), sc.ring_key(want).view(np.uint32)), label
    err = float(np.abs(sk - sc.sector_key(want)).max())
    assert err <= 1e-12, (label, err)
    return want


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_descriptor_sizes_strides_and_memory_kinds(mla, ctx, grid):
    """bit-equal descriptors for clouds of 0, 1, 63, 64, 65, 4 097 points and the sizes around the kernel's per-workgroup tile and its grid-stride wrap, as one
    to three clouds, strides 16 and 48, host and device records; at most 0.5 % of the points of these natural clouds are host-decided"""
    import torch
    o = sc.opts(**GRIDS[grid])
    _reset(mla, ctx, o)
    info = ctx.sc_info()
    tile, wrap = info["desc_tile_points"], info["desc_wrap_points"]
    assert tile >= 64 and wrap % tile == 0
    rng = np.random.default_rng(11)
    sizes = [0, 1, 63, 64, 65, 4097, tile - 1, tile, tile + 1] + ([wrap - 1, wrap, wrap + 1] if grid == "20x60" else [])
    for k, n in enumerate(sizes):
        cloud = sc.natural_cloud(rng, n, o) if n >= 1000 else sc.clean_cloud(rng, n, o)      # (a cloud too small for the 0.5 % rule to mean anything is a clean one)
        stride = (16, 48)[k % 2]
        n_parts = 1 + k % 3
        cuts = sorted(rng.integers(0, n + 1, n_parts - 1).tolist()) if n else [0] * (n_parts - 1)
        parts = [_records(c, stride) for c in np.split(cloud, cuts)]
        if k % 2:
            parts = [torch.from_numpy(p).cuda() for p in parts]
        before = ctx.sc_info()
        idx = ctx.sc_add(parts)
        assert idx == k
        _same_desc(ctx, idx, cloud, o, (grid, n))
        after = ctx.sc_info()
        decided = after["points_host_decided"] - before["points_host_decided"]
        assert after["last_host_decided"] == decided and decided <= 0.005 * n and after["points_skipped"] == before["points_skipped"]
        assert abs(decided - sc.band_count(cloud, o)) <= 2, (grid, n, decided)            # (a point within ulps of the band's own edge may fall either way)
    assert ctx.sc_info()["n_entries"] == len(sizes)


def test_descriptor_hand_placed_points(mla, ctx):
    """range exactly max_radius and just beyond, x = y = 0, quadrants, axes, signed zero, z' = -1000 and below, NaN / inf coordinates (skipped and counted); every
    point out of range gives the all-zero descriptor"""
    o = sc.opts()
    _reset(mla, ctx, o)
    pts, _ = sc.hand_points(o)
    i = ctx.sc_add(pts)
    want = _same_desc(ctx, i, pts, o, "hand")
    assert want[19, 0] == 3.0 and want[0, 0] == 5.0                     # the point at exactly max_radius; x = y = 0 in ring 1, sector 1
    info = ctx.sc_info()
    assert info["points_skipped"] == 3 and info["last_skipped"] == 3
    j = ctx.sc_add(np.array([[90.0, 0.0, 1.0], [0.0, -81.0, 2.0], [60.0, 60.0, 3.0]], np.float32))
    desc, rk, sk = ctx.sc_fetch(j)
    assert not desc.any() and not rk.any() and not sk.any()
    k = ctx.sc_add([])                                                   # no cloud at all
    assert not ctx.sc_fetch(k)[0].any()


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_band_points_are_decided_by_the_host(mla, ctx, grid):
    """200 points inside the band, among 300 clean ones: binned as the restatement's float expression says, and reported as host-decided; a clean cloud has none"""
    o = sc.opts(**GRIDS[grid])
    _reset(mla, ctx, o)
    rng = np.random.default_rng(23)
    band, clean = sc.band_cloud(rng, 200, o), sc.clean_cloud(rng, 300, o, radius=0.9 * o["max_radius"])
    cloud = np.concatenate([band, clean])[rng.permutation(500)]
    i = ctx.sc_add(cloud)
    _same_desc(ctx, i, cloud, o, grid)
    assert ctx.sc_info()["last_host_decided"] == 200
    j = ctx.sc_add(clean)
    _same_desc(ctx, j, clean, o, grid)
    info = ctx.sc_info()
    assert info["last_host_decided"] == 0 and info["points_host_decided"] == 200


def test_many_undecided_points(mla, ctx):
    """more undecided points than travel with the counters (2 048): the second copy"""
    o = sc.opts()
    _reset(mla, ctx, o)
    rng = np.random.default_rng(29)
    cloud = np.concatenate([sc.band_cloud(rng, 2500, o), sc.clean_cloud(rng, 100, o, radius=70.0)])
    i = ctx.sc_add(cloud)
    _same_desc(ctx, i, cloud, o)
    assert ctx.sc_info()["last_host_decided"] == 2500


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_pair_distance_and_shift(mla, ctx, grid):
    o = sc.opts(**GRIDS[grid])
    _reset(mla, ctx, o)
    rng = np.random.default_rng(31)
    w = sc.world(rng, 120, extent=1.6 * o["max_radius"])
    clouds = [sc.scan_of(w, np.array([0.0, 0.0, 0.0]), 0.0, o, rng), sc.scan_of(w, np.array([0.4, -0.2, 0.0]), 360.0 / o["num_sector"] * 2, o, rng),
              sc.clean_cloud(rng, 700, o), np.array([[2.0 * o["max_radius"], 0.0, 1.0]], np.float32)]
    descs = [sc.descriptor(c, o) for c in clouds]
    for c in clouds:
        ctx.sc_add(c)
    for i, j in ((0, 1), (1, 0), (0, 2), (2, 1), (0, 0)):
        d, s, seen, norms = sc.distance(descs[i], descs[j], o)
        v, n = sorted(x for x in seen.values() if x == x), np.sort(norms)
        assert (len(v) < 2 or v[1] - v[0] >= 1e-6 or i == j) and (n[1] - n[0] >= 1e-6 or i == j)
        got_d, got_s = ctx.sc_distance(i, j)
        print(f"{grid} ({i}, {j}): distance {got_d:.6f} (restated {d:.6f}, diff {abs(got_d - d):.1e}), shift {got_s}")
        assert got_s == s and abs(got_d - d) <= 1e-12, (grid, i, j)
    assert ctx.sc_distance(3, 0) == (10000000.0, 0) and ctx.sc_distance(0, 3) == (10000000.0, 0)      # an all-zero descriptor: NaN at every shift


@pytest.mark.parametrize("n_ring", [20, 5, 22])
def test_candidate_search(mla, ctx, n_ring):
    """candidate sets, their order and their f32 distances at searched-prefix sizes 1, 2, k - 1, k, k + 1, 65, 257, 1 025 (k = 50 candidates); 22 rings end in the
    two-element tail of the groups of four"""
    o = sc.opts(num_ring=n_ring)
    k = o["num_candidates"]
    _reset(mla, ctx, o)
    rng = np.random.default_rng(37 + n_ring)
    clouds = sc.key_database(rng, 1030, o)
    m = sc.Manager(o)
    for c in clouds:
        ctx.sc_add(c)
        m.add(c)
    for prefix in (1, 2, k - 1, k, k + 1, 65, 257, 1025):
        for que in (prefix, 1029):
            want_idx, want_d = m.candidates(que, prefix)
            all_d = sc.key_dist(m.ring_keys[que], np.array(m.ring_keys[:prefix]))
            assert len(set(all_d.tolist())) == prefix, "the generator's precondition: no two key distances equal"
            idx, d2 = ctx.sc_candidates(que, prefix)
            assert len(idx) == min(prefix, k)
            assert np.array_equal(idx, want_idx), (n_ring, prefix, que)
            assert np.array_equal(d2.view(np.uint32), want_d.view(np.uint32)), (n_ring, prefix, que)


def test_equal_key_distances_go_to_the_lower_index(mla, ctx):
    o = sc.opts(num_candidates=4)
    _reset(mla, ctx, o)
    rng = np.random.default_rng(41)
    clouds = sc.key_database(rng, 12, o)
    clouds[7] = clouds[3]
    clouds[9] = clouds[3]
    m = sc.Manager(o)
    for c in clouds:
        ctx.sc_add(c)
        m.add(c)
    que = ctx.sc_add(np.concatenate([clouds[3], np.array([[1.0, 0.5, 11.0]], np.float32)]))
    m.add(np.concatenate([clouds[3], np.array([[1.0, 0.5, 11.0]], np.float32)]))
    want_idx, _ = m.candidates(que, 12)
    assert want_idx[:3].tolist() == [3, 7, 9]
    idx, d2 = ctx.sc_candidates(que, 12)
    assert idx.tolist() == want_idx.tolist() and d2[0] == d2[1] == d2[2]
    idx, _ = ctx.sc_candidates(que, 9)                                   # the third twin is outside the prefix
    assert idx[:2].tolist() == [3, 7] and 9 not in idx.tolist()


@pytest.fixture(scope="module")
def sequence():
    o, steps = sc.track_sequence()
    m, out = sc.run_sequence(o, steps)
    return o, steps, m, out


def _same_result(got, want, label):
    for key in ("match_index", "nearest_index", "shift", "n_candidates_scored", "rejected_by_distance"):
        assert got[key] == want[key], (label, key, got, {k: want[k] for k in got})
    assert np.float32(got["yaw_diff_rad"]) == np.float32(want["yaw_diff_rad"]), label
    assert abs(got["score"] - want["score"]) <= 1e-12, (label, got["score"], want["score"])


def test_detect_sequence(mla, ctx, sequence):
    """30 add-then-detect steps with exclude 3, period 4, 3 candidates: the early returns, the stale prefix, the padded candidate lists and, from step 20 on, the
    revisit with the heading turned by 5 sectors -- every result equal to the restatement's"""
    o, steps, m, out = sequence
    _reset(mla, ctx, o)
    for i, (cloud, pos) in enumerate(steps):
        assert ctx.sc_add(cloud, pos) == i
        got = ctx.sc_detect(i)
        _same_result(got, out[i], f"step {i}")
        info = ctx.sc_info()
        assert info["searched_prefix"] == (0 if i < 4 else 4 * ((i - 4) // 4) + 1) and info["period_counter"] == max(0, i - 3)
    assert [r["match_index"] for r in out[20:]] == list(range(10)) and out[25]["shift"] == 55
    # detect is a query: asking again for an old index goes through the same bookkeeping as the restatement's
    for que in (29, 12, 29):
        _same_result(ctx.sc_detect(que), m.detect(que), f"again {que}")


def test_detect_distance_rejection_and_empty_query(mla, ctx, sequence):
    """a revisit whose position lies beyond loop_distance_threshold is reported with rejected_by_distance; without a position there is no rejection; an all-zero
    query descriptor scores NaN against everything: -1, 1e7, yaw 0"""
    o, steps, _, _ = sequence
    _reset(mla, ctx, o)
    m = sc.Manager(o)
    for i in range(8):
        ctx.sc_add(*steps[i]); m.add(*steps[i])
    far = steps[2][1] + np.array([0.0, 31.0, 0.0])
    for pos in (far, None, steps[2][1]):
        q = ctx.sc_add(steps[22][0], pos)
        assert q == m.add(steps[22][0], pos)
        got, want = ctx.sc_detect(q), m.detect(q)
        sc.check_detect_preconditions(want)
        _same_result(got, want, f"position {pos}")
        assert want["nearest_index"] == 2 and want["rejected_by_distance"] == (1 if pos is far else 0) and want["match_index"] == (-1 if pos is far else 2)
    empty = np.array([[500.0, 0.0, 1.0]], np.float32)
    q = ctx.sc_add(empty)
    m.add(empty)
    got, want = ctx.sc_detect(q), m.detect(q)
    _same_result(got, want, "empty query")
    assert (got["match_index"], got["nearest_index"], got["score"], got["yaw_diff_rad"], got["shift"]) == (-1, -1, 10000000.0, 0.0, 0) and got["n_candidates_scored"] == 3


def test_add_keyframe_equals_add_of_its_clouds(mla, ctx):
    o = sc.opts()
    _reset(mla, ctx, o)
    rng = np.random.default_rng(43)

    def cloud4(n):
        c = np.zeros((n, 4), np.float32)
        c[:, :3] = sc.clean_cloud(rng, n, o)
        c[:, 3] = rng.integers(0, 2, n)
        return c
    pose = np.array([12.0, -3.0, 0.5, 0.0, 0.0, np.sin(0.2), np.cos(0.2)])
    keys = []
    for surf, corner, outlier in ((cloud4(900), cloud4(300), cloud4(150)), (cloud4(500), cloud4(0), None), (cloud4(0), cloud4(257), cloud4(1))):
        key = ctx.keyframe_save(pose, np.eye(6) * 1e-4, surf, corner)
        if outlier is not None:
            ctx.keyframe_attach_outlier(key, outlier)
        keys.append((key, [surf, corner] + ([outlier] if outlier is not None else [])))
    for key, clouds in keys:
        a = ctx.sc_add_keyframe(key)
        b = ctx.sc_add(clouds, pose[:3])
        da, db = ctx.sc_fetch(a), ctx.sc_fetch(b)
        for x, y in zip(da, db):
            assert np.array_equal(x, y)
        assert np.array_equal(da[0], sc.descriptor(np.concatenate([c[:, :3] for c in clouds]), o))
    with pytest.raises(mla.MlhError):
        ctx.sc_add_keyframe(17)


def test_store_is_independent_of_keyframes_and_of_other_contexts(mla, ctx):
    o = sc.opts(num_exclude_recent=0, num_candidates=2, tree_making_period=1)
    other = mla.Context(0)
    try:
        assert other.lib.mlh_sc_add(other.h, None, None, 0, 16, 0, None, None) == ERR_STATE       # before the first reset
        _reset(mla, ctx, o)
        _reset(mla, other, sc.opts(num_ring=5, num_sector=7, max_radius=30.0))
        rng = np.random.default_rng(47)
        a, b = sc.clean_cloud(rng, 400, o), sc.clean_cloud(rng, 300, o)
        ctx.sc_add(a); ctx.sc_add(b); other.sc_add(b)
        ctx.keyframes_reset()
        assert ctx.sc_info()["n_entries"] == 2 and other.sc_info()["n_entries"] == 1
        assert np.array_equal(ctx.sc_fetch(0)[0], sc.descriptor(a, o)) and ctx.sc_fetch(1)[0].shape == (20, 60) and other.sc_fetch(0)[0].shape == (5, 7)
        assert ctx.sc_info()["bytes_hbm"] > 0
        for bad in (dict(num_ring=0), dict(num_sector=0), dict(num_ring=128, num_sector=65), dict(num_candidates=0), dict(num_candidates=257),
                    dict(max_radius=0.0), dict(max_radius=float("inf")), dict(tree_making_period=0), dict(num_exclude_recent=-1)):
            assert ctx.lib.mlh_sc_reset(ctx.h, mla.sc_opts(**bad)) == ERR_INVALID, bad
        assert ctx.sc_info()["n_entries"] == 2                             # a refused reset leaves the store alone
        for call in (lambda: ctx.sc_detect(2), lambda: ctx.sc_fetch(-1), lambda: ctx.sc_distance(0, 2), lambda: ctx.sc_candidates(0, 3)):
            with pytest.raises(mla.MlhError):
                call()
        _reset(mla, ctx, o)
        info = ctx.sc_info()
        assert (info["n_entries"], info["bytes_hbm"], info["period_counter"], info["searched_prefix"], info["points_host_decided"]) == (0, 0, 0, 0, 0)
        assert other.sc_info()["n_entries"] == 1
    finally:
        other.close()


def test_scancontext_selftest_facade_equals_the_c_abi():
    """m-loam_amd/host/scancontext_selftest: SCManager and detectLoop of the facade against the plain calls on a second context, 40 keyframes with a revisit"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "scancontext_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/scancontext_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "11 revisits found, 1 rejected by distance" in r.stdout and r.stdout.rstrip().endswith(": ok")
