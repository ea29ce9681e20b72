"""The NumPy restatement of the Scan Context front (tests/sc_cases.py) held against hand-computed values, the crafted scenes held to their own preconditions,
the host arithmetic the device shares (m-loam_amd/csrc/sc_host.hpp) held against the restatement, and the C-ABI of the store. CPU only;
tests/test_gpu_scancontext.py compares the device against this restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sc_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC_SYMBOLS = ["mlh_sc_reset", "mlh_sc_add", "mlh_sc_add_keyframe", "mlh_sc_detect", "mlh_sc_candidates", "mlh_sc_distance", "mlh_sc_fetch", "mlh_sc_info"]


def test_descriptor_of_five_hand_placed_points():
    """2 rings x 4 sectors, max_radius 10, lidar_height 1: ring 1 is range <= 5, sector k is the k-th quarter turn"""
    o = sc.opts(num_ring=2, num_sector=4, max_radius=10.0, lidar_height=1.0)
    pts = np.array([[1.0, 1.0, 0.5],        # range 1.41, 45 deg: ring 1, sector 1, z' 1.5
                    [2.0, 2.0, 2.0],        # the same cell, z' 3: the maximum
                    [-6.0, 1.0, -0.25],     # range 6.08, 170.5 deg: ring 2, sector 2, z' 0.75
                    [-1.0, -7.0, 4.0],      # range 7.07, 261.9 deg: ring 2, sector 3, z' 5
                    [3.0, -1.0, -3.0]],     # range 3.16, 341.6 deg: ring 1, sector 4, z' -2 (a negative maximum stays)
                   np.float32)
    want = np.array([[3.0, 0.0, 0.0, -2.0],
                     [0.0, 0.75, 5.0, 0.0]])
    assert np.array_equal(sc.descriptor(pts, o), want)
    assert np.array_equal(sc.descriptor(pts[::-1], o), want)                   # whatever the order
    assert np.array_equal(sc.descriptor(np.zeros((0, 3), np.float32), o), np.zeros((2, 4)))
    assert np.array_equal(sc.descriptor(np.array([[9.0, 9.0, 1.0]], np.float32), o), np.zeros((2, 4)))     # range 12.7: dropped


def test_hand_points_are_binned_as_documented():
    o = sc.opts()
    pts, what = sc.hand_points(o)
    b = sc.bin_points(pts, o)
    kept = dict(zip(np.flatnonzero(b["keep"]).tolist(), zip(b["ring"].tolist(), b["sector"].tolist())))
    assert kept[0] == (20, 1) and 1 not in kept, what[:2]                       # exactly max_radius stays, the next float is dropped
    assert kept[2] == (1, 1), what[2]                                           # x = y = 0
    assert [kept[i][1] for i in (3, 4, 5, 6)] == [9, 22, 39, 52]                # 53.13, 126.87, 233.13, 306.87 degrees over 6-degree sectors
    assert [kept[i][1] for i in (7, 8, 9, 10)] == [1, 15, 30, 45]               # the axes: 0, 90, 180, 270 degrees sit on sector edges
    assert kept[11][1] == 1 and kept[12][1] == 60, what[11:13]                  # x = -0: angles -90 and 450
    assert b["skipped"] == 3 and not b["keep"][15:].any()
    d = sc.descriptor(pts, o)
    assert d[kept[13][0] - 1, kept[13][1] - 1] == 0.0                           # z' = -1000 and below read as empty
    assert sc.descriptor(pts[[1]], o).any() == False                            # every point out of range: all zero


def test_keys_and_distance_of_two_hand_made_descriptors():
    """3 x 4, by hand. B is A's columns moved one to the right with column 0 of the result doubled (the cosine does not see the factor, the sector key does):
    A's sector key (column means) = [1, 2, 0, 1]; B's = [2, 1, 2, 0]; the alignment finds shift 3, where B's columns lie on A's again."""
    A = np.array([[1.0, 2.0, 0.0, 0.0],
                  [2.0, 2.0, 0.0, 3.0],
                  [0.0, 2.0, 0.0, 0.0]])
    B = np.roll(A, 1, axis=1)
    B[:, 0] *= 2.0
    assert np.array_equal(sc.ring_key(A), np.array([0.75, 1.75, 0.5], np.float32))
    assert np.array_equal(sc.sector_key(A), np.array([1.0, 2.0, 0.0, 1.0]))
    assert np.array_equal(sc.sector_key(B), np.array([2.0, 1.0, 2.0, 0.0]))
    np.testing.assert_allclose(sc.col_norms(A), [np.sqrt(5.0), np.sqrt(12.0), 0.0, 3.0], rtol=0, atol=1e-15)
    o = sc.opts(num_ring=3, num_sector=4, search_ratio=0.5)                    # radius round(0.5 * 0.5 * 4) = 1
    assert sc.search_radius(o) == 1
    # alignment: |kA - roll(kB, s)| for s = 0..3: roll(kB,0) = [2,1,2,0] -> sqrt(1+1+4+1); s=1: [0,2,1,2] -> sqrt(1+0+1+1); s=2: [2,0,2,1] -> sqrt(1+4+4+0); s=3: [1,2,0,2] -> 1
    align, norms = sc.fast_align(sc.sector_key(A), sc.sector_key(B))
    np.testing.assert_allclose(norms, [np.sqrt(7.0), np.sqrt(3.0), 3.0, 1.0], rtol=0, atol=1e-15)
    assert align == 3
    # shifts 2, 3, 0 are scored. roll(B, 3) = A with column 3 doubled: cosine 1 in the three non-empty columns -> distance 0
    d, s, seen, _ = sc.distance(A, B, o)
    assert sorted(seen) == [0, 2, 3] and s == 3 and abs(d) < 1e-15
    # shift 0: columns of A against B = [2 a3 | a0 | a1 | a2]: col 0: a0.a3 = 6 / (sqrt5 * 3), col 1: a1.a0 = 6 / (sqrt12 sqrt5), col 2: A's is empty, col 3: B's (a2) is empty
    want0 = 1.0 - (6.0 / (np.sqrt(5.0) * 3.0) + 6.0 / (np.sqrt(12.0) * np.sqrt(5.0))) / 2.0
    assert abs(seen[0] - want0) < 1e-15
    # the f32 key distance, groups of four then the tail: R = 6 -> one group and two singles
    q = np.array([1, 2, 3, 4, 5, 6], np.float32)
    k = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 7]], np.float32)
    assert np.array_equal(sc.key_dist(q, k), np.array([91.0, 1.0], np.float32))
    # all-zero query: no effective column, NaN, which never wins
    dz, sz, _, _ = sc.distance(np.zeros((3, 4)), A, o)
    assert dz == 10000000.0 and sz == 0
    assert sc.yaw_of(55, 60) == np.float32(5.759586334228516) and sc.yaw_of(0, 60) == 0.0


def test_early_return_stale_prefix_and_padded_candidates():
    """exclude 3, period 4, 3 candidates over 14 adds: queries 0..3 return early and do not advance the counter; the searched prefix is rebuilt at queries 4, 8, 12
    (counter 0, 4, 8) and stale in between; with fewer searched entries than candidates each is scored once"""
    o = sc.opts(**sc.SEQ_OPTS)
    rng = np.random.default_rng(3)
    m = sc.Manager(o)
    prefixes, scored, counters = [], [], []
    for i in range(14):
        m.add(sc.clean_cloud(rng, 200, o, radius=60.0))
        r = m.detect(i)
        prefixes.append(m.prefix); scored.append(r["n_candidates_scored"]); counters.append(m.counter)
        if i < 4:
            assert (r["match_index"], r["score"], r["yaw_diff_rad"], r["nearest_index"]) == (-1, -1.0, 0.0, -1)
        else:
            assert all(c < m.prefix for c in r["cand"]) and len(set(r["cand"])) == len(r["cand"])
    assert prefixes == [0, 0, 0, 0, 1, 1, 1, 1, 5, 5, 5, 5, 9, 9]
    assert scored == [0, 0, 0, 0, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3]
    assert counters == [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]


def test_track_sequence_meets_its_preconditions_and_finds_the_revisit():
    o, steps = sc.track_sequence()
    _, out = sc.run_sequence(o, steps)                                         # asserts the gaps of every step
    for i in range(20, 30):
        assert out[i]["match_index"] == i - 20 and out[i]["shift"] == 55, i    # the heading turned by +30 degrees = 5 sectors: the candidate moves by S - 5
    assert all(r["match_index"] == -1 for r in out[:20])
    rng = np.random.default_rng(1)
    assert sc.band_count(sc.natural_cloud(rng, 10000, o), o) <= 50
    assert sc.band_count(sc.band_cloud(rng, 200, o), o) == 200


def test_library_exports_the_scan_context_store(mla):
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(os.path.join(ROOT, "m-loam_amd", "lib", "libmloam_hip.so"))
    for nm in SC_SYMBOLS:
        assert re.search(r"\bint\s+" + nm + r"\s*\(\s*mlh_ctx\s*\*", hdr), nm
        assert nm in mla.EXPORTED_SYMBOLS, nm
        assert getattr(lib, nm) is not None, nm
    assert getattr(lib, "mlh_sc_opts_default") is not None and "mlh_sc_opts_default" in mla.EXPORTED_SYMBOLS
    assert C.sizeof(mla.ScOpts) == 64 and C.sizeof(mla.ScResult) == 32 and C.sizeof(mla.ScStoreInfo) == 56
    o = mla.sc_opts()
    assert (o.lidar_height, o.num_ring, o.num_sector, o.max_radius, o.num_exclude_recent, o.num_candidates, o.search_ratio, o.dist_thres, o.tree_making_period,
            o.loop_distance_threshold) == (2.0, 20, 60, 80.0, 50, 50, 0.1, 0.5, 10, 50.0)
    for name in ("sc_reset", "sc_add", "sc_add_keyframe", "sc_detect", "sc_distance", "sc_fetch", "sc_info"):
        assert callable(getattr(mla.Context, name)), name


def test_host_arithmetic_under_sanitizers_and_against_the_restatement(tmp_path):
    """m-loam_amd/csrc/sc_host.hpp in a stand-alone program built with -fsanitize=address,undefined and run directly: its own checks (option validation, period
    bookkeeping, encoding, yaw, rejection) pass, and the per-point arithmetic the kernel shares with the host -- ring, sector, band, z' -- agrees with the restatement
    on the hand-placed points, 3 000 random ones and 200 band points, for three grids"""
    exe = tmp_path / "sc_host_main"
    src = os.path.join(ROOT, "tests", "host", "sc_host_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), src, "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    rng = np.random.default_rng(17)
    for R, S, radius, h in ((20, 60, 80.0, 2.0), (5, 7, 30.0, 0.0), (64, 128, 80.0, 1.5)):
        o = sc.opts(num_ring=R, num_sector=S, max_radius=radius, lidar_height=h)
        hand = sc.hand_points(o)[0]
        pts = np.concatenate([hand[np.isfinite(hand).all(axis=1)], sc.natural_cloud(rng, 3000, o), sc.band_cloud(rng, 200, o)]).astype(np.float32)
        f = tmp_path / f"pts_{R}x{S}.f32"
        np.ascontiguousarray(pts).tofile(f)
        r = subprocess.run([str(exe), str(f), str(len(pts)), repr(radius), repr(h), str(R), str(S)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "sc_host: ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("P ")]
        assert len(lines) == len(pts)
        want = sc.bin_points(pts, o)
        band = sc.in_band(want["sv"])
        k = 0
        for i, ln in enumerate(lines):
            if not want["keep"][i]:
                assert ln[2] == "out", i
                continue
            got = tuple(int(v) for v in ln[2:])
            zbits = int(np.array([want["z"][k]], np.float32).view(np.int32)[0])
            u = (zbits & 0xffffffff) ^ 0x7fffffff
            enc = zbits if zbits >= 0 else (u - (1 << 32) if u >= (1 << 31) else u)
            assert got == (int(want["ring"][k]), int(want["sector"][k]), int(band[k]), enc), (R, S, i, pts[i], got)
            k += 1
        assert k == int(want["keep"].sum()) and band.sum() >= 200
