"""Crafted keyframes and the restated host plan of the batched place-index build (mlh_sc_add_keyframes; m-loam_amd/csrc/sc_host.hpp: sc_batch_plan, sc_grown_cap),
shared by tests/test_sc_batch_cases.py (CPU) and tests/test_gpu_sc_batch.py (GPU).

The keyframes' clouds have the sizes at which the kernels can go wrong -- 0, 1, 255, 256, 257, 513 points: the edges of the 256-point pass -- and among them: a
keyframe with no point at all (index 1), keyframes with points inside the sector-edge band (the host decides those), one with a non-finite point, one wholly beyond
max_radius. Everything else is clean of band points (sc_cases.clean_cloud asserts it), so how many points the host decides per keyframe is known on the CPU."""
import numpy as np

import sc_cases as sc

SIZES = (0, 1, 255, 256, 257, 513)
CHUNK_POINTS, MAX_CHUNKS = 256, 64
GRIDS = {"20x60": dict(num_ring=20, num_sector=60), "8x12": dict(num_ring=8, num_sector=12, max_radius=40.0, lidar_height=1.0),
         "64x128": dict(num_ring=64, num_sector=128, lidar_height=1.5)}       # 64 x 128 = 8 192 cells: the largest grid mlh_sc_reset accepts
QUERY = dict(num_exclude_recent=1, tree_making_period=3, num_candidates=4, loop_distance_threshold=-1.0)


def options(grid):
    return sc.opts(**{**QUERY, **GRIDS[grid]})


def sizes_of(i):
    """(surf, corner, outlier or None) lengths of keyframe i"""
    if i == 1:
        return 0, 0, None
    return SIZES[i % 6], SIZES[(i // 6 + i + 3) % 6], (None if i % 3 == 0 else SIZES[(i + 4) % 6])


def keyframes(K, o, seed=3):
    """K keyframes as (pose[7], surf, corner, outlier or None), clouds float32 (n, 4) {x, y, z, lidar}"""
    rng = np.random.default_rng(seed + 1000 * K + o["num_sector"])
    out = []
    for i in range(K):
        clouds = []
        for n in sizes_of(i):
            if n is None:
                clouds.append(None)
                continue
            c = np.zeros((n, 4), np.float32)
            c[:, :3] = sc.clean_cloud(rng, n, o)
            c[:, 3] = rng.integers(0, 2, n)
            clouds.append(c)
        big = max((k for k in range(3) if clouds[k] is not None), key=lambda k: len(clouds[k]))
        n_big = len(clouds[big])
        what = i % 8
        if what in (0, 5) and n_big:                       # points the host decides
            m = min(n_big, 7)
            clouds[big][n_big - m:, :3] = sc.band_cloud(rng, m, o)
        elif what == 2 and n_big:                          # a non-finite point: skipped and counted
            clouds[big][n_big // 2, 1] = np.nan
        elif what == 3:                                    # every point beyond max_radius: the all-zero descriptor
            for c in clouds:
                if c is not None and len(c):
                    th = rng.uniform(0, 2 * np.pi, len(c))
                    r = rng.uniform(1.2, 1.5, len(c)) * o["max_radius"]
                    c[:, 0], c[:, 1] = r * np.cos(th), r * np.sin(th)
        a = 0.05 * i
        pose = np.array([3.0 * i, -0.5 * i, 0.1, 0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])
        out.append((pose, clouds[0], clouds[1], clouds[2]))
    return out


def big_keyframe(o, seed=9):
    """one keyframe whose 2 500 band points exceed what travels with the counters (2 048) and whose 4 488 points are cut into several chunks, the cloud borders
    (2 600, 3 711) inside chunks"""
    rng = np.random.default_rng(seed)

    def c4(p):
        c = np.zeros((len(p), 4), np.float32)
        c[:, :3] = p
        return c
    surf = c4(np.concatenate([sc.band_cloud(rng, 2500, o), sc.clean_cloud(rng, 100, o)])[rng.permutation(2600)])
    return (np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0]), surf, c4(sc.clean_cloud(rng, 1111, o)), c4(sc.clean_cloud(rng, 777, o)))


def points_of(kf):
    """a keyframe's points in the order the kernels read them: surf, corner, outlier"""
    return np.concatenate([c[:, :3] for c in kf[1:] if c is not None]) if any(c is not None for c in kf[1:]) else np.zeros((0, 3), np.float32)


def host_decided(kf, o):
    """points of the keyframe the device leaves to the host (band points among the finite ones within max_radius)"""
    p = points_of(kf)
    return sc.band_count(p, o) if len(p) else 0


def skipped(kf):
    p = points_of(kf)
    return int((~np.isfinite(p).all(axis=1)).sum())


def chunks_wanted(n_entries, target):
    return max(1, min(MAX_CHUNKS, -(-target // n_entries))) if n_entries >= 1 else 1


def chunk_plan(n_points, target):
    """sc_batch_plan restated: [(entry, first, count)]"""
    wanted = chunks_wanted(len(n_points), target)
    out = []
    for e, n in enumerate(n_points):
        if n <= 0:
            continue
        passes = (n - 1) // CHUNK_POINTS + 1
        chunks = min(passes, wanted)
        per = ((passes - 1) // chunks + 1) * CHUNK_POINTS
        out += [(e, at, min(per, n - at)) for at in range(0, n, per)]
    return out


def grown_cap(n, cap, more):
    """the capacity `more` single adds leave behind at n entries: each doubles (from 64) when the store is full"""
    for _ in range(more):
        if n >= cap:
            cap = max(64, 2 * cap)
        n += 1
    return cap
