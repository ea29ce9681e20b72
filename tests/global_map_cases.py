"""Restatements shared by the global-map tests (tests/test_global_map_host.py, tests/test_gpu_global_map.py): the selection of pubGlobalMap / saveGlobalMap
(lidar_mapper_keyframe.cpp:804-810, 865-868) over the reference-built VoxelGridCovarianceMLOAM, and positions to run it on."""
import numpy as np


def select_restated(orc, positions, center, radius, kf_res):
    """radiusSearch around the f32 position (nearest first, equal distances by index; radius < 0: every keyframe in index order), then the hits, in that
    order, through the reference-built plain branch at kf_res with intensity = the keyframe's own index (cpp:666, 808)"""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    if radius < 0:
        hits = list(range(len(pos)))
    else:
        c = np.asarray(center, np.float32)
        r = np.float32(radius)
        hit = []
        for i, p in enumerate(pos):
            d = p - c
            d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            if d2 <= r * r:
                hit.append((d2, i))
        hits = [i for _, i in sorted(hit)]
    if not hits:
        return []
    pts = np.zeros((len(hits), 4), np.float32)
    pts[:, :3] = pos[hits]
    pts[:, 3] = hits
    return [int(v) for v in orc.ref_voxel_filter(pts, kf_res)[:, 3]]


def circle_positions(n=40, step=1.05, radius=6.0):
    """the keyframe positions of the 40-frame circle of tests/test_gpu_local_map.py (f32, as pose_keyframes_3d holds them)"""
    out = []
    for k in range(n):
        a = k * step / radius
        out.append([radius * np.cos(a) - radius, radius * np.sin(a), 0.3 + 0.02 * np.sin(k)])
    return np.array(out, np.float64).astype(np.float32)
