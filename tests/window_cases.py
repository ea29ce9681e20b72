"""Inputs shared by tests/test_gpu_window_map.py: a short drive of two simulated LiDARs through the 50k scene with the window clouds the estimator would
stack (estimator.cpp:485-496), the per-call loop over the existing ABI that mlh_window_build_local_map replaces, and the reference's CircularBuffer restated."""
import functools

import numpy as np

N_RINGS, N_COLS = 16, 900
LEAF_SURF, LEAF_CORNER = 0.4, 0.2          # down_size_filter_surf_ / down_size_filter_corner_ (estimator.cpp:73-74)
EMPTY = np.zeros((0, 4), np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _drive(n_frames, n_lidars):
    import importlib
    import oracle as orc
    from scipy.spatial.transform import Rotation as Rot
    synth = importlib.import_module("m-loam_amd.synth")
    orc.build()
    to_pose = lambda T: np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
    scene = synth.make_scene(seed=42, **synth.SCENE_PRESETS["50k"])
    exts_T = []
    for n in range(n_lidars):
        r = synth.HERCULES_BODY_T_LASER[n]
        exts_T.append(synth.pose_to_mat(np.concatenate([r[4:7], r[:4] / np.linalg.norm(r[:4])])))
    # conftest.make_window_case's motion: 0.4 m and about a degree per frame
    T = [synth.pose_to_mat(synth.gt_body_pose())]
    for i in range(1, n_frames):
        d = np.eye(4)
        d[:3, :3] = Rot.from_rotvec(np.deg2rad([0.3, -0.2, 1.0 + 0.2 * i])).as_matrix()
        d[:3, 3] = [0.4, 0.05, 0.01]
        T.append(T[-1] @ d)
    raw, stack = [], []
    for i in range(n_frames):
        raw.append([]); stack.append([])
        for n in range(n_lidars):
            scn = synth.simulate_scan(scene, to_pose(T[i]), synth.HERCULES_BODY_T_LASER[n], N_RINGS, n_cols=N_COLS, seed=100 + 10 * i + n)
            ex = orc.extract(scn.points, scn.scan_start, scn.scan_end)
            surf_in = np.ascontiguousarray(ex["less_flat_ds"][:, :4], np.float32)
            corner_in = np.ascontiguousarray(scn.points[ex["less_sharp"]], np.float32)
            raw[i].append(scn)
            stack[i].append((orc.voxel_grid(surf_in, LEAF_SURF), orc.voxel_grid(corner_in, LEAF_CORNER)))      # (surf, corner) as cpp:487-495 leaves them
    return dict(T=T, exts_T=exts_T, scans=raw, stack=stack, to_pose=to_pose)


def drive(n_frames=4, n_lidars=2):
    """n_frames poses of the body, per (frame, LiDAR) the simulated scan and the (surf, corner) clouds of its slot: LiDAR frame, intensity as the extractor
    leaves it. Computed once per process and shared: do not modify."""
    return _drive(n_frames, n_lidars)


def pose_local(d, pivot, slots, n_lidars, perturb=True):
    """pose_local_[n][i] = Pose(T_pivot^-1 T_i T_ext) (cpp:1181) for slot i = frame slots[i], each perturbed as conftest.make_window_case perturbs its
    relative poses (so every (n, i) has its own): (n_lidars, len(slots), 7)"""
    import importlib
    synth = importlib.import_module("m-loam_amd.synth")
    Tinv = np.linalg.inv(d["T"][pivot])
    out = np.zeros((n_lidars, len(slots), 7))
    for n in range(n_lidars):
        for i, f in enumerate(slots):
            rel = d["to_pose"](Tinv @ d["T"][f] @ d["exts_T"][n])
            out[n, i] = synth.perturbed_pose(rel, seed=200 + 10 * i + n, dt=0.05, drot_deg=0.5) if perturb else rel
    return out


def loop_maps(transform, voxel, clouds, poses, window, source_lidar, leaf_surf, leaf_corner):
    """buildLocalMap / buildCalibMap as INTEGRATION.md's per-call loop: clouds[n][slot] = (surf, corner); transform(cloud, pose) and voxel(cloud, leaf) are the
    existing ABI's (ctx.transform_point_cloud / ctx.voxel_grid) or the oracle's -> per LiDAR [(pre_surf, ds_surf), (pre_corner, ds_corner)]"""
    out = []
    for n in range(len(clouds)):
        src = n if source_lidar < 0 else source_lidar
        per_kind = []
        for kind in range(2):
            parts = [transform(clouds[src][i][kind], poses[src][i]) for i in range(window) if len(clouds[src][i][kind])]
            pre = np.concatenate(parts) if parts else EMPTY
            leaf = (leaf_surf, leaf_corner)[kind][n]
            per_kind.append((pre, voxel(pre, leaf) if len(pre) else EMPTY))
        out.append(per_kind)
    return out


class CircularBuffer:
    """utility/CircularBuffer.h restated: resize (:61-67), operator[] (:134-137), push (:186-197)"""

    def __init__(self, capacity):
        self.capacity, self.size, self.start = capacity, 0, 0
        self.buf = [EMPTY] * capacity

    def __getitem__(self, i):
        return self.buf[(self.start + i) % self.capacity]

    def __setitem__(self, i, v):
        self.buf[(self.start + i) % self.capacity] = v

    def push(self, element):
        if self.size < self.capacity:
            self.buf[self.size] = element
            self.size += 1
        else:
            self.buf[self.start] = element
            self.start = (self.start + 1) % self.capacity
