#!/usr/bin/env python
"""bench.py -- scan-to-map residuals+Jacobians/sec on MI355X (BASELINE.json metric), one rank per GPU.

A *step* is one frame of the mapper's scan-to-map optimisation on synthetic input already resident in HBM:
  [local-map index rebuild for both maps, as the reference does every frame (lidar_mapper_keyframe.cpp:433-434)]
  + 5 Gauss-Newton iterations, each = transform -> exact 5-NN -> line/plane fit + gates -> residual + 1x6 Jacobian ->
    Huber -> 6x6 normal-equation reduction [-> RCCL all-reduce when N > 1] -> degeneracy check -> 6x6 solve -> Plus,
  device-resident (mlh_gn_solve). value = features LINEARISED per second: the valid correspondences -- those whose
  residual + 1x6 Jacobian were produced and reduced into the normal equations -- summed over the 5 iterations / step time, whole
  job; every query (valid or rejected) per second is reported beside it as `queries_per_s`. Workload at N = 1: BASELINE.json configs[1] (2 x 64-ring scan vs ~500k-point local map, 5 GN iterations).
  At N > 1 the map grows with N (1M / 2M / 4M points, configs[2..3]) and is sharded spatially across the ranks, the
  scan stays the same 2 x 64 rings -> "scaling": "strong" (total feature work is fixed). Because the map differs from the N = 1 line's,
  every N > 1 line also carries `multi_gpu.n1_same_map_ms_per_step`: rank 0 alone, unsharded, on THIS line's map, measured in the
  same process before the sharded leg -- the reference a strong-scaling ratio on one problem needs.

Launch for N > 1: either the driver's  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
                   --master-port P bench.py --gpus N --steps K --warmup W
                  or simply  python bench.py --gpus N ...  -- with WORLD_SIZE unset the script spawns its N ranks itself (the same
                  torch.distributed.run line, a free port). WORLD_SIZE set but different from --gpus is an error (exit 2), never a
                  silently smaller run. Fewer GPUs than ranks (a one-GPU box): the ranks share devices through the mailbox
                  communicator -- a functional check of the N > 1 path, flagged `ranks_share_gpus` in the line, not a scaling number.

Default run: set-up, clock spin-up, W warm-up steps, K timed steps, one JSON line with the headline (`value`, `ms_per_step`, the workload's `config`,
`final_pose`). `--full` adds everything else the script measures or checks: extraction timings, the fully bracketed per-kernel pass, HIP events on the
dominant kernel inside the timed region, the synchronous / keyframe-cadence / scan2map / whole-frame / out-grown-box / saturation legs, predicted scaling,
both rooflines, the CPU baseline and, at N > 1, the same-map N = 1 reference and the per-rank figures. `--dump-outputs DIR` writes the pose the last timed
step returned to DIR/pose.npy (float64; with --config4 also DIR/config4_poses.npy); the inputs are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this driver: RCCL across processes needs it

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GN_ITERS = 5
MAP_PRESET_BY_N = {1: "500k", 2: "1M", 4: "2M", 8: "4M"}
N_LIDARS, N_RINGS = 2, 64


def _sha(a):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_workload(synth, preset, seed=42, n_lidars=None):
    sc = synth.make_scene(seed=seed, **synth.SCENE_PRESETS[preset])
    surf_map, corner_map = synth.sample_maps(sc, seed=seed, kf_rings=N_RINGS, kf_lidars=n_lidars or N_LIDARS)
    gt = synth.gt_body_pose()
    scans = [synth.simulate_scan(sc, gt, synth.HERCULES_BODY_T_LASER[i], N_RINGS, seed=7 + i) for i in range(n_lidars or N_LIDARS)]
    return sc, surf_map, corner_map, gt, scans


def fuse_features(synth, scans, extracted, thin=True):
    """per-LiDAR extraction results -> the mapper's two feature clouds (reference-LiDAR frame, intensity = LiDAR id,
    visualization.cpp:40-52), thinned at MAP_SURF_RES / MAP_CORNER_RES as downsampleCurrentScan does."""
    surf, corner = [], []
    for i, (sc, ex) in enumerate(zip(scans, extracted)):
        T = np.eye(4)
        T[:3, :3] = synth.quat_to_rot(synth.HERCULES_BODY_T_LASER[i][:4])
        T[:3, 3] = synth.HERCULES_BODY_T_LASER[i][4:7]
        for lst, key, res in ((corner, "less_sharp", None), (surf, "less_flat_raw", 0.2)):
            pts = sc.points[ex[key]][:, :3]
            if res and thin:   # the per-ring 0.2 m VoxelGrid of extractCloud (cpp:266-271), as data preparation here
                pts = synth.voxel_mean(pts, res)
            a = np.zeros((len(pts), 4), np.float32)
            a[:, :3] = synth.transform_points(pts, T)
            a[:, 3] = i
            lst.append(a)
    surf, corner = np.concatenate(surf), np.concatenate(corner)
    if thin:
        surf = synth.voxel_mean(surf, 0.4)
        corner = synth.voxel_mean(corner, 0.2)
    surf[:, 3] = np.round(surf[:, 3])
    corner[:, 3] = np.round(corner[:, 3])
    return np.ascontiguousarray(surf), np.ascontiguousarray(corner)


def candidate_stats(map_pts, feats_xyz_map, h):
    """Per query (properties of scene, N and pose): C = map points in the 27-cell neighbourhood; C_ball = map points in the cells that
    intersect the ball of the 5th-neighbour distance (capped at the acceptance radius) -- what an ideally pruned search has to read.
    Returns (mean C, mean C_ball) over the queries inside the grid."""
    from scipy.spatial import cKDTree
    o = map_pts.min(axis=0)
    ijk = np.floor((map_pts - o) / h).astype(np.int64)
    dims = ijk.max(axis=0) + 1
    cnt = np.zeros(tuple(dims + 2), np.int64)   # 1-cell border of zeros
    np.add.at(cnt, (ijk[:, 0] + 1, ijk[:, 1] + 1, ijk[:, 2] + 1), 1)
    rel = (feats_xyz_map - o) / h
    q = np.floor(rel).astype(np.int64)
    frac = (rel - q) * h
    ok = np.all((q >= -1) & (q <= dims), axis=1)
    q = np.clip(q, -1, dims) + 1
    if len(feats_xyz_map) == 0 or not ok.any():
        return 0.0, 0.0
    d5 = cKDTree(map_pts).query(feats_xyz_map, k=5)[0][:, 4] if len(map_pts) >= 5 else np.full(len(feats_xyz_map), np.inf)
    r2 = np.minimum(d5, h) ** 2
    tot = np.zeros(len(q), np.int64)
    ball = np.zeros(len(q), np.int64)
    gap = lambda d, f: np.where(d < 0, f, np.where(d > 0, h - f, 0.0))
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                a, b, c = q[:, 0] + dx, q[:, 1] + dy, q[:, 2] + dz
                inb = (a >= 0) & (a < dims[0] + 2) & (b >= 0) & (b < dims[1] + 2) & (c >= 0) & (c < dims[2] + 2)
                n = np.where(inb, cnt[np.clip(a, 0, dims[0] + 1), np.clip(b, 0, dims[1] + 1), np.clip(c, 0, dims[2] + 1)], 0)
                tot += n
                g2 = gap(dx, frac[:, 0]) ** 2 + gap(dy, frac[:, 1]) ** 2 + gap(dz, frac[:, 2]) ** 2
                ball += np.where(g2 <= r2, n, 0)
    return float(tot[ok].mean()), float(ball[ok].mean())


def predicted_scaling(mla, torch, shard, device, surf_map, corner_map, surf, corner, p_conv, center, reps=40):
    """What a run over N GPUs should show on THIS frame and map, stated before such a run exists (no multi-GPU box has been reachable: SCALE_r0N.json are `skipped`
    records). Every prospective rank's share -- its map shard (wedge + 1.1 m halo) or the whole map, its ownership test, all features staged -- runs ALONE on this GPU:
    the index build of its maps (host clock around mlh_map_set_pair) and ONE Gauss-Newton iteration at the converged pose, whose two launches are timed by their own
    dispatch timestamps (correspondence kernel; fit kernel with the classic finish a sharded iteration keeps). The degeneracy test is switched off for this
    measurement (map_eig_thre < 0): a rank's LOCAL sums are degenerate in a narrow wedge and would take the eigen-decomposition path, which the real iteration -- it
    solves on the exchanged, global sums -- does not (first version of this leg: 1.07 ms for an eighth of the features). A sharded step is then
    index build + 5 x (correspondence + fit + exchange) of the slowest rank; exchange_us is an ASSUMPTION until measured across xGMI: 5 us (a peer store + flag + poll
    round; 9.5 us was measured between two processes time-sharing one GPU, profiles/r03_p2p_multirank.txt)."""
    ex_us = 5.0
    per = {}
    c = mla.Context(device)
    try:
        opts = mla.default_opts(map_eig_thre=-1.0)
        d_s, d_c = torch.from_numpy(surf).cuda(), torch.from_numpy(corner).cuda()
        far = np.full((1, 3), 1.0e6, np.float32)
        c.set_gn_schedule(0, 0, 0)
        for mode in ("map", "features"):
            for n in (1, 2, 4, 8):
                if n == 1 and mode == "features":
                    continue
                ranks = []
                for r in range(n):
                    if mode == "map" and n > 1:
                        ms_ = shard.shard_points_mask(surf_map, center, n, r); mc_ = shard.shard_points_mask(corner_map, center, n, r)
                        lsm, lcm = np.ascontiguousarray(surf_map[ms_]), np.ascontiguousarray(corner_map[mc_])
                        lsm = lsm if len(lsm) else far; lcm = lcm if len(lcm) else far
                    else:
                        lsm, lcm = surf_map, corner_map
                    d_sm, d_cm = torch.from_numpy(np.ascontiguousarray(lsm)).cuda(), torch.from_numpy(np.ascontiguousarray(lcm)).cuda()
                    torch.cuda.synchronize()
                    c.shard_set(None, None)
                    c.shard_set_features(1, 0)
                    if n > 1 and mode == "map":
                        c.shard_set(*shard.wedge_planes(center, n, r))
                    elif n > 1:
                        c.shard_set_features(n, r)
                    c.map_set_pair(d_sm, d_cm)
                    c.features_set(mla.SURF, d_s); c.features_set(mla.CORNER, d_c)
                    for _ in range(5):
                        c.map_set_pair(d_sm, d_cm); c.gn_solve(p_conv, 1, opts, want_stats=False)
                    c.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        c.map_set_pair(d_sm, d_cm)
                    c.synchronize()
                    build_us = 1e6 * (time.perf_counter() - t0) / reps
                    c.profile_enable((1 << mla.K_KNN) | (1 << mla.K_FIT))
                    c.profile_reset()
                    for _ in range(reps):
                        c.gn_solve(p_conv, 1, opts, want_stats=False)
                    knn_ms, knn_n = c.profile_get(mla.K_KNN)
                    fit_ms, fit_n = c.profile_get(mla.K_FIT)
                    c.profile_enable(0)
                    ranks.append(dict(index_build_us=round(build_us, 2), knn_us=round(1e3 * knn_ms / max(knn_n, 1), 2), fit_us=round(1e3 * fit_ms / max(fit_n, 1), 2)))
                per[f"{mode}_n{n}"] = ranks
    finally:
        c.close()

    def step_ms(ranks, with_exchange):
        return max(r_["index_build_us"] + GN_ITERS * (r_["knn_us"] + r_["fit_us"] + (ex_us if with_exchange else 0.0)) for r_ in ranks) * 1e-3
    n1 = step_ms(per["map_n1"], False)
    pred = {}
    for k, v in per.items():
        if k == "map_n1":
            continue
        st = step_ms(v, True)
        pred[k] = dict(per_rank_alone=v, predicted_ms_per_step=round(st, 4), predicted_speedup_vs_n1=round(n1 / st, 3))
    return dict(n1_same_method_ms_per_step=round(n1, 4), n1_per_rank_alone=per["map_n1"], assumed_exchange_us=ex_us, splits=pred,
                note="each prospective rank's share of THIS frame alone on this GPU: index build of its maps + one classic-schedule GN iteration at the converged pose (kernel "
                     "durations from the dispatches' own timestamps, degeneracy test off: see predicted_scaling's docstring); predicted step = slowest rank's index build + 5 x "
                     "(correspondence + fit + assumed exchange). `map`: angular wedges + 1.1 m halo; `features`: whole map on every rank, features dealt round-robin. The frame does "
                     "not fill one GPU (21 k queries): a rank's launches are bound by the same latency chain whatever its share, so the wedge split buys index-build time and "
                     "little else, and no split of this frame approaches the north star's 6x at 8 GPUs. Stated so that the first cross-GPU SCALE run can be checked against it")


def single_gpu_reference(mla, torch, device, surf_map, corner_map, surf, corner, p0, steps, warmup):
    """the frame of this run on ONE GPU, whole map, no communicator: ms per step (map staging + index build + 5 GN iterations) with synchronous submission
    and with the pipelined + overlapped-staging submission of the N = 1 bench line. Used by rank 0 of an N > 1 run as the same-map reference."""
    c = mla.Context(device)
    try:
        d_sm, d_cm = torch.from_numpy(np.ascontiguousarray(surf_map)).cuda(), torch.from_numpy(np.ascontiguousarray(corner_map)).cuda()
        d_s, d_c = torch.from_numpy(surf).cuda(), torch.from_numpy(corner).cuda()
        torch.cuda.synchronize()
        c.map_set_pair(d_sm, d_cm)
        c.features_set(mla.SURF, d_s)
        c.features_set(mla.CORNER, d_c)
        opts = mla.default_opts()
        pose_conv, st = c.gn_solve(p0, GN_ITERS, opts, want_stats=True)
        n_valid = int(sum(int(x["n_surf"]) + int(x["n_corner"]) for x in st))
        t_sp = time.perf_counter()
        while time.perf_counter() - t_sp < 0.15:      # clocks up (see the spin-up note in main)
            c.map_set_pair(d_sm, d_cm)
            c.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        for _ in range(warmup):
            c.map_set_pair(d_sm, d_cm)
            c.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            c.map_set_pair(d_sm, d_cm)
            c.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        c.synchronize()
        ms_sync = 1e3 * (time.perf_counter() - t0) / steps
        # pipelined + overlapped staging, as main()'s N = 1 loop
        c.map_set_pair(d_sm, d_cm)
        c.gn_solve_begin(p0, GN_ITERS, opts)
        for _ in range(warmup):
            c.map_set_pair_overlapped(d_sm, d_cm)
            c.gn_solve_begin_chained(pose_conv, p0, GN_ITERS, opts)
            c.gn_solve_end()
        c.gn_solve_end()
        c.synchronize()
        t0 = time.perf_counter()
        c.map_set_pair(d_sm, d_cm)
        c.gn_solve_begin(p0, GN_ITERS, opts)
        for _ in range(steps - 1):
            c.map_set_pair_overlapped(d_sm, d_cm)
            c.gn_solve_begin_chained(pose_conv, p0, GN_ITERS, opts)
            c.gn_solve_end()
        c.gn_solve_end()
        c.synchronize()
        ms_pipe = 1e3 * (time.perf_counter() - t0) / steps
        return dict(ms_per_step=round(ms_sync, 4), ms_per_step_pipelined=round(ms_pipe, 4), valid_correspondences_per_step=n_valid,
                    value=round(n_valid / (1e-3 * ms_sync), 1), map_points=int(len(surf_map) + len(corner_map)),
                    submission="synchronous (as the sharded loop); `ms_per_step_pipelined` = the N = 1 bench line's submission mode on this map")
    finally:
        c.close()


CFG4_K, CFG4_THRE, CFG4_FREEZE = [5, 10, 10, 10], [100.0, 70.0, 70.0, 70.0], [0, 1, 1, 1]


def config4_blocks(mla, synth, ctx, scans4, gt):
    """BASELINE config 4's frame: per LiDAR its own feature clouds (less-sharp corners, per-ring-thinned less-flat surfs, thinned at the mapper's resolutions)
    and its own pose block -- the body pose for the reference LiDAR, the extrinsic-composed pose for the others (buildCalibMap, estimator.cpp:1067-1157)"""
    from scipy.spatial.transform import Rotation as Rot
    surf_b, corner_b, poses0 = [], [], []
    for i, s_ in enumerate(scans4):
        ex = ctx.extract(s_.points, s_.scan_start, s_.scan_end, voxel_leaf=0.2)
        c_ = np.zeros((len(ex["less_sharp"]), 4), np.float32)
        c_[:, :3] = s_.points[ex["less_sharp"]][:, :3]
        surf_b.append(np.ascontiguousarray(synth.voxel_mean(ex["less_flat_ds"].copy(), 0.4)))
        corner_b.append(np.ascontiguousarray(synth.voxel_mean(c_, 0.2)))
        bl = synth.HERCULES_BODY_T_LASER[i]
        T = synth.pose_to_mat(gt) @ np.block([[synth.quat_to_rot(bl[:4]), bl[4:7, None]], [np.zeros((1, 3)), np.ones((1, 1))]])
        gt_i = np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
        poses0.append(synth.perturbed_pose(gt_i, seed=50 + i, dt=0.1, drot_deg=1.0))
    return surf_b, corner_b, np.array(poses0)


def single_gpu_config4(mla, torch, device, surf_map, corner_map, surf_b, corner_b, poses0, steps, warmup):
    """config 4's frame on ONE GPU, whole map, no communicator (rank 0 of an N > 1 run: the same-map reference of the sharded config-4 leg)"""
    c = mla.Context(device)
    try:
        d_sm, d_cm = torch.from_numpy(np.ascontiguousarray(surf_map)).cuda(), torch.from_numpy(np.ascontiguousarray(corner_map)).cuda()
        torch.cuda.synchronize()
        c.map_set_pair(d_sm, d_cm)
        c.features_set_blocks(mla.SURF, surf_b)
        c.features_set_blocks(mla.CORNER, corner_b)
        o4 = mla.default_opts(flags=mla.FLAG_CHECK_FOV, huber_delta=1.0)

        def frame():
            c.map_set_pair(d_sm, d_cm)
            return c.gn_solve_blocks(poses0, GN_ITERS, CFG4_K, CFG4_THRE, CFG4_FREEZE, o4, want_stats=False)
        t_sp = time.perf_counter()
        while time.perf_counter() - t_sp < 0.15:
            frame()
        for _ in range(warmup):
            frame()
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out_ = frame()
        c.synchronize()
        return dict(ms_per_step=round(1e3 * (time.perf_counter() - t0) / steps, 4), poses=np.asarray(out_[0]).tolist())
    finally:
        c.close()


def block_sharded_config4(mla, torch, dist, dist_dev, device, rank, world, surf_map, corner_map, surf_b, corner_b, poses0, steps, warmup):
    """config 4's frame with its POSE BLOCKS dealt over the ranks and the map replicated: the blocks' normal equations are independent (one 7-parameter block per
    LiDAR: LidarOnlineCalib* factors carry a single parameter block each, estimator.cpp:1067-1157), so no rank ever needs another rank's sums -- no collective in the
    data path, one barrier around the timed region. Every rank: its own context (no communicator), the WHOLE map staged + indexed per step, its blocks through
    mlh_gn_solve_blocks. Returns (max-over-ranks seconds per step, poses of all blocks gathered on every rank, owner table)."""
    owner = importlib.import_module("m-loam_amd.shard").block_owner(len(surf_b), world)
    mine = [b for b, r_ in enumerate(owner) if r_ == rank]
    c = mla.Context(device)
    try:
        d_sm, d_cm = torch.from_numpy(np.ascontiguousarray(surf_map)).cuda(), torch.from_numpy(np.ascontiguousarray(corner_map)).cuda()
        torch.cuda.synchronize()
        o4 = mla.default_opts(flags=mla.FLAG_CHECK_FOV, huber_delta=1.0)
        if mine:
            c.map_set_pair(d_sm, d_cm)
            c.features_set_blocks(mla.SURF, [surf_b[b] for b in mine])
            c.features_set_blocks(mla.CORNER, [corner_b[b] for b in mine])
        k_, t_, f_ = [CFG4_K[b] for b in mine], [CFG4_THRE[b] for b in mine], [CFG4_FREEZE[b] for b in mine]
        p_ = np.ascontiguousarray(np.asarray(poses0)[mine]) if mine else None
        out_ = [None]

        def frame():
            if mine:
                c.map_set_pair(d_sm, d_cm)
                out_[0] = c.gn_solve_blocks(p_, GN_ITERS, k_, t_, f_, o4, want_stats=False)[0]
        t_sp = time.perf_counter()
        while time.perf_counter() - t_sp < 0.15:
            frame()
        for _ in range(warmup):
            frame()
        c.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            frame()
        c.synchronize()
        dist.barrier()
        tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dist_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        poses = torch.zeros((len(surf_b), 7), dtype=torch.float64, device=dist_dev)
        for i_, b in enumerate(mine):
            poses[b] = torch.from_numpy(np.asarray(out_[0])[i_]).to(dist_dev)
        dist.all_reduce(poses)          # every block has exactly one owner: the sum is a gather
        return float(tt.item()) / steps, poses.cpu().numpy(), owner
    finally:
        c.close()


def framebench_cpp(all_pts, all_start, all_end, ring_ofs, ext, covs, meas, surf_map, corner_map, p0, frames=60, mode="all", timeout=240):
    """The frame driven from C++ threads through the C-ABI (m-loam_amd/host/framebench.cpp): an estimator-side thread and a mapper-side thread on two contexts
    (the reference's process structure: estimator.cpp:100 process_thread_, lidar_mapper_keyframe.cpp:1315 mapping_process) -> frame PERIOD; K independent
    pipelines on the one GPU -> aggregate frames per second. The executable is built by __graft_entry__.build() and travels with the snapshot; its scans are HOST
    buffers (every frame pays its upload)."""
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "m-loam_amd", "host", "framebench")
    if not os.path.exists(exe):
        return dict(error="m-loam_amd/host/framebench has not been built (__graft_entry__.build())")
    with tempfile.TemporaryDirectory() as d:
        np.ascontiguousarray(all_pts, np.float32).tofile(os.path.join(d, "fb_points.f32"))
        np.concatenate([all_start, all_end]).astype(np.int32).tofile(os.path.join(d, "fb_rings.i32"))
        np.asarray(ring_ofs, np.int32).tofile(os.path.join(d, "fb_ring_ofs.i32"))
        np.ascontiguousarray(ext, np.float64).tofile(os.path.join(d, "fb_ext.f64"))
        np.ascontiguousarray(covs, np.float64).tofile(os.path.join(d, "fb_covs.f64"))
        np.ascontiguousarray(meas, np.float64).tofile(os.path.join(d, "fb_meas.f64"))
        sm, cm = np.ascontiguousarray(surf_map, np.float32), np.ascontiguousarray(corner_map, np.float32)
        sm.tofile(os.path.join(d, "fb_surf_map.f32")); cm.tofile(os.path.join(d, "fb_corner_map.f32"))
        np.array([sm.shape[1] * 4, 1], np.int32).tofile(os.path.join(d, "fb_meta.i32"))
        np.ascontiguousarray(p0, np.float64).tofile(os.path.join(d, "fb_pose.f64"))
        r = subprocess.run([exe, d, str(int(frames)), mode], capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return dict(error=(r.stderr.strip() or r.stdout.strip())[-300:], rc=r.returncode)
    return json.loads(lines[-1])


def self_launch(n_ranks):
    """`python bench.py --gpus N` without a launcher: re-run this very command line under torch.distributed.run with N ranks and pass its exit code on"""
    import socket
    import subprocess
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"bench.py: --gpus {n_ranks} without a launcher (WORLD_SIZE unset): spawning the ranks: {' '.join(cmd)}")
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n_ranks)))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-map-rebuild", action="store_true", help="leave the map index build out of the step")
    ap.add_argument("--map-rebuild-only", action="store_true",
                    help="per step only re-index the resident map (mlh_map_rebuild: no staging, no bounds pass) instead of mlh_map_set")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--dense-features", action="store_true",
                    help="supplementary saturation run: do NOT thin the scan features at MAP_SURF_RES/MAP_CORNER_RES (not BASELINE's workload)")
    ap.add_argument("--lidars", type=int, default=N_LIDARS, choices=[1, 2, 3, 4],
                    help="supplementary: number of 64-ring LiDARs in the frame (BASELINE's metric is quoted on 2)")
    ap.add_argument("--map-preset", default=None, choices=["50k", "500k", "1M", "2M", "4M"],
                    help="supplementary: local-map size (default: 500k at N=1, 500k x N at N GPUs as BASELINE's configs 2-4 grow it)")
    ap.add_argument("--shard-mode", default="map", choices=["map", "features"],
                    help="N > 1: 'map' = angular wedges of the map + halo, ownership by position (BASELINE's partition); 'features' = whole map on every "
                         "rank, features dealt round-robin (SURVEY 8e's balanced alternative)")
    ap.add_argument("--config4", action="store_true",
                    help="the step is BASELINE config 4's frame instead of config 2's: 4 x 64 rings, one pose block per LiDAR (body pose + 3 extrinsics; N_NEIGH 5/10/10/10, "
                         "CHECK_FOV, freeze-on-degenerate, Huber 1.0) through mlh_gn_solve_blocks, sharded like the single-pose frame. At --gpus 8 the same frame is "
                         "measured as a supplementary leg (`config4` in the line) even without this flag")
    ap.add_argument("--comm", default="p2p", choices=["p2p", "rccl", "both"],
                    help="N > 1: the collective behind the sharded solver -- 'p2p' = the mailbox communicator (hipIpc-mapped mailboxes, one kernel per all-reduce; "
                         "falls back to RCCL if it cannot be set up or its first all-reduce does not add up), 'rccl' = ncclAllReduce, 'both' = the timed loop once "
                         "with each (value from the mailbox run, the RCCL run reported beside it; needs a GPU per rank)")
    ap.add_argument("--no-overlap-staging", action="store_true",
                    help="pipelined submission, but the next frame's maps are staged on the solver's own stream (queued behind the solve) instead of on a second stream")
    ap.add_argument("--synchronous", action="store_true",
                    help="read every frame's pose before the next frame's map staging is enqueued (rounds 1-2's loop) instead of one frame late")
    ap.add_argument("--restage-every", type=int, default=0,
                    help="every K-th frame is saved as a KEYFRAME: the local map of the frame after it contains that frame's own cloud at its solved pose "
                         "(lidar_mapper_keyframe.cpp:641-688, 254-354), so its staging cannot be overlapped with the solve -- the pose is collected first, the maps are staged "
                         "on an idle stream, the solve starts from a host-side pose. 0: never (every frame reuses the previous frame's local map, as the reference does "
                         "between keyframes: cpp:257-261). The default line reports the cadences 1 / 2 / 5 / 10 beside `value` (`keyframe_cadence`)")
    ap.add_argument("--no-supplementary", action="store_true",
                    help="only the contract's loop and the per-kernel pass: no saturation leg (un-thinned features), no keyframe-cadence loops, no scan2map / out-grown-box legs -- "
                         "for kernel traces and PMC passes, whose per-kernel averages should be the headline workload's alone")
    ap.add_argument("--spinup-ms", type=float, default=150.0,
                    help="milliseconds of an unrelated torch matmul before the warm-up steps (clock ramp of a GPU that idled through the host-side setup); 0: none")
    ap.add_argument("--profile-events", type=int, default=None,
                    help="1: HIP-event bracket the dominant kernel (surf correspondence) inside the timed region; 0: none. Default: 1 with --full "
                         "(the roofline reads them), 0 otherwise")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: per-LiDAR extraction timings, the fully bracketed per-kernel pass, the synchronous and keyframe-cadence "
                         "loops, scan2map / whole-frame / out-grown-box / saturation legs, predicted scaling, both rooflines, the CPU baseline and, at N > 1, the "
                         "same-map N = 1 reference and the per-rank figures. Without it the run sets up, warms up, times the steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step to DIR/<name>.npy (float64): pose.npy = the pose of the "
                         "last timed frame [x, y, z, qx, qy, qz, qw]; with --config4 also config4_poses.npy = its four pose blocks")
    args = ap.parse_args()
    full = args.full
    if args.profile_events is None:
        args.profile_events = 1 if full else 0

    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)                      # does not return

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        # never a silently smaller (or larger) job than the one asked for: the line's n_gpus would not be the caller's N
        log(f"bench.py: FATAL: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
        raise SystemExit(2)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    # More ranks than GPUs (a one-GPU box, for checking the N > 1 path): the ranks share devices -- the mailbox communicator allows that, RCCL and the "nccl"
    # process group do not, so the bookkeeping collectives below go through gloo on host tensors then. On a node with a GPU per rank nothing changes.
    shared_gpus = world > torch.cuda.device_count()
    if shared_gpus:
        local_rank = local_rank % torch.cuda.device_count()
        if args.comm == "rccl":
            raise SystemExit("bench.py: fewer GPUs than ranks needs --comm p2p (RCCL wants a GPU per rank)")
    torch.cuda.set_device(local_rank)
    dist_dev = "cpu" if shared_gpus else "cuda"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (gloo announces its connections on the process's stdout, from C++: kept off the line this script owes its caller)
        sys.stdout.flush()
        _fd1 = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("gloo" if shared_gpus else "nccl", rank=rank, world_size=world)
        finally:
            sys.stdout.flush()
            os.dup2(_fd1, 1)
            os.close(_fd1)

    mla = importlib.import_module("m-loam_amd")
    synth = importlib.import_module("m-loam_amd.synth")
    shard = importlib.import_module("m-loam_amd.shard")

    preset = args.map_preset or MAP_PRESET_BY_N.get(world, "500k")
    t0 = time.time()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sc, surf_map, corner_map, gt, scans = build_workload(synth, preset, n_lidars=args.lidars)
    p0 = synth.perturbed_pose(gt, seed=43)
    ctx = mla.Context(local_rank)

    # --- feature extraction on the GPU (the product's extractCloud), one launch set per LiDAR; timed separately (--full)
    extracted, extract_ms = [], []
    for s in scans:
        ctx.scan_upload(s.points, s.scan_start, s.scan_end)
        ctx.extract_run()          # warm (without --full: the one run whose lists the features are made of)
        if full:
            ctx.synchronize()
            ctx.profile_enable(1 << mla.K_EXTRACT)
            ctx.profile_reset()
            for _ in range(10):
                ctx.extract_run()
            ms, n = ctx.profile_get(mla.K_EXTRACT)
            ctx.profile_enable(0)
            extract_ms.append(ms / max(n, 1))
        extracted.append(ctx.extract_fetch())
    # all LiDARs of the frame as ONE scan (clouds concatenated, ring tables offset): a ring is a workgroup, so the launch set costs the
    # same as for one LiDAR
    offs = np.cumsum([0] + [len(s.points) for s in scans])
    all_pts = np.concatenate([s.points for s in scans])
    all_start = np.concatenate([s.scan_start + offs[i] for i, s in enumerate(scans)]).astype(np.int32)
    all_end = np.concatenate([s.scan_end + offs[i] for i, s in enumerate(scans)]).astype(np.int32)
    if full:
        ctx.scan_upload(all_pts, all_start, all_end)
        ctx.extract_run()
        ctx.synchronize()
        ctx.profile_enable(1 << mla.K_EXTRACT)
        ctx.profile_reset()
        for _ in range(10):
            ctx.extract_run()
        ms, nn = ctx.profile_get(mla.K_EXTRACT)
        ctx.profile_enable(0)
        extract_all_ms = ms / max(nn, 1)
        both = ctx.extract_fetch()
        n_sharp_each = sum(len(e["sharp"]) for e in extracted)
        assert len(both["sharp"]) == n_sharp_each, "batched extraction must give the per-LiDAR results back to back"
    surf, corner = fuse_features(synth, scans, extracted, thin=not args.dense_features)
    n_scan_points = int(sum(len(s.points) for s in scans))

    # --- N > 1, before anything is sharded: the SAME frame on the SAME (whole) map by rank 0 alone, unsharded, no communicator -- the N = 1 reference of this line's
    #     problem (the N = 1 bench line uses the 500k map; a ratio against it would compare two problems). Synchronous submission, like the sharded loop below, and
    #     the pipelined form beside it. A context of its own, closed before the sharded leg starts; the other ranks wait at the barrier.
    n1_ref = None
    if world > 1 and full:
        if rank == 0:
            n1_ref = single_gpu_reference(mla, torch, local_rank, surf_map, corner_map, surf, corner, p0, args.steps, args.warmup)
            log(f"[rank 0] same-map N=1 reference ({preset}): {n1_ref}")
        dist.barrier()

    # --- map shards (N > 1): angular wedges around the predicted sensor position, halo 1.1 m
    center = p0[:2]
    comm_state = dict(kind=None, ranks_seen=None)

    def comm_setup(want):
        """joins the ranks with the mailbox communicator ('p2p', falling back to RCCL) or RCCL ('rccl'); exits the whole job (3) when neither comes up"""
        comm_kind = "rccl"
        if want == "p2p":
            # the mailbox communicator: handles all-gathered through the process group, every rank maps every mailbox, one all-reduce of ones as the check
            ok_p2p = 1
            try:
                handles = [None] * world
                dist.all_gather_object(handles, ctx.p2p_mailbox())
                ctx.p2p_comm_init(world, rank, handles)
            except Exception as e:   # noqa: BLE001 -- reported below, never silent
                ok_p2p = 0
                log(f"[rank {rank}] mailbox communicator not available: {e!r}")
            flag = torch.tensor([ok_p2p], dtype=torch.int32, device=dist_dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 1:
                try:
                    ok_p2p = int(float(ctx.allreduce_f64(np.ones(32))[0]) == float(world))
                except Exception as e:   # noqa: BLE001
                    ok_p2p = 0
                    log(f"[rank {rank}] mailbox all-reduce failed: {e!r}")
                flag = torch.tensor([ok_p2p], dtype=torch.int32, device=dist_dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 1:
                comm_kind = "p2p"
            else:
                ctx.comm_finalize()
                log(f"[rank {rank}] falling back to RCCL")
        comm_ok, comm_err = 1, ""
        uid = [None]
        if rank == 0 and comm_kind == "rccl":
            try:
                uid[0] = mla.comm_unique_id()
            except Exception as e:   # noqa: BLE001 -- reported, never silent
                comm_err = repr(e)
        dist.broadcast_object_list(uid, src=0)      # always executed, so no rank is left waiting
        if uid[0] is None and comm_kind == "rccl":
            comm_ok = 0
        else:
            try:
                if args.shard_mode == "map":
                    ctx.shard_set(lo, hi)
                else:
                    ctx.shard_set_features(world, rank)
                if comm_kind == "rccl":
                    if shared_gpus:
                        raise RuntimeError("RCCL needs a GPU per rank; this box has fewer GPUs than ranks")
                    ctx.comm_init(world, rank, uid[0])
            except Exception as e:   # noqa: BLE001
                comm_ok, comm_err = 0, repr(e)
        flag = torch.tensor([comm_ok], dtype=torch.int32, device=dist_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            # no silent degradation to independent replicas: a sharded run without its collective is not a scaling measurement
            log(f"[rank {rank}] FATAL: no communicator ({comm_err or 'failed on another rank'})")
            dist.destroy_process_group()
            raise SystemExit(3)
        comm_state["kind"] = comm_kind
        comm_state["ranks_seen"] = int(round(float(ctx.allreduce_f64(np.ones(32))[0])))      # what the collective itself says the job's size is
        if comm_state["ranks_seen"] != world:
            log(f"[rank {rank}] FATAL: the communicator spans {comm_state['ranks_seen']} ranks, not {world}")
            dist.destroy_process_group()
            raise SystemExit(3)
        return comm_kind

    if world > 1:
        if args.shard_mode == "map":
            ms_ = shard.shard_points_mask(surf_map, center, world, rank)
            mc_ = shard.shard_points_mask(corner_map, center, world, rank)
            local_surf_map, local_corner_map = np.ascontiguousarray(surf_map[ms_]), np.ascontiguousarray(corner_map[mc_])
        else:
            local_surf_map, local_corner_map = surf_map, corner_map
        far = np.full((1, 3), 1.0e6, np.float32)     # a wedge without any map point still needs a (never matched) record
        if len(local_surf_map) == 0:
            local_surf_map = far
        if len(local_corner_map) == 0:
            local_corner_map = far
        lo, hi = shard.wedge_planes(center, world, rank)
        comm_kind = comm_setup("rccl" if args.comm == "rccl" else "p2p")
    else:
        local_surf_map, local_corner_map = surf_map, corner_map
        comm_kind = None
    # inputs resident in HBM before the timed region
    d_surf_map = torch.from_numpy(local_surf_map).cuda()
    d_corner_map = torch.from_numpy(local_corner_map).cuda()
    d_surf, d_corner = torch.from_numpy(surf).cuda(), torch.from_numpy(corner).cuda()
    torch.cuda.synchronize()    # the library works on its own stream: the uploads above (torch's stream) must have landed first
    ctx.map_set(mla.SURF, d_surf_map)
    ctx.map_set(mla.CORNER, d_corner_map)
    ctx.features_set(mla.SURF, d_surf)
    ctx.features_set(mla.CORNER, d_corner)
    opts = mla.default_opts()
    m_total = len(surf) + len(corner)
    log(f"[rank {rank}] workload {args.lidars}x{N_RINGS} rings ({n_scan_points} pts) vs {preset} map "
        f"(surf {len(surf_map)} corner {len(corner_map)}; local {len(local_surf_map)}/{len(local_corner_map)}), "
        f"features surf {len(surf)} corner {len(corner)}; setup {time.time() - t0:.1f}s")

    def stage_maps():
        # a frame's local map arrives as a (device-resident) cloud: mlh_map_set = staging + bounds pass + index build, what the
        # reference pays as kdtree->setInputCloud every frame (lidar_mapper_keyframe.cpp:433-434)
        if args.map_rebuild_only:
            ctx.map_rebuild(mla.ALL_KINDS)
        elif not args.no_map_rebuild:
            if pipelined and in_flight[0] and not args.no_overlap_staging:
                ctx.map_set_pair_overlapped(d_surf_map, d_corner_map)      # next frame's index built on a second stream, into the other map set
            else:
                ctx.map_set_pair(d_surf_map, d_corner_map)

    def step_sync():
        stage_maps()
        return ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)[0]

    # Frame submission (round 3). A step is the same work as before -- staging + index build of both maps, then 5 Gauss-Newton iterations -- but frame k's
    # solve is SUBMITTED (mlh_gn_solve_begin) and its pose collected (mlh_gn_solve_end) after frame k + 1's map staging has been enqueued behind it: the GPU no
    # longer idles through the host's turn-around at every frame boundary (~16 us of a 183 us step in the synchronous loop, profiles/r03_step_timeline.txt).
    # Every pose is still read by the host, one frame late; the timed region ends with the last pose collected and the stream drained.
    # Several ranks: synchronous. (With the mailbox communicator the split submission works -- the exchange lives inside the launches -- and was tried with ranks
    # SHARING a GPU: 0.23 -> 0.52 ms per step at N = 2, because queued launches of one process spin on flags that the other process's launches, queued behind
    # them on the same device, are to set. With a GPU per rank that does not arise; not measurable here, so not the default.)
    pipelined = (world == 1) and not args.synchronous
    in_flight = [False]

    frame_no = [0]
    cadence = [args.restage_every]

    def step():
        if not pipelined:
            return step_sync()
        frame_no[0] += 1
        if cadence[0] > 0 and in_flight[0] and frame_no[0] % cadence[0] == 0:
            # the previous frame was saved as a keyframe: this frame's local map needs that frame's pose. Collect it, stage on the idle stream, start from a host pose
            pose_prev = drain()
            stage_maps()
            ctx.gn_solve_begin(p0, GN_ITERS, opts)
            in_flight[0] = True
            return pose_prev
        stage_maps()
        if in_flight[0]:
            # frame k submitted behind frame k - 1, which is still running: its start pose is the reference's chain -- transformUpdate with frame k - 1's result,
            # transformAssociateToMap with frame k's odometry (lidar_mapper_keyframe.cpp:145-160) -- evaluated on the device (mlh_gn_solve_begin_chained). The
            # synthetic odometry says "frame k - 1 ended at the converged pose, frame k starts at p0 again", so every frame starts within 1e-15 of p0 and does
            # the work of the solve counted above; the dependency on the previous frame's result is real and stays on the device.
            ctx.gn_solve_begin_chained(pose_converged, p0, GN_ITERS, opts)
            pose_prev = ctx.gn_solve_end()               # ... then frame k - 1's pose collected: the GPU goes from one frame straight into the next
        else:
            ctx.gn_solve_begin(p0, GN_ITERS, opts)
            pose_prev = None
        in_flight[0] = True
        return pose_prev

    def drain():
        if in_flight[0]:
            in_flight[0] = False
            return ctx.gn_solve_end()
        return None

    # valid correspondences per iteration (deterministic: the timed steps repeat exactly this solve)
    if world > 1 and comm_kind == "p2p":
        # the first SHARDED solve is the mailbox communicator's first exchange inside a solver launch (peer stores + flags between GPUs while kernels run). If it
        # fails on any rank -- a peer's flag never becomes visible, reported by the solve itself after its 5 s bound -- every rank moves to RCCL together
        # instead of the job dying with its measurement
        ok_first = 1
        try:
            ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        except Exception as e:   # noqa: BLE001 -- reported, never silent
            ok_first = 0
            log(f"[rank {rank}] first sharded solve over the mailbox communicator failed: {e!r}")
        flag = torch.tensor([ok_first], dtype=torch.int32, device=dist_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            log(f"[rank {rank}] falling back to RCCL for the sharded solver")
            ctx.comm_finalize()
            comm_kind = comm_setup("rccl")
            comm_state["fallback"] = "the first sharded solve over the mailbox communicator failed; the run continued over RCCL"
    pose_converged, it_stats = ctx.gn_solve(p0, GN_ITERS, opts, want_stats=True)
    n_valid_iter = [(int(s_["n_surf"]), int(s_["n_corner"])) for s_ in it_stats]
    # (N > 1: the counts come out of the all-reduced record, i.e. they are already the whole job's)
    n_valid_step = int(sum(a_ + b_ for a_, b_ in n_valid_iter))

    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.synchronize()

    # Clock spin-up, NOT warm-up of the hot path: the setup above leaves the GPU idle for seconds (workload generation on the host), and a timed
    # region of a few milliseconds right after an idle phase was twice observed 3-12x slow on a fresh box (scripts/calibbench.py: 4.3 and 1.1 ms
    # where every later process read 0.36 ms -- consistent with the clocks still ramping, not proven). Round 2 ran 600 untimed STEPS here, which made
    # `--warmup` mean something else than it says (VERDICT / ADVICE r02). Now: ~0.15 s of an unrelated dense product on torch's stream -- it touches
    # none of the library's buffers, caches or state -- and then exactly W warm-up steps and K timed steps. Reported as `gpu_clock_spinup_ms`.
    spin_ms = 0.0
    if args.spinup_ms > 0:
        a_ = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        t_sp = time.perf_counter()
        while 1e3 * (time.perf_counter() - t_sp) < args.spinup_ms:
            for _ in range(8):
                a_ = (a_ @ a_) * 1e-3
            torch.cuda.synchronize()
        spin_ms = 1e3 * (time.perf_counter() - t_sp)
        del a_
    knn_forms = {}

    def timed_region(step_fn, drain_fn, steps, warmup):
        """the contract's loop: W untimed steps, then exactly K timed ones between barrier + synchronize on both sides; max over the ranks"""
        sync_all()
        pose_ = None
        for _ in range(warmup):
            step_fn()
        drain_fn()
        # the dominant kernel is bracketed with HIP events on the context's stream INSIDE the timed region: one launch in 2 * GN_ITERS + 1 of each of its two
        # forms (iteration 0's launch: the search alone; iterations 1..4: the search behind the prologue that completes the previous iteration) -- the bracket
        # rotates through the iterations, ~70 + ~18 samples over the default 200 steps. An event pair costs ~6 us of queue time of its own: bracketing all five
        # launches of a step would slow the measured step by ~17 %, this costs ~2 %
        ctx.profile_enable(((1 << mla.K_KNN) | (1 << mla.K_KNN_PRE)) if args.profile_events else 0)
        ctx.profile_sample(2 * GN_ITERS + 1)
        ctx.profile_reset()
        sync_all()
        t_start = time.perf_counter()
        for _ in range(steps):
            pose_ = step_fn()
        last = drain_fn()
        pose_ = last if last is not None else pose_
        sync_all()
        elapsed_ = time.perf_counter() - t_start
        knn_ms_, knn_n_ = ctx.profile_get(mla.K_KNN)
        pre_ms_, pre_n_ = ctx.profile_get(mla.K_KNN_PRE)
        knn_forms.clear()
        knn_forms.update(search_only=(knn_ms_, knn_n_), with_prologue=(pre_ms_, pre_n_))
        if pre_n_ > 0:          # the form 4 of a step's 5 launches take is the dominant kernel
            knn_ms_, knn_n_ = pre_ms_, pre_n_
        ctx.profile_enable(0)
        ctx.profile_sample(1)
        if world > 1:
            tt = torch.tensor([elapsed_], dtype=torch.float64, device=dist_dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed_ = float(tt.item())
        return elapsed_, pose_, knn_ms_, knn_n_

    elapsed, pose, knn_ms, knn_n = timed_region(step, drain, args.steps, args.warmup)
    knn_forms_main = dict(knn_forms)
    ms_per_step = 1e3 * elapsed / args.steps
    value = n_valid_step / (elapsed / args.steps)
    queries_per_s = m_total * GN_ITERS / (elapsed / args.steps)

    # a second, fully instrumented pass (every kernel bracketed) for the per-kernel breakdown; not part of `value` (--full)
    if full:
        n_prof = max(args.steps // 4, 5)
        ctx.profile_enable(mla.K_ALL)
        ctx.profile_reset()
        sync_all()
        t1 = time.perf_counter()
        for _ in range(n_prof):
            step()
        drain()
        sync_all()
        ms_per_step_all_events = 1e3 * (time.perf_counter() - t1) / n_prof
        prof = {k: ctx.profile_get(k) for k in range(9)}
        ctx.profile_enable(0)
        # the same frames submitted synchronously (pose read before the next frame's staging is enqueued): what rounds 1 and 2 reported
        # (this loop also brackets iteration 0's launch -- the search alone, which a pipelined, chained frame no longer has: its first launch completes the previous frame)
        ctx.profile_enable((1 << mla.K_KNN) if args.profile_events else 0)
        ctx.profile_sample(3)
        ctx.profile_reset()
        sync_all()
        t1s = time.perf_counter()
        for _ in range(n_prof):
            step_sync()
        sync_all()
        ms_per_step_sync = 1e3 * (time.perf_counter() - t1s) / n_prof
        cold_sync = ctx.profile_get(mla.K_KNN)
        ctx.profile_enable(0)
        ctx.profile_sample(1)

    # the same timed loop at the reference's keyframe cadences (a frame is saved as a keyframe after DISTANCE_KEYFRAMES = 1 m or ORIENTATION_KEYFRAMES = 1 deg of motion,
    # config_realvehicle_hercules.yaml:142-143: every frame for a vehicle at >= 10 m/s and 10 Hz, every ~10th at walking pace): the frame after a keyframe cannot have
    # its maps staged beside the previous solve
    keyframe_cadence = None
    if full and pipelined and args.restage_every == 0 and not args.no_supplementary:
        keyframe_cadence = {}
        for kc in (1, 2, 5, 10):
            cadence[0], frame_no[0] = kc, 0
            el_k, _, _, _ = timed_region(step, drain, max(args.steps // 2, 10), min(args.warmup, 5))
            keyframe_cadence[f"every_{kc}"] = round(1e3 * el_k / max(args.steps // 2, 10), 4)
        cadence[0] = 0
        keyframe_cadence["never (= ms_per_step)"] = round(ms_per_step, 4)

    # --- N > 1: what every rank measured, the exchange by itself, and (--comm both) the same loop over the other communicator
    per_rank = exchange_us = other_comm = None
    if world > 1 and full:
        mine = dict(rank=rank, device=local_rank,
                    knn_us=(round(1e3 * prof[mla.K_KNN][0] / prof[mla.K_KNN][1], 3) if prof[mla.K_KNN][1] else None),
                    fit_us=(round(1e3 * prof[mla.K_FIT][0] / prof[mla.K_FIT][1], 3) if prof[mla.K_FIT][1] else None),
                    index_build_us=(round(1e3 * prof[mla.K_GRID_BUILD][0] / prof[mla.K_GRID_BUILD][1], 3) if prof[mla.K_GRID_BUILD][1] else None),
                    allreduce_us=(round(1e3 * prof[mla.K_ALLREDUCE][0] / prof[mla.K_ALLREDUCE][1], 3) if prof[mla.K_ALLREDUCE][1] else None),
                    solve_update_us=(round(1e3 * prof[mla.K_SOLVE][0] / prof[mla.K_SOLVE][1], 3) if prof[mla.K_SOLVE][1] else None))
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
        # one all-reduce of a 32-double record by itself, host to host (launch + exchange + read-back; every rank enters together): an upper bound of what an
        # iteration's exchange costs -- inside the solver the mailbox exchange has no launch of its own (it rides in the fit kernel's finishing workgroup)
        rec = np.ones(32)
        for _ in range(5):
            ctx.allreduce_f64(rec)
        sync_all()
        t_x = time.perf_counter()
        for _ in range(50):
            ctx.allreduce_f64(rec)
        exchange_us = round(1e6 * (time.perf_counter() - t_x) / 50, 2)
        if args.comm == "both":
            if comm_kind != "p2p" or shared_gpus:
                other_comm = dict(skipped="the RCCL leg needs a GPU per rank and a mailbox leg to compare with" if shared_gpus else "the mailbox communicator did not come up: the main loop already ran over RCCL")
            else:
                ctx.comm_finalize()
                comm_setup("rccl")
                stage_maps()
                chk = ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)[0]
                el2, pose2, _, _ = timed_region(step, drain, args.steps, args.warmup)
                other_comm = dict(comm="RCCL ncclAllReduce (fit kernel reduces locally, one all-reduce launch, one solve launch per iteration)",
                                  ms_per_step=round(1e3 * el2 / args.steps, 4), value=round(n_valid_step / (el2 / args.steps), 1), ranks_seen=comm_state["ranks_seen"],
                                  pose_vs_mailbox_run=float(np.abs(np.asarray(pose2) - np.asarray(pose)).max()), first_solve_vs_mailbox=float(np.abs(np.asarray(chk) - np.asarray(pose)).max()))

    # supplementary: the reference's own per-frame call, scan2MapOptimization = index build + 2 outer x (match all, evalHessian +
    # evalDegenracy, Ceres-shaped Levenberg-Marquardt <= 30 iterations) -- not `value`, reported beside it
    s2m_ms = None
    if full and world == 1 and not args.no_supplementary:
        for _ in range(3):
            ctx.map_rebuild(mla.ALL_KINDS)
            s2m_pose, s2m_stats = ctx.scan2map(p0, opts)
        n_s2m = max(args.steps // 2, 50)        # (round 4 took steps // 10 = 5 frames under the driver's --steps 20: the pipelined figure was all fill and drain)
        sync_all()
        t2 = time.perf_counter()
        for _ in range(n_s2m):
            ctx.map_rebuild(mla.ALL_KINDS)
            s2m_pose, _ = ctx.scan2map(p0, opts, want_stats=False)
        sync_all()
        s2m_ms = 1e3 * (time.perf_counter() - t2) / n_s2m
        # the same call with the frame's maps STAGED (mlh_map_set_pair from the device-resident clouds, as the GN step does) instead of re-indexed in place, and then
        # submitted / collected separately with the next frame's maps staged beside the solve and its start pose chained on the device (mlh_scan2map_begin_chained):
        # the per-frame call of the reference under the GN loop's submission mode
        for _ in range(3):
            ctx.map_set_pair(d_surf_map, d_corner_map)
            ctx.scan2map(p0, opts, want_stats=False)
        sync_all()
        t2 = time.perf_counter()
        for _ in range(n_s2m):
            ctx.map_set_pair(d_surf_map, d_corner_map)
            s2m_pose_staged, _ = ctx.scan2map(p0, opts, want_stats=False)
        sync_all()
        s2m_staged_ms = 1e3 * (time.perf_counter() - t2) / n_s2m
        s2m_status = []

        def s2m_pipe(n_frames):
            ctx.map_set_pair(d_surf_map, d_corner_map)
            ctx.scan2map_begin(p0, opts)
            out_ = None
            for _ in range(n_frames - 1):
                ctx.map_set_pair_overlapped(d_surf_map, d_corner_map)
                ctx.scan2map_begin_chained(s2m_pose_staged, p0, opts)       # synthetic odometry: the previous frame ended at its converged pose, this one starts at p0 again
                out_, st_ = ctx.scan2map_end()
                s2m_status.append(st_)
            last_, st_ = ctx.scan2map_end()
            s2m_status.append(st_)
            return out_ if out_ is not None else last_, last_
        s2m_pipe(4)
        del s2m_status[:]
        sync_all()
        t2 = time.perf_counter()
        s2m_pose_pipe, _ = s2m_pipe(n_s2m)
        sync_all()
        s2m_pipe_ms = 1e3 * (time.perf_counter() - t2) / n_s2m

    # supplementary: ONE WHOLE MAPPER FRAME (lidar_mapper_keyframe.cpp:1000-1112 with the estimator's front end in front of it): the two raw 64-ring scans resident in
    # HBM -> extractCloud (both LiDARs, one launch set) -> per-ring 0.2 m voxel thinning -> fusion of the LiDARs' features -> downsampleCurrentScan for both kinds
    # (covariance voxel filter in the reference's std::sort member order + evalPointUncertainty) -> index build of both maps -> scan2MapOptimization -> pose.
    # A context of its own (the main context's staged features stay what the other legs expect). Two clocks: every stage followed by a wait (ms per stage; the
    # waits are part of what is measured), and the frame with no wait but the one for the pose (ms_per_frame).
    frame = None
    if full and world == 1 and not args.no_supplementary and len(scans) >= 2 and not args.dense_features:
        fctx = mla.Context(local_rank)
        try:
            f_ext = np.array([np.concatenate([r_[4:7], r_[:4]]) for r_ in synth.HERCULES_BODY_T_LASER])[:len(scans)]
            for e_ in f_ext:
                e_[3:] /= np.linalg.norm(e_[3:])
            f_covs = np.stack([np.zeros((6, 6))] + [np.diag([0.0025] * 3 + [0.00030461] * 3)] * (len(scans) - 1))
            f_meas = np.diag([0.0025] * 3)
            f_opts = mla.default_opts(flags=mla.FLAG_WITH_UA)
            ring_ofs = np.cumsum([0] + [s_.n_rings for s_ in scans])
            d_pts = torch.from_numpy(np.ascontiguousarray(all_pts, np.float32)).cuda()
            d_start, d_end = torch.from_numpy(all_start).cuda(), torch.from_numpy(all_end).cuda()
            fctx.map_set_pair(d_surf_map, d_corner_map)

            def frame_once(t=None):
                c0 = time.perf_counter()
                fctx.fuse_reset()
                fctx.scan_upload(d_pts, d_start, d_end); fctx.extract_run(); fctx.extract_voxel_run(0.2)
                for i_ in range(len(scans)):
                    fctx.fuse_add_rings(ring_ofs[i_], ring_ofs[i_ + 1], i_, f_ext[i_])
                if t is not None:
                    fctx.synchronize()
                c1 = time.perf_counter()
                cnt = fctx.downsample_current_scan_pair(fctx.fused_cloud(mla.SURF), fctx.fused_cloud(mla.CORNER), 0.4, 0.2, f_ext, f_covs, f_meas, True, 0.6)
                c2 = time.perf_counter()
                fctx.map_set_pair(d_surf_map, d_corner_map)
                if t is not None:
                    fctx.synchronize()
                c3 = time.perf_counter()
                fpose, _ = fctx.scan2map(p0, f_opts, want_stats=False)
                c4 = time.perf_counter()
                if t is not None:
                    for k_, v_ in zip(("extract_fuse", "downsample_current_scan", "map_index_build", "scan2map"), (c1 - c0, c2 - c1, c3 - c2, c4 - c3)):
                        t[k_] = t.get(k_, 0.0) + v_
                return fpose, cnt
            for _ in range(5):
                frame_once()
            n_fr = 40
            sync_all()
            c0 = time.perf_counter()
            for _ in range(n_fr):
                frame_pose, frame_counts = frame_once()
            frame_ms = 1e3 * (time.perf_counter() - c0) / n_fr
            # the same frame with the local map staged and indexed BESIDE the front end (second stream, the other map set): the map is made of earlier keyframes and
            # does not wait for the scan (the whole-frame form)
            def frame_once_staged_beside():
                fctx.fuse_reset()
                fctx.scan_upload(d_pts, d_start, d_end); fctx.extract_run(); fctx.extract_voxel_run(0.2)
                for i_ in range(len(scans)):
                    fctx.fuse_add_rings(ring_ofs[i_], ring_ofs[i_ + 1], i_, f_ext[i_])
                fctx.map_set_pair_overlapped(d_surf_map, d_corner_map)
                fctx.downsample_current_scan_pair(fctx.fused_cloud(mla.SURF), fctx.fused_cloud(mla.CORNER), 0.4, 0.2, f_ext, f_covs, f_meas, True, 0.6)
                return fctx.scan2map(p0, f_opts, want_stats=False)[0]
            # ... and with thinning + solve as one call that reads nothing back in between (mlh_downsample_scan2map: the thinned counts stay on the device)
            def frame_once_fused_call():
                fctx.fuse_reset()
                fctx.scan_upload(d_pts, d_start, d_end); fctx.extract_run(); fctx.extract_voxel_run(0.2)
                for i_ in range(len(scans)):
                    fctx.fuse_add_rings(ring_ofs[i_], ring_ofs[i_ + 1], i_, f_ext[i_])
                fctx.map_set_pair_overlapped(d_surf_map, d_corner_map)
                return fctx.downsample_scan2map(fctx.fused_cloud(mla.SURF), fctx.fused_cloud(mla.CORNER), 0.4, 0.2, f_ext, f_covs, f_meas, p0, f_opts)
            frame_fused_ms, frame_fused_same = None, None
            try:
                for _ in range(5):
                    frame_once_fused_call()
                sync_all()
                c0 = time.perf_counter()
                for _ in range(n_fr):
                    pose_fused, cnt_fused = frame_once_fused_call()
                frame_fused_ms = 1e3 * (time.perf_counter() - c0) / n_fr
                frame_fused_same = bool(np.array_equal(pose_fused, frame_pose)) and tuple(cnt_fused) == tuple(int(x) for x in frame_counts)
            except Exception as ex:      # (a supplementary leg must not cost the line)
                frame_fused_ms = None
                print(f"[rank {rank}] frame, thinning + solve in one call: {str(ex)[:200]}", file=sys.stderr)
            frame_beside_ms, frame_beside_same = None, None
            try:
                for _ in range(5):
                    frame_once_staged_beside()
                sync_all()
                c0 = time.perf_counter()
                for _ in range(n_fr):
                    pose_beside = frame_once_staged_beside()
                frame_beside_ms = 1e3 * (time.perf_counter() - c0) / n_fr
                frame_beside_same = bool(np.array_equal(pose_beside, frame_pose))
            except Exception as ex:      # (a supplementary leg must not cost the line)
                frame_beside_ms = None
                print(f"[rank {rank}] frame, map staged beside the front end: {str(ex)[:200]}", file=sys.stderr)
            fctx.map_set_pair(d_surf_map, d_corner_map)
            st_t = {}
            for _ in range(n_fr):
                frame_once(st_t)
            frame = dict(ms_per_frame=round(frame_ms, 4), ms_per_frame_map_staged_beside_the_front_end=(round(frame_beside_ms, 4) if frame_beside_ms else None),
                         map_staged_beside_same_pose=frame_beside_same,
                         ms_per_frame_map_beside_and_thinning_plus_solve_in_one_call=(round(frame_fused_ms, 4) if frame_fused_ms else None),
                         one_call_same_pose_and_counts=frame_fused_same, stages_ms_each_followed_by_a_wait={k_: round(1e3 * v_ / n_fr, 4) for k_, v_ in st_t.items()},
                         scan_points=int(len(all_pts)), thinned_features=dict(surf=int(frame_counts[0]), corner=int(frame_counts[1])), pose=[round(float(x), 9) for x in frame_pose],
                         host_reads_between_scan_and_pose=2,
                         note="supplementary: the two raw scans resident in HBM -> extractCloud + per-ring voxel thinning + fusion -> downsampleCurrentScan (both kinds, one "
                              "pipeline) -> index build of both maps -> scan2MapOptimization -> pose; frames one after the other, host waits for every pose. Two host reads "
                              "inside the frame, each a spin on a pinned record a kernel publishes: the fused clouds' counts and bounds (they size the thinning's launches and "
                              "its voxel grids), and the thinned feature counts (they size the solve's launches). The `..._in_one_call` figure uses mlh_downsample_scan2map, where the "
                              "second of the two is gone (the solve reads the counts on the device). The scans' upload (a real frame's ~70 us pageable H2D + 8 us "
                              "pack) is OUTSIDE these figures; `from_cpp_threads` below starts from host buffers and pays it")
        finally:
            fctx.close()
        # the same frame from C++ threads through the C-ABI, host scans in: the estimator / mapper pair's frame period and K independent pipelines per GPU
        try:
            cpp = framebench_cpp(all_pts, all_start, all_end, ring_ofs, f_ext, f_covs, f_meas, surf_map, corner_map, p0)
            if frame is not None:
                frame["from_cpp_threads"] = cpp
                if "period_ms_two_contexts" in cpp:
                    frame["period_ms_two_contexts"] = cpp["period_ms_two_contexts"]
                if "period_ms_two_contexts_upload_ahead" in cpp:
                    frame["period_ms_two_contexts_upload_ahead"] = cpp["period_ms_two_contexts_upload_ahead"]
                if "period_ms_two_contexts_mlh_scan_upload_ahead" in cpp:
                    frame["period_ms_two_contexts_mlh_scan_upload_ahead"] = cpp["period_ms_two_contexts_mlh_scan_upload_ahead"]
                if "frames_per_s_at_K_upload_ahead" in cpp:
                    frame["frames_per_s_at_K_upload_ahead"] = {k_: v_["frames_per_s"] for k_, v_ in cpp["frames_per_s_at_K_upload_ahead"].items()}
                if "frames_per_s_at_K" in cpp:
                    frame["frames_per_s_at_K"] = {k_: v_["frames_per_s"] for k_, v_ in cpp["frames_per_s_at_K"].items()}
                # the frame from RAW clouds, ImageSegmenter included (the reference's default front end): one context | a context + thread per LiDAR gathered by
                # mlh_fuse_add_scan_from | the same with the next frame's front end started behind the appends
                try:
                    raw = framebench_cpp(all_pts, all_start, all_end, ring_ofs, f_ext, f_covs, f_meas, surf_map, corner_map, p0, frames=40, mode="raw", timeout=120)
                    raw["note"] = ("raw host clouds -> per LiDAR segmentCloud (its cluster search is ~1.3 ms of sequential HOST work per 64-ring cloud: DESIGN 9) -> extractCloud -> "
                                   "fusion -> thinning -> index -> scan2map -> pose; `context_per_lidar`: the LiDARs' searches side by side on a thread + context each")
                    frame["raw_frame_with_segmenter"] = raw
                except Exception as ex:
                    frame["raw_frame_with_segmenter"] = dict(error=str(ex)[:200])
                frame["from_cpp_threads_note"] = ("m-loam_amd/host/framebench.cpp: host scans in (upload inside the frame), pose out. two contexts = an estimator-side thread "
                                                  "(upload, extract, fuse, thin) and a mapper-side thread (index, scan2map) with a device-to-device hand-over, as the reference "
                                                  "runs estimator and mapper concurrently (`..._upload_ahead`: the same pair with the NEXT scan's upload issued ahead by the caller -- page-locked "
                                                  "scans, a copy stream of its own, MLH_MEM_DEVICE -- so that the copy engine works beside the kernels: a replayed bag, not a live 10 Hz sensor; "
                                                  "`..._mlh_scan_upload_ahead`: the same through the library's own look-ahead on the caller's pageable buffer); "
                                                  "K = independent whole-frame pipelines (own thread + context each) sharing the GPU; "
                                                  "every frame of every pipeline returns the single pipeline's pose bits")
        except Exception as ex:      # (a supplementary leg must not cost the line)
            print(f"[rank {rank}] frame from C++ threads: {str(ex)[:200]}", file=sys.stderr)

    # supplementary (N = 1): what N = 2 / 4 / 8 should show on this frame, per split, from each rank's share solved alone on this GPU
    predicted = None
    if full and world == 1 and not args.no_supplementary and not args.dense_features:
        try:
            predicted = predicted_scaling(mla, torch, shard, local_rank, surf_map, corner_map, surf, corner, np.asarray(pose, np.float64), center)
        except Exception as ex:      # (a supplementary leg must not cost the line)
            predicted = dict(error=str(ex)[:200])
        # ... and on the configurations the north star quotes its multi-GPU target on (config 4 on the 4 M map; the un-thinned frame): too long for the default run
        # (a 4 M-point map is built), so the committed result of scripts/predict_multi_gpu.py -- same method, same kernels, its own gpurun call -- is attached
        try:
            with open(os.path.join(ROOT, "profiles", "r06_multi_gpu_predicted.json")) as f_:
                ns = json.load(f_)
            def _brief(cfg):
                return dict(n1_ms_per_step=cfg["n1_ms_per_step"], splits={k_: dict(ms_per_step=v_["predicted_ms_per_step"], speedup=v_["predicted_speedup_vs_n1"]) for k_, v_ in cfg["splits"].items()})
            predicted["north_star_configurations"] = dict(
                source="profiles/r06_multi_gpu_predicted.json (scripts/predict_multi_gpu.py, one MI355X, not measured in this run)",
                config4_on_the_4M_map=_brief(ns["config4_4M"]), config2_unthinned_228k_queries=_brief(ns["config2_unthinned_500k"]),
                target=ns["north_star_target"], predicted_best_speedup_at_8_gpus=ns["predicted_best_speedup_at_8_gpus_config4_4M"], meets_target=ns["meets_target"],
                verdict=ns["verdict"])
        except Exception as ex:
            if isinstance(predicted, dict):
                predicted["north_star_configurations"] = dict(error=str(ex)[:200])

    # --- roofline of the dominant kernel (correspondence kernel, surf + corner features in one launch):
    #     algorithmic bytes per launch / duration from the dispatch's own start/stop timestamps (HIP events)
    h = float(np.sqrt(opts.min_match_sq_dis)) * 1.001
    Tm = synth.pose_to_mat(p0)
    planes = shard.wedge_planes(center, world, rank)
    bytes_per_launch, bytes_ball, cbars, cballs, n_owned = 0.0, 0.0, {}, {}, {}
    if full:       # (candidate counts over the map on the host: seconds at 500k points)
        for name, feats, lmap in (("surf", surf, local_surf_map), ("corner", corner, local_corner_map)):
            fm = synth.transform_points(feats[:, :3], Tm)
            own = (shard.owned_mask(fm, *planes) if args.shard_mode == "map" else (np.arange(len(feats)) % world) == rank) if world > 1 else np.ones(len(feats), bool)
            cb, cball = candidate_stats(lmap, fm[own], h)
            cbars[name], cballs[name], n_owned[name] = round(cb, 2), round(cball, 2), int(own.sum())
            # B_feat = 16 (query) + 27 x 8 (cell begin/end) + 12 x C-bar (candidate xyz); the partial normal equations
            # (232 B per 256-feature tile) are negligible. This is the figure `achieved` uses.
            bytes_per_launch += int(own.sum()) * (16.0 + 27 * 8 + 12.0 * cb)
            # the same formula with only the cells an exact search cannot avoid (those the 5th-neighbour ball touches): the near-cells-first
            # search reads between this and the 27-cell figure
            bytes_ball += int(own.sum()) * (16.0 + 27 * 8 + 12.0 * cball)
    roofline = None
    if full and knn_n > 0:
        dur_s = 1e-3 * knn_ms / knn_n
        ach = bytes_per_launch / dur_s / 1e9
        _lanes = (ctx.map_info(mla.SURF)["knn_lanes"], ctx.map_info(mla.CORNER)["knn_lanes"])
        _pre = knn_forms_main.get("with_prologue", (0, 0))[1] > 0
        roofline = dict(bound="hbm", kernel=(f"knn_features_kernel<.., PRE, WARM> (iterations 1..{GN_ITERS - 1} of a solve, {GN_ITERS - 1} of its {GN_ITERS} correspondence launches: every workgroup first completes "
                                             f"the previous iteration -- sums the fit tiles' records, 6x6 solve, Plus -- then the exact 5-NN search of surf + corner queries, bounded by the previous "
                                             f"iteration's neighbours; lanes per query surf/corner = {_lanes[0]}/{_lanes[1]})" if _pre else
                                             f"knn_features_kernel (correspondence search, surf + corner queries of one GN iteration; lanes per query surf/corner = {_lanes[0]}/{_lanes[1]})"),
                        achieved=round(ach, 2), peak=8000.0, unit="GB/s",
                        frac=round(ach / 8000.0, 5), traffic=None, avg_kernel_us=round(1e6 * dur_s, 3), launches=int(knn_n),
                        algorithmic_bytes_per_launch=int(bytes_per_launch), bytes_convention="SURVEY 8(d): 16 + 27*8 + 12*C-bar per query (all 27 cells)",
                        mean_candidates_per_feature=cbars, owned_features=n_owned,
                        unavoidable_bytes_per_launch=int(bytes_ball), mean_candidates_in_cells_touching_the_kth_ball=cballs,
                        achieved_on_unavoidable_bytes_GBps=round(bytes_ball / dur_s / 1e9, 2),
                        floor_132B_per_feature_GBps=round(m_total * 132 / dur_s / 1e9, 2),
                        note="`achieved` follows the survey's 27-cell convention; the kernel searches near cells first and skips cells farther than "
                             "the K-th distance found, so it READS fewer bytes than that (between the `unavoidable` and the 27-cell figure). "
                             "The map (<= 128 MB) is L2/Infinity-Cache resident: measured HBM bytes (PMC, collected offline, profiles/) are far "
                             "below either figure, so HBM bandwidth is not what binds this launch. Round 2 called it VALU-issue bound (SQ counters: ~60-70 % VALU "
                             "utilisation, ~5 wavefronts per SIMD); round 3's knock-out runs (profiles/r03_knockout_experiments.txt) say otherwise: with ALL top-K "
                             "bookkeeping removed the launch still takes 8.7 of 10.7 us, and a 2.5x cheaper sorted insertion (v_min_f64 / v_max_f64 on the keys) changed "
                             "nothing -- the duration is the dependent chain feature -> cell_start words -> candidate trips (median workgroup 3.3 us, slowest 7.0) -> "
                             "winner gather -> store. `frac` is reported against the HBM peak because that is the contract's roof; it is not the binding one")
        so_ms, so_n = knn_forms_main.get("search_only", (0, 0))
        if cold_sync[1] > so_n:        # pipelined, chained frames: iteration 0's plain launch only exists in the synchronous pass
            so_ms, so_n = cold_sync
        if _pre and so_n > 0:
            so_s = 1e-3 * so_ms / so_n
            roofline["search_only_launch"] = dict(kernel="knn_features_kernel (iteration 0's launch: the search alone, no prologue, no bound from a previous iteration -- the kernel rounds 1-3 reported)",
                                                  avg_kernel_us=round(1e6 * so_s, 3), launches=int(so_n), achieved=round(bytes_per_launch / so_s / 1e9, 2), frac=round(bytes_per_launch / so_s / 1e9 / 8000.0, 5),
                                                  unavoidable_frac=round(bytes_ball / so_s / 1e9 / 8000.0, 5))
            roofline["prologue_note"] = ("the dominant launch carries the previous iteration's finish (~3.5 us: one trip for the 88 records, the solve on one wavefront, a barrier), which round 3's fit "
                                         "kernel paid as a ~7 us serial tail of its last workgroup; `achieved` divides the SEARCH's algorithmic bytes by the whole launch, prologue included")
        # what binds, as first-class fields: the fraction on the bytes an exact search cannot avoid, and the binding resource
        roofline["unavoidable_frac"] = round(bytes_ball / dur_s / 1e9 / 8000.0, 5)
        roofline["binding"] = "latency"          # dependent memory round trips per query (see `note`); not HBM bandwidth, not VALU issue
        pmc_path = os.path.join(ROOT, "profiles", "pmc_knn.json")
        if os.path.exists(pmc_path):
            try:
                pmc = json.load(open(pmc_path))
                if pmc.get("workload", "").startswith(f"{N_LIDARS}x{N_RINGS}_vs_{preset}_r") and world == 1 and not args.dense_features and args.lidars == N_LIDARS:
                    roofline["traffic"] = pmc.get("hbm_bytes_per_launch")
                    roofline["traffic_source"] = pmc.get("source")
                    if "search_only_launch" in roofline and "search_only_kernel" in pmc:
                        roofline["search_only_launch"]["traffic"] = pmc["search_only_kernel"].get("hbm_bytes_per_launch")
                    if pmc.get("valu_issue_utilisation") is not None:
                        roofline["valu_issue_utilisation"] = pmc.get("valu_issue_utilisation")      # SQ_INSTS_VALU x 4 cycles / (SIMDs x busy cycles), offline pass
                        roofline["valu_insts_per_launch"] = pmc.get("valu_insts_per_launch")
            except Exception:
                pass

    # second roofline object: the TIME-dominant kernel (fit + gates + residual / Jacobian + reduction + the fused Gauss-Newton finish). Duration from the
    # fully instrumented pass (every kernel bracketed; not the timed region, where only the correspondence kernel carries events).
    roofline_fit = None
    if full and prof[mla.K_FIT][1]:
        fit_s = 1e-3 * prof[mla.K_FIT][0] / prof[mla.K_FIT][1]
        n_own = sum(n_owned.values())
        tiles = (len(surf) + 255) // 256 + (len(corner) + 255) // 256
        fit_bytes = n_own * (16 + 16 * 5 + 32) + 256 * tiles          # feature + 5 neighbour records + correspondence record; one partial record per tile
        roofline_fit = dict(bound="hbm", kernel="fit_linearize_kernel<5> (line / plane fit + gates + residual + 1x6 Jacobian + normal-equation reduction + fused GN finish)",
                            achieved=round(fit_bytes / fit_s / 1e9, 2), peak=8000.0, unit="GB/s", frac=round(fit_bytes / fit_s / 1e9 / 8000.0, 5), traffic=None,
                            avg_kernel_us=round(1e6 * fit_s, 3), launches=int(prof[mla.K_FIT][1]), algorithmic_bytes_per_launch=int(fit_bytes),
                            binding="latency", timing="HIP events, separate fully-bracketed pass",
                            note="a few MB per launch: nowhere near any bandwidth roof. What bounds it is a dependent chain -- f32 eigen / QR fit per lane, f64 "
                                 "residual + Jacobian, the workgroup reduction, then the serial finish (sum of the tiles' records, 6x6 solve, Plus) in the last workgroup")
        try:                     # HBM bytes of this kernel from the same offline PMC passes as the correspondence kernel's (profiles/pmc_knn.json: fit_kernel)
            pmc_f = json.load(open(os.path.join(ROOT, "profiles", "pmc_knn.json")))
            if pmc_f.get("workload", "").startswith(f"{N_LIDARS}x{N_RINGS}_vs_{preset}_") and world == 1 and not args.dense_features and "fit_kernel" in pmc_f:
                roofline_fit["traffic"] = pmc_f["fit_kernel"].get("hbm_bytes_per_launch")
        except Exception:
            pass
    # supplementary: a frame whose map has OUTGROWN the sticky grid box: every step stages a cloud that alternately has / has not a few points 40 m
    # outside the box of the previous one, so the bounds pass + re-layout path of mlh_map_set_pair is what is timed. Not `value`.
    outgrow_ms = None
    if full and world == 1 and not args.no_map_rebuild and not args.map_rebuild_only and not args.no_supplementary:
        ext = torch.tensor([[1.0, 1.0, 0.0], [-1.0, -1.0, 0.0]], device="cuda") * float(np.abs(local_surf_map[:, :2]).max() + 40.0)
        grown = torch.cat([d_surf_map[:, :3], ext.to(d_surf_map.dtype)], dim=0).contiguous()
        plain = d_surf_map[:, :3].contiguous()
        torch.cuda.synchronize()
        for i in range(6):
            ctx.map_set_pair(grown if i % 2 == 0 else plain, d_corner_map)
            ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        n_og = max(args.steps // 4, 6)
        sync_all()
        t3 = time.perf_counter()
        for i in range(n_og):
            ctx.map_set_pair(grown if i % 2 == 0 else plain, d_corner_map)
            ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        sync_all()
        outgrow_ms = 1e3 * (time.perf_counter() - t3) / n_og
        ctx.map_set_pair(d_surf_map, d_corner_map)

    # --- where the kernels leave the latency regime: the same frame WITHOUT thinning the scan features at the mapper's resolutions (every less-flat / less-sharp
    #     point is a query: ~10x the launch), same maps, same solve. Supplementary (`roofline.saturated`): it says at which launch size the correspondence kernel's
    #     rate stops being set by the length of one query's dependent chain.
    saturated = None
    if full and world == 1 and not args.dense_features and roofline is not None and not args.no_supplementary:
        surf_d, corner_d = fuse_features(synth, scans, extracted, thin=False)
        ctx.features_set(mla.SURF, torch.from_numpy(surf_d).cuda())
        ctx.features_set(mla.CORNER, torch.from_numpy(corner_d).cuda())
        torch.cuda.synchronize()
        for _ in range(3):
            ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        ctx.profile_enable((1 << mla.K_KNN) | (1 << mla.K_KNN_PRE) | (1 << mla.K_FIT))
        ctx.profile_sample(1)
        ctx.profile_reset()
        for _ in range(10):
            ctx.gn_solve(p0, GN_ITERS, opts, want_stats=False)
        ctx.synchronize()
        sat = {k: ctx.profile_get(k) for k in (mla.K_KNN, mla.K_KNN_PRE, mla.K_FIT)}
        ctx.profile_enable(0)
        b27 = bball = 0.0
        cb_d = {}
        for name, feats, lmap in (("surf", surf_d, local_surf_map), ("corner", corner_d, local_corner_map)):
            cb, cball = candidate_stats(lmap, synth.transform_points(feats[:, :3], Tm), h)
            cb_d[name] = round(cb, 2)
            b27 += len(feats) * (16.0 + 27 * 8 + 12.0 * cb)
            bball += len(feats) * (16.0 + 27 * 8 + 12.0 * cball)
        def us(k):
            return 1e3 * sat[k][0] / sat[k][1] if sat[k][1] else None
        t_cold, t_pre = us(mla.K_KNN), us(mla.K_KNN_PRE)
        t_dom = t_pre if t_pre else t_cold
        saturated = dict(features=int(len(surf_d) + len(corner_d)), features_surf=int(len(surf_d)), features_corner=int(len(corner_d)),
                         knn_search_only_us=(round(t_cold, 2) if t_cold else None), knn_with_prologue_us=(round(t_pre, 2) if t_pre else None),
                         fit_us=(round(us(mla.K_FIT), 2) if us(mla.K_FIT) else None), algorithmic_bytes_per_launch=int(b27), mean_candidates_per_feature=cb_d,
                         frac=round(b27 / (1e-6 * t_dom) / 1e9 / 8000.0, 5), unavoidable_frac=round(bball / (1e-6 * t_dom) / 1e9 / 8000.0, 5),
                         frac_search_only=(round(b27 / (1e-6 * t_cold) / 1e9 / 8000.0, 5) if t_cold else None),
                         queries_per_s_of_the_dominant_launch=round((len(surf_d) + len(corner_d)) / (1e-6 * t_dom), 1),
                         note="the frame's scan features NOT thinned at MAP_SURF_RES / MAP_CORNER_RES (not BASELINE's workload): same kernels, ~10x the queries per launch; HIP events on every launch of 10 solves")
        roofline["saturated"] = saturated
        ctx.features_set(mla.SURF, d_surf)
        ctx.features_set(mla.CORNER, d_corner)

    # --- BASELINE config 4's frame (4 x 64 rings, one pose block per LiDAR: N_NEIGH 5/10/10/10, CHECK_FOV, freeze-on-degenerate, Huber 1.0) through
    #     mlh_gn_solve_blocks on this run's map, sharded like the single-pose frame: the headline with --config4, a supplementary leg at --gpus 8 (the
    #     configuration BASELINE.json quotes config 4 on) otherwise. Last thing measured: it replaces the context's staged features.
    cfg4 = None
    if args.config4 or (full and world == 8):
        scans4 = list(scans)[:4] + [synth.simulate_scan(sc, gt, synth.HERCULES_BODY_T_LASER[i], N_RINGS, seed=7 + i) for i in range(len(scans), 4)]
        surf_b, corner_b, poses0 = config4_blocks(mla, synth, ctx, scans4, gt)
        ref4 = None
        if world > 1 and full:
            if rank == 0:
                ref4 = single_gpu_config4(mla, torch, local_rank, surf_map, corner_map, surf_b, corner_b, poses0, args.steps, args.warmup)
            dist.barrier()
        ctx.features_set_blocks(mla.SURF, surf_b)
        ctx.features_set_blocks(mla.CORNER, corner_b)
        o4 = mla.default_opts(flags=mla.FLAG_CHECK_FOV, huber_delta=1.0)

        def step4():
            if not args.no_map_rebuild:
                if args.map_rebuild_only:
                    ctx.map_rebuild(mla.ALL_KINDS)
                else:
                    ctx.map_set_pair(d_surf_map, d_corner_map)
            return ctx.gn_solve_blocks(poses0, GN_ITERS, CFG4_K, CFG4_THRE, CFG4_FREEZE, o4, want_stats=False)[0]
        poses4, st4 = ctx.gn_solve_blocks(poses0, GN_ITERS, CFG4_K, CFG4_THRE, CFG4_FREEZE, o4, want_stats=True)
        n_valid4 = [[(int(st4[it][b_]["n_surf"]), int(st4[it][b_]["n_corner"])) for b_ in range(4)] for it in range(GN_ITERS)]
        n_valid4_step = int(sum(a_ + b_ for row in n_valid4 for a_, b_ in row))
        el4, poses4_t, _, _ = timed_region(step4, lambda: None, args.steps, args.warmup)
        m4 = int(sum(len(x) for x in surf_b) + sum(len(x) for x in corner_b))
        cfg4 = dict(workload=f"4x{N_RINGS}-ring synthetic scan vs {preset} local map, 4 pose blocks (body + 3 extrinsics; N_NEIGH 5/10/10/10, CHECK_FOV, freeze-on-degenerate, Huber 1.0), "
                             f"{GN_ITERS} GN iterations/frame re-matched every iteration (mlh_gn_solve_blocks; buildCalibMap + LidarOnlineCalib* structure, estimator.cpp:1067-1157)",
                    ms_per_step=round(1e3 * el4 / args.steps, 4), value=round(n_valid4_step / (el4 / args.steps), 1), unit="features/s",
                    queries_per_s=round(m4 * GN_ITERS / (el4 / args.steps), 1), features_per_block_surf=[len(x) for x in surf_b], features_per_block_corner=[len(x) for x in corner_b],
                    n_valid_per_iter_per_block_surf_corner=n_valid4, valid_correspondences_per_step=n_valid4_step, final_poses=np.round(np.asarray(poses4_t), 9).tolist(),
                    n1_same_map_ms_per_step=(ref4 or {}).get("ms_per_step"),
                    speedup_vs_n1_same_map=(round(ref4["ms_per_step"] / (1e3 * el4 / args.steps), 4) if ref4 else None),
                    pose_vs_n1_same_map_m=(float(np.abs(np.asarray(ref4["poses"])[:, :3] - np.asarray(poses4_t)[:, :3]).max()) if ref4 else None))
        if world > 1 and full:
            # the same frame with the BLOCKS dealt over the ranks instead of the map (replicated here): no exchange at all, and the only split of this path that can
            # shorten a frame whose kernels are latency-bound
            s_b, poses_b, owner_b = block_sharded_config4(mla, torch, dist, dist_dev, local_rank, rank, world, surf_map, corner_map, surf_b, corner_b, poses0,
                                                         args.steps, args.warmup)
            ref_p = np.asarray(ref4["poses"]) if ref4 else None
            cfg4["blocks_over_ranks"] = dict(
                what="pose blocks dealt over the ranks (block b -> rank b mod min(N, 4)), whole map replicated, staged and indexed on every rank per step, "
                     "no collective in the data path (the blocks' normal equations are independent); timed between barriers, max over the ranks",
                block_owner=owner_b, ranks_without_a_block=max(0, world - len(surf_b)),
                ms_per_step=round(1e3 * s_b, 4), value=round(n_valid4_step / s_b, 1),
                speedup_vs_n1_same_map=(round(ref4["ms_per_step"] / (1e3 * s_b), 4) if ref4 else None),
                poses_equal_n1_same_map_bit_for_bit=(bool(np.array_equal(ref_p, poses_b)) if ref4 else None),
                pose_vs_n1_same_map_m=(float(np.abs(ref_p[:, :3] - poses_b[:, :3]).max()) if ref4 else None),
                ranks_share_gpus=bool(shared_gpus))

    owned_all = local_map_all = None
    if world > 1 and full:
        t_own = torch.zeros((world, 2), dtype=torch.int64, device=dist_dev)
        t_own[rank, 0], t_own[rank, 1] = n_owned["surf"], n_owned["corner"]
        dist.all_reduce(t_own)
        owned_all = t_own.tolist()
        t_map = torch.zeros((world, 2), dtype=torch.int64, device=dist_dev)
        t_map[rank, 0], t_map[rank, 1] = len(local_surf_map), len(local_corner_map)
        dist.all_reduce(t_map)
        local_map_all = t_map.tolist()
    out = None
    if rank == 0:
        out = dict(metric="scan-to-map residuals+Jacobians/sec (features linearised per second, 5 GN iters/frame)",
                   value=round(value, 1), unit="features/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
                   ms_per_step=round(ms_per_step, 4), higher_is_better=True, scaling="strong", vs_baseline=None,
                   dtype="f32 search/fit + f64 residual/Jacobian/normal equations", data="synthetic",
                   config=dict(workload=f"{args.lidars}x{N_RINGS}-ring synthetic scan ({n_scan_points} pts) vs {preset} local map "
                                        f"({len(surf_map) + len(corner_map)} pts), {GN_ITERS} GN iters/frame, re-matched every iteration",
                               features_surf=len(surf), features_corner=len(corner), gn_iters_per_step=GN_ITERS,
                               n_valid_per_iter_surf_corner=n_valid_iter,
                               map_index=dict(surf=ctx.map_info(mla.SURF), corner=ctx.map_info(mla.CORNER)),
                               input_sha1=dict(surf_map=_sha(surf_map), corner_map=_sha(corner_map), surf_features=_sha(surf), corner_features=_sha(corner)),
                               corner_map="less-sharp points of 10 earlier keyframes x LiDARs, thinned at 0.2 m (as the mapper builds it)",
                               scan_features_thinned=not args.dense_features,
                               map_index_per_step=("none" if args.no_map_rebuild else ("mlh_map_rebuild (re-index only)" if args.map_rebuild_only
                                                                                      else "mlh_map_set_pair from device-resident clouds (staging + fit check + index build)")),
                               parallelism=("1 GPU" if world == 1 else (f"map sharded in {world} angular wedges (+1.1 m halo), ownership by position" if args.shard_mode == "map"
                                                                       else f"map replicated, features dealt round-robin over {world} ranks") + " + ONE RCCL all-reduce of 32 f64 per GN iteration"),
                               hip_events_in_timed_region=(f"dominant kernel, 1 launch in {2 * GN_ITERS + 1} of each of its two forms" if args.profile_events else "none")),
                   queries_per_s=round(queries_per_s, 1), valid_correspondences_per_step=n_valid_step,
                   ms_per_gn_iter=round(ms_per_step / GN_ITERS, 4),
                   frame_submission=(("pipelined + overlapped staging: frame k+1's maps are staged and indexed on a second stream, into the other map set, while frame k's solve "
                                      "runs (mlh_map_set_pair_overlapped); frame k+1's solve is submitted behind it with its start pose chained on the device from frame k's result "
                                      "(mlh_gn_solve_begin_chained: transformUpdate + transformAssociateToMap); poses are collected one frame late (mlh_gn_solve_end)" if not args.no_overlap_staging else
                                      "pipelined: frame k's pose is collected after frame k+1's map staging and solve (start pose chained on the device) have been enqueued behind its solve")
                                     if pipelined else "synchronous: every pose is read before the next frame is staged"),
                   multi_gpu=(None if world == 1 else dict(
                       shard_mode=args.shard_mode,
                       communicator=("mailbox" if comm_kind == "p2p" else "rccl"), communicator_requested=args.comm, ranks_seen_by_the_collective=comm_state["ranks_seen"],
                       communicator_fallback=comm_state.get("fallback"),
                       comm=("mailbox communicator (mlh_p2p_*): the summed record is exchanged inside the fit kernel's finishing workgroup, one hop, no extra launch" if comm_kind == "p2p" else "RCCL ncclAllReduce"),
                       ranks_share_gpus=bool(shared_gpus), gpus_visible=int(torch.cuda.device_count()),
                       cross_gpu_measurement=(False if shared_gpus else True),
                       cross_gpu_note=("ranks SHARE devices on this box: this line checks the N > 1 path end to end, it is NOT a scaling measurement -- no cross-GPU (xGMI) number exists in this "
                                       "repository's history until a run with a GPU per rank has been recorded" if shared_gpus else "one GPU per rank: peer stores / RCCL over xGMI"),
                       n1_same_map=n1_ref,
                       n1_same_map_ms_per_step=(n1_ref or {}).get("ms_per_step"),
                       speedup_vs_n1_same_map=(round(n1_ref["ms_per_step"] / ms_per_step, 4) if n1_ref else None),
                       owned_features_per_rank=owned_all, local_map_points_per_rank=local_map_all,
                       per_rank_kernel_us=per_rank, exchange_us_standalone_allreduce_of_32_f64=exchange_us, other_communicator=other_comm,
                       allreduce_us_per_call_rank0=(round(1e3 * prof[mla.K_ALLREDUCE][0] / prof[mla.K_ALLREDUCE][1], 3) if full and prof[mla.K_ALLREDUCE][1] else None),
                       solve_update_us_per_call_rank0=(round(1e3 * prof[mla.K_SOLVE][0] / prof[mla.K_SOLVE][1], 3) if full and prof[mla.K_SOLVE][1] else None),
                       note=("per GN iteration and rank: correspondence kernel + fit kernel whose finishing workgroup exchanges the 32-double record with the peers and solves (2 launches, as unsharded)" if comm_kind == "p2p" else "per GN iteration and rank: correspondence kernel + fit kernel (local reduce) + ONE ncclAllReduce of 32 f64 + the redundant 6x6 solve launch"))),
                   final_pose=[round(float(x), 9) for x in pose],
                   gpu_clock_spinup_ms=round(spin_ms, 1))
        if full:       # what the default run leaves out: the per-kernel and submission-mode figures, the extraction timings, the rooflines
            out.update(ms_per_step_all_kernels_bracketed=round(ms_per_step_all_events, 4),
                       ms_per_step_synchronous_submission=round(ms_per_step_sync, 4),
                       ms_per_step_by_keyframe_cadence=keyframe_cadence,
                       keyframe_cadence_note=("`value` / ms_per_step: no frame of the timed region is a keyframe, i.e. every frame reuses the previous frame's local map, which is what the reference does between "
                                              "keyframes (lidar_mapper_keyframe.cpp:257-261) and what makes staging beside the solve legal. every_K: each K-th frame is saved as a keyframe, the "
                                              "next frame's maps are staged only after its pose has been read (facade: PipelinedMapper; every_1 = a keyframe per frame = synchronous staging)"),
                       kernel_us_per_launch={name: (round(1e3 * prof[k][0] / prof[k][1], 3) if prof[k][1] else None)
                                             for name, k in (("knn_features (surf+corner)", mla.K_KNN),
                                                             ("knn_features behind the previous iteration's finish (iterations >= 1)", mla.K_KNN_PRE),
                                                             ("knn_features of a chained frame's iteration 0 (previous frame's final + publication + chain, then the cold search)", mla.K_KNN_FIRST),
                                                             ("fit_linearize+gn_finish (surf+corner)", mla.K_FIT),
                                                             ("map_index_build (both maps, 4 launches)", mla.K_GRID_BUILD))},
                       extract_ms_per_lidar_scan=[round(x, 4) for x in extract_ms],
                       extract_points_per_s=round(n_scan_points / (1e-3 * sum(extract_ms)), 1),
                       extract_ms_all_lidars_one_launch_set=round(extract_all_ms, 4),
                       ms_per_step_map_outgrows_its_grid_box=(round(outgrow_ms, 4) if outgrow_ms is not None else None),
                       roofline=roofline, roofline_time_dominant_kernel=roofline_fit)
        if cfg4 is not None:
            out["config4"] = cfg4
            if args.config4:      # config 4's frame is the headline; the single-pose frame's numbers stay in the line as `config2_leg`
                out["config2_leg"] = dict(value=out["value"], ms_per_step=out["ms_per_step"], workload=out["config"]["workload"], queries_per_s=out["queries_per_s"],
                                          valid_correspondences_per_step=out["valid_correspondences_per_step"])
                out["value"], out["ms_per_step"], out["queries_per_s"] = cfg4["value"], cfg4["ms_per_step"], cfg4["queries_per_s"]
                out["valid_correspondences_per_step"] = cfg4["valid_correspondences_per_step"]
                out["ms_per_gn_iter"] = round(cfg4["ms_per_step"] / GN_ITERS, 4)
                out["config"]["workload"] = cfg4["workload"]
                out["metric"] = "scan-to-map residuals+Jacobians/sec (features linearised per second, 5 GN iters/frame, 4 pose blocks: pose + 3 extrinsic SE3)"
        if frame is not None:
            out["frame"] = frame
        if predicted is not None:
            out["multi_gpu_predicted"] = predicted
        if s2m_ms is not None:
            out["scan2map"] = dict(ms_per_frame=round(s2m_ms, 4), ms_per_frame_synchronous_maps_staged=round(s2m_staged_ms, 4), ms_per_frame_pipelined=round(s2m_pipe_ms, 4),
                                   pipelined_frames_inside_the_lookahead=int(sum(1 for x in s2m_status if x == 0)), pipelined_frames=len(s2m_status),
                                   pipelined_pose_vs_synchronous=float(np.abs(np.asarray(s2m_pose_pipe) - np.asarray(s2m_pose_staged)).max()),
                                   submission_note="ms_per_frame = mlh_map_rebuild + mlh_scan2map, host waits for every pose; ..._synchronous_maps_staged = mlh_map_set_pair + mlh_scan2map; "
                                                   "..._pipelined = mlh_map_set_pair_overlapped + mlh_scan2map_begin_chained, pose collected one frame late (mlh_scan2map_end)",
                                   lm_iterations=[int(st["lm_iterations"]) for st in s2m_stats],
                                   note="supplementary: mlh_map_rebuild + mlh_scan2map (2 outer iterations, Ceres-shaped LM, Huber 0.1), "
                                        "the call the reference makes once per frame (lidar_mapper_keyframe.cpp:423-639)")

    # --- CPU baseline: the oracle (port of the reference's CPU path), bounded sample, rank 0 at N = 1 only
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        O.build()
        ms_, mc_ = O.Map(surf_map), O.Map(corner_map)
        prm = O.mapper_params()
        frames, t_total, t_kd = 0, 0.0, 0.0
        while t_total < args.cpu_seconds and frames < 50:
            tk = ms_.rebuild_seconds() + mc_.rebuild_seconds()
            r = O.gn_iterations(ms_, mc_, surf, corner, p0, prm, GN_ITERS, 1)
            t_kd += tk
            t_total += tk + r["seconds"]
            frames += 1
        n_valid_cpu = int(sum(i_["n_surf"] + i_["n_corner"] for i_ in r["iters"]))
        cpu_value = frames * n_valid_cpu / t_total
        ncores = min(os.cpu_count() or 1, 32)
        r_all = O.gn_iterations(ms_, mc_, surf, corner, p0, prm, GN_ITERS, ncores)
        tk_all = ms_.rebuild_seconds() + mc_.rebuild_seconds()
        out["cpu_baseline"] = dict(value=round(cpu_value, 1), unit="features/s", cores=1, kind="port",
                                   sample=f"{frames} full frames of the same workload (kd-tree rebuild for both maps + {GN_ITERS} GN iterations), "
                                          f"single thread as the reference mapper (no OpenMP in lidarMapper/, Ceres num_threads=1)",
                                   ms_per_frame=round(1e3 * t_total / frames, 2), kdtree_build_ms_per_frame=round(1e3 * t_kd / frames, 2),
                                   all_cores=dict(cores=ncores, value=round(n_valid_cpu / (r_all["seconds"] + tk_all), 1),
                                                  note="generous row: same code, OpenMP over features, kd-tree build still serial"),
                                   pose_agreement_m=float(np.linalg.norm(np.array(r["pose"][:3]) - np.array(pose[:3]))))
        if "scan2map" in out:
            import time as _t
            t3 = _t.perf_counter()
            tk3 = ms_.rebuild_seconds() + mc_.rebuild_seconds()
            rs = O.scan2map(ms_, mc_, surf, corner, p0, prm)
            out["scan2map"]["cpu_port_ms_per_frame"] = round(1e3 * (_t.perf_counter() - t3), 2)
            out["scan2map"]["cpu_port_lm_iterations"] = [int(o["lm_iterations"]) for o in rs["outer"]]
            out["scan2map"]["pose_agreement_m"] = float(np.linalg.norm(np.array(rs["pose"][:3]) - np.array(s2m_pose[:3])))
            # the reference's OWN lines of scan2MapOptimization (oracle/_ref: lidar_mapper_keyframe.cpp:423-639 compiled over the shim -- kd-tree, Eigen and the LM
            # iteration are restated there, everything else is the reference's text), one frame, kd-tree set-up included as in the reference: a second CPU figure for
            # the call, and one more check of the pose (checker only; skipped when the prebuilt library did not travel)
            try:
                if O.ref_lib() is not None:
                    import contextlib, io
                    t4 = _t.perf_counter()
                    with contextlib.redirect_stdout(io.StringIO()):
                        rr = O.ref_scan2map(surf_map, corner_map, surf, corner, p0)
                    out["scan2map"]["cpu_reference_lines_ms_per_frame"] = round(1e3 * (_t.perf_counter() - t4), 2)
                    out["scan2map"]["cpu_reference_lines_lm_iterations"] = [int(o["lm_iterations"]) for o in rr["solves"]]
                    out["scan2map"]["pose_agreement_with_reference_lines_m"] = float(np.linalg.norm(np.array(rr["pose"][:3]) - np.array(s2m_pose[:3])))
            except Exception as ex:                       # (a checker's failure must not cost the bench line)
                out["scan2map"]["cpu_reference_lines_error"] = str(ex)[:200]
        if "frame" in out:
            # the same frame through the CPU port, once: extractCloud per LiDAR -> fusion -> the plain covariance voxel filter in the std::sort member order +
            # evalPointUncertainty + trace gate -> kd-trees -> scan2MapOptimization (checker only: the GPU frame's pose against it, and a CPU figure beside it)
            try:
                import time as _t
                tf0 = _t.perf_counter()
                lists_ = []
                for s_ in scans:
                    ex_ = O.extract(s_.points, s_.scan_start, s_.scan_end)
                    lists_.append((s_.points, ex_["less_sharp"], ex_["less_flat_ds"]))
                surf_c, corner_c = [], []
                for i_, (pts_, ls_, lf_) in enumerate(lists_):
                    T_ = np.eye(4); T_[:3, :3] = synth.quat_to_rot(synth.HERCULES_BODY_T_LASER[i_][:4]); T_[:3, 3] = synth.HERCULES_BODY_T_LASER[i_][4:7]
                    for dst_, xyz_ in ((corner_c, pts_[ls_][:, :3]), (surf_c, lf_[:, :3])):
                        a_ = np.empty((len(xyz_), 4), np.float32)
                        a_[:, :3] = synth.transform_points(xyz_, T_); a_[:, 3] = i_
                        dst_.append(a_)
                f_ext = np.array([np.concatenate([r_[4:7], r_[:4]]) for r_ in synth.HERCULES_BODY_T_LASER])[:len(scans)]
                for e_ in f_ext:
                    e_[3:] /= np.linalg.norm(e_[3:])
                f_covs = np.stack([np.zeros((6, 6))] + [np.diag([0.0025] * 3 + [0.00030461] * 3)] * (len(scans) - 1))
                feats_ = []
                for cloud_, leaf_ in ((np.concatenate(surf_c), 0.4), (np.concatenate(corner_c), 0.2)):
                    ds_ = O.voxel_grid_mloam_plain(cloud_, leaf_, 0)
                    o_ = np.zeros((len(ds_), 11), np.float32); o_[:, :4] = ds_
                    for lid_ in range(len(scans)):
                        m_ = ds_[:, 3] == lid_
                        R_ = synth.quat_to_rot(f_ext[lid_][3:])
                        sel_ = ((ds_[m_, :3].astype(np.float64) - f_ext[lid_][:3]) @ R_).astype(np.float32)
                        c_ = O.eval_point_uncertainty(sel_, f_ext[lid_], f_covs[lid_], np.diag([0.0025] * 3))
                        o_[m_, 4:10] = np.stack([c_[:, 0, 0], c_[:, 0, 1], c_[:, 0, 2], c_[:, 1, 1], c_[:, 1, 2], c_[:, 2, 2]], axis=1)
                    o_[:, 10] = o_[:, 4] + o_[:, 7] + o_[:, 9]
                    feats_.append(o_[o_[:, 10] <= 0.6])
                ms2_, mc2_ = O.Map(surf_map), O.Map(corner_map)
                ms2_.rebuild_seconds(); mc2_.rebuild_seconds()
                rf_ = O.scan2map(ms2_, mc2_, feats_[0], feats_[1], p0, O.mapper_params(with_ua=True))
                out["frame"]["cpu_port_ms_per_frame"] = round(1e3 * (_t.perf_counter() - tf0), 1)
                out["frame"]["cpu_port_thinned_features"] = dict(surf=int(len(feats_[0])), corner=int(len(feats_[1])))
                out["frame"]["pose_vs_cpu_port_frame_m"] = float(np.linalg.norm(np.array(rf_["pose"][:3]) - np.array(out["frame"]["pose"][:3])))
                out["frame"]["pose_vs_cpu_port_frame_rad"] = float(2.0 * np.linalg.norm(np.array(rf_["pose"][3:6]) - np.array(out["frame"]["pose"][3:6])))
            except Exception as ex:
                out["frame"]["cpu_port_error"] = str(ex)[:200]
    if rank == 0:
        if args.dump_outputs:
            # what the caller of the timed path received from its last step (every rank holds the same pose: the solve's sums are all-reduced)
            dumped = dict(pose=np.asarray(pose, np.float64))
            if args.config4:
                dumped["config4_poses"] = np.asarray(poses4_t, np.float64)
            os.makedirs(args.dump_outputs, exist_ok=True)
            for name_, a_ in dumped.items():
                np.save(os.path.join(args.dump_outputs, f"{name_}.npy"), a_)
        print(json.dumps(out))
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
