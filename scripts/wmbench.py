"""One odometry window frame on the MI355X: the newest slot is set, the local map of every LiDAR is built (buildLocalMap, estimator.cpp:1159-1204), the maps and
the features of every (LiDAR, frame pivot + 1 .. WINDOW_SIZE) are staged for the matching (cpp:1228-1266; the matching itself is the same in every leg and is
left out), the window slides. Two sizes: the shipped hercules configuration (4 LiDARs x 16 rings, window 3) and 2 LiDARs x 64 rings. Three legs:
  a  host_loop     the per-call loop of INTEGRATION.md 4c' with host clouds: mlh_transform_point_cloud per (LiDAR, slot, kind), concatenation on the host,
                   mlh_voxel_grid per map cloud, mlh_map_set_pair / mlh_features_set from host arrays;
  b  device_loop   the same loop over caller-owned device buffers (copies on the context's stream, mlh_transform_point_cloud / mlh_voxel_grid /
                   mlh_map_set_pair / mlh_features_set with MLH_MEM_DEVICE);
  c  window_store  mlh_window_set + mlh_window_build_local_map + mlh_map_set_pair / mlh_features_set from mlh_window_map_cloud / mlh_window_cloud +
                   mlh_window_slide (new clouds handed over from host arrays, c_host, or from device buffers, c_device).
Legs a and b use only entry points that exist without the window store: they are the baseline. Host clock around whole frames (the last call of a frame waits
for the stream), median of --reps frames after --warmup. transform_launches / host_waits: per frame, for the map build, by construction of the calls
(a host-cloud transform waits once; a voxel grid with a caller's output waits three times: bounds, count, result; the store's build waits twice).
One JSON line per (size, leg) on stdout.  Usage: python scripts/wmbench.py [--reps 60] [--warmup 10] [--sizes hercules,2x64]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(hercules=dict(n_lidar=4, n_rings=16, n_cols=1800), **{"2x64": dict(n_lidar=2, n_rings=64, n_cols=1800)})
WINDOW, PIVOT = 3, 1                       # WINDOW_SIZE 3, OPT_WINDOW_SIZE 2
D2D = 3                                    # hipMemcpyDeviceToDevice


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def make_inputs(synth, orc, cfg, n_poses=5):
    """per pose and LiDAR the (surf, corner) clouds of a slot (cpp:487-495) and pose_local (cpp:1181) for a window of WINDOW + 1 consecutive poses"""
    from scipy.spatial.transform import Rotation as Rot
    to_pose = lambda T: np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
    scene = synth.make_scene(seed=42, **synth.SCENE_PRESETS["50k"])
    T = [synth.pose_to_mat(synth.gt_body_pose())]
    for i in range(1, n_poses):
        d = np.eye(4)
        d[:3, :3] = Rot.from_rotvec(np.deg2rad([0.3, -0.2, 1.0])).as_matrix()
        d[:3, 3] = [0.4, 0.05, 0.01]
        T.append(T[-1] @ d)
    exts = []
    for n in range(cfg["n_lidar"]):
        r = synth.HERCULES_BODY_T_LASER[n]
        exts.append(synth.pose_to_mat(np.concatenate([r[4:7], r[:4] / np.linalg.norm(r[:4])])))
    pool = []
    for i in range(n_poses):
        pool.append([])
        for n in range(cfg["n_lidar"]):
            scn = synth.simulate_scan(scene, to_pose(T[i]), synth.HERCULES_BODY_T_LASER[n], cfg["n_rings"], n_cols=cfg["n_cols"], seed=100 + 10 * i + n)
            ex = orc.extract(scn.points, scn.scan_start, scn.scan_end)
            pool[i].append((orc.voxel_grid(np.ascontiguousarray(ex["less_flat_ds"][:, :4]), 0.4), orc.voxel_grid(np.ascontiguousarray(scn.points[ex["less_sharp"]]), 0.2)))
    Tinv = np.linalg.inv(T[PIVOT])
    poses = np.stack([np.stack([to_pose(Tinv @ T[i] @ exts[n]) for i in range(WINDOW + 1)]) for n in range(cfg["n_lidar"])])
    return pool, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="hercules,2x64")
    ap.add_argument("--legs", default="host_loop,device_loop,window_store")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    synth = importlib.import_module("m-loam_amd.synth")
    import oracle as orc
    orc.build()
    hip = mla._hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    legs = args.legs.split(",")
    for size in args.sizes.split(","):
        cfg = SIZES[size]
        L = cfg["n_lidar"]
        pool, poses = make_inputs(synth, orc, cfg)
        opts = mla.window_map_opts(cfg["n_rings"], L, WINDOW)
        leaf = float(opts.leaf_surf[0])
        new_cloud = lambda f, n: pool[f % len(pool)][n]
        n_seg = L * WINDOW * 2
        info = dict(size=size, n_lidar=L, n_rings=cfg["n_rings"], window=WINDOW, leaf=round(leaf, 4),
                    slot_points=[int(np.mean([len(p[n][k]) for p in pool for n in range(L)])) for k in range(2)])

        def timed(frame, ctx):
            ts = []
            for f in range(args.warmup + args.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                out = frame(f)
                ts.append(time.perf_counter() - t0)
            return out, stats(ts[args.warmup:])

        if "host_loop" in legs:
            ctx = mla.Context(0)
            stack = [[new_cloud(i, n) for i in range(WINDOW + 1)] for n in range(L)]

            def frame_a(f):
                n_ds = []
                for n in range(L):
                    stack[n][WINDOW] = new_cloud(f, n)
                for n in range(L):
                    ds = []
                    for k in range(2):
                        pre = np.concatenate([ctx.transform_point_cloud(stack[n][i][k], poses[n][i]) for i in range(WINDOW)])
                        ds.append(ctx.voxel_grid(pre, leaf))
                    ctx.map_set_pair(ds[0], ds[1])
                    for i in range(PIVOT + 1, WINDOW + 1):
                        for k in range(2):
                            ctx.features_set(k, stack[n][i][k])
                    n_ds.append([len(ds[0]), len(ds[1])])
                for n in range(L):
                    stack[n] = stack[n][1:] + [stack[n][WINDOW]]
                return n_ds
            n_ds, st = timed(frame_a, ctx)
            print(json.dumps(dict(info, leg="a_host_loop", n_ds=n_ds, transform_launches=n_seg, host_waits=n_seg + 3 * 2 * L, **st)), flush=True)
            ctx.close()

        dev_pool = None
        if "device_loop" in legs or "window_store" in legs:
            dev_pool = [[tuple(torch.from_numpy(c).cuda() for c in pool[i][n]) for n in range(L)] for i in range(len(pool))]
            torch.cuda.synchronize()
        if "device_loop" in legs:
            ctx = mla.Context(0)
            lib, st_ = ctx.lib, ctx.stream()
            cap = max(len(c) for p in pool for pn in p for c in pn) * WINDOW + 1
            acc = [torch.zeros((cap, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
            out = [torch.zeros((cap, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            stack = [[dev_pool[i % len(pool)][n] for i in range(WINDOW + 1)] for n in range(L)]
            pose_c = np.ascontiguousarray(poses, np.float64)

            def frame_b(f):
                n_ds = []
                for n in range(L):
                    stack[n][WINDOW] = dev_pool[f % len(pool)][n]
                for n in range(L):
                    cnt = [C.c_int32(0), C.c_int32(0)]
                    for k in range(2):
                        fill = 0
                        for i in range(WINDOW):
                            seg = stack[n][i][k]
                            m = seg.shape[0]
                            dst = C.c_void_p(acc[k].data_ptr() + 16 * fill)
                            assert hip.hipMemcpyAsync(dst, C.c_void_p(seg.data_ptr()), 16 * m, D2D, st_) == 0
                            ctx._ck(lib.mlh_transform_point_cloud(ctx.h, dst, 16, m, pose_c[n, i].ctypes.data_as(C.c_void_p), mla.MEM_DEVICE))
                            fill += m
                        ctx._ck(lib.mlh_voxel_grid(ctx.h, C.c_void_p(acc[k].data_ptr()), 16, fill, 12, leaf, C.c_void_p(out[k].data_ptr()), C.byref(cnt[k]), mla.MEM_DEVICE))
                    ctx.map_set_pair(out[0][:cnt[0].value], out[1][:cnt[1].value])
                    for i in range(PIVOT + 1, WINDOW + 1):
                        for k in range(2):
                            ctx.features_set(k, stack[n][i][k])
                    n_ds.append([cnt[0].value, cnt[1].value])
                for n in range(L):
                    stack[n] = stack[n][1:] + [stack[n][WINDOW]]
                return n_ds
            n_ds, st = timed(frame_b, ctx)
            print(json.dumps(dict(info, leg="b_device_loop", n_ds=n_ds, transform_launches=n_seg, host_waits=3 * 2 * L, **st)), flush=True)
            ctx.close()

        if "window_store" in legs:
            for name, src in (("c_window_store_host_input", pool), ("c_window_store_device_input", dev_pool)):
                ctx = mla.Context(0)
                ctx.window_reset(L, WINDOW)
                for i in range(WINDOW + 1):              # fill the buffer as the INITIAL phase does: slot i pushed onto itself
                    for n in range(L):
                        ctx.window_set(n, i, *src[i % len(pool)][n])
                    ctx.window_slide(i)                  # (from here on the buffer is full: every further slide drops the oldest slot)

                def frame_c(f):
                    for n in range(L):
                        ctx.window_set(n, WINDOW, *src[f % len(pool)][n])
                    r = ctx.window_build_local_map(poses, opts)
                    for n in range(L):
                        ctx.map_set_pair(ctx.window_map_cloud(n, mla.SURF), ctx.window_map_cloud(n, mla.CORNER))
                        for i in range(PIVOT + 1, WINDOW + 1):
                            for k in range(2):
                                ctx.features_set(k, ctx.window_cloud(n, i, k))
                    ctx.window_slide(WINDOW)
                    return r["n_ds"].tolist()
                n_ds, st = timed(frame_c, ctx)
                print(json.dumps(dict(info, leg=name, n_ds=n_ds, transform_launches=1, host_waits=2, allocations=ctx.window_info()["allocations"], **st)), flush=True)
                ctx.close()


if __name__ == "__main__":
    main()
