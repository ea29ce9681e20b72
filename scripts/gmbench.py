"""The global map built from the keyframe store (pubGlobalMap / saveGlobalMap, lidar_mapper_keyframe.cpp:796-849, 853-901) on the MI355X at BASELINE config-2
keyframe sizes (2 x 64-ring LiDARs, features thinned at 0.4 / 0.2 m, the outlier cloud at 0.8 m), K selected keyframes on a square grid 1.05 m apart (a
compact site: on a long line the trace gate drops every point of a keyframe far from the origin, and the map stops growing with K), both modes:
  publish  one cloud (per keyframe surf, corner, outlier), filtered at MAP_SURF_RES;
  save     two clouds (surf + outlier, corner), each filtered at 2 * MAP_SURF_RES.
Three ways: the new call (mlh_global_map_assemble), the per-keyframe C-ABI loop on device buffers it replaces (mlh_cloud_uct_associate_to_map per keyframe and
kind into an accumulator, then mlh_voxel_filter per output cloud) and the CPU restatement over the reference-built calls (once). Host clock around synchronised
calls after warm-up. One JSON line per (K, mode, way) on stdout.
--tree DIR measures the loop with the package and library of another checkout of this repository (the parent commit: the bar the new call is held against);
the new call is then skipped.
Usage: python scripts/gmbench.py [--reps 20] [--warmup 3] [--ks 10,60,300] [--ways device_call,abi_loop,cpu] [--tree DIR]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEAS = np.diag([0.0025] * 3)
MODES = dict(publish=dict(split=0, leaf=0.4, groups=[[0, 1, 2]]), save=dict(split=1, leaf=0.8, groups=[[0, 2], [1]]))


def ext_and_cov(synth):
    ext = np.array([np.concatenate([r[4:7], r[:4]]) for r in synth.HERCULES_BODY_T_LASER])[:2]
    for e in ext:
        e[3:] /= np.linalg.norm(e[3:])
    return ext, np.stack([np.zeros((6, 6)), np.diag([0.0025] * 3 + [0.00030461] * 3)])


def frame_clouds(synth, orc, scene, pose):
    pts = []
    for i in range(2):
        sc = synth.simulate_scan(scene, pose, synth.HERCULES_BODY_T_LASER[i], 64, n_cols=1800, seed=11 + i)
        T = np.eye(4)
        T[:3, :3] = synth.quat_to_rot(synth.HERCULES_BODY_T_LASER[i][:4])
        T[:3, 3] = synth.HERCULES_BODY_T_LASER[i][4:7]
        p = np.zeros((len(sc.points), 4), np.float32)
        p[:, :3] = synth.transform_points(sc.points[:, :3], T)
        p[:, 3] = i
        pts.append(p)
    p = np.ascontiguousarray(np.concatenate(pts))
    return (orc.ref_voxel_filter(p, 0.4), orc.ref_voxel_filter(np.ascontiguousarray(p[::3]), 0.2), orc.ref_voxel_filter(np.ascontiguousarray(p[1::7]), 0.8))


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="10,60,300")
    ap.add_argument("--ways", default="device_call,abi_loop,cpu")
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    ways = [w for w in args.ways.split(",") if not (args.tree and w == "device_call")]
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    synth = importlib.import_module("m-loam_amd.synth")
    import oracle as orc
    scene = synth.make_scene(seed=42, **synth.SCENE_PRESETS["50k"])
    ext, ext_cov = ext_and_cov(synth)
    clouds = frame_clouds(synth, orc, scene, synth.gt_body_pose())
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    cov = A @ A.T * 2e-5
    spacing = 1.05
    label = "parent_tree" if args.tree else "this_tree"
    for K in [int(k) for k in args.ks.split(",")]:
        side_n = int(np.ceil(np.sqrt(K)))
        poses = [np.array([spacing * (i % side_n), spacing * (i // side_n), 0.3, 0, 0, 0, 1.0]) for i in range(K)]
        info = dict(K=K, surf_per_kf=len(clouds[0]), corner_per_kf=len(clouds[1]), outlier_per_kf=len(clouds[2]), tree=label)
        if "device_call" in ways:
            ctx = mla.Context(0)
            for j, p in enumerate(poses):
                ctx.keyframe_save(p, cov, clouds[0], clouds[1])
                ctx.keyframe_attach_outlier(j, clouds[2])
            for mode, m in MODES.items():
                # kf_res below the keyframe spacing: every one of the K keyframes is selected
                opts = mla.global_map_opts(for_save=(mode == "save"), kf_res=0.5, leaf=m["leaf"], trace_threshold=0.6, with_ua=True, cov_measurement=MEAS)
                ts = []
                for r in range(args.warmup + args.reps):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    out = ctx.global_map_assemble(poses[K // 2], ext, ext_cov, opts)
                    ts.append(time.perf_counter() - t0)
                assert len(out["kf_ids"]) == K
                print(json.dumps(dict(info, mode=mode, way="device_call", n_pre=out["n_pre"], n_ds=out["n_ds"], **stats(ts[args.warmup:]))), flush=True)
            ctx.close()
        if "abi_loop" in ways:
            side = mla.Context(0)
            d_src = [torch.from_numpy(np.pad(c, ((0, 0), (0, 7)))).cuda() for c in clouds]
            n_all = sum(len(c) for c in clouds)
            d_acc = [torch.zeros((K * n_all + 1, 11), dtype=torch.float32, device="cuda"), torch.zeros((K * len(clouds[1]) + 1, 11), dtype=torch.float32, device="cuda")]
            d_ds = [torch.zeros_like(d_acc[0]), torch.zeros_like(d_acc[1])]
            torch.cuda.synchronize()
            for mode, m in MODES.items():
                def abi_loop():
                    n_ds = []
                    for g, kinds in enumerate(m["groups"]):
                        fill = 0
                        for i in range(K):
                            for k in kinds:
                                fill += side.cloud_uct_associate_to_map_device(d_src[k], d_acc[g][fill:], poses[i], cov, ext, ext_cov, MEAS, True, 0.6)
                        n_ds.append(side.voxel_filter_device(d_acc[g][:fill], d_ds[g], m["leaf"], 0.6))
                    return n_ds
                ts = []
                for r in range(args.warmup + args.reps):
                    side.synchronize()
                    t0 = time.perf_counter()
                    n_ds = abi_loop()
                    ts.append(time.perf_counter() - t0)
                print(json.dumps(dict(info, mode=mode, way="abi_loop_per_keyframe", n_ds=n_ds, **stats(ts[args.warmup:]))), flush=True)
            side.close()
            del d_acc, d_ds, d_src
            torch.cuda.empty_cache()
        if "cpu" in ways:
            c11 = [np.pad(c, ((0, 0), (0, 7))).astype(np.float32) for c in clouds]
            for mode, m in MODES.items():
                t0 = time.perf_counter()
                for kinds in m["groups"]:
                    pre = [orc.ref_cloud_uct_associate_to_map(c11[k], poses[i], cov, ext, ext_cov, MEAS, True, 0.6) for i in range(K) for k in kinds]
                    orc.ref_voxel_filter(np.concatenate(pre), m["leaf"], 0.6)
                print(json.dumps(dict(info, mode=mode, way="cpu_restatement_once", ms=round((time.perf_counter() - t0) * 1e3, 2))), flush=True)


if __name__ == "__main__":
    main()
