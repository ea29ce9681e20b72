"""Local-map assembly from keyframes (extractSurroundingKeyFrames, lidar_mapper_keyframe.cpp:254-354) on the MI355X at BASELINE config-2 keyframe sizes
(2 x 64-ring LiDARs, features thinned at 0.4 / 0.2 m), K surrounding keyframes:
  first   all K keyframes enter (an empty cache), then the two covariance filters;
  steady  one keyframe enters and one leaves (the vehicle moved one keyframe spacing), after a clearCloud.
Three ways: the new call (mlh_local_map_assemble), today's per-keyframe C-ABI loop on device buffers (mlh_cloud_uct_associate_to_map per keyframe and kind,
then mlh_voxel_filter x 2; it has no cache, so it transforms every surrounding keyframe on every rebuild), and the CPU restatement over the reference-built
calls (once, first assembly only). Host clock around synchronised calls after warm-up. One JSON line per (K, leg, way) on stdout.
Usage: python scripts/kfbench.py [--reps 50] [--warmup 5] [--ks 10,30,60]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MEAS = np.diag([0.0025] * 3)


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
    return orc.ref_voxel_filter(p, 0.4), orc.ref_voxel_filter(np.ascontiguousarray(p[::3]), 0.2)


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="10,30,60")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    synth = importlib.import_module("m-loam_amd.synth")
    import oracle as orc
    scene = synth.make_scene(seed=42, **synth.SCENE_PRESETS["50k"])
    ext, ext_cov = ext_and_cov(synth)
    surf, corner = frame_clouds(synth, orc, scene, synth.gt_body_pose())
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    cov = A @ A.T * 2e-5
    spacing = 1.05
    for K in [int(k) for k in args.ks.split(",")]:
        n_kf = K + args.reps + args.warmup + 2
        poses = [np.array([spacing * i, 0.0, 0.3, 0, 0, 0, 1.0]) for i in range(n_kf)]
        radius = (K - 1) / 2 * spacing + 0.01
        opts = mla.local_map_opts(surrounding_kf_radius=radius, map_sur_kf_res=1.0, leaf_surf=0.4, leaf_corner=0.2, trace_threshold=0.6, with_ua=True,
                                  cov_measurement=MEAS)
        centre = lambda i: np.array([spacing * (i + (K - 1) / 2), 0.0, 0.3, 0, 0, 0, 1.0])   # keyframes i .. i + K - 1 in the radius
        ctx = mla.Context(0)
        for p in poses:
            ctx.keyframe_save(p, cov, surf, corner)
        info = dict(K=K, surf_per_kf=len(surf), corner_per_kf=len(corner))
        # ---- the new call: first assembly (fresh cache each time: a reset store would re-upload, so the cache is emptied by a far-away call)
        far = np.array([-1e4, 0, 0, 0, 0, 0, 1.0])
        t_first = []
        for r in range(args.warmup + args.reps):
            ctx.local_map_clear()
            ctx.local_map_assemble(far, ext, ext_cov, opts)            # nothing in the radius: the cache empties
            ctx.local_map_clear()
            ctx.synchronize()
            t0 = time.perf_counter()
            out = ctx.local_map_assemble(centre(0), ext, ext_cov, opts)
            t_first.append(time.perf_counter() - t0)
            assert out["rebuilt"] and len(out["kf_ids"]) >= 1
        n_pre = (ctx.local_map_cloud(mla.SURF, False).n, ctx.local_map_cloud(mla.CORNER, False).n)
        n_ds = (out["n_surf_ds"], out["n_corner_ds"])
        print(json.dumps(dict(info, leg="first", way="device_call", ids=len(out["kf_ids"]), n_pre=n_pre, n_ds=n_ds, **stats(t_first[args.warmup:]))), flush=True)
        # ---- steady state: one in, one out
        t_steady = []
        for r in range(args.warmup + args.reps):
            ctx.local_map_clear()
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.local_map_assemble(centre(r + 1), ext, ext_cov, opts)
            t_steady.append(time.perf_counter() - t0)
        print(json.dumps(dict(info, leg="steady", way="device_call", **stats(t_steady[args.warmup:]))), flush=True)
        # ---- today's per-keyframe C-ABI loop on device buffers (every surrounding keyframe transformed on every rebuild; the same ds selection)
        side = mla.Context(0)
        d_s = torch.from_numpy(np.pad(surf, ((0, 0), (0, 7)))).cuda()
        d_c = torch.from_numpy(np.pad(corner, ((0, 0), (0, 7)))).cuda()
        d_acc = [torch.zeros((K * len(surf) + 1, 11), dtype=torch.float32, device="cuda"), torch.zeros((K * len(corner) + 1, 11), dtype=torch.float32, device="cuda")]
        d_ds = [torch.zeros_like(d_acc[0]), torch.zeros_like(d_acc[1])]
        torch.cuda.synchronize()

        def abi_loop(first):
            fill = [0, 0]
            for i in range(first, first + K):
                for k, src in ((0, d_s), (1, d_c)):
                    fill[k] += side.cloud_uct_associate_to_map_device(src, d_acc[k][fill[k]:], poses[i], cov, ext, ext_cov, MEAS, True, 0.6)
            return [side.voxel_filter_device(d_acc[k][:fill[k]], d_ds[k], (0.4, 0.2)[k], 0.6) for k in range(2)]
        t_abi = []
        for r in range(args.warmup + args.reps):
            side.synchronize()
            t0 = time.perf_counter()
            abi_loop(r % 3)
            t_abi.append(time.perf_counter() - t0)
        print(json.dumps(dict(info, leg="first_or_steady", way="abi_loop_per_keyframe", **stats(t_abi[args.warmup:]))), flush=True)
        side.close()
        # ---- the CPU restatement over the reference-built calls, once
        if not args.no_cpu:
            t0 = time.perf_counter()
            pre = [[], []]
            s11 = np.pad(surf, ((0, 0), (0, 7))).astype(np.float32)
            c11 = np.pad(corner, ((0, 0), (0, 7))).astype(np.float32)
            for i in range(K):
                pre[0].append(orc.ref_cloud_uct_associate_to_map(s11, poses[i], cov, ext, ext_cov, MEAS, True, 0.6))
                pre[1].append(orc.ref_cloud_uct_associate_to_map(c11, poses[i], cov, ext, ext_cov, MEAS, True, 0.6))
            for k, leaf in ((0, 0.4), (1, 0.2)):
                orc.ref_voxel_filter(np.concatenate(pre[k]), leaf, 0.6)
            print(json.dumps(dict(info, leg="first", way="cpu_restatement_once", ms=round((time.perf_counter() - t0) * 1e3, 2))), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
