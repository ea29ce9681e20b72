"""Loop-corrected poses into the keyframe store (include/mloam_hip.h (f15)) on the MI355X: what a correction of EVERY stored keyframe costs, at K stored keyframes
of BASELINE config-2 sizes (2 x 64-ring LiDARs, features thinned at 0.4 / 0.2 m) on a square grid 1.05 m apart, with the surrounding radius of the shipped config
(50 m; map_sur_kf_res 1.0, leaves 0.4 / 0.2, with_ua, trace threshold 0.6). Three legs, host clock around the calls, median of --reps with p10-p90:
  a  mlh_keyframes_update_from_pose_graph alone (the pose graph in a context of its own): one strided copy of 56 bytes per keyframe, one host wait, the host rules;
  b  a, then the mlh_local_map_assemble that rebuilds: the in-radius keyframes re-associated in one batch, the two covariance filters;
  c  the only route without the entry points: mlh_keyframes_reset, every keyframe saved again from host clouds at the corrected poses, then the same assemble.
Before every timed a / b the store is put back to the uncorrected poses and assembled there (untimed), so the cache is filled and every keyframe changes. The pose
graph holds the corrected poses as added (a smooth correction growing to 0.3 m and 3 degrees): the hand-over reads records, whichever pass wrote them.
One JSON line per K on stdout. Usage: python scripts/kubench.py [--reps 30] [--warmup 2] [--ks 100,1000,5000] [--legs a,b,c] [--parent COMMIT]
(--parent: the commit this tree sits on, recorded in every line; default: asked of git, null where there is no repository)"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), n=len(a))


def corrected(P0):
    P1 = P0.copy()
    for k in range(len(P0)):
        s = (k + 1) / len(P0)
        h = np.deg2rad(3.0 * s) / 2
        c, sn = np.cos(2 * h), np.sin(2 * h)
        x, y = P0[k, 0], P0[k, 1]
        P1[k, :3] = [c * x - sn * y + 0.3 * s, sn * x + c * y - 0.2 * s, P0[k, 2] + 0.05 * s]
        P1[k, 3:] = [0, 0, np.sin(h), np.cos(h)]             # (the grid's keyframes have identity rotations)
    return P1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="100,1000,5000")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    legs = args.legs.split(",")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    mla = importlib.import_module("m-loam_amd")
    synth = importlib.import_module("m-loam_amd.synth")
    import oracle as orc
    parent = args.parent
    if parent is None:
        try:
            parent = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            parent = None
    scene = synth.make_scene(seed=42, **synth.SCENE_PRESETS["50k"])
    ext, ext_cov = ext_and_cov(synth)
    surf, corner = frame_clouds(synth, orc, scene, synth.gt_body_pose())
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    cov = A @ A.T * 2e-5
    opts = mla.local_map_opts(surrounding_kf_radius=50.0, map_sur_kf_res=1.0, leaf_surf=0.4, leaf_corner=0.2, trace_threshold=0.6, with_ua=True, cov_measurement=MEAS)
    for K in [int(k) for k in args.ks.split(",")]:
        side_n = int(np.ceil(np.sqrt(K)))
        P0 = np.array([[1.05 * (i % side_n), 1.05 * (i // side_n), 0.3, 0, 0, 0, 1.0] for i in range(K)])
        P1 = corrected(P0)
        ctx, g = mla.Context(0), mla.Context(0)
        for k in range(K):
            g.pg_add_keyframe(P1[k])

        def save_all(poses):
            for k in range(K):
                ctx.keyframe_save(poses[k], cov, surf, corner)
        save_all(P0)
        c0, c1 = P0[K // 2], P1[K // 2]
        out = dict(K=K, surf_per_kf=len(surf), corner_per_kf=len(corner), radius=50.0, bytes_moved_a=56 * K, parent=parent)
        t = dict(a=[], b=[], c=[])
        for r in range(args.warmup + args.reps):
            if "a" in legs or "b" in legs:
                ctx.keyframes_update_poses(0, P0)
                ctx.local_map_clear()
                ctx.local_map_assemble(c0, ext, ext_cov, opts)
                ctx.synchronize()
                g.synchronize()
                t0 = time.perf_counter()
                up = ctx.keyframes_update_from_pose_graph(g)
                t1 = time.perf_counter()
                res = ctx.local_map_assemble(c1, ext, ext_cov, opts)
                t2 = time.perf_counter()
                assert up["n_changed"] == K and res["rebuilt"]
                t["a"].append(t1 - t0)
                t["b"].append(t2 - t0)
                out.update(n_changed=up["n_changed"], n_kf_in_map=len(res["kf_ids"]), n_cached=ctx.local_map_info()["n_cached"], n_surf_ds=res["n_surf_ds"],
                           n_corner_ds=res["n_corner_ds"])
            if "c" in legs:
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.keyframes_reset()
                save_all(P1)
                res = ctx.local_map_assemble(c1, ext, ext_cov, opts)
                t["c"].append(time.perf_counter() - t0)
                assert res["rebuilt"]
                if "n_surf_ds" in out:
                    assert (res["n_surf_ds"], res["n_corner_ds"]) == (out["n_surf_ds"], out["n_corner_ds"])       # the same map either way
        for leg, name in (("a", "update_from_pose_graph"), ("b", "update_then_assemble"), ("c", "reset_save_all_assemble")):
            if t[leg]:
                out[name] = stats(t[leg][args.warmup:])
        print(json.dumps(out), flush=True)
        ctx.close()
        g.close()


if __name__ == "__main__":
    main()
