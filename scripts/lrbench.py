"""Loop-closure local registration on the MI355X (mlh_loop_build_clouds, mlh_loop_register; m-loam_amd/csrc/loopreg.hip) at the reference's sizes: 21 data + 41
model keyframes of a street scene (a road, two facades, poles, facade edges, kerbs), 14.5 k surf / 2.7 k corner data features after the 0.4 m filters (the sizes
in the comment at mloam_loop/src/loop_registration.cpp:159), from a start whose yaw sits on Scan Context's 6-degree grid and whose translation is 0.73 m off:
  build_clouds  constructLocalMap: one transform launch over all keyframe segments, four voxel-grid filters; two host waits
  register      performLocalRegistration: staging of the two model clouds into the map indexes, then 2 outer iterations x (both matches, 1 + 5 evaluate launches,
                1 + 5 LM launches); one host wait per outer iteration. register_warm: the same call again (the model clouds are still staged)
  register_split   per call, from mlh_profile_*: match = the two match launches, evaluate = the evaluate launches, lm = the one-workgroup LM launches (event
                brackets: measured in runs of their own, their sum is not the host clock's time)
  cpu_loop      the same arithmetic as a plain single-threaded C++ loop on this machine's CPU: the restatement the tests compare against
                (tests/host/loopreg_ref.cpp, g++ -O2; k-d tree search instead of the cell grid) for register, the checker's transform + VoxelGrid for build_clouds
Host clock around the calls (each ends in a host wait) after warm-up; median with p10 / p90. One JSON line per leg on stdout and appended to --out.
Usage: python scripts/lrbench.py [--reps 30] [--warmup 5] [--cpu-reps 5] [--out profiles/f12_lrbench.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DATA, N_MODEL = 21, 41
SURF_PER_KF, CORNER_PER_KF = 1050, 420


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), reps=len(a))


def yaw_T(deg, t=(0.0, 0.0, 0.0)):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


def keyframe(rng, T, n_surf, n_corner):
    """what a keyframe at T sees within 30 m along the street: the road z = 0 (|y| < 12), the facades y = +-12 (8 m high), poles every 1.5 m at y = +-9 (5 m high),
    facade edges every 4 m (8 m high) and the kerbs y = +-8; 0.02 m jitter; in the keyframe's frame"""
    x0 = T[0, 3]
    part = rng.choice(3, n_surf, p=[0.5, 0.25, 0.25])
    x = x0 + rng.uniform(-30.0, 30.0, n_surf)
    y = np.where(part == 0, rng.uniform(-12.0, 12.0, n_surf), np.where(part == 1, 12.0, -12.0))
    z = np.where(part == 0, 0.0, rng.uniform(0.0, 8.0, n_surf))
    surf = np.stack([x, y, z], 1)
    kind = rng.choice(3, n_corner, p=[0.45, 0.4, 0.15])
    u = x0 + rng.uniform(-30.0, 30.0, n_corner)
    px = np.where(kind == 0, np.round(u / 1.5) * 1.5, np.where(kind == 1, np.round(u / 4.0) * 4.0 + 0.5, u))
    py = np.where(kind == 0, 9.0, np.where(kind == 1, 11.6, 8.0)) * rng.choice([-1.0, 1.0], n_corner)
    pz = np.where(kind == 2, 0.15, rng.uniform(0.0, 1.0, n_corner) * np.where(kind == 0, 5.0, 8.0))
    corner = np.stack([px, py, pz], 1)
    Ti = np.linalg.inv(T)
    out = []
    for w in (surf, corner):
        w = w + rng.normal(0.0, 0.02, w.shape)
        loc = w @ Ti[:3, :3].T + Ti[:3, 3]
        out.append(np.ascontiguousarray(np.concatenate([loc, np.zeros((len(loc), 1))], 1), np.float32))
    return out


def make_case(rng):
    """keys 0..40 the first pass (1 m apart), 41..61 the second pass displaced by `truth`; the lists of constructLocalMap for the query at the second pass's last
    keyframe and the match at the first pass's 20th"""
    truth = yaw_T(25.0, (0.6, -0.4, 0.1))
    poses, clouds = [], []
    for k in range(N_MODEL + N_DATA):
        base = np.eye(4)
        base[:3, 3] = [float(k if k < N_MODEL else k - N_MODEL), 0.0, 1.5]
        T = base if k < N_MODEL else base @ truth
        poses.append(T)
        clouds.append(keyframe(rng, T, SURF_PER_KF, CORNER_PER_KF))
    que, match = N_MODEL + N_DATA - 1, 20
    data = [(k, (np.linalg.inv(poses[que]) @ poses[k]).astype(np.float32)) for k in range(N_MODEL, N_MODEL + N_DATA)]
    model = [(k, (np.linalg.inv(poses[match]) @ poses[k]).astype(np.float32)) for k in range(N_MODEL)]
    T_true = np.linalg.inv(poses[match]) @ poses[que]
    T_ini = T_true.copy()
    T_ini[:3, :3] = yaw_T(24.0)[:3, :3]
    T_ini[:3, 3] = T_true[:3, 3] + np.array([-0.6, 0.4, -0.1])               # FGR's / the odometry's translation, off by the scene's displacement
    return poses, clouds, data, model, T_ini, T_true


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-only", action="store_true", help="sizes and the CPU loop only (no GPU needed)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import loopreg_cases as lc          # the restatement = the CPU loop
    import oracle as orc
    orc.build()
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(2)
    poses, clouds, data, model, T_ini, T_true = make_case(rng)
    lines = []

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    # the CPU loop (also the sizes)
    ts_build, ts_reg, c4, want = [], [], None, None
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        pre = [np.concatenate([lc.transform(clouds[k][kind], Tf) for k, Tf in lst]) for lst in (model, data) for kind in (0, 1)]
        c4 = [orc.voxel_grid(p, 0.4) for p in pre]
        ts_build.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = lc.register(c4, T_ini)
        ts_reg.append(time.perf_counter() - t0)
    info = dict(data_keyframes=N_DATA, model_keyframes=N_MODEL, n_pre=[len(p) for p in pre], n_ds=[len(c) for c in c4])
    emit(**info, leg="cpu_loop_build_clouds", **stats(ts_build), note="single thread: f32 transform + concatenation + the checker's pcl::VoxelGrid x 4")
    emit(**info, leg="cpu_loop_register", **stats(ts_reg), surf_num=[o["surf_num"] for o in want["outer"]], corner_num=[o["corner_num"] for o in want["outer"]],
         lm_iterations=[o["lm_iterations"] for o in want["outer"]], opti_cost=round(want["opti_cost"], 4), err_vs_truth=float(np.abs(want["T_relative"] - T_true).max()),
         note="single thread, g++ -O2: k-d tree build x 2, then per outer iteration both matches and the Ceres-shaped LM")
    if not args.cpu_only:
        import torch
        torch.cuda.init()
        mla = importlib.import_module("m-loam_amd")
        ctx = mla.Context(0)
        for T, (surf, corner) in zip(poses, clouds):
            ctx.keyframe_save(np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()]), np.eye(6) * 1e-4, surf, corner)
        ts = []
        for _ in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            n_pre, n_ds = ctx.loop_build_clouds(data, model)
            ts.append(time.perf_counter() - t0)
        assert list(n_ds) == info["n_ds"], (list(n_ds), info["n_ds"])
        emit(**info, leg="build_clouds", **stats(ts[args.warmup:]), allocations=ctx.loop_info()["allocations"])
        cold, warm = [], []
        for _ in range(args.warmup + args.reps):
            ctx.loop_build_clouds(data, model)                                # (a new build: the next register stages the model clouds again)
            ctx.synchronize()
            t0 = time.perf_counter()
            got = ctx.loop_register(T_ini)
            cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.loop_register(T_ini)
            warm.append(time.perf_counter() - t0)
        res = dict(surf_num=[o["surf_num"] for o in got["outer"]], corner_num=[o["corner_num"] for o in got["outer"]], lm_iterations=[o["lm_iterations"] for o in got["outer"]],
                   opti_cost=round(got["opti_cost"], 4), accepted=got["accepted"], err_vs_cpu_loop=float(np.abs(got["T_relative"] - want["T_relative"]).max()))
        emit(**info, leg="register", **stats(cold[args.warmup:]), **res)
        emit(**info, leg="register_warm", **stats(warm[args.warmup:]))
        ids = dict(match=mla.K_KNN, evaluate=mla.K_LINEARIZE, lm=mla.K_SOLVE)
        ctx.profile_enable(sum(1 << v for v in ids.values()))
        ctx.profile_reset()
        n_prof = max(5, args.reps // 3)
        for _ in range(n_prof):
            ctx.loop_register(T_ini)
        split = {}
        for name, kid in ids.items():
            ms, launches = ctx.profile_get(kid)
            split[name + "_ms"] = round(ms / n_prof, 4)
            split[name + "_brackets"] = int(launches // n_prof)
        ctx.profile_enable(0)
        emit(**info, leg="register_split", calls=n_prof, **split, note="event brackets per call of register_warm's kind; brackets add queue time of their own")
        ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
